"""CPU: guidance_interval= / uncond_cache_interval= on the emulated operator layer (tests/fake_ops.py plus the new operator's emulation in
tests/uncond_cache_ref.py): every refusal, the defaults as the parent's call list, the schedule of off / full / cached steps, and the loop against its
restatement.

Bound of the last.  The restated loop (uncond_cache_ref.denoise_loop) makes the pipeline's own UNet calls and rounds its latents to fp16 after every
step, so the two differ by the tail only: fp32 against float64 in front of one fp16 rounding.  Where the two tails fall on different sides of a
rounding boundary an element differs by one fp16 ulp, 2^-10 relative at most, and the next UNet call sees it; elsewhere they are equal.  A rel-L2 of
2^-10 would need EVERY element one ulp off: the test asks for rel-L2 <= 2^-10 and cosine >= 1 - 2^-20."""
import pytest
import torch
import torch.distributed as dist

import fake_ops
import mikudance_amd as M
import uncond_cache_ref as UR
from loop_helpers import CountingUNet, cosine, rel_l2, run_world, small_cpu, small_inputs, worker_setup, zero_inputs  # noqa: F401
from mikudance_amd.selftest import SCHED_KWARGS
from mikudance_amd.synth import synth_inputs

G = 3.0
PLAN_KW = dict(guidance_rescale=0.0, strength=1.0, context_fuse="flat", free_init_iters=1, free_init_filter="butterworth", free_init_order=4,
               free_init_spatial_stop=0.25, free_init_temporal_stop=0.25, free_init_fast=False, apg=False, apg_eta=0.0, apg_norm_threshold=0.0,
               apg_momentum=0.0, pag_scale=0.0, pag_adaptive_scale=0.0, pag_applied_layers=("mid",), kv_downsample=1, kv_downsample_mode="nearest",
               seg_scale=0.0, seg_blur_sigma=100.0, seg_applied_layers=("mid",))


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _pipe(small_cpu, sch=None):
    ref, den, _, _ = small_cpu
    return M.MikuDanceVideoPipeline(None, None, ref, den, sch or _ddim())


class _Spy:
    """Every forward_nhwc call of a denoise(): batch, conditional=, perturbed?, its keywords."""

    def __init__(self, den, monkeypatch):
        self.calls = []
        real = den.forward_nhwc

        def forward_nhwc(x, nb, f, t, cross, **kw):
            self.calls.append(dict(nb=nb, rows=x.shape[0], f=f, cond=bool(kw.get("conditional")), pert="pag" in kw or "seg" in kw, kw=sorted(kw)))
            return real(x, nb, f, t, cross, **kw)

        monkeypatch.setattr(den, "forward_nhwc", forward_nhwc, raising=False)

    def main(self):
        return [c for c in self.calls if not c["pert"]]


def _per_step():
    """[(step operator, [(mode, scale, delta given?) of the cfg_uncond_cache calls in front of it])] from the call log."""
    out, pending = [], []
    for name, d in fake_ops.CALLS:
        if name == "cfg_uncond_cache":
            pending.append((d["mode"], d["scale"], "delta" in d["keywords"]))
        elif name.startswith("cfg_") and "_step" in name:
            out.append((name, pending))
            pending = []
    assert not pending
    return out


FULL, CACHED, OFF = [(0, 1.0, True)], [(1, 1.0, True)], [(1, 0.0, False)]
OPS = {"full": FULL, "cached": CACHED, "off": OFF}


def _check(spy, kinds, n):
    """One window per step: the main call's batch and the operator calls follow `kinds`."""
    main = spy.main()
    assert [(c["nb"], c["cond"]) for c in main] == [(2, False) if k == "full" else (1, True) for k in kinds], main
    assert all(c["rows"] == c["nb"] * c["f"] for c in main)
    want = [([] if n == 1 else FULL) if k == "full" else OPS[k] for k in kinds]
    assert [p for _, p in _per_step()] == want, _per_step()


# ---- 1. refusals, before either UNet is called
@pytest.mark.parametrize("kw,msg", [
    (dict(guidance_interval=(0.5, 0.25)), r"guidance_interval must be two finite numbers \(lo, hi\) with 0 <= lo <= hi <= 1, got \(0.5, 0.25\)"),
    (dict(guidance_interval=(-0.1, 1.0)), "guidance_interval must be two finite numbers"),
    (dict(guidance_interval=(0.0, 1.5)), "guidance_interval must be two finite numbers"),
    (dict(guidance_interval=(0.0, float("nan"))), "guidance_interval must be two finite numbers"),
    (dict(guidance_interval=(float("-inf"), 1.0)), "guidance_interval must be two finite numbers"),
    (dict(guidance_interval=0.5), "guidance_interval must be two finite numbers"),
    (dict(guidance_interval=(0.0, 0.5, 1.0)), "guidance_interval must be two finite numbers"),
    (dict(guidance_interval=("a", "b")), "guidance_interval must be two finite numbers"),
    (dict(guidance_interval=None), "guidance_interval must be two finite numbers"),
    (dict(uncond_cache_interval=0), "uncond_cache_interval must be an integer >= 1, got 0"),
    (dict(uncond_cache_interval=-2), "uncond_cache_interval must be an integer >= 1, got -2"),
    (dict(uncond_cache_interval=2.0), "uncond_cache_interval must be an integer >= 1, got 2.0"),
    (dict(uncond_cache_interval=True), "uncond_cache_interval must be an integer >= 1, got True"),
    (dict(uncond_cache_interval="2"), "uncond_cache_interval must be an integer >= 1, got '2'"),
    (dict(uncond_cache_interval=None), "uncond_cache_interval must be an integer >= 1, got None"),
    (dict(uncond_cache_interval=2, deep_cache_interval=2), "guidance_interval / uncond_cache_interval cannot be combined with deep_cache_interval > 1"),
    (dict(guidance_interval=(0.0, 0.5), deep_cache_interval=3), "guidance_interval / uncond_cache_interval cannot be combined with deep_cache_interval > 1"),
])
@pytest.mark.parametrize("g", [G, 1.0])
def test_refusals_come_before_any_unet(kw, msg, g):
    ref, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(*zero_inputs(), 2, g, **kw)                          # checked whether or not guidance is on
    assert ref.calls == den.calls == 0


def test_the_deep_cache_refusal_says_why():
    with pytest.raises(ValueError, match="DeepCache slot is shaped by the batch"):
        M.MikuDanceVideoPipeline.sampling_plan(4, G, False, (2, 16, 16), **PLAN_KW, uncond_cache_interval=2, deep_cache_interval=2)


def test_the_plan_field():
    plan = lambda g, **kw: M.MikuDanceVideoPipeline.sampling_plan(8, g, False, (2, 16, 16), **PLAN_KW, **kw)
    assert plan(G).uncond is None and plan(G, guidance_interval=(0.0, 1.0), uncond_cache_interval=1).uncond is None
    assert plan(G, guidance_interval=(0, 1)).uncond is None
    assert plan(G, uncond_cache_interval=3).uncond == (0.0, 1.0, 3)
    assert plan(G, guidance_interval=(0.25, 0.75)).uncond == (0.25, 0.75, 1)
    assert plan(1.0, guidance_interval=(0.25, 0.75), uncond_cache_interval=2).uncond is None      # inert without guidance
    assert plan(G, deep_cache_interval=2).uncond is None and plan(G, deep_cache_interval=2).deep == (2, 3)


# ---- 2. the defaults are the parent's loop
def test_defaults_are_the_same_call_log_and_the_same_bits(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)                                         # the parent's emulations only: a cfg_uncond_cache call would raise
    from mikudance_amd import ops
    monkeypatch.setattr(ops, "cfg_uncond_cache", lambda *a, **k: pytest.fail("cfg_uncond_cache called"))
    den = small_cpu[1]
    lat, rl, emb = (t.half() for t in small_inputs(2, 41))
    spy = _Spy(den, monkeypatch)
    pipe = _pipe(small_cpu)
    empties = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (empties.append((a, k.get("dtype"))), real_empty(*a, **k))[1])
    a = pipe.denoise(lat, rl, emb, 3, G)
    calls_a, empties_a, kws_a = list(fake_ops.CALLS), list(empties), [c["kw"] for c in spy.calls]
    for kw in (dict(guidance_interval=(0.0, 1.0)), dict(uncond_cache_interval=1), dict(guidance_interval=[0, 1], uncond_cache_interval=1)):
        del fake_ops.CALLS[:], empties[:], spy.calls[:]
        b = pipe.denoise(lat, rl, emb, 3, G, **kw)
        assert torch.equal(a, b) and calls_a == fake_ops.CALLS            # the same operator calls, one for one
        assert empties == empties_a                                       # no extra buffer
        assert [c["kw"] for c in spy.calls] == kws_a and all(k == ["halves_identical", "two_queues"] for k in kws_a)
    # without guidance the keywords are inert: the guidance_scale = 1 loop, call for call
    del fake_ops.CALLS[:]
    c = pipe.denoise(lat, rl, emb[1:], 3, 1.0)
    calls_c = list(fake_ops.CALLS)
    del fake_ops.CALLS[:]
    d = pipe.denoise(lat, rl, emb[1:], 3, 1.0, guidance_interval=(0.0, 0.5), uncond_cache_interval=2)
    assert torch.equal(c, d) and calls_c == fake_ops.CALLS


# ---- 3. the schedule of step kinds
def test_interval_2_of_6_steps(monkeypatch, small_cpu):
    UR.install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 42))
    spy = _Spy(small_cpu[1], monkeypatch)
    pipe = _pipe(small_cpu)
    out = pipe.denoise(lat, rl, emb, 6, G, uncond_cache_interval=2)
    assert torch.isfinite(out).all()
    _check(spy, ["full", "cached"] * 3, 2)
    assert [c["nb"] for c in spy.main()] == [2, 1, 2, 1, 2, 1]
    assert [[m for m, _, _ in p] for _, p in _per_step()] == [[0], [1], [0], [1], [0], [1]]
    assert all(c["kw"] == (["conditional"] if c["cond"] else ["halves_identical", "two_queues"]) for c in spy.calls)
    del fake_ops.CALLS[:]
    assert not torch.equal(out, pipe.denoise(lat, rl, emb, 6, G))         # the keyword is not silently ignored


def test_interval_3_inside_a_guidance_interval_of_8_steps(monkeypatch, small_cpu):
    UR.install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 43))
    spy = _Spy(small_cpu[1], monkeypatch)
    out = _pipe(small_cpu).denoise(lat, rl, emb, 8, G, uncond_cache_interval=3, guidance_interval=(0.25, 0.75))
    assert torch.isfinite(out).all()
    kinds = ["off", "off", "full", "cached", "cached", "full", "off", "off"]
    _check(spy, kinds, 3)
    assert UR.step_kinds(8, range(8), 0.25, 0.75, 3) == kinds


def test_interval_alone_makes_no_store_and_allocates_no_delta(monkeypatch, small_cpu):
    UR.install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 44))
    spy = _Spy(small_cpu[1], monkeypatch)
    _pipe(small_cpu).denoise(lat, rl, emb, 4, G, guidance_interval=(0.0, 0.5))
    _check(spy, ["full", "full", "off", "off"], 1)
    assert all("delta" not in d["keywords"] for _, d in UR.calls())


def test_free_init_starts_every_pass_with_an_empty_cache(monkeypatch, small_cpu):
    UR.install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 45))
    spy = _Spy(small_cpu[1], monkeypatch)
    _pipe(small_cpu).denoise(lat, rl, emb, 3, G, uncond_cache_interval=2, free_init_iters=2, generator=torch.Generator().manual_seed(1))
    _check(spy, ["full", "cached", "full"] * 2, 2)                        # step 0 of pass 2 is full, not the cached step the count would give


def test_video_to_video_counts_schedule_indices(monkeypatch, small_cpu):
    """strength 0.5 of 6 steps keeps k = 3, 4, 5.  (0, 0.75): k < 4.5, so 3 and 4 are guided and 5 is off; counted from 0 it would be full, cached, full."""
    UR.install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 46))
    spy = _Spy(small_cpu[1], monkeypatch)
    _pipe(small_cpu).denoise(lat, rl, emb, 6, G, uncond_cache_interval=2, guidance_interval=(0.0, 0.75), init_latents=lat * 0.5, strength=0.5)
    _check(spy, ["full", "cached", "off"], 2)
    assert UR.step_kinds(6, range(3, 6), 0.0, 0.75, 2) == ["full", "cached", "off"]


def test_the_perturbed_plane_is_evaluated_on_every_kind_of_step(monkeypatch, small_cpu):
    UR.install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 47))
    spy = _Spy(small_cpu[1], monkeypatch)
    _pipe(small_cpu).denoise(lat, rl, emb, 4, G, uncond_cache_interval=2, guidance_interval=(0.0, 0.75), pag_scale=1.0, pag_applied_layers=("mid",))
    _check(spy, ["full", "cached", "full", "off"], 2)
    assert [c["pert"] for c in spy.calls] == [False, True] * 4            # one perturbed call behind every main call
    assert [n for n, _ in _per_step()] == ["cfg_ddim_step_pag"] * 4


# ---- 4. window parallelism
WP = dict(context_frames=8, context_stride=1, context_overlap=2)           # 16 frames: 3 windows, the last one wraps


def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    import uncond_cache_ref
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    uncond_cache_ref.install_process()
    reduces = []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (reduces.append(1), real(*a, **k))[1]
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=523))
    kw = dict(WP, uncond_cache_interval=2, guidance_interval=(0.0, 0.75))      # 3 steps: full, cached, off
    pipe = MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    plain = pipe.denoise(lat, rl, emb, 3, G, window_parallel=dp.WindowParallel(), **WP)
    n_plain = len(reduces)
    out = pipe.denoise(lat, rl, emb, 3, G, window_parallel=dp.WindowParallel(), **kw)
    n_kw = len(reduces) - n_plain
    dist.all_reduce = real
    got = dp.gather_latents(out)
    counts = dp.gather_objects((n_plain, n_kw))
    if rank == 0:
        one = pipe.denoise(lat, rl, emb, 3, G, **kw)
        q.put(dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                   finite=bool(torch.isfinite(out).all()), differs_from_plain=not torch.equal(out, plain),
                   collectives_per_step_unchanged=all(a == b and a > 0 and a % 3 == 0 for a, b in counts)))
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank_with_no_new_collective():
    res = run_world(3, _wp_worker)
    assert all(res.values()), res


# ---- 5. the emulated loop against the restated one
@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_the_emulated_loop_equals_the_restated_loop(monkeypatch, small_cpu, sampler):
    import dpmpp_ref
    from oracle import cpu_ref as O
    UR.install(monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(2, 48))
    sch = M.DPMSolverMultistepScheduler(**SCHED_KWARGS) if sampler == "2m" else _ddim()
    pipe = _pipe(small_cpu, sch)
    kw = dict(uncond_cache_interval=2, guidance_interval=(0.0, 0.75))
    got = pipe.denoise(lat, rl, emb, 4, G, **kw).float()
    seen = []
    want = UR.denoise_loop(pipe, lat, rl, emb, 4, G, dpmpp_ref.Restated() if sampler == "2m" else O.DDIM(), interval=kw["guidance_interval"], n=2,
                           on_step=lambda k, kind: seen.append(kind))
    assert seen == ["full", "cached", "full", "off"]
    r, c = rel_l2(got, want), cosine(got, want)
    print(f"\nUNCOND_CACHE_HOST {sampler} 4 steps n 2 (0, 0.75): rel_l2 {r:.3e} 1 - cos {1 - c:.3e}")
    assert torch.isfinite(got).all() and r <= 2.0 ** -10 and c >= 1 - 2.0 ** -20, (r, c)
    plain = pipe.denoise(lat, rl, emb, 4, G).float()
    assert rel_l2(plain, want) > 4 * r                                    # and the restatement is not simply the plain loop


# ---- 6. the operator's emulation against float64, the script's flags
def test_emulated_operator_against_float64():
    g = torch.Generator().manual_seed(5)
    ns = torch.randn(2, 3, 5, 4, generator=g)
    cnt = torch.tensor([1.0, 2.0, 3.0])
    delta = torch.empty(3, 5, 4)
    keep = ns.clone()
    UR.cfg_uncond_cache(ns, cnt, delta, 3, 5, 0)
    assert torch.equal(ns, keep)
    assert torch.allclose(delta.double(), UR.store64(ns, cnt), rtol=0, atol=4 * 2.0 ** -24 * float(ns.abs().max()) * 2)
    UR.cfg_uncond_cache(ns, cnt, delta, 3, 5, 1, scale=1.0)
    assert torch.equal(ns[1], keep[1]) and torch.allclose(ns[0], keep[0], rtol=0, atol=1e-5)
    UR.cfg_uncond_cache(ns, cnt, None, 3, 5, 1, scale=0.0)
    assert torch.equal(ns[0], ns[1])


def test_script_flags():
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.guidance_interval, a.uncond_cache_interval) == ((0.0, 1.0), 1)
    a = IV.parse_args(["--guidance_interval", "0.1,0.8", "--uncond_cache_interval", "3"])
    assert (a.guidance_interval, a.uncond_cache_interval) == ((0.1, 0.8), 3)
    for bad in (["--guidance_interval", "0.5"], ["--guidance_interval", "a,b"], ["--uncond_cache_interval", "two"]):
        with pytest.raises(SystemExit):
            IV.parse_args(bad)
    assert "guidance_interval=--guidance_interval, uncond_cache_interval=--uncond_cache_interval" in IV.__doc__
