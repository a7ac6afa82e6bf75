"""CPU: perturbed-attention guidance (pag_scale=, arXiv 2403.17377) -- the argument checks of both entry points, the layer-name matching against
a real block list, the s_t schedule, the host graph of the perturbed evaluation on emulated operators against tests/pag_ref.py (values and call
log), the whole loop of MikuDanceVideoPipeline.denoise() against the restated loop (one rank and three gloo ranks), and the script's flags."""
import collections
import math
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist

import mikudance_amd as M
from mikudance_amd import ReferenceAttentionControl
from mikudance_amd.selftest import SCHED_KWARGS
from oracle import cpu_ref as O

import dpmpp_ref as R
import fake_ops
import fusion_ref as FR
import pag_ref as P
from loop_helpers import (CountingUNet, cosine, fake_pipeline_builder, rel_l2, run_world, script_tree, small_cpu, small_inputs,  # noqa: F401
                          worker_setup, zero_inputs)

WRAP12 = dict(context_frames=8, context_stride=1, context_overlap=4)      # f = 12: three windows, the last two wrap
DEFAULTS = dict(pag_scale=0.0, pag_adaptive_scale=0.0, pag_applied_layers=("mid",))
BOUND = dict(rel=2e-2, cos=0.999)                                          # tests/test_host_graph_cpu.py, forward and loop alike


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


def _names():
    return [n for n, _ in P.step_calls()]


def _inputs8(frames, seed):
    """small_inputs cut down to an 8 x 8 latent."""
    lat, rl, emb = small_inputs(frames, seed)
    return lat[..., :8, :8].contiguous(), rl[..., :8, :8].contiguous(), emb


# ---- 1. argument checks, both entry points
nan, inf = float("nan"), float("inf")
BAD = [(dict(pag_scale=-0.1), "pag_scale"), (dict(pag_scale=nan), "pag_scale"), (dict(pag_scale=inf), "pag_scale"),
       (dict(pag_adaptive_scale=-1e-3), "pag_adaptive_scale"), (dict(pag_adaptive_scale=nan), "pag_adaptive_scale"),
       (dict(pag_adaptive_scale=inf), "pag_adaptive_scale"), (dict(pag_scale=3.0, pag_adaptive_scale=-inf), "pag_adaptive_scale"),
       (dict(pag_scale=3.0, guidance_rescale=0.7), "cannot be combined with guidance_rescale"),
       (dict(pag_scale=3.0, apg=True), "cannot be combined with apg"),
       (dict(pag_scale=3.0, pag_applied_layers=("middle",)), "unknown layer name"),
       (dict(pag_applied_layers=("down_blocks.x",)), "unknown layer name"),
       (dict(pag_scale=3.0, pag_applied_layers=("mid", "up_blocks.1.attn1")), "unknown layer name"),
       (dict(pag_scale=3.0, pag_applied_layers=()), "pag_applied_layers is empty")]


@pytest.mark.parametrize("kw,msg", BAD)
@pytest.mark.parametrize("make", [_ddim, _dpm], ids=["ddim", "dpm"])
def test_bad_arguments_raise_before_any_unet(monkeypatch, kw, msg, make):
    fake_ops.install(monkeypatch)
    refu, den = CountingUNet(), CountingUNet()
    pipe = M.MikuDanceVideoPipeline(None, None, refu, den, make())
    with pytest.raises(ValueError, match=msg):
        pipe.denoise(*zero_inputs(), 4, 3.5, **kw)
    assert refu.calls == 0 and den.calls == 0 and fake_ops.CALLS == []


def test_a_name_that_selects_no_block_raises_before_anything_runs(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    lat, rl, emb = (t.half() for t in small_inputs(2, 3))
    for name in ("down_blocks.3", "up_blocks.0", "down_blocks.0.attentions.2", "up_blocks.7"):
        with pytest.raises(ValueError, match="selects no attention block"):
            pipe.denoise(lat, rl, emb, 2, 3.5, pag_scale=3.0, pag_applied_layers=("mid", name))
        assert fake_ops.CALLS == []
    pipe.denoise(lat, rl, emb, 1, 3.5, pag_scale=0.0, pag_applied_layers=("up_blocks.7",))      # off: the names select nothing, nothing asks


def test_call_refuses_before_clip_and_vae_and_forwards_the_keywords(monkeypatch):
    from PIL import Image
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append({k: v for k, v in kw.items() if k.startswith("pag")})
        return latents

    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    custom = dict(pag_scale=3.0, pag_adaptive_scale=0.002, pag_applied_layers=("mid", "up_blocks.1"))
    for cls in (M.MikuDanceVideoPipeline, M.Pose2VideoPipeline):
        del seen[:]
        clip = fake_ops.FakeCLIP()
        calls = []
        clip.register_forward_hook(lambda *a: calls.append(1))
        asked = []
        stub = types.SimpleNamespace(in_channels=4, pag_blocks=lambda names: asked.append(tuple(names)))
        pipe = cls(vae=fake_ops.FakeVAE(), image_encoder=clip, reference_unet=None, denoising_unet=stub, scheduler=_ddim())
        args = (img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, 4, 4), dtype=np.float32), 32, 32, 2, 2, 3.5)
        for kw, msg in BAD:
            with pytest.raises(ValueError, match=msg):
                pipe(*args, generator=torch.Generator().manual_seed(0), **kw)
        assert not calls and not seen
        pipe(*args, generator=torch.Generator().manual_seed(0))
        pipe(*args, generator=torch.Generator().manual_seed(0), **custom)
        assert seen == [DEFAULTS, custom]
        assert asked == [custom["pag_applied_layers"]]                     # the UNet is asked once, for the call with PAG on, before CLIP runs


def test_call_checks_the_names_against_the_unet_before_clip(small_cpu):
    from PIL import Image
    _, den, _, _ = small_cpu
    clip = fake_ops.FakeCLIP()
    calls = []
    clip.register_forward_hook(lambda *a: calls.append(1))
    pipe = M.MikuDanceVideoPipeline(vae=fake_ops.FakeVAE(), image_encoder=clip, reference_unet=None, denoising_unet=den, scheduler=_ddim())
    img = Image.new("RGB", (32, 32), (40, 80, 120))
    with pytest.raises(ValueError, match="selects no attention block"):
        pipe(img, img, [img, img], [img, img], [img, img], np.zeros((2, 2, 4, 4), dtype=np.float32), 32, 32, 2, 2, 3.5, pag_scale=3.0,
             pag_applied_layers=("down_blocks.3",))
    assert not calls


# ---- 2. layer matching against the real block list of a small UNet
def test_layer_names_select_the_documented_blocks(small_cpu):
    _, den, _, den_sd = small_cpu
    table = den.attention_block_prefixes()
    prefixes = [p for p, _ in table]
    assert sorted(prefixes) == sorted(P.block_prefixes(den_sd)) and len(prefixes) == 16
    assert [b for _, b in table] and all(isinstance(b, M.blocks.TransformerBlock) for _, b in table)
    of = {id(b): p for p, b in table}
    picked = lambda names: [of[id(b)] for b in den.pag_blocks(names)]
    assert picked(("mid",)) == picked(("mid_block",)) == picked("mid") == ["mid_block.attentions.0"]
    assert picked(("up_blocks.1",)) == [f"up_blocks.1.attentions.{j}" for j in range(3)]
    assert picked(("down_blocks.0.attentions.1",)) == ["down_blocks.0.attentions.1"]
    assert picked(("down_blocks.1", "down_blocks.1.attentions.0", "mid")) == ["down_blocks.1.attentions.0", "down_blocks.1.attentions.1",
                                                                             "mid_block.attentions.0"]
    for names in (("mid",), ("up_blocks.1",), ("down_blocks.0.attentions.1",), ("down_blocks.1", "up_blocks.2.attentions.0")):
        assert sorted(picked(names)) == sorted(P.select(prefixes, names))
    # "down_blocks.1" is no prefix of "down_blocks.10": the match is on whole key components
    assert P.select(["down_blocks.1.attentions.0", "down_blocks.10.attentions.0"], ["down_blocks.1"]) == ["down_blocks.1.attentions.0"]
    for bad in ((), ("up_blocks.0",), ("down_blocks.3",)):
        with pytest.raises(ValueError):
            den.pag_blocks(bad)
        with pytest.raises(ValueError):
            P.select(prefixes, bad)


# ---- 3. the s_t schedule, and when the perturbed evaluation runs
class _Spy:
    """Counts the calls of den.forward_nhwc, main and perturbed, per timestep."""

    def __init__(self, den, monkeypatch):
        self.main, self.pert = collections.Counter(), collections.Counter()
        real = den.forward_nhwc

        def fwd(x, nb, f, timesteps, cross, **kw):
            (self.main if kw.get("pag") is None else self.pert)[int(timesteps[0])] += 1
            return real(x, nb, f, timesteps, cross, **kw)

        monkeypatch.setattr(den, "forward_nhwc", fwd, raising=False)


def test_schedule_matches_the_restatement_and_skips_the_evaluation_at_zero(monkeypatch, small_cpu):
    sch = _ddim()
    sch.set_timesteps(20)
    ts = [int(t) for t in sch.timesteps]
    assert ts == [int(t) for t in O.DDIM().set_timesteps(20)] and ts[0] == 999 and len(ts) == 20
    adaptive = 3.0 / (1000 - ts[8])                                        # reaches 0 exactly at the ninth step
    want = [P.pag_scale_at(3.0, adaptive, t) for t in ts]
    assert want[0] == pytest.approx(3.0 - adaptive) and all(w > 0 for w in want[:8]) and all(w == 0.0 for w in want[8:])
    got = [M.MikuDanceVideoPipeline._pag_scale_at(3.0, adaptive, t) for t in ts]
    assert got == want and [M.MikuDanceVideoPipeline._pag_scale_at(3.0, 0.0, t) for t in ts] == [3.0] * 20
    # the loop: 20 steps on a 2-frame 8 x 8 clip, the perturbed evaluation runs at the first eight timesteps only
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    spy = _Spy(den, monkeypatch)
    lat, rl, emb = (t.half() for t in _inputs8(2, 31))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, sch)
    pipe.denoise(lat, rl, emb, 20, 3.5, pag_scale=3.0, pag_adaptive_scale=adaptive)
    assert spy.main == collections.Counter(ts) and spy.pert == collections.Counter(ts[:8])
    steps = P.step_calls()
    assert [n for n, _ in steps] == ["cfg_ddim_step_pag"] * 8 + ["cfg_ddim_step"] * 12
    assert [d["pag_scale"] for n, d in steps[:8]] == want[:8]
    assert all(d["halves"] == 2 for _, d in steps)


def test_scale_zero_never_runs_the_perturbed_evaluation_and_keeps_the_bits(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    spy = _Spy(den, monkeypatch)
    lat, rl, emb = (t.half() for t in small_inputs(4, 19))
    for make, step in ((_ddim, "cfg_ddim_step"), (_dpm, "cfg_multistep_step")):
        pipe = M.MikuDanceVideoPipeline(None, None, ref, den, make())
        del fake_ops.CALLS[:]
        a = pipe.denoise(lat, rl, emb, 2, 3.5)
        calls_a = list(fake_ops.CALLS)
        del fake_ops.CALLS[:]
        b = pipe.denoise(lat, rl, emb, 2, 3.5, pag_scale=0.0, pag_adaptive_scale=0.5, pag_applied_layers=("up_blocks.1",))
        assert torch.equal(a, b) and calls_a == fake_ops.CALLS and _names() == [step] * 2      # the same operator calls, one for one
        assert not spy.pert
        del fake_ops.CALLS[:]
        c = pipe.denoise(lat, rl, emb, 2, 3.5, pag_scale=3.0, pag_applied_layers=("up_blocks.1",))
        assert not torch.equal(a, c) and _names() == [step + "_pag"] * 2 and sum(spy.pert.values()) == 2
        spy.pert.clear()


# ---- 4. the host graph of the perturbed evaluation
def _attention_logged(monkeypatch):
    """fake_ops.attention does not log itself: record (B, Lq, Lk) of every launch in the same call list."""
    from mikudance_amd import ops
    real = ops.attention

    def attention(q, k, vt, B, H, D, Lq, Lk, **kw):
        fake_ops.CALLS.append(("attention", (B, Lq, Lk)))
        return real(q, k, vt, B, H, D, Lq, Lk, **kw)

    monkeypatch.setattr(ops, "attention", attention)


def _launches():
    return collections.Counter((n, d) for n, d in fake_ops.CALLS if n in ("gemm", "attention", "gemm_ln", "conv", "groupnorm"))


@pytest.fixture
def read_state(request, monkeypatch, small_cpu):
    """The denoising UNet in read mode with the banks of one 2-frame window, as denoise() sets it up under CFG.  8 x 8 unless the test asks
    for another size (indirect parameter)."""
    fake_ops.install(monkeypatch)
    _attention_logged(monkeypatch)
    ref, den, ref_sd, den_sd = small_cpu
    f, t = 2, 601
    h = w = getattr(request, "param", 8)
    lat, rl, emb = _inputs8(f, 41) if h == 8 else small_inputs(f, 41)
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    writer = ReferenceAttentionControl(ref, do_classifier_free_guidance=True, mode="write", batch_size=1, fusion_blocks="full")
    reader = ReferenceAttentionControl(den, do_classifier_free_guidance=True, mode="read", batch_size=1, fusion_blocks="full")
    ref.skip_dead_tail = True
    pipe._write_banks(writer, reader, emb.half(), rl.half(), torch.arange(f), f, True, literal=False)
    st = lat.half().stride()
    packed = fake_ops.pack_nhwc(lat.half(), f, f, (0, st[2], st[1], st[3], st[4]), 0, 4, 4, h, w)
    x = fake_ops.pack_nhwc(packed, 2 * f, f, (0, h * w * 4, 1, w * 4, 4), 0, 4, 64, h, w)
    cross = den._cross(emb.half(), [i // f for i in range(2 * f)], torch.device("cpu"))
    # the oracle side reads the SAME banks (the writer's, fp16): its own reference UNet cannot run on an 8 x 8 latent, which reaches 1 x 1 at
    # the last level where torch's instance_norm refuses a single spatial element; the writer is tests/test_host_graph_cpu.py's subject
    banks = {p + ".transformer_blocks.0.": blk.bank[0].float().reshape(f, -1, blk.dim) for p, blk in den.attention_block_prefixes()}
    st_ = types.SimpleNamespace(den=den, den_sd=den_sd, f=f, h=h, w=w, t=t, lat=lat, emb=emb, x=x, cross=cross, banks=banks)
    try:
        yield st_
    finally:
        ref.skip_dead_tail = False
        reader.clear(); writer.clear()
        den.clear_context_cache(); ref.clear_context_cache()


def _main(s):
    return s.den.forward_nhwc(s.x, 2, s.f, torch.full((2,), float(s.t)), s.cross, halves_identical=True)


def _perturbed(s, names):
    return s.den.forward_nhwc(s.x[s.f:], 1, s.f, torch.full((1,), float(s.t)), s.cross.rows(s.f, 2 * s.f), pag=s.den.pag_blocks(names) if names else ())


@pytest.mark.parametrize("read_state,names", [(8, ("mid",)), (8, ("down_blocks.1", "up_blocks.2.attentions.0")), (16, ("mid",))],
                         ids=["8x8-mid", "8x8-down1-up2.0", "16x16-mid"], indirect=["read_state"])
def test_perturbed_forward_matches_the_perturbed_oracle(read_state, names):
    s = read_state
    got = _perturbed(s, names).float().view(s.f, s.h, s.w, 4).permute(3, 0, 1, 2)[None]
    with torch.no_grad():
        want = P.perturbed_forward(s.den_sd, s.lat, torch.tensor(s.t), s.emb[1:2], s.banks, names)
        plain = O.denoising_unet_forward(s.den_sd, s.lat, torch.tensor(s.t), s.emb[1:2], s.banks, cfg=False)
    r, c, d = rel_l2(got, want), cosine(got, want), rel_l2(plain, want)
    print(f"\nPAG_HOST_FORWARD {names} rel_l2 {r:.3e} cos {c:.7f} (unperturbed conditional oracle vs perturbed: {d:.3e})")
    assert r < BOUND["rel"] and c > BOUND["cos"], (r, c)
    # 8 x 8: the mid block sees ONE token per frame, and softmax over one key is the identity already; 16 x 16 gives it 2 x 2 tokens and the
    # perturbation shows.  d is a figure of the two oracles alone; it has to exceed the parity bound, for then a forward that ignored the
    # selection (and so matched the unperturbed oracle) cannot pass the assertion above
    if names == ("mid",):
        assert d == 0.0 if s.h == 8 else d > BOUND["rel"], d
    else:
        assert d > 0.1, d


def test_call_log_of_the_perturbed_evaluation(read_state):
    s = read_state
    _main(s)                                                               # first call: projects the context K / V of every block
    del fake_ops.CALLS[:]
    m1 = _main(s)
    main_log = list(fake_ops.CALLS)
    del fake_ops.CALLS[:]
    p_none = _perturbed(s, ())                                             # no block selected: the conditional-only read everywhere
    none_log = _launches()
    # ... which is the conditional half of the main call, to fp16 rounding (torch's CPU matmul sums in an order that depends on the row count)
    assert rel_l2(p_none.view(s.f, -1).float(), m1.view(2, s.f, -1)[1].float()) < 5e-3
    table = dict(s.den.attention_block_prefixes())
    for names in (("mid",), ("down_blocks.1", "up_blocks.2.attentions.0")):
        del fake_ops.CALLS[:]
        _perturbed(s, names)
        sel_log = _launches()
        gone = collections.Counter()
        for p in P.select(list(table), names):
            C = table[p].dim
            lvl = int(p.split(".")[1]) if p.startswith("down") else (3 - int(p.split(".")[1]) if p.startswith("up") else 3)
            L = (s.h >> lvl) * (s.w >> lvl)
            Mrows = s.f * L
            # per selected block: q, k (row-major C x C) and V^T go, one attention launch goes, the row-major V comes
            gone[("gemm", (Mrows, C, C, 0, False, None))] += 2 - 1
            gone[("gemm", (Mrows, C, C, 0, True, None))] += 1
            gone[("attention", (s.f, L, L))] += 1
        assert none_log - sel_log == gone, (names, none_log - sel_log, gone)
        assert not (sel_log - none_log), sel_log - none_log
    # the main evaluation is untouched by the perturbed ones: the same launches, the same bits, no context K / V projected again
    del fake_ops.CALLS[:]
    m2 = _main(s)
    assert list(fake_ops.CALLS) == main_log and torch.equal(m1, m2)


def test_perturbed_evaluation_is_refused_inside_other_evaluations(read_state):
    s = read_state
    sel = s.den.pag_blocks(("mid",))
    for kw in (dict(two_queues=True), dict(halves_identical=True)):
        with pytest.raises(ValueError, match="perturbed evaluation"):
            s.den.forward_nhwc(s.x[s.f:], 1, s.f, torch.full((1,), 601.0), s.cross.rows(s.f, 2 * s.f), pag=sel, **kw)
    with pytest.raises(ValueError, match="perturbed evaluation"):
        s.den.forward_nhwc(s.x, 2, s.f, torch.full((2,), 601.0), s.cross, pag=sel)


# ---- 5. the whole loop on the emulated operators, against the restated loop
LAYERS = ("mid", "up_blocks.1")
LOOPS = {"ddim-1win": dict(frames=4, steps=3, guidance=3.5), "wrap-flat": dict(frames=12, steps=2, guidance=3.5, win=WRAP12),
         "wrap-pyramid": dict(frames=12, steps=2, guidance=3.5, win=WRAP12, fuse="pyramid"), "no-cfg": dict(frames=4, steps=3, guidance=1.0),
         "no-cfg-wrap-flat": dict(frames=12, steps=2, guidance=1.0, win=WRAP12), "2m": dict(frames=4, steps=3, guidance=3.5, sampler="2m")}


@pytest.mark.parametrize("case", list(LOOPS))
def test_host_loop_matches_restatement(monkeypatch, small_cpu, case):
    fake_ops.install(monkeypatch)
    cfg = LOOPS[case]
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(cfg["frames"], 70 + cfg["frames"])
    g, steps, win, fuse = cfg["guidance"], cfg["steps"], cfg.get("win", {}), cfg.get("fuse", "flat")
    if g <= 1.0:
        emb = emb[1:]
    two_m = cfg.get("sampler") == "2m"
    mk_rs = lambda: R.Restated(2, "dpmsolver++", "midpoint") if two_m else None
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _dpm() if two_m else _ddim())
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), steps, g, context_fuse=fuse, pag_scale=3.0, pag_applied_layers=LAYERS, **win)
    nb = 2 if g > 1.0 else 1
    step = "cfg_multistep_step_pag" if two_m else "cfg_ddim_step_pag"
    assert _names() == [step] * steps and all(d["halves"] == nb and d["pag_scale"] == 3.0 for _, d in P.step_calls())
    acc = [d["halves"] for n, d in fake_ops.tail_calls("window_accumulate", "window_accumulate_weighted")]
    n_win = len(FR.make_windows("uniform", cfg["frames"], **(win or dict(context_frames=30, context_stride=1, context_overlap=8))))
    assert acc == [nb, 1] * (steps * n_win) and n_win == (3 if win else 1)                     # main planes, then the perturbed plane
    with torch.no_grad():
        kw = dict(guidance_scale=g, fuse=fuse, pag_layers=LAYERS, **win)
        want = P.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, scheduler=mk_rs(), pag_scale=3.0, **kw)
        plain = P.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, scheduler=mk_rs(), pag_scale=0.0, **kw)
    e, c, d = rel_l2(out.float(), want), cosine(out.float(), want), rel_l2(plain, want)
    print(f"\nPAG_HOST_LOOP {case} rel_l2 {e:.3e} cos {c:.7f} (pag_scale 0 vs 3 restated: {d:.3e})")
    assert torch.isfinite(out).all() and e < BOUND["rel"] and c > BOUND["cos"], (e, c)
    assert d > 5 * BOUND["rel"], d                                         # PAG moves the result by far more than the bound ...
    assert rel_l2(out.float(), plain) > 5 * BOUND["rel"]                   # ... so a loop that ignored the keywords fails here


def test_restated_loop_with_scale_zero_is_the_oracle_loop(small_cpu):
    _, _, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(12, 82)
    with torch.no_grad():
        want = O.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, reduced=True, **WRAP12)
        got = P.denoise_loop(ref_sd, den_sd, lat, rl, emb, 2, guidance_scale=3.5, pag_scale=0.0, **WRAP12)
    assert torch.equal(got, want)


def test_combination_rule_limits():
    g = torch.Generator().manual_seed(0)
    u, c, p = (torch.randn(3, 5, 4, generator=g, dtype=torch.float64) for _ in range(3))
    assert torch.equal(P.combine(u, c, p, 3.5, 0.0), u + 3.5 * (c - u)) and torch.equal(P.combine_sum(c, p, 0.0), c)
    assert torch.allclose(P.combine(u, c, p, 1.0, 2.0), P.combine_sum(c, p, 2.0), rtol=1e-14, atol=1e-14)     # g = 1: the no-CFG rule on means
    assert torch.equal(P.combine(u, c, c, 3.5, 3.0), u + 3.5 * (c - u))                                       # p == c: nothing to steer away from


def test_eta_and_sde_draws_reach_the_pag_steps(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 22))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    pipe.denoise(lat, rl, emb, 2, 3.5, pag_scale=3.0, eta=0.5, generator=torch.Generator().manual_seed(1))
    assert [(n, d["keywords"]) for n, d in P.step_calls()] == [("cfg_ddim_step_pag", ("variance_noise",))] * 2
    del fake_ops.CALLS[:]
    sde = M.DPMSolverMultistepScheduler(**SCHED_KWARGS, algorithm_type="sde-dpmsolver++")
    M.MikuDanceVideoPipeline(None, None, ref, den, sde).denoise(lat, rl, emb, 2, 3.5, pag_scale=3.0, generator=torch.Generator().manual_seed(1))
    assert [(n, d["keywords"]) for n, d in P.step_calls()] == [("cfg_multistep_step_pag", ("variance_noise",))] * 2


def test_every_free_init_pass_is_guided(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 23))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    pipe.denoise(lat, rl, emb, 2, 3.5, pag_scale=3.0, free_init_iters=2, generator=torch.Generator().manual_seed(2))
    names = [n for n, _ in fake_ops.CALLS if n.startswith("cfg_") or n == "free_init_mix"]
    assert names == ["cfg_ddim_step_pag"] * 2 + ["free_init_mix"] + ["cfg_ddim_step_pag"] * 2


def test_literal_reference_pass_reads_the_conditional_part_of_the_bank(monkeypatch, small_cpu):
    """reference_reuse off: the banks hold 2f frames and the perturbed rows read the conditional part.  The literal writer runs 2f frames
    through torch's CPU matmul, whose summation order depends on the row count, so the banks (and the result) agree to fp16 rounding, not bitwise:
    the host-graph bound.  Reading the unconditional part instead (banks of the zero context) is far outside it."""
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(2, 24))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    a = pipe.denoise(lat, rl, emb, 2, 3.5, pag_scale=3.0)
    pipe.reference_reuse = False
    b = pipe.denoise(lat, rl, emb, 2, 3.5, pag_scale=3.0)
    assert rel_l2(b.float(), a.float()) < 2e-2 and not torch.equal(a, pipe.denoise(lat, rl, emb, 2, 3.5))


# ---- 6. window parallelism: three gloo ranks
def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=521))
    # 3 windows, the last one wraps
    kw = dict(context_frames=8, context_stride=1, context_overlap=2, pag_scale=3.0, pag_applied_layers=("mid", "up_blocks.1"))
    res = {}
    for name, sch, extra in (("ddim", M.DDIMScheduler(**SCHED_KWARGS), {}), ("2m-pyramid", M.DPMSolverMultistepScheduler(**SCHED_KWARGS),
                                                                               dict(context_fuse="pyramid"))):
        pipe = MikuDanceVideoPipeline(None, None, ref, den, sch)
        out = pipe.denoise(lat, rl, emb, 2, 3.5, window_parallel=dp.WindowParallel(), **kw, **extra)
        got = dp.gather_latents(out)
        if rank == 0:
            one = pipe.denoise(lat, rl, emb, 2, 3.5, **kw, **extra)
            plain = pipe.denoise(lat, rl, emb, 2, 3.5, **dict(kw, pag_scale=0.0), **extra)
            res[name] = dict(identical_on_all_ranks=all(torch.equal(g, got[0]) for g in got), equals_one_rank=torch.equal(out, one),
                             finite=bool(torch.isfinite(out).all()), guided=not torch.equal(out, plain))
    if rank == 0:
        q.put(res)
    dist.destroy_process_group()


def test_window_parallel_world3_equals_one_rank():
    res = run_world(3, _wp_worker)
    assert sorted(res) == ["2m-pyramid", "ddim"]
    for name, r in res.items():
        assert all(r.values()), (name, r)


# ---- 7. the script
def test_script_flags_parse():
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.pag_scale, a.pag_adaptive_scale, a.pag_layers) == (0.0, 0.0, "mid")
    a = IV.parse_args(["--pag_scale", "3", "--pag_adaptive_scale", "0.002", "--pag_layers", "mid,up_blocks.1"])
    assert (a.pag_scale, a.pag_adaptive_scale, a.pag_layers) == (3.0, 0.002, "mid,up_blocks.1")
    with pytest.raises(SystemExit):
        IV.parse_args(["--pag_scale", "high"])
    assert "pag_scale=--pag_scale" in IV.__doc__


def test_script_help_marks_the_flags_as_additions(capsys):
    from mikudance_amd import inference_video as IV
    with pytest.raises(SystemExit):
        IV.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for flag in ("--pag_scale PAG_SCALE (addition)", "--pag_adaptive_scale PAG_ADAPTIVE_SCALE (addition)", "--pag_layers PAG_LAYERS (addition)"):
        assert flag in text, flag


def test_script_flags_reach_denoise(monkeypatch, tmp_path):
    from mikudance_amd import inference_video as IV
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append(tuple(kw[k] for k in ("pag_scale", "pag_adaptive_scale", "pag_applied_layers")))
        return latents

    build = fake_pipeline_builder(IV)

    def build_with_block_list(*a, **kw):
        pipe = build(*a, **kw)
        pipe.denoising_unet.pag_blocks = lambda names: ()                  # the stand-in UNet of the builder has no blocks to ask
        return pipe

    monkeypatch.setattr(IV, "build_pipeline", build_with_block_list)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path)
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")]
    IV.main(base)
    IV.main(base + ["--pag_scale", "3", "--pag_layers", "mid"])
    IV.main(base + ["--pag_scale", "2.5", "--pag_adaptive_scale", "0.002", "--pag_layers", "down_blocks.2, up_blocks.1.attentions.0"])
    assert seen == [(0.0, 0.0, ("mid",)), (3.0, 0.0, ("mid",)), (2.5, 0.002, ("down_blocks.2", "up_blocks.1.attentions.0"))]
    assert math.isfinite(seen[1][0])
