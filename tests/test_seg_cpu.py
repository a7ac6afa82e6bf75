"""CPU: smoothed-energy guidance -- the blur's definition on hand-computed grids, the clamp and reflect rules, the operator's emulation against the
definition, every refusal before any UNet call, the default against the plain loop, the host graph and the host loop on the emulated operator
layer against tests/seg_ref.py, three gloo ranks against one, and the script's flags."""
import math

import pytest
import torch
import torch.distributed as dist

import mikudance_amd as M
from mikudance_amd import ops
from mikudance_amd.selftest import SCHED_KWARGS

import dpmpp_ref as R
import fake_ops
import pag_ref as P
import seg_ref as S
from loop_helpers import (CountingUNet, cosine, fake_pipeline_builder, rel_l2, run_world, script_tree, small_cpu, small_inputs,  # noqa: F401
                          worker_setup, zero_inputs)
from test_pag_cpu import _attention_logged, _launches, read_state  # noqa: F401  (the read-mode UNet of one 2-frame window)

INF = math.inf
nan = float("nan")
BOUND = dict(rel=2e-2, cos=0.999)                                          # tests/test_host_graph_cpu.py, forward and loop alike


def _ddim():
    return M.DDIMScheduler(**SCHED_KWARGS)


def _dpm():
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS)


def _names():
    return [n for n, _ in P.step_calls()]


# ---- 1. the definition
def test_hand_computed_grids():
    one = torch.tensor([[3.0] * 8])
    assert torch.equal(S.blur64(one, 1, 1, 1, 1.0), one.double()) and torch.equal(S.blur64(one, 1, 1, 1, INF), one.double())
    # 2 x 2, sigma 100: k = 3, taps ~ 1/3 each; position 0 reads (1, 0, 1), position 1 reads (0, 1, 0) per axis
    g = torch.tensor([1.0, 2.0, 3.0, 4.0]).view(4, 1)
    w = S.taps(100.0, 2)
    a, b = float(w[1]), float(w[0] + w[2])                                 # own weight, the other's weight
    want = [a * a * 1 + a * b * 2 + b * a * 3 + b * b * 4, a * a * 2 + a * b * 1 + b * a * 4 + b * b * 3,
            a * a * 3 + a * b * 4 + b * a * 1 + b * b * 2, a * a * 4 + a * b * 3 + b * a * 2 + b * b * 1]
    assert torch.allclose(S.blur64(g, 1, 2, 2, 100.0).view(-1), torch.tensor(want, dtype=torch.float64), rtol=0, atol=1e-14)
    assert abs(a - 1 / 3) < 1e-4 and torch.equal(S.blur64(g, 1, 2, 2, INF), torch.full((4, 1), 2.5, dtype=torch.float64))
    # 1 x 5 row, sigma 1: k = 5 (clamped from 7), w = e^{-j^2/2} / sum
    e = [math.exp(-0.5 * j * j) for j in (-2, -1, 0, 1, 2)]
    w5 = [v / sum(e) for v in e]
    assert S.kernel_size(1.0, 5) == 5 and torch.allclose(S.taps(1.0, 5), torch.tensor(w5, dtype=torch.float64), rtol=0, atol=1e-15)
    row = [1.0, 10.0, 100.0, 1000.0, 10000.0]
    idx = [[2, 1, 0, 1, 2], [1, 0, 1, 2, 3], [0, 1, 2, 3, 4], [1, 2, 3, 4, 3], [2, 3, 4, 3, 2]]
    want = [sum(w5[j] * row[i] for j, i in enumerate(r)) for r in idx]
    got = S.blur64(torch.tensor(row).view(5, 1), 1, 1, 5, 1.0).view(-1)
    assert torch.allclose(got, torch.tensor(want, dtype=torch.float64), rtol=1e-13, atol=0)


def test_clamp_rule_reflect_indices_and_host_tables():
    assert [S.kernel_size(100.0, n) for n in (1, 2, 3, 4, 5, 96, 97)] == [1, 3, 3, 5, 5, 97, 97]
    assert [S.kernel_size(s, 96) for s in (0.1, 0.3, 0.5, 1.0, 1.5, 16.0, 17.0)] == [1, 3, 3, 7, 9, 97, 97]
    assert [S.reflect(i, 5) for i in range(-3, 8)] == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1] and S.reflect(0, 1) == 0
    assert [S.reflect(i, 2) for i in (-1, 0, 1, 2)] == [1, 0, 1, 0]
    for sigma, n in ((0.8, 7), (100.0, 12), (1.5, 8), (3.0, 23), (100.0, 1), (100.0, 2)):
        assert ops.blur_kernel_size(sigma, n) == S.kernel_size(sigma, n)
        t = torch.tensor(ops.blur_taps(sigma, n), dtype=torch.float64)
        assert len(t) == S.kernel_size(sigma, n) and float((t - S.taps(sigma, n)).abs().max()) < 1e-15 and abs(float(t.sum()) - 1) < 1e-15


@pytest.mark.parametrize("B,Hh,Ww,C", [(2, 5, 7, 16), (1, 8, 8, 8), (3, 6, 4, 24)])
def test_emulation_equals_the_definition(B, Hh, Ww, C):
    x = torch.randn((B * Hh * Ww, C), generator=torch.Generator().manual_seed(B + C)).half()
    for sigma in (0.8, 1.5, 100.0, INF):
        ref, bound = S.bound(x, B, Hh, Ww, sigma)
        got = S.token_blur(x, B, Hh, Ww, sigma)
        assert got.dtype == torch.float16 and ((got.double() - ref).abs() <= bound).all(), sigma
        if sigma == INF:
            assert torch.allclose(ref.view(B, Hh * Ww, C), x.double().view(B, Hh * Ww, C).mean(1, keepdim=True).expand(B, Hh * Ww, C))
    assert torch.equal(S.token_blur(x, B, Hh, Ww, 0.1), x)                  # k = 1


# ---- 2. refusals, both entry points of the loop
BAD = [(dict(seg_scale=-0.1), "seg_scale"), (dict(seg_scale=nan), "seg_scale"), (dict(seg_scale=INF), "seg_scale"),
       (dict(seg_blur_sigma=0.0), "seg_blur_sigma"), (dict(seg_blur_sigma=-1.0), "seg_blur_sigma"), (dict(seg_blur_sigma=nan), "seg_blur_sigma"),
       (dict(seg_scale=3.0, seg_blur_sigma=-INF), "seg_blur_sigma"),
       (dict(seg_scale=3.0, pag_scale=1.0), "cannot be combined with pag_scale"),
       (dict(seg_scale=3.0, guidance_rescale=0.7), "cannot be combined with guidance_rescale"),
       (dict(seg_scale=3.0, apg=True), "cannot be combined with apg"),
       (dict(seg_scale=3.0, seg_applied_layers=("middle",)), "seg_applied_layers: unknown layer name"),
       (dict(seg_applied_layers=("down_blocks.x",)), "seg_applied_layers: unknown layer name"),
       (dict(seg_scale=3.0, seg_applied_layers=()), "seg_applied_layers is empty")]


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
    lat, rl, emb = (t.half() for t in small_inputs(4, 19))
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _ddim())
    with pytest.raises(ValueError, match="seg_applied_layers: 'down_blocks.3' selects no attention block"):
        pipe.denoise(lat, rl, emb, 2, 3.5, seg_scale=3.0, seg_applied_layers=("down_blocks.3",))
    assert fake_ops.CALLS == []
    pipe.denoise(lat, rl, emb, 1, 3.5, seg_scale=3.0, seg_blur_sigma=INF)   # inf is a value, not a refusal


# ---- 3. the default
def test_default_is_the_plain_loop_call_for_call(monkeypatch, small_cpu):
    fake_ops.install(monkeypatch)
    ref, den, _, _ = small_cpu
    lat, rl, emb = (t.half() for t in small_inputs(4, 19))
    for make, step in ((_ddim, "cfg_ddim_step"), (_dpm, "cfg_multistep_step")):
        pipe = M.MikuDanceVideoPipeline(None, None, ref, den, make())
        del fake_ops.CALLS[:]
        a = pipe.denoise(lat, rl, emb, 2, 3.5)
        calls_a = list(fake_ops.CALLS)
        del fake_ops.CALLS[:]
        b = pipe.denoise(lat, rl, emb, 2, 3.5, seg_scale=0.0, seg_blur_sigma=2.0, seg_applied_layers=("up_blocks.1",))
        assert torch.equal(a, b) and calls_a == fake_ops.CALLS and _names() == [step] * 2
        assert not any(n == "token_blur" for n, _ in fake_ops.CALLS)
        del fake_ops.CALLS[:]
        c = pipe.denoise(lat, rl, emb, 2, 3.5, seg_scale=3.0, seg_applied_layers=("up_blocks.1",))
        assert not torch.equal(a, c) and _names() == [step + "_pag"] * 2


# ---- 4. the host graph of the perturbed evaluation
def _perturbed(s, names, sigma):
    sel = s.den.pag_blocks(names, "seg_applied_layers") if names else ()
    return s.den.forward_nhwc(s.x[s.f:], 1, s.f, torch.full((1,), float(s.t)), s.cross.rows(s.f, 2 * s.f), seg=(sel, sigma))


@pytest.mark.parametrize("read_state", [16], indirect=True)
def test_call_log_and_forward_of_the_perturbed_evaluation(monkeypatch, read_state):
    import collections
    s = read_state
    monkeypatch.setattr(ops, "token_blur", S.token_blur, raising=False)
    s.den.forward_nhwc(s.x, 2, s.f, torch.full((2,), float(s.t)), s.cross, halves_identical=True)      # projects the context K / V
    del fake_ops.CALLS[:]
    p_none = _perturbed(s, (), 1.5)
    none_log = _launches()
    assert not any(n == "token_blur" for n, _ in fake_ops.CALLS)
    del fake_ops.CALLS[:]
    p_pag = s.den.forward_nhwc(s.x[s.f:], 1, s.f, torch.full((1,), float(s.t)), s.cross.rows(s.f, 2 * s.f), pag=())
    assert _launches() == none_log and torch.equal(p_none, p_pag)          # unselected: the conditional half's calls, PAG's unselected form
    table = dict(s.den.attention_block_prefixes())
    for names, sigma in ((("mid", "up_blocks.1"), 100.0), (("down_blocks.1", "up_blocks.2.attentions.0"), 1.5)):
        del fake_ops.CALLS[:]
        got = _perturbed(s, names, sigma)
        sel_log = _launches()
        blurs = [d for n, d in fake_ops.CALLS if n == "token_blur"]
        want_blurs = []
        for p in P.select(list(table), names):
            C = table[p].dim
            lvl = int(p.split(".")[1]) if p.startswith("down") else (3 - int(p.split(".")[1]) if p.startswith("up") else 3)
            want_blurs.append((s.f, s.h >> lvl, s.w >> lvl, C, float(sigma)))
        # the selected block reads the bank, so q, k and V^T were separate GEMMs already: the same launches, the attention included, plus the blur
        assert sel_log == none_log and sorted(blurs) == sorted(want_blurs), (blurs, want_blurs)
        got = got.float().view(s.f, s.h, s.w, 4).permute(3, 0, 1, 2)[None]
        with torch.no_grad():
            want = S.perturbed_forward(s.den_sd, s.lat, torch.tensor(s.t), s.emb[1:2], s.banks, names, sigma)
            plain = S.O.denoising_unet_forward(s.den_sd, s.lat, torch.tensor(s.t), s.emb[1:2], s.banks, cfg=False)
        r, c, d = rel_l2(got, want), cosine(got, want), rel_l2(plain, want)
        print(f"\nSEG_HOST_FORWARD {names} sigma {sigma} rel_l2 {r:.3e} cos {c:.7f} (unperturbed conditional oracle vs perturbed: {d:.3e})")
        assert r < BOUND["rel"] and c > BOUND["cos"] and d > BOUND["rel"], (r, c, d)
    sel = s.den.pag_blocks(("mid",))
    for kw in (dict(two_queues=True), dict(halves_identical=True), dict(pag=sel)):
        with pytest.raises(ValueError, match="perturb"):
            s.den.forward_nhwc(s.x[s.f:], 1, s.f, torch.full((1,), 601.0), s.cross.rows(s.f, 2 * s.f), seg=(sel, 1.5), **kw)
    with pytest.raises(ValueError, match="perturbed evaluation"):
        s.den.forward_nhwc(s.x, 2, s.f, torch.full((2,), 601.0), s.cross, seg=(sel, 1.5))


# ---- 5. the whole loop on the emulated operators, against the restated loop
LAYERS = ("mid", "up_blocks.1")
LOOPS = {"ddim": dict(guidance=3.5, sigma=100.0), "no-cfg-inf": dict(guidance=1.0, sigma=INF), "2m": dict(guidance=3.5, sampler="2m", sigma=1.5)}


@pytest.mark.parametrize("case", list(LOOPS))
def test_host_loop_matches_restatement(monkeypatch, small_cpu, case):
    fake_ops.install(monkeypatch)
    cfg = LOOPS[case]
    ref, den, ref_sd, den_sd = small_cpu
    lat, rl, emb = small_inputs(4, 74)
    g, steps, sigma = cfg["guidance"], 3, cfg["sigma"]
    if g <= 1.0:
        emb = emb[1:]
    two_m = cfg.get("sampler") == "2m"
    mk_rs = lambda: R.Restated(2, "dpmsolver++", "midpoint") if two_m else None
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _dpm() if two_m else _ddim())
    out = pipe.denoise(lat.half(), rl.half(), emb.half(), steps, g, seg_scale=3.0, seg_blur_sigma=sigma, seg_applied_layers=LAYERS)
    nb = 2 if g > 1.0 else 1
    step = "cfg_multistep_step_pag" if two_m else "cfg_ddim_step_pag"
    assert _names() == [step] * steps and all(d["halves"] == nb and d["pag_scale"] == 3.0 for _, d in P.step_calls())
    assert [d["halves"] for n, d in fake_ops.tail_calls("window_accumulate", "window_accumulate_weighted")] == [nb, 1] * steps
    assert sum(1 for n, d in fake_ops.CALLS if n == "token_blur" and d[-1] == float(sigma)) == steps * 4      # mid + the three of up_blocks.1
    with torch.no_grad():
        kw = dict(guidance_scale=g, seg_layers=LAYERS, seg_blur_sigma=sigma, scheduler=mk_rs())
        want = S.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, seg_scale=3.0, **kw)
        kw["scheduler"] = mk_rs()
        plain = S.denoise_loop(ref_sd, den_sd, lat, rl, emb, steps, seg_scale=0.0, **kw)
    e, c, d = rel_l2(out.float(), want), cosine(out.float(), want), rel_l2(plain, want)
    print(f"\nSEG_HOST_LOOP {case} rel_l2 {e:.3e} cos {c:.7f} (seg_scale 0 vs 3 restated: {d:.3e})")
    assert torch.isfinite(out).all() and e < BOUND["rel"] and c > BOUND["cos"], (e, c)
    assert d > 2 * BOUND["rel"] and rel_l2(out.float(), plain) > 2 * BOUND["rel"], d      # a loop that ignored the keywords fails here


# ---- 6. window parallelism: three gloo ranks
def _wp_worker(rank, world, port, q):
    worker_setup(rank, world, port)
    from mikudance_amd import MikuDanceVideoPipeline, dp
    from mikudance_amd.selftest import build_models
    from mikudance_amd.synth import synth_inputs
    ref, den, _, _ = build_models(device="cpu", keep_state_dicts=False)
    lat, rl, emb = (t.half() for t in synth_inputs(16, 16, 16, ctx_len=5, ctx_dim=64, seed=521))
    kw = dict(context_frames=8, context_stride=1, context_overlap=2, seg_scale=3.0, seg_blur_sigma=1.5, seg_applied_layers=("mid", "up_blocks.1"))
    res = {}
    for name, sch, extra in (("ddim", M.DDIMScheduler(**SCHED_KWARGS), {}), ("2m-pyramid", M.DPMSolverMultistepScheduler(**SCHED_KWARGS),
                                                                               dict(context_fuse="pyramid"))):
        pipe = MikuDanceVideoPipeline(None, None, ref, den, sch)
        out = pipe.denoise(lat, rl, emb, 2, 3.5, window_parallel=dp.WindowParallel(), **kw, **extra)
        got = dp.gather_latents(out)
        if rank == 0:
            one = pipe.denoise(lat, rl, emb, 2, 3.5, **kw, **extra)
            plain = pipe.denoise(lat, rl, emb, 2, 3.5, **dict(kw, seg_scale=0.0), **extra)
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
def test_script_flags_parse_and_reach_denoise(monkeypatch, tmp_path, capsys):
    from mikudance_amd import inference_video as IV
    a = IV.parse_args([])
    assert (a.seg_scale, a.seg_blur_sigma, a.seg_layers) == (0.0, 100.0, "mid")
    a = IV.parse_args(["--seg_scale", "3", "--seg_blur_sigma", "inf", "--seg_layers", "mid,up_blocks.1"])
    assert (a.seg_scale, a.seg_blur_sigma, a.seg_layers) == (3.0, INF, "mid,up_blocks.1")
    with pytest.raises(SystemExit):
        IV.parse_args(["--seg_blur_sigma", "wide"])
    assert "seg_scale=--seg_scale" in IV.__doc__
    seen = []

    def spy(self, latents, *a, **kw):
        seen.append(tuple(kw[k] for k in ("seg_scale", "seg_blur_sigma", "seg_applied_layers")))
        return latents

    build = fake_pipeline_builder(IV)

    def build_with_block_list(*a, **kw):
        pipe = build(*a, **kw)
        pipe.denoising_unet.pag_blocks = lambda names, *rest: ()            # the stand-in UNet of the builder has no blocks to ask
        return pipe

    monkeypatch.setattr(IV, "build_pipeline", build_with_block_list)
    monkeypatch.setattr(M.MikuDanceVideoPipeline, "denoise", spy)
    cfg, size = script_tree(tmp_path)
    base = ["--config", cfg, "-W", str(size), "-H", str(size), "--steps", "2", "--output_dir", str(tmp_path / "out")]
    IV.main(base)
    IV.main(base + ["--seg_scale", "3", "--seg_blur_sigma", "inf"])
    IV.main(base + ["--seg_scale", "2.5", "--seg_blur_sigma", "4", "--seg_layers", "down_blocks.2, up_blocks.1.attentions.0"])
    assert seen == [(0.0, 100.0, ("mid",)), (3.0, INF, ("mid",)), (2.5, 4.0, ("down_blocks.2", "up_blocks.1.attentions.0"))]
