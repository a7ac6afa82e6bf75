"""GPU: guidance_interval= / uncond_cache_interval= on the MI355X -- md_cfg_uncond_cache against float64, its refusals, and the HIP loop against the
restated loop of tests/uncond_cache_ref.py.

Bounds.  The kernel makes at most three fp32 roundings per mode (store: 1 / cnt, the product, the difference; restore: delta cnt, scale t, the
difference), each 2^-24 relative, so with e = 4 * 2^-24:
  store    |delta cnt - (c_sum - u_sum)|   <= e (|c_sum| + |u_sum|)      per element, measured on delta * cnt in float64
  restore  |u_sum' - (c_sum - delta cnt)|  <= e (|c_sum| + |delta cnt|)
  store, then restore with scale 1 gives u_sum back within the sum of the two.  Restore with scale 0 is a copy: torch.equal.
Loops: rel-L2 <= 3e-2 and cosine >= 0.999, the loop bound of the other option tests, against the restated loop (the same UNet calls on the device,
everything behind them in float64 on the host; one reference per case, computed once).  profiles/uncond_cache_tests.log holds every printed figure of a run on an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402

import uncond_cache_ref as UR  # noqa: E402

DEV = torch.device("cuda:0")
E = 4 * 2.0 ** -24
ROUND = 4096 * 256                                                         # pixels of one grid round (one thread per pixel, the step kernels' cap)
SHAPES = [(1, 1), (3, 5), (2, 4099), (5, 459 * 457)]                        # the last: 1 048 815 pixels, 239 past one round, the boundary inside frame 4


def _case(ftot, hw, counters, seed=0):
    """(noise_sum, counter, delta) on the host: normal draws scaled by the counter (they are window sums), one pixel row near the fp16 maximum."""
    g = torch.Generator().manual_seed(seed + ftot * 7919 + hw)
    if counters == "int":
        cnt = (torch.arange(ftot) % 3 + 1).float()
    else:                                                                  # what pyramid fusion leaves: 1 up to a few fp32 roundings
        cnt = 1.0 + (torch.randint(-4, 5, (ftot,), generator=g).float() * 2.0 ** -23)
    ns = torch.randn(2, ftot, hw, 4, generator=g) * cnt.view(1, -1, 1, 1)
    ns[:, ftot - 1, hw // 2] = torch.tensor([[65000.0, -64000.0, 60000.0, 65504.0], [64500.0, 63000.0, -65504.0, 65000.0]]) * cnt[ftot - 1]
    delta = torch.randn(ftot, hw, 4, generator=g)
    delta[ftot - 1, hw // 2] = torch.tensor([500.0, -127000.0, 125504.0, -504.0])
    return ns, cnt, delta


def _check(tag, err, bound, second_round_from=None):
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"\nUNCOND_CACHE_KERNEL {tag}: max err / bound {ratio:.3f}")
    assert torch.isfinite(err).all() and bool((err <= bound).all()), (tag, ratio)
    if second_round_from is not None:                                      # the pixels a thread reaches in its second round, on their own
        e2, b2 = err.reshape(-1, 4)[second_round_from:], bound.reshape(-1, 4)[second_round_from:]
        assert e2.numel() > 0 and bool((e2 <= b2).all()) and float(b2.max()) > 0


@pytest.mark.parametrize("counters", ["int", "near1"])
@pytest.mark.parametrize("ftot,hw", SHAPES)
def test_kernel_matches_float64(ftot, hw, counters):
    ns, cnt, delta = _case(ftot, hw, counters)
    past = ROUND if ftot * hw > ROUND else None
    cd = cnt.double().view(-1, 1, 1)
    ns_d, cnt_d = ns.to(DEV), cnt.to(DEV)
    # store
    out = torch.full((ftot, hw, 4), float("nan"), device=DEV)
    ops.cfg_uncond_cache(ns_d, cnt_d, out, ftot, hw, 0)
    assert torch.equal(ns_d.cpu(), ns)                                     # noise_sum is left untouched
    stored = out.cpu()
    b_store = E * (ns[1].abs().double() + ns[0].abs().double())
    _check(f"store F {ftot} HW {hw} {counters}", (stored.double() * cd - (ns[1].double() - ns[0].double())).abs(), b_store, past)
    # restore, scale 1, from an independent delta
    work = ns_d.clone()
    ops.cfg_uncond_cache(work, cnt_d, delta.to(DEV), ftot, hw, 1, scale=1.0)
    got = work.cpu()
    assert torch.equal(got[1], ns[1])                                      # the u plane only
    want = UR.restore64(ns, cnt, delta, 1.0)
    _check(f"restore F {ftot} HW {hw} {counters}", (got[0].double() - want).abs(), E * (ns[1].abs().double() + (delta.double() * cd).abs()), past)
    # store, then restore: u_sum comes back within the sum of both bounds
    work = ns_d.clone()
    work[0].fill_(float("nan"))
    ops.cfg_uncond_cache(work, cnt_d, out, ftot, hw, 1)                    # scale defaults to 1
    b_rt = b_store + E * (ns[1].abs().double() + (stored.double() * cd).abs())
    _check(f"round trip F {ftot} HW {hw} {counters}", (work[0].cpu().double() - ns[0].double()).abs(), b_rt, past)


@pytest.mark.parametrize("ftot,hw", [(3, 5), (2, 4099)])
def test_restore_with_scale_0_is_the_conditional_plane_bit_for_bit(ftot, hw):
    ns, cnt, _ = _case(ftot, hw, "int", seed=3)
    ns_d, cnt_d = ns.to(DEV), cnt.to(DEV)
    for delta in (None, torch.full((ftot, hw, 4), float("nan"), device=DEV)):
        work = ns_d.clone()
        work[0].fill_(float("inf"))
        ops.cfg_uncond_cache(work, cnt_d, delta, ftot, hw, 1, scale=0.0)
        assert torch.equal(work[0], work[1]) and torch.equal(work[1], ns_d[1])
    # the step on the restored planes is the step on the conditional mean.  md_cfg_ddim_step at halves == 1 takes the plane as it is (the reference's
    # sum quirk: no division by the counter), so the mean is restated here as the step kernels form it: c_sum * (1 / cnt), both rounded to fp32
    small = ns_d.clone()
    small[:, ftot - 1, hw // 2] = 1.0                                     # (the fp16-maximum row would overflow the fp16 latents of either step)
    ops.cfg_uncond_cache(small, cnt_d, None, ftot, hw, 1, scale=0.0)
    lat0 = torch.randn(ftot, hw, 4, generator=torch.Generator().manual_seed(9)).half().to(DEV)
    a, b = lat0.clone(), lat0.clone()
    ops.cfg_ddim_step(a, small, cnt_d, ftot, hw, 7.5, 0.6, 0.8, halves=2)
    mean = (small[1] * (1.0 / cnt_d).view(-1, 1, 1))[None].contiguous()
    ops.cfg_ddim_step(b, mean, cnt_d, ftot, hw, 7.5, 0.6, 0.8, halves=1)
    assert torch.isfinite(a.float()).all() and not torch.equal(a, lat0)
    assert torch.equal(a, b)


def test_refusals_leave_the_buffers_untouched():
    lib = M._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ftot, hw = 2, 8
    big_ns = torch.randn(2 * ftot * hw * 4 + 8, device=DEV)
    big_d = torch.randn(ftot * hw * 4 + 8, device=DEV)
    big_c = torch.ones(ftot + 2, device=DEV)
    raw_c = torch.zeros(2 * (ftot + 2), dtype=torch.int16, device=DEV)
    ns, d, c = big_ns[:2 * ftot * hw * 4], big_d[:ftot * hw * 4], big_c[:ftot]
    keep = [t.clone() for t in (big_ns, big_d, big_c)]
    p = lambda t: t.data_ptr()
    assert lib.md_cfg_uncond_cache(p(ns), p(c), p(d), ftot, hw, 0, 1.0, st) == 0
    torch.cuda.synchronize()
    keep[1] = big_d.clone()
    bad = {"null noise_sum": (0, p(c), p(d), ftot, hw, 1, 1.0), "null counter": (p(ns), 0, p(d), ftot, hw, 1, 1.0),
           "null delta, store": (p(ns), p(c), 0, ftot, hw, 0, 1.0), "null delta, restore at scale 1": (p(ns), p(c), 0, ftot, hw, 1, 1.0),
           "null delta, store at scale 0": (p(ns), p(c), 0, ftot, hw, 0, 0.0),
           "Ftot 0": (p(ns), p(c), p(d), 0, hw, 1, 1.0), "Ftot < 0": (p(ns), p(c), p(d), -1, hw, 0, 1.0), "HW 0": (p(ns), p(c), p(d), ftot, 0, 1, 1.0),
           "HW < 0": (p(ns), p(c), p(d), ftot, -3, 0, 1.0), "mode 2": (p(ns), p(c), p(d), ftot, hw, 2, 1.0), "mode -1": (p(ns), p(c), p(d), ftot, hw, -1, 1.0),
           "scale nan": (p(ns), p(c), p(d), ftot, hw, 1, float("nan")), "scale inf": (p(ns), p(c), p(d), ftot, hw, 1, float("inf")),
           # misalignment: offset views of larger valid buffers (4 and 8 bytes off a 16-byte boundary; the counter 2 bytes off, through an int16 buffer)
           "noise_sum off by 4 bytes": (p(big_ns[1:]), p(c), p(d), ftot, hw, 1, 1.0), "delta off by 4 bytes": (p(ns), p(c), p(big_d[1:]), ftot, hw, 0, 1.0),
           "delta off by 8 bytes": (p(ns), p(c), p(big_d[2:]), ftot, hw, 1, 1.0), "counter off by 2 bytes": (p(ns), p(raw_c[1:]), p(d), ftot, hw, 1, 1.0)}
    for what, args in bad.items():
        assert lib.md_cfg_uncond_cache(*args, st) == -1, what              # MD_ERR_ARG
        with pytest.raises(M._lib.MdanceHipError, match="md_cfg_uncond_cache"):
            M._lib.call("md_cfg_uncond_cache", *args, st)
    torch.cuda.synchronize()
    for t, k in zip((big_ns, big_d, big_c), keep):
        assert torch.equal(t, k)
    assert lib.md_cfg_uncond_cache(p(ns), p(c), 0, ftot, hw, 1, 0.0, st) == 0      # the one place delta may be NULL
    with pytest.raises(M._lib.MdanceHipError, match="must live on the GPU"):
        ops.cfg_uncond_cache(ns.cpu(), c, d, ftot, hw, 1)
    with pytest.raises(M._lib.MdanceHipError, match="must be torch.float32"):
        ops.cfg_uncond_cache(ns, c, d.half(), ftot, hw, 1)
    with pytest.raises(AssertionError):
        ops.cfg_uncond_cache(ns, c, d[:-4], ftot, hw, 1)


# ---- the loop
STEPS, G = 6, 3.0
CASES = {"n2": dict(uncond_cache_interval=2), "half": dict(guidance_interval=(0.0, 0.5)),
         "n2-half-pag": dict(uncond_cache_interval=2, guidance_interval=(0.0, 0.5), pag_scale=1.0, pag_applied_layers=("mid",))}
CLIPS = {"two-windows": (6, dict(context_frames=4, context_stride=1, context_overlap=2)), "whole": (4, {})}


@pytest.fixture(scope="module")
def small():
    return build_models()


def _inputs(frames, seed=611):
    return tuple(t.half() for t in synth_inputs(frames, 16, 16, ctx_len=5, ctx_dim=64, seed=seed))


def _make(sampler):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS) if sampler == "2m" else M.DDIMScheduler(**SCHED_KWARGS)


def _loop(small, frames, sampler="ddim", g=G, embeds=slice(None), **kw):
    lat, rl, emb = _inputs(frames)
    pipe = M.MikuDanceVideoPipeline(None, None, small[0], small[1], _make(sampler))
    out = pipe.denoise(lat.to(DEV), rl.to(DEV), emb[embeds].to(DEV), STEPS, g, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


_RESTATED = {}


def _restated(small, frames, sampler, win, kw):
    """The restated loop, once per (clip, sampler, case)."""
    import dpmpp_ref
    from oracle import cpu_ref as O
    key = (frames, sampler, repr(sorted(kw.items())))
    if key not in _RESTATED:
        lat, rl, emb = (t.to(DEV) for t in _inputs(frames))
        pipe = M.MikuDanceVideoPipeline(None, None, small[0], small[1], _make(sampler))
        _RESTATED[key] = UR.denoise_loop(pipe, lat, rl, emb, STEPS, G, dpmpp_ref.Restated() if sampler == "2m" else O.DDIM(),
                                         interval=kw.get("guidance_interval", (0.0, 1.0)), n=kw.get("uncond_cache_interval", 1),
                                         pag_scale=kw.get("pag_scale", 0.0), pag_layers=kw.get("pag_applied_layers", ("mid",)), **win)
    return _RESTATED[key]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("sampler", ["ddim", "2m"])
@pytest.mark.parametrize("clip", list(CLIPS))
def test_loop_matches_the_restated_loop(small, clip, sampler, case):
    frames, win = CLIPS[clip]
    kw = CASES[case]
    want = _restated(small, frames, sampler, win, kw)
    got = _loop(small, frames, sampler, **win, **kw)
    e, c = rel_l2(got, want), cosine(got, want)
    print(f"\nUNCOND_CACHE_LOOP {clip} {sampler} {case} {STEPS} steps g {G}: rel_l2 {e:.3e} cos {c:.7f}")
    assert torch.isfinite(got).all() and e <= 3e-2 and c >= 0.999, (e, c)


def test_an_empty_interval_is_the_unguided_loop_on_window_means(small):
    """guidance_interval=(0, 0): every step is conditional-only and the step sees the window MEAN of c.  A guidance_scale = 1.0 run hands the
    scheduler the mean under context_fuse="pyramid" (the sum under "flat"): on a clip of one window the two fusions are the same bits, so that
    run is the reference.  The two take different batch sizes through the UNet: no bitwise claim.

    THE EMBEDDINGS.  Under CFG the reference UNet writes its banks with the contexts interleaved [u, c, u, c, ...] over the frames (the reference's
    embeds.repeat((f, 1, 1)), kept by _write_banks), so with image_prompt_embeds = [zeros, CLIP tokens] every other frame's bank comes from the ZERO
    embedding, while a guidance_scale = 1.0 run writes every bank from the CLIP tokens.  The conditional half of a CFG run is therefore not the
    prediction of the run without CFG, whatever this feature does: with [zeros, CLIP tokens] the comparison gives rel-L2 1.6e-1, cosine 0.987 on the
    MI355X, and 1.6e-1 on the CPU emulation, where the same comparison with the CLIP tokens in BOTH rows is 0.0 exactly (the unconditional row
    then reaches nothing but the banks: with an empty interval the unconditional half is never evaluated).  The assertion is made on those inputs,
    at the loop tolerance; the figure for [zeros, CLIP tokens] is printed beside it."""
    frames, win = CLIPS["whole"]                                          # (where windows overlap, pyramid weights are not the flat mean)
    want = _loop(small, frames, g=1.0, embeds=slice(1, 2), context_fuse="pyramid", **win)
    literal = _loop(small, frames, guidance_interval=(0.0, 0.0), **win)
    got = _loop(small, frames, embeds=[1, 1], guidance_interval=(0.0, 0.0), **win)
    e, c = rel_l2(got, want), cosine(got, want)
    print(f"\nUNCOND_CACHE_EMPTY_INTERVAL whole: rel_l2 {e:.3e} cos {c:.7f} with the CLIP tokens in both rows; "
          f"rel_l2 {rel_l2(literal, want):.3e} cos {cosine(literal, want):.7f} with [zeros, CLIP tokens] (the banks' interleaved contexts)")
    assert torch.isfinite(got).all() and e <= 3e-2 and c >= 0.999, (e, c)


def test_defaults_are_bitwise_and_runs_repeat(small):
    frames, win = CLIPS["two-windows"]
    plain = _loop(small, frames, **win)
    assert torch.equal(plain, _loop(small, frames, guidance_interval=(0.0, 1.0), uncond_cache_interval=1, **win))
    a = _loop(small, frames, uncond_cache_interval=2, **win)
    b = _loop(small, frames, uncond_cache_interval=2, **win)
    assert torch.equal(a, b) and not torch.equal(a, plain)
    print(f"\nUNCOND_CACHE_EFFECT two-windows n 2: rel_l2 from the plain loop {rel_l2(a, plain):.3e}")
