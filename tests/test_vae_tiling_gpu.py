"""GPU: tiled / sliced AutoencoderKL on the MI355X -- md_tile_blend_f16 against the float64 restatement of tests/vae_tiling_ref.py (every element of
the updated tile and of the destination within one fp16 ulp, the bound md_latent_resize_f16 is held to; nothing written outside the kept window
and the valid channels; two calls the same bits; every refusal without a launch), tiled_decode / tiled_encode with the real kernels against the
restatement fed with the same path's own untiled per-tile outputs (one fp16 ulp) and against the oracle's vae_* per tile blended in float64
(relative L2 at most 1.5 x what the untiled path shows against the oracle on one full tile), slicing, and one end-to-end call.

The VAE is the smallest configuration the issue names and the kernels accept it: block_out_channels (64, 64, 64, 64), sample_size 128."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import AutoencoderKL, _lib, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_state_dict  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

import vae_tiling_ref as R  # noqa: E402
from fake_ops import FakeCLIP  # noqa: E402

DEV = torch.device("cuda:0")
F16 = torch.float16
SENTINEL = 123.0

# (B, Th, Tw, C, ldc, Ah, Lw, ev, eh, keep_h, keep_w); Ah / Lw = 0: no such neighbour
BASE = dict(B=2, Th=16, Tw=16, C=8, ldc=64, Ah=16, Lw=16, ev=4, eh=4, kh=12, kw=12)
CASES = {
    "both-c8-ld64": dict(),
    "both-c3-ld3": dict(C=3, ldc=3),                          # the decoder's image: one thread per pixel
    "none": dict(Ah=0, Lw=0),
    "above-only": dict(Lw=0),
    "left-only": dict(Ah=0),
    "left-only-c3": dict(Ah=0, C=3, ldc=3),
    "edge-tile-10x6": dict(Th=10, Tw=6, kh=10, kw=6, Lw=16, Ah=16),
    "edge-tile-10x6-c3": dict(Th=10, Tw=6, kh=10, kw=6, C=3, ldc=3),
    "thinner-than-extent": dict(Th=2, kh=2),                  # ev = 4 clamped to 2
    "narrow-neighbours": dict(Ah=3, Lw=2),                    # clamped to the neighbour's size
    "ev0": dict(ev=0),
    "eh0-c3": dict(eh=0, C=3, ldc=3),
    "c6-ld8": dict(C=6, ldc=8),                               # a channel group that is half padding
    "c5-ld7": dict(C=5, ldc=7),                               # no vector path: odd pitch
    "past-the-grid-cap": dict(B=9, Th=256, Tw=256, C=3, ldc=3, Ah=8, Lw=8, ev=8, eh=8, kh=192, kw=192),       # 589 824 threads > the 524 288 of a full grid
    "past-the-grid-cap-c8": dict(B=5, Th=256, Tw=256, C=8, ldc=8, Ah=8, Lw=8, ev=8, eh=8, kh=192, kw=192),      # 655 360 threads, two per pixel
}


def _tiles(p, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: (torch.rand(s, generator=g, dtype=torch.float64) * 8 - 4).to(F16)
    cur = rnd(p["B"], p["Th"], p["Tw"], p["ldc"])
    above = rnd(p["B"], p["Ah"], p["Tw"], p["ldc"]) if p["Ah"] else None
    left = rnd(p["B"], p["Th"], p["Lw"], p["ldc"]) if p["Lw"] else None
    return cur, above, left


def _blend(p, cur, above, left, dtype):
    """ops.tile_blend into the middle of a larger sentinel-filled NCHW tensor -> (cur after, the big tensor, the window's offsets)."""
    big = torch.full((p["B"], p["C"] + 2, p["kh"] + 5, p["kw"] + 7), SENTINEL, device=DEV, dtype=dtype)
    oy, ox = 2, 3
    dst = big[:, 1:1 + p["C"], oy:oy + p["kh"], ox:ox + p["kw"]]
    cur_d = cur.to(DEV)
    ops.tile_blend(cur_d, dst, p["C"], None if above is None else above.to(DEV), None if left is None else left.to(DEV), (p["ev"], p["eh"]))
    torch.cuda.synchronize()
    return cur_d.cpu(), big.cpu(), (oy, ox)


@pytest.mark.parametrize("dtype", [F16, torch.float32], ids=["dst16", "dst32"])
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_matches_float64(case, dtype):
    p = dict(BASE, **CASES[case])
    cur, above, left = _tiles(p, seed=len(case) * 7 + p["Th"])
    C, kh, kw = p["C"], p["kh"], p["kw"]
    ref = R.blend_ref(cur[..., :C], None if above is None else above[..., :C], None if left is None else left[..., :C], p["ev"], p["eh"])
    got, big, (oy, ox) = _blend(p, cur, above, left, dtype)
    ok_c, worst_c = R.within_one_ulp(got[..., :C], ref)
    win = big[:, 1:1 + C, oy:oy + kh, ox:ox + kw]
    ok_d, worst_d = R.within_one_ulp(win, ref[:, :kh, :kw].permute(0, 3, 1, 2))
    print(f"\nTILE_BLEND {case} {dtype}: worst |y - ref| / bound cur {worst_c:.4f} dst {worst_d:.4f}, cur equal to fp16(ref) {torch.equal(got[..., :C], ref.to(F16))}")
    assert ok_c and ok_d, (worst_c, worst_d)
    assert torch.equal(got[..., C:], cur[..., C:])                             # the padding channels of cur keep their bits
    outside = big.clone()
    outside[:, 1:1 + C, oy:oy + kh, ox:ox + kw] = SENTINEL
    assert (outside == SENTINEL).all() and (win != SENTINEL).any()             # nothing outside the kept window
    if dtype == F16:
        assert torch.equal(win, got[:, :kh, :kw, :C].permute(0, 3, 1, 2))      # an fp16 destination holds the tile's own bits
    if not p["Ah"] and not p["Lw"] or (p["ev"] == 0 and not p["Lw"]):
        assert torch.equal(got, cur)
    again, big2, _ = _blend(p, cur, above, left, dtype)
    assert torch.equal(again, got) and torch.equal(big2, big)                  # two calls, the same bits


def _constructed_tile(a_vals, v_vals, rows, seed, e=3):
    """An e-row tile and the e-row tile above it (blended over ev = e rows: weights y / e) with case k at pixel k // 4, channel k % 4, row rows[k]:
    cur = v_vals[k], above = a_vals[k]; every other element random."""
    n = len(a_vals)
    tw = (n + 3) // 4
    g = torch.Generator().manual_seed(seed)
    cur = (torch.rand((1, e, tw, 4), generator=g, dtype=torch.float64) * 8 - 4).to(F16)
    above = (torch.rand((1, e, tw, 4), generator=g, dtype=torch.float64) * 8 - 4).to(F16)
    k = torch.arange(n)
    cur[0, rows, k // 4, k % 4] = v_vals
    above[0, rows, k // 4, k % 4] = a_vals
    return cur, above, (rows, k // 4, k % 4)


def _blend_above(cur, above, ldc):
    """cur over above with ev = the tiles' rows, through the 4-channel flavour (ldc = 4) or the per-pixel one (ldc = 5: an odd pitch) -> (cur after, dst fp32)."""
    B, Th, Tw, C = cur.shape
    pad = lambda t: torch.cat([t, torch.zeros((B, Th, Tw, ldc - C), dtype=F16)], -1).contiguous().to(DEV)
    cur_d, dst = pad(cur), torch.zeros((B, C, Th, Tw), device=DEV, dtype=torch.float32)
    ops.tile_blend(cur_d, dst, C, above=pad(above), extent=(Th, 0))
    torch.cuda.synchronize()
    return cur_d.cpu()[..., :C], dst.cpu().permute(0, 2, 3, 1)


@pytest.mark.parametrize("ldc", [4, 5], ids=["per-8-bytes", "per-pixel"])
def test_kernel_blend_that_cancels(ldc):
    """above (1 - t) + cur t with cur = -above (1 - t) / t exactly (t = 1/3: cur = -2 above; t = 2/3: above = -2 cur), operands up to +-65504: the
    float64 value is 0 up to 1e-11, and one fp16 ulp of it is 2^-24.  The weights 1/3 and 2/3 are no fp32 numbers: a blend in plain fp32 leaves
    |above| (1 - 3 fl(1/3)) = 3e-8 |above|, from 5e-7 (|above| = 16) to 1e-3 here, 8 to 10^4 x the bound.  The kernel's pairs of floats leave 1e-10.  Also the same operands a few
    fp16 steps off the exact cancellation."""
    g = torch.Generator().manual_seed(3)
    n = 256
    big = (torch.rand(n, generator=g, dtype=torch.float64) * 31000 + 1000).to(F16) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).to(F16)
    big[:4] = torch.tensor([32752.0, -32752.0, 16.0, -1000.0], dtype=F16)       # 2 x 32752 = 65504, the largest fp16
    rows = torch.randint(1, 3, (n,), generator=g)
    rows[:2] = torch.tensor([1, 2])
    a_vals = torch.where(rows == 1, big, -2 * big)                               # row 1: a 2/3 + v 1/3 with v = -2 a; row 2: a 1/3 + v 2/3 with a = -2 v
    v_vals = torch.where(rows == 1, -2 * big, big)
    assert torch.isfinite(a_vals).all() and torch.isfinite(v_vals).all() and float(torch.maximum(a_vals.abs(), v_vals.abs()).max()) == 65504.0
    for steps in (0, 1, -3):                                                     # exact cancellation, then the smaller operand a few fp16 steps off it
        off = lambda t: (t.view(torch.int16) + steps).view(F16)
        a_s, v_s = torch.where(rows == 1, off(a_vals), a_vals), torch.where(rows == 1, v_vals, off(v_vals))
        cur, above, at = _constructed_tile(a_s, v_s, rows, seed=steps + 5)
        ref = R.blend_ref(cur, above, None, 3, 0)
        if steps == 0:
            assert float(ref[0][at].abs().max()) < 1e-10
            t32 = torch.tensor(1.0, dtype=torch.float32) / 3                      # what plain fp32 weights would leave: far outside the bound
            assert float((big.double().abs() * float((1 - 3 * t32.double()).abs())).min()) > 4 * 2.0 ** -24
        got, dst = _blend_above(cur, above, ldc)
        ok_c, worst_c = R.within_one_ulp(got, ref)
        ok_d, worst_d = R.within_one_ulp(dst, ref)
        print(f"\nTILE_BLEND cancelling, {steps} steps off, ldc {ldc}: worst |y - ref| / bound cur {worst_c:.4f} dst {worst_d:.4f}")
        assert ok_c and ok_d, (steps, worst_c, worst_d)


@pytest.mark.parametrize("ldc", [4, 5], ids=["per-8-bytes", "per-pixel"])
def test_kernel_rounds_once(ldc):
    """The header's ONE rounding.  Constructed: ev = 4, row 1 (weights 3/4 and 1/4, exact), `above` every fp16 number in [1, 4) whose 3/4 is the
    MIDPOINT of two fp16 numbers, `cur` = +-2^-24 or +-2^-23, so that the blend is that midpoint +-2^-26 or +-2^-25: below half an fp32 step.  h + l
    rounded to fp32 is then the midpoint itself, and a second rounding to fp16 goes to the even neighbour whatever side the value is on; the
    kernel rounds the pair to odd in between and must give fp16(float64 value) bit for bit.  With blend extents that are powers of two (a quarter
    of sample_size) this is the only way a blend rounds twice: a neighbour many binades smaller than the tile.  Chained over a tile grid, a tile
    stored one ulp off moves the next blend by up to (1 - t) ulp on top of its own half, so the one-ulp bound of the whole-VAE tests rests on it."""
    every = torch.arange(0x3C00, 0x4400, dtype=torch.int16).view(F16).numpy()                  # [1, 4)
    a = np.repeat(every, 4)
    v = np.tile(np.array([2.0 ** -24, -2.0 ** -24, 2.0 ** -23, -2.0 ** -23], dtype=np.float16), len(every))
    exact = (a.astype(np.float64) * 3 + v.astype(np.float64)) / 4                                # exact in float64
    twice = exact.astype(np.float32).astype(np.float16)
    hit = np.flatnonzero(twice != exact.astype(np.float16))
    assert len(hit) >= 200, len(hit)
    cur, above, at = _constructed_tile(torch.from_numpy(a[hit]), torch.from_numpy(v[hit]), torch.ones(len(hit), dtype=torch.long), seed=2, e=4)
    ref = R.blend_ref(cur, above, None, 4, 0)
    want = torch.from_numpy(ref.numpy().astype(np.float16))                      # numpy rounds float64 -> fp16 once
    assert torch.equal(want[0][at], torch.from_numpy(exact[hit].astype(np.float16))) and (want[0][at] != torch.from_numpy(twice[hit])).all()
    got, dst = _blend_above(cur, above, ldc)
    print(f"\nTILE_BLEND rounds once, ldc {ldc}: {len(hit)} midpoint cases, {int((got[0][at] != want[0][at]).sum())} differ from fp16(float64)")
    assert torch.equal(got, want) and R.within_one_ulp(dst, ref)[0]


def test_kernel_refuses_bad_arguments():
    B, Th, Tw, C, ldc = 2, 8, 8, 8, 16
    cur = torch.full((B, Th, Tw, ldc), 1.0, device=DEV, dtype=F16)
    above, left = torch.full_like(cur, 2.0), torch.full_like(cur, 3.0)
    dst = torch.full((B, C, Th, Tw), SENTINEL, device=DEV, dtype=torch.float32)
    X, A, L, D, st = cur.data_ptr(), above.data_ptr(), left.data_ptr(), dst.data_ptr(), ops._st()
    sB, sC, sY, sX = dst.stride()
    ok = dict(cur=X, ldc=ldc, above=A, Ah=Th, left=L, Lw=Tw, dst=D, f32=1, B=B, Th=Th, Tw=Tw, C=C, ev=2, eh=2, kh=6, kw=6)
    bad = [dict(cur=0), dict(dst=0), dict(B=0), dict(Th=0), dict(Tw=-1), dict(C=0), dict(ldc=0), dict(C=17), dict(ldc=4), dict(ev=-1), dict(eh=-1), dict(kh=9),
           dict(kw=9), dict(kh=0), dict(kw=-2), dict(Ah=0), dict(Lw=0), dict(Ah=-4), dict(f32=2), dict(cur=X + 1), dict(above=A + 1), dict(left=L + 1),
           dict(dst=D + 2), dict(dst=D + 1, f32=0), dict(above=X), dict(left=X + 64), dict(above=X - 32), dict(B=2 ** 20, Th=2 ** 10, Tw=2 ** 10),
           dict(Ah=2 ** 30), dict(Lw=2 ** 30)]
    order = ("cur", "ldc", "above", "Ah", "left", "Lw", "dst", "f32", "B", "Th", "Tw", "C", "ev", "eh", "kh", "kw")
    for change in bad:
        a = dict(ok, **change)
        args = tuple(a[k] for k in order) + (sB, sC, sY, sX, st)
        with pytest.raises(_lib.MdanceHipError, match="md_tile_blend_f16"):
            _lib.call("md_tile_blend_f16", *args)
        assert _lib.load().md_tile_blend_f16(*args) == -1, change              # MD_ERR_ARG
        assert _lib.load().md_last_error().decode().startswith("md_tile_blend_f16"), change
    torch.cuda.synchronize()
    assert (cur == 1.0).all() and (above == 2.0).all() and (left == 3.0).all() and (dst == SENTINEL).all()       # nothing was launched
    _lib.call("md_tile_blend_f16", *(ok[k] for k in order), sB, sC, sY, sX, st)
    torch.cuda.synchronize()
    assert (dst[:, :, :6, :6] != SENTINEL).all() and (dst[:, :, 6:] == SENTINEL).all() and (dst[:, :, :, 6:] == SENTINEL).all()
    for call, msg in ((lambda: ops.tile_blend(cur.cpu(), dst, C), "GPU"), (lambda: ops.tile_blend(cur.float(), dst, C), "float16"),
                      (lambda: ops.tile_blend(cur[:, :, ::2], dst, C), "contiguous"), (lambda: ops.tile_blend(cur, dst, C, above=above[:, :, :4].contiguous()), "above must be"),
                      (lambda: ops.tile_blend(cur, dst, C, left=left[:, :4].contiguous()), "left must be"), (lambda: ops.tile_blend(cur, dst[:, :4], C), "dst must be"),
                      (lambda: ops.tile_blend(cur, dst.double(), C), "fp16/fp32")):
        with pytest.raises(_lib.MdanceHipError, match=msg):
            call()


# ---- the whole VAE
CHANS = (64, 64, 64, 64)


@pytest.fixture(scope="module")
def small_vae():
    vae = AutoencoderKL(block_out_channels=CHANS, sample_size=128)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed=77)
    vae.load_state_dict(sd, strict=True)
    return vae.half().to(DEV).eval(), sd


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def test_tiled_decode_against_its_own_tiles_and_the_oracle(small_vae):
    vae, sd = small_vae
    z = torch.randn(2, 4, 28, 40, generator=torch.Generator().manual_seed(6)).half()
    got = vae.tiled_decode(z.to(DEV)).sample.cpu()
    assert tuple(got.shape) == (2, 3, 224, 320) and got.dtype == F16
    # 1. the tiling logic alone: the restatement on the same path's own untiled per-tile outputs
    own = R.tiled_ref(z, lambda t: _nhwc(vae.decode(t.to(DEV)).sample).cpu(), 128, 16, 0.25, 8, encode=False)
    ok, worst = R.within_one_ulp(got, own)
    print(f"\nVAE_TILED decode vs own tiles: worst |y - ref| / bound {worst:.4f}, bitwise {torch.equal(got, own.to(F16))}")
    assert ok, worst
    # 2. the oracle per tile, blended in float64, against the untiled path's own error on one full tile
    with torch.no_grad():
        full = O.vae_decode(sd, z[:, :, :16, :16].float())
        want = R.tiled_ref(z, lambda t: _nhwc(O.vae_decode(sd, t.float())), 128, 16, 0.25, 8, encode=False)
    yard = rel_l2(vae.decode(z[:, :, :16, :16].to(DEV)).sample.float().cpu(), full)
    r = rel_l2(got.float(), want.float())
    print(f"VAE_TILED decode vs oracle tiles: rel-L2 {r:.3e}, the untiled path on one tile {yard:.3e}")
    assert r <= 1.5 * yard, (r, yard)
    vae.enable_tiling()
    try:
        assert torch.equal(vae.decode(z.to(DEV)).sample.cpu(), got)            # decode() takes the same road
    finally:
        vae.disable_tiling()
    assert not torch.equal(vae.decode(z.to(DEV)).sample.cpu(), got)


def test_tiled_encode_against_its_own_tiles_and_the_oracle(small_vae):
    vae, sd = small_vae
    x = (torch.rand(2, 3, 224, 320, generator=torch.Generator().manual_seed(5)) * 2 - 1).half()
    moments = lambda v, t: torch.cat([v.encode(t.to(DEV)).latent_dist.mean, v.encode(t.to(DEV)).latent_dist.logvar], 1).cpu()
    post = vae.tiled_encode(x.to(DEV)).latent_dist
    got = torch.cat([post.mean, post.logvar], 1).cpu()
    assert tuple(got.shape) == (2, 8, 28, 40)
    # the logvar half of an untiled encode is clamped to [-30, 20] by DiagonalGaussian; synthetic weights stay far inside, checked here
    own_tiles = lambda t: _nhwc(moments(vae, t))
    own = R.tiled_ref(x, own_tiles, 128, 16, 0.25, 8, encode=True)
    assert own[:, 4:].abs().max() < 20
    ok, worst = R.within_one_ulp(got, own)
    print(f"\nVAE_TILED encode vs own tiles: worst |y - ref| / bound {worst:.4f}, bitwise {torch.equal(got, own.to(F16))}")
    assert ok, worst
    with torch.no_grad():
        full = O.vae_encode_moments(sd, x[:, :, :128, :128].float())
        want = R.tiled_ref(x, lambda t: _nhwc(O.vae_encode_moments(sd, t.float())), 128, 16, 0.25, 8, encode=True)
    yard = rel_l2(moments(vae, x[:, :, :128, :128]).float(), full)
    r = rel_l2(got.float(), want.float())
    print(f"VAE_TILED encode vs oracle tiles: rel-L2 {r:.3e}, the untiled path on one tile {yard:.3e}")
    assert r <= 1.5 * yard, (r, yard)


def _record_flavours(monkeypatch, fn):
    """fn() with every GEMM, convolution and GroupNorm of the VAE answering, before it runs, which kernel flavour the call AS IT IS MADE dispatches
    to (md_gemm_plan_call with its row blocks, md_conv_plan_call, md_groupnorm_plan with its launch geometry) -> (result, [(operator, problem, flavour)])."""
    import ctypes
    log = []
    gemm, conv, gn = ops.gemm, ops.conv3x3, ops.groupnorm

    def rec_gemm(a, w, *args, **kw):
        log.append(("gemm", (w.shape[0], w.shape[1], bool(kw.get("transpose_out", False))), ops.gemm_plan(a, w, *args, blocks=True, **kw)))
        return gemm(a, w, *args, **kw)

    def rec_conv(x, w, cout, *args, **kw):
        log.append(("conv", (tuple(x.shape[1:]), cout, kw.get("stride", 1), bool(kw.get("upsample", False))), ops.conv_plan(x, w, cout, *args, **kw)))
        return conv(x, w, cout, *args, **kw)

    def rec_gn(x, gamma, beta, groups, *args, **kw):
        B, C = x.shape[0], x.shape[-1]
        HW = x.numel() // (B * C)
        geo = [ctypes.c_int(0) for _ in range(4)]
        code = _lib.load().md_groupnorm_plan(B, HW, C, groups, x.stride(-2), int(x.data_ptr() % 16 == 0), 0, *(ctypes.byref(g) for g in geo))
        log.append(("groupnorm", (HW, C), (code,) + tuple(g.value for g in geo)))
        return gn(x, gamma, beta, groups, *args, **kw)

    with monkeypatch.context() as m:
        m.setattr(ops, "gemm", rec_gemm)
        m.setattr(ops, "conv3x3", rec_conv)
        m.setattr(ops, "groupnorm", rec_gn)
        out = fn()
    assert all(f[2][0] > 0 if isinstance(f[2], tuple) else f[2] > 0 for f in log), [f for f in log if (f[2][0] if isinstance(f[2], tuple) else f[2]) <= 0]
    return out, log


def _flavour_differences(unsliced, sliced, B):
    """The launches whose flavour differs between one call on B images and B calls on one image.  The sliced log is B times the same list; the
    unsliced one makes the same launches once on B images, except the mid-block attention's per-frame loop (V^T, Q K^T, P V: three GEMMs from the
    transposed one on), which it makes B times."""
    n = len(sliced) // B
    one = sliced[:n]
    assert len(sliced) == B * n and all(sliced[k * n:(k + 1) * n] == one for k in range(B))
    i = next(k for k, f in enumerate(one) if f[0] == "gemm" and f[1][2])
    expanded = one[:i] + one[i:i + 3] * B + one[i + 3:]
    assert [f[:2] for f in expanded] == [f[:2] for f in unsliced]                # the same launches on the same per-image problems
    return [(k, e, u) for k, (e, u) in enumerate(zip(expanded, unsliced)) if e[2] != u[2]]


# The case of the shape below, stated: every launch of the sliced call (B = 1) dispatches to the flavour the unsliced call (B = 3) runs, so the
# results must be BITWISE equal.  The test asks the dispatch and fails if that statement stops being true.
SLICING_SAME_FLAVOUR = True


def test_slicing_equals_the_unsliced_call(small_vae, monkeypatch):
    """enable_slicing() with B = 3 at 4 x 6 latents / 32 x 48 pixels against the unsliced call.  Which case this shape is comes from the dispatch
    itself: every GEMM, convolution (stride 1, stride 2, upsampling, conv_in / conv_out) and GroupNorm launch of both calls is asked for its
    flavour as the call is made (plan code, row blocks, GroupNorm launch geometry).  This shape is the SAME-FLAVOUR case (SLICING_SAME_FLAVOUR,
    asserted): the sliced results must be torch.equal to the unsliced ones.  Were a flavour to differ, the bound would be the untiled path's own
    error against the oracle (x 1.5), and only then."""
    vae, sd = small_vae
    z = torch.randn(3, 4, 4, 6, generator=torch.Generator().manual_seed(2)).half().to(DEV)
    x = (torch.rand(3, 3, 32, 48, generator=torch.Generator().manual_seed(1)) * 2 - 1).half().to(DEV)
    want_x, flav_x = _record_flavours(monkeypatch, lambda: vae.decode(z).sample)
    want_m, flav_m = _record_flavours(monkeypatch, lambda: vae.encode(x).latent_dist.mean)
    vae.enable_slicing()
    try:
        got_x, sliced_x = _record_flavours(monkeypatch, lambda: vae.decode(z).sample)
        got_m, sliced_m = _record_flavours(monkeypatch, lambda: vae.encode(x).latent_dist.mean)
    finally:
        vae.disable_slicing()
    differ = _flavour_differences(flav_x, sliced_x, 3) + _flavour_differences(flav_m, sliced_m, 3)
    same = not differ
    print(f"\nVAE_SLICING {len(flav_x)} + {len(flav_m)} launches asked; flavours differing between B = 1 and B = 3: {differ}; "
          f"decode bitwise {torch.equal(got_x, want_x)}, encode bitwise {torch.equal(got_m, want_m)}")
    assert same == SLICING_SAME_FLAVOUR, differ
    if same:
        assert torch.equal(got_x, want_x) and torch.equal(got_m, want_m)
    else:
        with torch.no_grad():
            yard_x = rel_l2(want_x.float().cpu(), O.vae_decode(sd, z.float().cpu()))
            yard_m = rel_l2(want_m.float().cpu(), O.vae_encode_moments(sd, x.float().cpu())[:, :4])
        assert rel_l2(got_x.float(), want_x.float()) <= 1.5 * yard_x and rel_l2(got_m.float(), want_m.float()) <= 1.5 * yard_m


# ---- the pipeline
W, H, F_ = 128, 96, 2


def test_pipeline_call_with_vae_tiling(small_vae):
    vae, _ = small_vae
    ref, den, _, _ = build_models(keep_state_dicts=False)
    pipe = M.MikuDanceVideoPipeline(vae=vae, image_encoder=FakeCLIP(), reference_unet=ref, denoising_unet=den, scheduler=M.DDIMScheduler(**SCHED_KWARGS))
    pipe.to("cuda", dtype=F16)
    from PIL import Image
    rng = np.random.default_rng(9)
    img = lambda: Image.fromarray(rng.integers(0, 255, (120, 144, 3), dtype=np.uint8))
    clip = (img(), img(), [img() for _ in range(F_)], [img() for _ in range(F_)], [img() for _ in range(F_)], rng.uniform(-0.03, 0.03, (F_, 2, H // 8, W // 8)))
    finals = []
    decode = pipe.decode_latents
    pipe.decode_latents = lambda latents: (finals.append(latents.clone()), decode(latents))[1]
    a = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7)).videos
    b = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), vae_tiling=False, vae_tile_size=None).videos
    assert torch.isfinite(a).all() and torch.equal(a, b)                       # the default is the call it was
    t = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), vae_tiling=True, vae_tile_size=64).videos
    assert (vae.use_tiling, vae.tile_sample_min_size, vae.tile_latent_min_size) == (False, 128, 16)
    assert tuple(t.shape) == (1, 3, F_, H, W) and torch.isfinite(t).all() and not torch.equal(t, a)
    # the frames are the final latents through tiled_decode: 12 x 16 latents in tiles of 8
    lat = (1 / 0.18215 * finals[-1]).permute(0, 2, 1, 3, 4).reshape(F_, 4, H // 8, W // 8).to(F16)
    vae.set_tile_size(64)
    try:
        rows, cols, _ = vae.tile_grid(H // 8, W // 8, encode=False)
        assert len(rows) * len(cols) == 6
        want = vae.tiled_decode(lat).sample
    finally:
        vae.set_tile_size(128)
    want = (want.reshape(1, F_, 3, H, W).permute(0, 2, 1, 3, 4) / 2 + 0.5).clamp(0, 1).cpu().float()
    assert torch.equal(t, want)
    with pytest.raises(ValueError, match=r"tile \(row"):
        pipe(*clip, W, H, F_, 2, 3.5, vae_tiling=True, vae_tile_size=32)       # tiles of 4 latents every 3: a last column 1 wide
