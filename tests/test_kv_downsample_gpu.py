"""GPU: K / V token downsampling on the MI355X -- md_token_pool_f16 against torch at the smallest shapes where it can go wrong (bitwise for
nearest, 1 fp16 ulp for the mean, zero pad rows, nothing written behind the output, repeatable bits, every refusal), one TransformerBlock in
every reference mode against tests/todo_ref.py, the whole loop at reduced width (one queue and two, with PAG), and the drop-in script with
--kv_downsample.  Bounds: rel-L2 <= 3e-2 and cosine >= 0.999, the standing bound of the block and loop checks.
profiles/kv_downsample_tests.log holds every printed figure of a run on an MI355X.

Figures of that run.  Kernel: nearest bitwise, mean 0 fp16 ulp from the rounded float64 mean at all four shapes.  Block (320, 8 heads, 2 frames
per clip-half), rel-L2 against the restatement over the reference modes: 8 x 8 nearest 4.2e-4 ... 5.6e-4 (1.06-1.08 x the same block with
kv_pool=None), 5 x 7 nearest 4.5e-4 ... 5.5e-4 (1.08-1.11 x), mean 3.8e-4 ... 5.0e-4 (0.96-0.98 x); the bank bitwise the unpooled one.  Loop,
3 steps, plain loop 7.7e-3: (2,) nearest 9.1e-3 (1.18 x), (2, 2) mean 7.0e-3 (0.91 x), two queues 8.8e-3 (1.14 x), with PAG 1.28e-2 (1.67 x);
the pooled result is 0.73 (rel-L2) from the plain one on these synthetic weights."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import _lib, blocks, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402

import fusion_ref as FR  # noqa: E402
import todo_ref as T  # noqa: E402

DEV = torch.device("cuda:0")
G = 3.5
SENTINEL = 12345.0
GUARD = 64                                                                 # rows behind the output that must stay untouched


# ---- 1. the kernel
def _tokens(B, Hh, Ww, C, seed):
    """fp16 tokens on a 2^-6 grid in [-8, 8]: every fp32 sum of <= 64 of them is exact, so the kernel's mean is off from the exact mean by the
    rounding of 1 / s^2 alone (2^-24 relative), and after the ONE rounding to fp16 within 1 fp16 ulp of the rounded exact mean."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((B * Hh * Ww, C), generator=g) * 2).clamp(-8, 8).mul(64).round().div(64).half()


def _pool(x, B, Hh, Ww, C, s, mode, out_stride):
    """One call on a sentinel-filled buffer of B * out_stride + GUARD rows -> the whole buffer on the host."""
    y = torch.full((B * out_stride + GUARD, C), SENTINEL, dtype=torch.float16, device=DEV)
    _lib.call("md_token_pool_f16", x.data_ptr(), y.data_ptr(), B, Hh, Ww, C, s, ops.POOL_MODES[mode], out_stride, ops._st())
    torch.cuda.synchronize()
    return y.cpu()


def _ulp16(v):
    return torch.maximum(torch.tensor(2.0 ** -24, dtype=torch.float64), 2.0 ** (torch.floor(torch.log2(v.double().abs().clamp_min(2.0 ** -14))) - 10))


KERNEL_CASES = [(2, 5, 7, 320, 2, 8), (1, 8, 8, 640, 4, 8), (3, 6, 4, 1280, 3, 8), (2, 16, 16, 320, 2, 72)]


@pytest.mark.parametrize("B,Hh,Ww,C,s,out_stride", KERNEL_CASES)
@pytest.mark.parametrize("mode", ["nearest", "mean"])
def test_kernel_matches_torch(B, Hh, Ww, C, s, out_stride, mode):
    x = _tokens(B, Hh, Ww, C, seed=B + Hh * Ww + s)
    Lk = (Hh // s) * (Ww // s)
    assert out_stride >= (Lk + 7) // 8 * 8 and (out_stride > (Lk + 7) // 8 * 8) == (out_stride == 72)
    xd = x.to(DEV)
    y = _pool(xd, B, Hh, Ww, C, s, mode, out_stride)
    body = y[:B * out_stride].view(B, out_stride, C)
    if mode == "nearest":
        grid = x.view(B, Hh, Ww, C)
        iy = torch.arange(Hh // s) * s
        ix = torch.arange(Ww // s) * s
        want = grid[:, iy][:, :, ix].reshape(B, Lk, C)                     # the gather, and the torch one-liner gives the same
        assert torch.equal(want, T.pool(x, B, Hh, Ww, s, "nearest"))
        assert torch.equal(body[:, :Lk], want)
        err = 0.0
    else:
        want = T.pool(x.double(), B, Hh, Ww, s, "mean").half()
        d = (body[:, :Lk].double() - want.double()).abs() / _ulp16(want)
        err = float(d.max())
        assert err <= 1.0, err
    print(f"\nTODO_KERNEL B{B} {Hh}x{Ww} C{C} s{s} stride {out_stride} {mode}: Lk {Lk}, max error {err:.3g} fp16 ulp")
    pad = body[:, Lk:]
    assert pad.numel() == B * (out_stride - Lk) * C and (pad == 0).all() and not torch.signbit(pad).any()        # exact +0
    assert (y[B * out_stride:] == SENTINEL).all()                          # nothing behind the B * out_stride rows
    assert torch.equal(y, _pool(xd, B, Hh, Ww, C, s, mode, out_stride))    # the same bits again
    # the wrapper: stride = roundup8(Lk), the same rows
    out, lk, stride = ops.token_pool(xd, B, Hh, Ww, s, mode)
    torch.cuda.synchronize()
    assert (lk, stride) == (Lk, (Lk + 7) // 8 * 8) and out.shape == (B * stride, C)
    assert torch.equal(out.cpu().view(B, stride, C)[:, :Lk], body[:, :Lk]) and (out.view(B, stride, C)[:, Lk:] == 0).all()


def test_kernel_covers_more_than_one_grid_round():
    """B * out_stride * C / 8 items beyond 2048 workgroups of 256 lanes: the grid-stride loop runs more than once."""
    B, Hh, Ww, C, s = 6, 96, 96, 320, 2
    x = torch.randn((B * Hh * Ww, C), generator=torch.Generator().manual_seed(1)).half()
    Lk = 48 * 48
    assert B * Lk * (C // 8) > 2048 * 256
    y = _pool(x.to(DEV), B, Hh, Ww, C, s, "nearest", Lk)
    assert torch.equal(y[:B * Lk].view(B, Lk, C), T.pool(x, B, Hh, Ww, s, "nearest")) and (y[B * Lk:] == SENTINEL).all()


def test_bad_arguments_raise_and_leave_y_alone():
    B, Hh, Ww, C = 2, 5, 7, 320
    x = _tokens(B, Hh, Ww, C, 3).to(DEV)
    y = torch.full((B * 8 + GUARD, C), SENTINEL, dtype=torch.float16, device=DEV)
    X, Y = x.data_ptr(), y.data_ptr()
    call = lambda xp=X, yp=Y, b=B, hh=Hh, ww=Ww, c=C, s=2, mode=0, stride=8: _lib.call("md_token_pool_f16", xp, yp, b, hh, ww, c, s, mode, stride,
                                                                                    ops._st())
    cases = (dict(s=1), dict(s=9), dict(s=0), dict(s=-2), dict(mode=2), dict(mode=-1), dict(c=324), dict(c=4), dict(c=0), dict(s=6), dict(s=8),
             dict(hh=1), dict(ww=1, hh=35), dict(stride=0), dict(stride=5), dict(stride=12), dict(stride=4), dict(xp=0), dict(yp=0),
             dict(yp=X), dict(yp=X + 16 * C), dict(xp=Y + 2 * C * 8), dict(xp=X + 2), dict(yp=Y + 8), dict(b=0))
    for kw in cases:
        with pytest.raises(_lib.MdanceHipError):
            call(**kw)
        torch.cuda.synchronize()
        assert (y == SENTINEL).all(), kw                                   # nothing was launched
    call()
    torch.cuda.synchronize()
    assert not (y[:B * 8] == SENTINEL).any() and (y[B * 8:] == SENTINEL).all()
    # the wrapper's own refusals
    with pytest.raises(_lib.MdanceHipError, match="no CPU path"):
        ops.token_pool(x.cpu(), B, Hh, Ww, 2)
    with pytest.raises(_lib.MdanceHipError, match="mode"):
        ops.token_pool(x, B, Hh, Ww, 2, mode="area")
    with pytest.raises(_lib.MdanceHipError, match="contiguous"):
        ops.token_pool(x, B, Hh, Ww + 1, 2)
    with pytest.raises(_lib.MdanceHipError):
        ops.token_pool(x.float(), B, Hh, Ww, 2)


# ---- 2. one TransformerBlock(320, 8 heads), 2 frames per clip-half, every reference mode
@pytest.mark.parametrize("Hh,Ww", [(8, 8), (5, 7)])
@pytest.mark.parametrize("mode", ["nearest", "mean"])
def test_block_matches_restatement_in_every_reference_mode(Hh, Ww, mode):
    st = T.block_setup(320, 64, Hh, Ww, 2, DEV)
    plain = T.block_runs(st, None)
    runs = T.block_runs(st, (Hh, Ww, 2, mode))
    torch.cuda.synchronize()
    for case, (got, want) in runs.items():
        r, c, r0 = rel_l2(got, want), cosine(got, want), rel_l2(*plain[case])
        print(f"\nTODO_BLOCK {Hh}x{Ww} s2 {mode} {case}: rel_l2 {r:.3e} cos {c:.7f} (kv_pool=None, same block {r0:.3e}, ratio {r / r0:.2f}; "
              f"restated plain vs pooled {rel_l2(plain[case][1], want):.3e})")
        assert torch.isfinite(got).all() and r <= 3e-2 and c >= 0.999, (case, r, c)
        if case == "write-bank":
            assert torch.equal(got, plain[case][0])                        # the bank is the full-resolution norm1(x), pooled or not
        else:
            assert rel_l2(got, plain[case][0]) > 3e-2                      # pooling moves the block's output by more than the bound
    # kv_pool=None is the block as called today, bit for bit
    h = st.x.reshape(-1, 320).to(DEV)
    with torch.no_grad():
        a = st.blk(h.clone(), 4, Hh * Ww, st.cross)
        b = st.blk(h.clone(), 4, Hh * Ww, st.cross, sa=blocks.SelfAttnCall(pool=None))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a.float().cpu().view(4, Hh * Ww, 320), plain["plain"][0])


# ---- 3. the loop on the small models, 16 x 16 latents, 3 steps
@pytest.fixture(scope="module")
def small():
    return build_models()


@pytest.fixture(scope="module")
def clip():
    """The inputs, the plain loop's result on the device and the oracle's, shared by the loop tests."""
    return {}


STEPS = 3


def _inputs():
    return tuple(t.half().float() for t in synth_inputs(4, 16, 16, ctx_len=5, ctx_dim=64, seed=504))


def _loop(models, inputs, two_queues=False, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, M.DDIMScheduler(**SCHED_KWARGS))
    pipe.two_queues = two_queues
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), STEPS, G, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def _plain(small, clip):
    if "plain" not in clip:
        _, _, ref_sd, den_sd = small
        clip["inputs"] = _inputs()
        clip["plain"] = _loop(small, clip["inputs"])
        with torch.no_grad():
            clip["plain_want"] = FR.denoise_loop(ref_sd, den_sd, *clip["inputs"], STEPS, guidance_scale=G, reduced=True)
        clip["plain_err"] = rel_l2(clip["plain"], clip["plain_want"])
    return clip


def test_factor_one_is_bitwise_the_plain_loop_and_a_factor_is_not_ignored(small, clip, monkeypatch):
    c = _plain(small, clip)
    names, real = [], _lib.call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(_lib, "call", spy)
    a = _loop(small, c["inputs"])
    seen_a = list(names)
    for kw in (dict(kv_downsample=1), dict(kv_downsample=(1, 1, 1, 1), kv_downsample_mode="mean")):
        del names[:]
        b = _loop(small, c["inputs"], **kw)
        assert torch.equal(a, b) and torch.equal(a, c["plain"]) and seen_a == names      # launch for launch
    assert "md_token_pool_f16" not in seen_a
    del names[:]
    d = _loop(small, c["inputs"], kv_downsample=(2,))
    assert names.count("md_token_pool_f16") == 5 * STEPS                   # the five level-0 blocks, once per step
    e = rel_l2(d, a)
    print(f"\nTODO_EFFECT rel_l2(kv_downsample (2,), plain) {e:.3e}")
    assert not torch.equal(d, a) and e > 3e-2, e                           # the keyword is not silently ignored


LOOPS = {"2-nearest": dict(kv=(2,), mode="nearest"), "2.2-mean": dict(kv=(2, 2), mode="mean"),
         "2-nearest-two-queues": dict(kv=(2,), mode="nearest", two_queues=True),
         "2-nearest-pag": dict(kv=(2,), mode="nearest", pag=dict(pag_scale=3.0, pag_applied_layers=("mid", "up_blocks.1")))}


@pytest.mark.parametrize("case", list(LOOPS))
def test_loop_vs_restatement_reduced_width(small, clip, case):
    c = _plain(small, clip)
    cfg = LOOPS[case]
    _, _, ref_sd, den_sd = small
    pag = cfg.get("pag", {})
    rkw = dict(guidance_scale=G)
    if pag:
        rkw.update(pag_scale=pag["pag_scale"], pag_layers=pag["pag_applied_layers"])
    with torch.no_grad():
        want = T.denoise_loop(ref_sd, den_sd, *c["inputs"], STEPS, kv_downsample=cfg["kv"], mode=cfg["mode"], **rkw)
    out = _loop(small, c["inputs"], two_queues=cfg.get("two_queues", False), kv_downsample=cfg["kv"], kv_downsample_mode=cfg["mode"], **pag)
    e, cs = rel_l2(out, want), cosine(out, want)
    print(f"\nTODO_LOOP {case} {STEPS} steps rel_l2 {e:.3e} cos {cs:.7f} (plain loop, same clip {c['plain_err']:.3e}, ratio {e / c['plain_err']:.2f}; "
          f"pooled vs plain result {rel_l2(out, c['plain']):.3e})")
    assert torch.isfinite(out).all() and e <= 3e-2 and cs >= 0.999, (e, cs)
    assert c["plain_err"] <= 3e-2


def test_script_kv_downsample(tmp_path, golden_dir):
    """The drop-in script end to end, with and without --kv_downsample 2, on the synthetic weight tree of the other GPU script tests at
    128 x 128 pixels: a 16 x 16 latent, whose level 0 pools 256 tokens to 64."""
    from mikudance_amd import inference_video
    from mikudance_amd import io_utils as U
    from dpm_script_tree import make_tree
    cfg, W, H, F_ = make_tree(tmp_path, golden_dir, width=128, height=128)
    base = ["--config", cfg, "-W", str(W), "-H", str(H), "--steps", "3", "--seed", "7"]
    on = U.read_frames(inference_video.main(base + ["--kv_downsample", "2", "--output_dir", str(tmp_path / "on")]))
    off = U.read_frames(inference_video.main(base + ["--output_dir", str(tmp_path / "off")]))
    a, b = (np.stack([np.asarray(fr, dtype=np.float32) for fr in frames]) for frames in (on, off))
    assert len(on) == len(off) == F_ and np.isfinite(a).all() and a[:, :, 2 * (W + 2):].std() > 0
    print(f"\nTODO_SCRIPT mean |on - off| over the generated panel {float(np.abs(a - b)[:, :, 2 * (W + 2):].mean()):.3f} (of 255)")
    assert not np.array_equal(a, b)
