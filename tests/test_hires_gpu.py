"""GPU: two-pass high-resolution sampling on the MI355X -- md_latent_resize_f16 against the float64 reference of tests/hires_ref.py (nearest bitwise,
bilinear / bicubic within one fp16 ulp of the float64 value with no element exempt, the identity bitwise, +-65504 and subnormals, nothing written
outside the output, every refusal without a launch), ops.latent_resize's own checks, and MikuDanceVideoPipeline.__call__(hires_scale=2) bitwise
against the hand-written composition prepare_latents x 2 -> denoise -> upscale_latents -> denoise(init_latents=, strength=) -> decode, with both
schedulers and with kv_downsample + DeepCache; hires_scale=1 bitwise the call without the keyword."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import _lib, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models  # noqa: E402

import hires_ref as R  # noqa: E402
from fake_ops import FakeCLIP, FakeVAE  # noqa: E402  (duck-typed VAE / CLIP stand-ins)

DEV = torch.device("cuda:0")
F16 = torch.float16
MODES = ["nearest", "bilinear", "bicubic"]
GUARD = 64                                       # fp16 elements either side of the output (128 bytes: the 8-byte alignment is kept)
SENTINEL = 123.0


def _resize_guarded(x, ho, wo, mode):
    """The raw entry point into the middle of a larger buffer -> (y, the guard elements in front, behind)."""
    f, hi, wi, _ = x.shape
    n = f * ho * wo * 4
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=F16)
    _lib.call("md_latent_resize_f16", x.data_ptr(), buf[GUARD:].data_ptr(), f, hi, wi, ho, wo, ops.RESIZE_MODES[mode], ops._st())
    torch.cuda.synchronize()
    buf = buf.cpu()
    return buf[GUARD:GUARD + n].view(f, ho, wo, 4), buf[:GUARD], buf[GUARD + n:]


# ---- 1. the kernel
@pytest.mark.parametrize("kind", ["random", "extreme"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=[f"F{f}-{hi}x{wi}-to-{ho}x{wo}" for f, (hi, wi), (ho, wo) in R.SHAPES])
def test_kernel_matches_float64(shape, mode, kind):
    f, (hi, wi), (ho, wo) = shape
    x = (R.random_latents if kind == "random" else R.extreme_latents)(f, hi, wi, 100 + hi * wi + ho)
    if kind == "extreme":
        assert (x.abs() == 65504).any() and ((x != 0) & (x.abs() < 2.0 ** -14)).any()
    ref = R.resize_ref(x, ho, wo, mode)
    y, front, back = _resize_guarded(x.to(DEV), ho, wo, mode)
    assert (front == SENTINEL).all() and (back == SENTINEL).all()
    ok, worst = R.within_one_ulp(y, ref)
    print(f"\nHIRES_KERNEL {mode} {kind} F={f} {hi}x{wi}->{ho}x{wo}: worst |y - ref| / bound {worst:.4f}, equal to fp16(ref) {torch.equal(y, ref.to(F16))}")
    if mode == "nearest" or (hi, wi) == (ho, wo):
        assert torch.equal(y, ref.to(F16))                                  # a copy / the identity: bitwise
        if (hi, wi) == (ho, wo):
            assert torch.equal(y, x)
    assert ok, worst                                                     # every element within one fp16 ulp of the float64 value; inf where fp16(ref) is
    y2 = ops.latent_resize(x.to(DEV), f, hi, wi, ho, wo, mode)
    assert tuple(y2.shape) == (f, ho, wo, 4) and torch.equal(y2.cpu(), y)   # the wrapper, and the same bits twice


def test_bicubic_overshoot_beyond_fp16_is_infinite():
    x = torch.zeros((1, 4, 4, 4), dtype=F16)
    x[0, :, 1::2] = 65504.0
    x[0, :, 0::2] = -65504.0
    ref = R.resize_ref(x, 8, 8, "bicubic")
    assert torch.isinf(ref.to(F16)).any() and torch.isfinite(ref).all()
    y = ops.latent_resize(x.to(DEV), 1, 4, 4, 8, 8, "bicubic").cpu()
    assert torch.equal(y, ref.to(F16)) and R.within_one_ulp(y, ref)[0]


def test_kernel_refuses_bad_arguments():
    x = torch.zeros((2, 4, 4, 4), device=DEV, dtype=F16)
    y = torch.full((2 * 8 * 8 * 4 + 8,), SENTINEL, device=DEV, dtype=F16)
    X, Y, st = x.data_ptr(), y.data_ptr(), ops._st()
    ok = dict(x=X, y=Y, F=2, Hi=4, Wi=4, Ho=8, Wo=8, mode=2)
    bad = [dict(x=0), dict(y=0), dict(x=X + 2), dict(x=X + 4), dict(y=Y + 2), dict(y=Y + 6), dict(F=0), dict(F=-1), dict(Hi=0), dict(Wi=-3), dict(Ho=0),
           dict(Wo=-8), dict(mode=3), dict(mode=-1), dict(F=2, Hi=46341, Wi=46341), dict(F=2, Ho=46341, Wo=46341), dict(F=2 ** 31 - 1, Hi=2 ** 31 - 1, Wi=2 ** 31 - 1),
           dict(F=2 ** 31 - 1, Ho=2 ** 31 - 1, Wo=2 ** 31 - 1), dict(y=X), dict(y=X + 8), dict(x=Y + 16)]
    for change in bad:
        a = dict(ok, **change)
        args = (a["x"], a["y"], a["F"], a["Hi"], a["Wi"], a["Ho"], a["Wo"], a["mode"], st)
        with pytest.raises(_lib.MdanceHipError, match="md_latent_resize_f16"):
            _lib.call("md_latent_resize_f16", *args)
        assert _lib.load().md_latent_resize_f16(*args) == -1, change         # MD_ERR_ARG
        assert _lib.load().md_last_error().decode().startswith("md_latent_resize_f16"), change
    torch.cuda.synchronize()
    assert (y == SENTINEL).all() and not x.any()                          # nothing was launched
    _lib.call("md_latent_resize_f16", *(ok[k] for k in ("x", "y", "F", "Hi", "Wi", "Ho", "Wo", "mode")), st)
    torch.cuda.synchronize()
    assert not y[:-8].any() and (y[-8:] == SENTINEL).all()


def test_operator_checks_and_profile_record():
    x = R.random_latents(2, 4, 6, 1).to(DEV)
    for call, msg in ((lambda: ops.latent_resize(x.cpu(), 2, 4, 6, 8, 12), "GPU"), (lambda: ops.latent_resize(x.float(), 2, 4, 6, 8, 12), "float16"),
                      (lambda: ops.latent_resize(x, 2, 4, 6, 8, 12, mode="area"), "mode must be"), (lambda: ops.latent_resize(x, 3, 4, 6, 8, 12), "F\\*hi\\*wi\\*4"),
                      (lambda: ops.latent_resize(x.permute(0, 2, 1, 3), 2, 6, 4, 8, 12), "contiguous"), (lambda: ops.latent_resize(x, 2, 4, 6, 0, 12), "positive"),
                      (lambda: ops.latent_resize(x, 2, 4, 6, 8, 12, out=torch.empty((2, 8, 11, 4), device=DEV, dtype=F16)), "out must be"),
                      (lambda: ops.latent_resize(x, 2, 4, 6, 8, 12, out=torch.empty((2, 8, 12, 4), device=DEV)), "float16")):
        with pytest.raises(_lib.MdanceHipError, match=msg):
            call()
    out = torch.empty((2 * 8 * 12 * 4,), device=DEV, dtype=F16)
    _lib.PROFILER.start()
    try:
        got = ops.latent_resize(x, 2, 4, 6, 8, 12, "bilinear", out=out)
    finally:
        _lib.PROFILER.stop()
    torch.cuda.synchronize()
    assert got is out and torch.equal(out.view(2, 8, 12, 4).cpu(), R.resize_ref(x.cpu(), 8, 12, "bilinear").to(F16))
    (label, rec), = _lib.PROFILER.summary().items()
    assert label.startswith("latent_resize") and rec["count"] == 1 and rec["bytes"] == 8.0 * (2 * 4 * 6 + 2 * 8 * 12)


# ---- 2. the call against its composition
W, H, F_, STEPS, STRENGTH = 128, 96, 4, 4, 0.5


@pytest.fixture(scope="module")
def small():
    return build_models(keep_state_dicts=False)


@pytest.fixture(scope="module")
def clip():
    from PIL import Image
    rng = np.random.default_rng(9)
    img = lambda: Image.fromarray(rng.integers(0, 255, (120, 144, 3), dtype=np.uint8))
    return (img(), img(), [img() for _ in range(F_)], [img() for _ in range(F_)], [img() for _ in range(F_)], rng.uniform(-0.03, 0.03, (F_, 2, H // 8, W // 8)))


def _pipe(small, scheduler):
    ref, den, _, _ = small
    pipe = M.MikuDanceVideoPipeline(vae=FakeVAE(), image_encoder=FakeCLIP(), reference_unet=ref, denoising_unet=den, scheduler=scheduler).to("cuda", dtype=F16)
    pipe.hires_min_side = 48                                         # 128 x 96 -> 64 x 48
    return pipe


CASES = {"ddim": (lambda: M.DDIMScheduler(**SCHED_KWARGS), {}), "dpm": (lambda: M.DPMSolverMultistepScheduler(**SCHED_KWARGS), {}),
         "ddim-kv2-deepcache2": (lambda: M.DDIMScheduler(**SCHED_KWARGS), dict(kv_downsample=2, deep_cache_interval=2))}


@pytest.mark.parametrize("case", list(CASES))
def test_call_is_bitwise_its_composition(small, clip, case):
    make, kw = CASES[case]
    pipe = _pipe(small, make())
    out = pipe(*clip, W, H, F_, STEPS, 3.5, generator=torch.manual_seed(42), hires_scale=2, hires_strength=STRENGTH, hires_mode="bicubic",
               output_type="tensor", **kw).videos
    # by hand: the noise of the low size first, then of the full size, from one generator
    g = torch.manual_seed(42)
    emb = pipe.clip_embeds(clip[0])
    emb = torch.cat([torch.zeros_like(emb), emb], dim=0)
    noise_lo = pipe.prepare_latents(1, 4, W // 2, H // 2, F_, emb.dtype, DEV, g)
    noise = pipe.prepare_latents(1, 4, W, H, F_, emb.dtype, DEV, g)
    assert tuple(noise_lo.shape) == (1, 4, F_, 6, 8) and tuple(noise.shape) == (1, 4, F_, 12, 16)
    images = (clip[0], clip[1], [list(clip[2]), list(clip[3]), list(clip[4])])
    rl_lo, _ = pipe._condition_latents(*images, None, pipe.lowres_scene_motion(clip[5], H // 16, W // 16), H // 2, W // 2, F_)
    rl, _ = pipe._condition_latents(*images, None, clip[5], H, W, F_)
    low = pipe.denoise(noise_lo, rl_lo, emb, STEPS, 3.5, generator=g, **kw)
    up = pipe.upscale_latents(low, H, W, "bicubic")
    assert tuple(up.shape) == (1, 4, F_, 12, 16) and up.is_cuda and up.dtype == low.dtype
    high = pipe.denoise(noise, rl, emb, STEPS, 3.5, generator=g, init_latents=up, strength=STRENGTH, **kw)
    want = torch.from_numpy(pipe.decode_latents(high))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 3, F_, H, W) and torch.isfinite(out).all() and out.std() > 0
    assert torch.equal(out, want)
    # the resampling inside is the operator's: the float64 rule on the packed fp16 latents, within one ulp
    packed = low[0].permute(1, 2, 3, 0).contiguous().cpu()
    assert R.within_one_ulp(up[0].permute(1, 2, 3, 0).cpu(), R.resize_ref(packed, 12, 16, "bicubic"))[0]
    # and the second pass matters: it is not the enlarged first pass
    assert not torch.equal(high, up)


def test_scale_1_is_bitwise_the_call_without_the_keyword(small, clip):
    pipe = _pipe(small, M.DDIMScheduler(**SCHED_KWARGS))
    a = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7)).videos
    b = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), hires_scale=1).videos
    c = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), hires_scale=1.0, hires_strength=0.3, hires_mode="nearest", hires_steps=9).videos
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
