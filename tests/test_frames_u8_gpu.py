"""GPU: uint8 frame output on the MI355X -- md_frames_u8 must equal tests/frames_ref.py's u8_ref (torch on the CPU, the float path's own expression)
EXACTLY, every byte: every fp16 bit pattern in both arithmetics, fp32 sources around the k / 255 edges, every call form (NHWC pitch 3 and 8, NCHW,
an odd-offset NCHW view, C = 1 and 4, fp16 source with fp32 arithmetic), a window of a sentinel-filled canvas, past one grid round, two calls the
same bits, every refusal without a launch; AutoencoderKL.decode_u8 / AutoencoderKLTemporalDecoder.decode_u8 against u8_ref(decode(z).sample)
untiled, tiled and sliced; one end-to-end __call__(output_type="uint8") against the float call cast."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import AutoencoderKL, AutoencoderKLTemporalDecoder, _lib, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models  # noqa: E402
from mikudance_amd.synth import synth_state_dict  # noqa: E402

import frames_ref as R  # noqa: E402
from fake_ops import FakeCLIP  # noqa: E402

DEV = torch.device("cuda:0")
F16 = torch.float16
SENTINEL = 0xA5


def _want(src, f32_math):
    """u8_ref of a (B, C, H, W)-shaped source, in the operator's layout."""
    return R.u8_ref(src, f32_math).permute(0, 2, 3, 1).contiguous()


def _check(src, f32_math=None, out=None):
    got = ops.frames_u8(src, out, f32_math=f32_math)
    torch.cuda.synchronize()
    want = _want(src, (src.dtype == torch.float32) if f32_math is None else f32_math)
    diff = int((got.cpu() != want).sum())
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape) and diff == 0, f"{diff} of {want.numel()} bytes differ"
    return got


# ---- the arithmetic
@pytest.mark.parametrize("f32_math", [False, True], ids=["f16-chain", "f32-chain"])
def test_every_fp16_bit_pattern(f32_math):
    x = R.all_fp16()
    g = torch.Generator().manual_seed(1)
    planes = torch.stack([x, x[torch.randperm(65536, generator=g)], x.flip(0)]).view(1, 3, 256, 256)
    got = _check(planes.to(DEV), f32_math).cpu()
    nan = torch.isnan(planes).permute(0, 2, 3, 1)
    assert int(nan.sum()) == 3 * 2046 and (got[nan] == 0).all()                 # NaN -> 0
    assert len(torch.unique(got)) == 256
    _check(planes.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2), f32_math)              # and from the NHWC side
    if not f32_math:
        assert int((got != R.one_expression(planes).permute(0, 2, 3, 1)).sum()) == 3 * 544                # the chain, not the shortcut


def test_fp32_sources_around_the_byte_edges():
    g = torch.Generator().manual_seed(2)
    x = torch.rand(4, 3, 5, 7, generator=g) * 3 - 1.5
    _check(x.to(DEV))
    _check(x.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2))
    # s = v / 2 + 0.5 lands on k / 255 and one ulp either side of it: v = 2 (k / 255 -+ ulp) - 1 for every k, and k / 255 +- ulp themselves as inputs
    k = torch.arange(256, dtype=torch.float32) / 255
    lo, hi = torch.nextafter(k, torch.tensor(-1.0)), torch.nextafter(k, torch.tensor(2.0))
    edges = torch.cat([2 * e - 1 for e in (lo, k, hi)] + [lo, k, hi])                                    # 1536 values
    special = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0, -0.0, 1.0, -1.0, 3e38, -3e38, 1e-45, -1e-45, 1.0000001, -1.0000001, 0.99999994])
    v = torch.cat([edges, special, torch.zeros(1536 + 48 - len(edges) - len(special))]).view(1, 3, 16, 33)
    got = _check(v.to(DEV)).cpu()
    assert len(torch.unique(got)) == 256
    _check(v.permute(0, 2, 3, 1).contiguous().to(DEV).permute(0, 3, 1, 2))


# ---- the call forms
def _values(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g) * 3 - 1.5).to(dtype)
    flat = x.view(-1)
    flat[::37] = float("nan"); flat[5::41] = float("inf"); flat[7::43] = float("-inf")
    return x


def _nhwc(B, C, H, W, ldc, dtype=F16, seed=3, offset=0):
    buf = _values((B * H * W * ldc + offset,), dtype, seed).to(DEV)
    return buf[offset:].view(B, H, W, ldc)[..., :C].permute(0, 3, 1, 2)


def _nchw_view(B, C, H, W, dtype=F16, seed=4):
    big = _values((B, C + 1, H + 3, W + 5), dtype, seed).to(DEV)
    return big[:, 1:, 1:1 + H, 3:3 + W]                                        # odd element offsets: no aligned group of 4


FORMS = {
    "nhwc-ld3": lambda B, H, W: (_nhwc(B, 3, H, W, 3), None),
    "nhwc-ld8-c3": lambda B, H, W: (_nhwc(B, 3, H, W, 8), None),
    "nchw": lambda B, H, W: (_values((B, 3, H, W), F16, 5).to(DEV), None),
    "nchw-odd-view": lambda B, H, W: (_nchw_view(B, 3, H, W), None),
    "c1-nchw": lambda B, H, W: (_values((B, 1, H, W), F16, 6).to(DEV), None),
    "c1-nhwc-ld8": lambda B, H, W: (_nhwc(B, 1, H, W, 8), None),
    "c4-nchw": lambda B, H, W: (_values((B, 4, H, W), F16, 7).to(DEV), None),
    "c4-nhwc-ld4": lambda B, H, W: (_nhwc(B, 4, H, W, 4), None),
    "c2-nhwc-ld2": lambda B, H, W: (_nhwc(B, 2, H, W, 2), None),
    "f16-src-f32-math-nhwc": lambda B, H, W: (_nhwc(B, 3, H, W, 3), True),
    "f16-src-f32-math-nchw": lambda B, H, W: (_values((B, 3, H, W), F16, 8).to(DEV), True),
    "f32-nchw": lambda B, H, W: (_values((B, 3, H, W), torch.float32, 9).to(DEV), None),
    "f32-nhwc-ld3": lambda B, H, W: (_nhwc(B, 3, H, W, 3, torch.float32), None),
    "f32-nchw-odd-view": lambda B, H, W: (_nchw_view(B, 3, H, W, torch.float32), None),
    # pitch 4 / 8 with padding channels: vector loads with the padding dropped, element loads on the last unit of every row
    "nhwc-ld4-c3": lambda B, H, W: (_nhwc(B, 3, H, W, 4), None),
    "c2-nhwc-ld4": lambda B, H, W: (_nhwc(B, 2, H, W, 4), None),
    "c2-nhwc-ld8": lambda B, H, W: (_nhwc(B, 2, H, W, 8), None),
    "nhwc-ld8-c3-2byte-base": lambda B, H, W: (_nhwc(B, 3, H, W, 8, offset=1), None),      # aligned to its element only: element loads
    "f32-nhwc-ld4-c3": lambda B, H, W: (_nhwc(B, 3, H, W, 4, torch.float32), None),
}


@pytest.mark.parametrize("size", [(2, 5, 7), (2, 16, 16)], ids=["2x5x7", "2x16x16"])
@pytest.mark.parametrize("form", list(FORMS))
def test_call_forms(form, size):
    src, f32_math = FORMS[form](*size)
    assert tuple(src.shape[2:]) == size[1:]
    _check(src, f32_math)


def _window(B, H, W, C, pitch_extra=11):
    """A (B, H, W, C) window at byte offset (2, 3 * 3 + 1) of every frame of a sentinel-filled canvas with a wider row pitch."""
    P = (W * C + 3 * 3 + 1 + pitch_extra) | 1                                  # an odd pitch: the rows start at every alignment
    canvas = torch.full((B, H + 5, P), SENTINEL, device=DEV, dtype=torch.uint8)
    return canvas, canvas.as_strided((B, H, W, C), ((H + 5) * P, P, C, 1), 2 * P + 10)


@pytest.mark.parametrize("size", [(2, 5, 7), (2, 16, 16)], ids=["2x5x7", "2x16x16"])
@pytest.mark.parametrize("form", ["nhwc-ld3", "nchw", "c4-nchw", "c1-nchw", "nhwc-ld8-c3"])
def test_window_of_a_canvas(form, size):
    B, H, W = size
    src, f32_math = FORMS[form](*size)
    C = src.shape[1]
    canvas, out = _window(B, H, W, C)
    got = _check(src, f32_math, out)
    assert got.data_ptr() == out.data_ptr()
    c = canvas.cpu()
    inside = torch.zeros_like(c, dtype=torch.bool)
    inside[:, 2:2 + H, 10:10 + W * C] = True
    assert (c[~inside] == SENTINEL).all()                                      # nothing outside the B H rows of W C bytes
    assert torch.equal(c[:, 2:2 + H, 10:10 + W * C].reshape(B, H, W, C), _want(src, bool(f32_math)))
    canvas1, out1 = _window(B, H, W, C, pitch_extra=12)                        # an odd first byte as well
    out1 = canvas1.as_strided(out1.shape, out1.stride(), out1.storage_offset() + 1)
    _check(src, f32_math, out1)
    assert int((canvas1 != SENTINEL).sum()) <= B * H * W * C and (canvas1[:, :2] == SENTINEL).all() and (canvas1[:, 2 + H:] == SENTINEL).all()
    assert (canvas1[:, :, :11] == SENTINEL).all() and (canvas1[:, :, 11 + W * C:] == SENTINEL).all()


@pytest.mark.parametrize("B,form", [(9, "nhwc-ld3"), (9, "nchw"), (33, "nhwc-ld3"), (33, "nchw-odd-view"), (33, "nhwc-ld8-c3")])
def test_past_one_grid_round(B, form):
    """B = 9 of 256 x 256 x 3: 589 824 pixels, more than 2048 x 256 threads.  The kernel gives a thread 4 pixels of a row, so ITS grid-stride loop
    starts a second round at B = 33 (540 672 groups of 4 > 524 288 threads): both sizes run."""
    src, _ = FORMS[form](B, 256, 256)
    canvas, out = _window(B, 256, 256, 3)
    a = ops.frames_u8(src, out).clone()
    canvas.fill_(SENTINEL)
    b = ops.frames_u8(src, out)
    torch.cuda.synchronize()
    assert torch.equal(a, b)                                                   # two calls give the same bits
    diff = int((b.cpu() != _want(src, False)).sum())
    assert diff == 0, f"{diff} bytes differ"
    assert (canvas[:, :2] == SENTINEL).all() and (canvas[:, 258:] == SENTINEL).all() and (canvas[:, :, :10] == SENTINEL).all() and (canvas[:, :, 778:] == SENTINEL).all()


def test_two_calls_give_the_same_bits():
    src, _ = FORMS["nhwc-ld8-c3"](2, 16, 16)
    a, b = ops.frames_u8(src), ops.frames_u8(src)
    assert torch.equal(a, b)


# ---- the refusals
def test_kernel_refuses_bad_arguments():
    B, H, W, C = 2, 6, 5, 3
    src = torch.zeros((B, C, H, W), device=DEV, dtype=torch.float32)           # fp32 storage: both element sizes can be named on it
    dst = torch.full((B, H, W * C + 4), SENTINEL, device=DEV, dtype=torch.uint8)
    S, D, st = src.data_ptr(), dst.data_ptr(), ops._st()
    dY = W * C + 4
    ok = dict(src=S, f32=0, math=0, dst=D, B=B, H=H, W=W, C=C, sB=C * H * W, sC=H * W, sY=W, sX=1, dB=H * dY, dY=dY)
    bad = [dict(src=0), dict(dst=0), dict(C=0), dict(C=5), dict(C=-1), dict(B=0), dict(H=0), dict(W=0), dict(B=-2), dict(H=-1), dict(W=-7),
           dict(B=2 ** 11, H=2 ** 10, W=2 ** 10, dB=2 ** 40, dY=2 ** 20), dict(dY=W * C - 1), dict(dY=0), dict(dY=-dY), dict(dB=(H - 1) * dY + W * C - 1), dict(dB=0),
           dict(dB=-H * dY), dict(f32=1, math=0), dict(f32=2, math=1), dict(math=2), dict(math=-1), dict(src=S + 1), dict(src=S + 2, f32=1, math=1),
           dict(src=S + 1, f32=1, math=1), dict(src=S + 3, f32=1, math=1)]
    order = ("src", "f32", "math", "dst", "B", "H", "W", "C", "sB", "sC", "sY", "sX", "dB", "dY")
    for change in bad:
        a = dict(ok, **change)
        args = tuple(a[k] for k in order) + (st,)
        with pytest.raises(_lib.MdanceHipError, match="md_frames_u8"):
            _lib.call("md_frames_u8", *args)
        assert _lib.load().md_frames_u8(*args) == -1, change                   # MD_ERR_ARG
        assert _lib.load().md_last_error().decode().startswith("md_frames_u8"), change
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all()                                             # nothing was launched
    for good in (dict(), dict(math=1), dict(f32=1, math=1), dict(src=S + 2), dict(dst=D + 1, dB=H * dY - 1), dict(dB=(H - 1) * dY + W * C, B=1)):
        a = dict(ok, **good)
        _lib.call("md_frames_u8", *(a[k] for k in order), st)
    torch.cuda.synchronize()
    assert (dst[:, :, W * C + 1:] == SENTINEL).all()


def test_operator_refuses_bad_arguments():
    src = torch.zeros((2, 3, 6, 5), device=DEV, dtype=F16)
    out = torch.full((2, 6, 5, 3), SENTINEL, device=DEV, dtype=torch.uint8)
    wide = torch.full((2, 6, 5, 4), SENTINEL, device=DEV, dtype=torch.uint8)
    for call, msg in ((lambda: ops.frames_u8(src.cpu()), "CUDA fp16/fp32"), (lambda: ops.frames_u8(src.double()), "CUDA fp16/fp32"),
                      (lambda: ops.frames_u8(src[0]), r"\(B, C, H, W\)"), (lambda: ops.frames_u8(src.expand(2, 3, 6, 5).repeat(1, 2, 1, 1)), "C in 1..4"),
                      (lambda: ops.frames_u8(src[:, :, :0]), "no empty"), (lambda: ops.frames_u8(src, f32_math=1), "True, False or None"),
                      (lambda: ops.frames_u8(src.float(), f32_math=False), "needs f32_math=True"), (lambda: ops.frames_u8(src, out.cpu()), "CUDA uint8"),
                      (lambda: ops.frames_u8(src, out.to(torch.int8)), "CUDA uint8"), (lambda: ops.frames_u8(src, out[:, :5]), "out must be"),
                      (lambda: ops.frames_u8(src, out.permute(0, 2, 1, 3)), "out must be"), (lambda: ops.frames_u8(src, wide[..., :3]), "packed pixels"),
                      (lambda: ops.frames_u8(src, out.permute(0, 3, 1, 2)), "out must be")):
        with pytest.raises(_lib.MdanceHipError, match=msg):
            call()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (wide == SENTINEL).all()
    _lib.PROFILER.start()
    try:
        ops.frames_u8(src, out)
    finally:
        _lib.PROFILER.stop()
    torch.cuda.synchronize()
    (label, rec), = _lib.PROFILER.summary().items()
    assert label.startswith("frames_u8") and rec["count"] == 1 and rec["bytes"] == 3.0 * 2 * 3 * 6 * 5                 # 2 bytes read, 1 written per element


# ---- the VAEs
CHANS = (64, 64, 64, 64)


def _load(vae, seed):
    vae.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed=seed), strict=True)
    return vae.half().to(DEV).eval()


@pytest.fixture(scope="module")
def small_vae():
    return _load(AutoencoderKL(block_out_channels=CHANS, sample_size=128), 77)


def _latents(*shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).half().to(DEV)


def _decode_u8_equals_decode(vae, z, f32_math=False, **kw):
    want = _want(vae.decode(z, **kw).sample, f32_math)
    got = vae.decode_u8(z, **kw)
    torch.cuda.synchronize()
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == tuple(want.shape)
    diff = int((got.cpu() != want).sum())
    assert diff == 0 and len(torch.unique(want)) > 50, f"{diff} of {want.numel()} bytes differ"
    return got


def test_decode_u8_untiled(small_vae, monkeypatch):
    z = _latents(2, 4, 8, 8, seed=1)
    unpacks = []
    unpack = ops.unpack_nhwc
    got = _decode_u8_equals_decode(small_vae, z)
    monkeypatch.setattr(ops, "unpack_nhwc", lambda *a: (unpacks.append(1), unpack(*a))[1])
    assert torch.equal(small_vae.decode_u8(z), got) and unpacks == []          # no NCHW tensor on this road
    _decode_u8_equals_decode(small_vae, z.float(), f32_math=True)              # an fp32 boundary: the fp32 chain
    out = torch.zeros((2, 64, 64, 3), device=DEV, dtype=torch.uint8)
    assert small_vae.decode_u8(z, out=out) is out and torch.equal(out, got)


def test_decode_u8_tiled(small_vae):
    z = _latents(1, 4, 24, 16, seed=2)
    small_vae.enable_tiling()
    try:
        rows, cols, _ = small_vae.tile_grid(24, 16, encode=False)
        assert len(rows) * len(cols) == 4
        tiled = _decode_u8_equals_decode(small_vae, z)
    finally:
        small_vae.disable_tiling()
    assert not torch.equal(small_vae.decode_u8(z), tiled)


def test_decode_u8_sliced(small_vae):
    z = _latents(3, 4, 8, 8, seed=3)
    small_vae.enable_slicing()
    try:
        _decode_u8_equals_decode(small_vae, z)
    finally:
        small_vae.disable_slicing()


def test_decode_u8_temporal():
    vae = _load(AutoencoderKLTemporalDecoder(block_out_channels=CHANS), 31)
    z = _latents(4, 4, 8, 8, seed=4)
    _decode_u8_equals_decode(vae, z, num_frames=4)
    _decode_u8_equals_decode(vae, z, num_frames=2)


# ---- the pipeline
W, H, F_ = 128, 96, 2


def test_pipeline_call_uint8(small_vae):
    ref, den, _, _ = build_models(keep_state_dicts=False)
    pipe = M.MikuDanceVideoPipeline(vae=small_vae, image_encoder=FakeCLIP(), reference_unet=ref, denoising_unet=den, scheduler=M.DDIMScheduler(**SCHED_KWARGS))
    pipe.to("cuda", dtype=F16)
    pipe.vae_batch = 2
    from PIL import Image
    rng = np.random.default_rng(9)
    img = lambda: Image.fromarray(rng.integers(0, 255, (120, 144, 3), dtype=np.uint8))
    clip = (img(), img(), [img() for _ in range(F_)], [img() for _ in range(F_)], [img() for _ in range(F_)], rng.uniform(-0.03, 0.03, (F_, 2, H // 8, W // 8)))
    want = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7)).videos
    got = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), output_type="uint8").videos
    assert want.dtype == torch.float32 and tuple(want.shape) == (1, 3, F_, H, W) and torch.isfinite(want).all()
    assert got.dtype == torch.uint8 and not got.is_cuda and tuple(got.shape) == (1, F_, H, W, 3)
    cast = torch.from_numpy((want * 255).numpy().astype(np.uint8)).permute(0, 2, 3, 4, 1)
    assert torch.equal(got, cast) and len(torch.unique(got)) > 50
    pil = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), output_type="pil").videos
    assert torch.equal(torch.from_numpy(np.stack([np.asarray(im) for im in pil[0]]))[None], got)
