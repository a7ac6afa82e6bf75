"""GPU: colour matching on the MI355X.  md_color_moments against float64 sums of the same source values, within the bound its stated summation
order gives ((d + 3) 2^-24 relative, d = color_match_ref.moments_depth), bitwise repeatable, on every source form and load path, one unit past a
full round of workgroups, with the clamp, NaN and Inf; md_color_apply bit for bit against the numpy float32 restatement
(color_match_ref.apply_ref) on the same source forms into both destinations, inside a sentinel-filled canvas, with coefficients that clamp, NaN,
one row of coefficients per frame; every refusal of both operators without a launch; __call__(color_match=...) end to end against the
restatement evaluated on the sums the device returned."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import AutoencoderKL, _lib, color_match as CM, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models  # noqa: E402
from mikudance_amd.synth import synth_state_dict  # noqa: E402

import color_match_ref as R  # noqa: E402
from fake_ops import FakeCLIP  # noqa: E402

DEV = torch.device("cuda:0")
F16 = torch.float16
U = 2.0 ** -24
SENTINEL = 0xA5


# ---- the source forms: (B, 3, H, W)-shaped views
def _values(shape, dtype, seed, special=False):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(shape, generator=g) * 3 - 1.5).to(dtype)                   # a third of the values outside [-1, 1]: the clamp works
    if special:
        flat = x.view(-1)
        flat[::37] = float("nan"); flat[5::41] = float("inf"); flat[7::43] = float("-inf")
    return x


def _nhwc(B, H, W, ldc, dtype=F16, seed=3, special=False, offset=0):
    buf = _values((B * H * W * ldc + offset,), dtype, seed, special).to(DEV)
    return buf[offset:].view(B, H, W, ldc)[..., :3].permute(0, 3, 1, 2)


def _nchw_view(B, H, W, dtype=F16, seed=4, special=False):
    big = _values((B, 4, H + 3, W + 5), dtype, seed, special).to(DEV)
    return big[:, 1:, 1:1 + H, 3:3 + W]                                        # odd element offsets: no aligned group


FORMS = {
    "nhwc-ld3": lambda B, H, W, sp: _nhwc(B, H, W, 3, special=sp),
    "nhwc-ld4": lambda B, H, W, sp: _nhwc(B, H, W, 4, special=sp),
    "nhwc-ld8": lambda B, H, W, sp: _nhwc(B, H, W, 8, special=sp),
    "nhwc-ld3-2byte-base": lambda B, H, W, sp: _nhwc(B, H, W, 3, special=sp, offset=1),        # aligned to its element only: element loads
    "nhwc-ld8-2byte-base": lambda B, H, W, sp: _nhwc(B, H, W, 8, special=sp, offset=1),
    "nchw": lambda B, H, W, sp: _values((B, 3, H, W), F16, 5, sp).to(DEV),
    "nchw-odd-view": lambda B, H, W, sp: _nchw_view(B, H, W, special=sp),
    "f32-nchw": lambda B, H, W, sp: _values((B, 3, H, W), torch.float32, 9, sp).to(DEV),
    "f32-nhwc-ld3": lambda B, H, W, sp: _nhwc(B, H, W, 3, torch.float32, special=sp),
    "f32-nhwc-ld4": lambda B, H, W, sp: _nhwc(B, H, W, 4, torch.float32, special=sp),
}
# 41 x 200: U = 41 * 25 = 1025 units of 8 pixels, one past the 1024 of one workgroup -> 2 workgroups per frame and the iteration count changes;
# 16 x 16 has whole units only (every vector path), 5 x 7 and 1 x 1 tails only (element loads)
SIZES = [(1, 1, 1), (3, 5, 7), (2, 16, 16), (2, 41, 200)]


def _check_moments(src):
    B, _, H, W = src.shape
    got = ops.color_moments(src)
    again = ops.color_moments(src)
    for ws in ops._workspaces["color_moments"].values():                       # an unrelated kernel writes the workspace
        ws.fill_(float("nan"))
    third = ops.color_moments(src)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, 9) and got.device == src.device
    assert torch.equal(got.view(torch.int64), again.view(torch.int64)) and torch.equal(got.view(torch.int64), third.view(torch.int64))
    got, want = got.cpu().numpy(), R.sums_f64(src)
    bound = (R.moments_depth(H, W) + 3) * U * want
    err = np.abs(got - want)
    print(f"moments {tuple(src.shape)} strides {tuple(src.stride())}: worst error / bound = {np.nanmax(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.isfinite(want).all() and (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    return got, want


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", list(FORMS))
def test_moments_against_float64(form, size):
    src = FORMS[form](*size, False)
    assert tuple(src.shape) == (size[0], 3) + size[1:]
    got, want = _check_moments(src)
    assert got.shape == want.shape and (size[1] * size[2] == 1 or (want[:, 3:6] > 0).all())


def test_moments_depth_restates_the_kernel():
    assert [R.moments_depth(h, w) for h, w in ((1, 1), (16, 16), (32, 256), (41, 200), (768, 768), (1024, 1024))] == [17, 17, 20, 19, 20, 20]
    lib = _lib.load()
    assert lib.md_color_moments_workspace_bytes(1, 1, 1) == 36 and lib.md_color_moments_workspace_bytes(2, 41, 200) == 2 * 2 * 36
    assert lib.md_color_moments_workspace_bytes(8, 1024, 1024) == 8 * 128 * 36 and lib.md_color_moments_workspace_bytes(0, 4, 4) == 0
    assert lib.md_color_moments_workspace_bytes(1 << 12, 1 << 10, 1 << 10) == 0


def test_moments_whose_terms_are_all_zero_are_exactly_zero():
    src = FORMS["nhwc-ld3"](2, 16, 24, False)
    src[:, 0] = -2.0                                                           # s0 = 0 everywhere: sums 0, 3, 6, 7
    src[1, 2] = -1.0                                                           # s2 = 0 exactly at the edge of the clamp, frame 1 only
    got, _ = _check_moments(src)
    assert (got[:, [0, 3, 6, 7]] == 0).all() and (got[1, [2, 5, 8]] == 0).all() and (got[0, [2, 5, 8]] > 0).all() and (got[:, [1, 4]] > 0).all()
    src[:] = 7.0                                                               # everything clamps to 1: the sums count the pixels, exactly
    assert (ops.color_moments(src).cpu().numpy() == 16 * 24).all()


@pytest.mark.parametrize("form", ["nhwc-ld3", "nhwc-ld8", "nchw", "nchw-odd-view", "f32-nchw"])
def test_moments_nan_and_inf(form):
    src = FORMS[form](2, 16, 24, False)
    want = R.sums_f64(src)
    src[1, 0, 15, 23] = float("nan")                                           # channel 0 of the last pixel of frame 1
    got = ops.color_moments(src).cpu().numpy()
    bound = (R.moments_depth(16, 24) + 3) * U * want
    assert np.isnan(got[1, [0, 3, 6, 7]]).all() and (np.abs(got - want) <= bound)[1, [1, 2, 4, 5, 8]].all() and (np.abs(got - want) <= bound)[0].all()
    src[1, 0, 15, 23] = float("inf")                                           # +-Inf are outside [-1, 1] like any other value: they clamp to 1 / 0
    src[0, 1, 0, 0] = float("-inf")
    got, want = ops.color_moments(src).cpu().numpy(), R.sums_f64(src)
    assert np.isfinite(got).all() and (np.abs(got - want) <= (R.moments_depth(16, 24) + 3) * U * want).all()
    _check_moments(FORMS[form](2, 5, 7, False))


# ---- apply
def _coef(B, seed, scale=1.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 12, generator=g) * scale).float().to(DEV)           # every row its own; many y below 0 and above 1


def _check_apply(src, coef, out=None, dtype=torch.uint8):
    got = ops.color_apply(src, coef, out, dtype=dtype)
    torch.cuda.synchronize()
    want = R.apply_ref(src, coef, dtype == torch.uint8)
    g = got.cpu().numpy()
    assert g.dtype == want.dtype and g.shape == want.shape
    same = (g == want) | (np.isnan(g) & np.isnan(want)) if dtype == torch.float32 else g == want
    assert same.all(), f"{int((~same).sum())} of {want.size} differ"
    return got, want


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32], ids=["u8", "f32"])
@pytest.mark.parametrize("size", [(3, 5, 7), (3, 16, 16)], ids=["3x5x7", "3x16x16"])
@pytest.mark.parametrize("form", list(FORMS))
def test_apply_bit_for_bit(form, size, dtype):
    src = FORMS[form](*size, True)                                             # NaN and +-Inf among the values
    got, want = _check_apply(src, _coef(3, 11), dtype=dtype)
    nan = torch.isnan(src).any(1).cpu().numpy()                                # a NaN in any channel of a pixel reaches its three outputs
    assert nan.any()
    if dtype == torch.uint8:
        assert (want[nan] == 0).all() and len(np.unique(want)) > 20 and (want == 0).any() and (want == 255).any()
    else:
        assert np.isnan(want.transpose(0, 2, 3, 1)[nan]).all() and not np.isnan(want.transpose(0, 2, 3, 1)[~nan]).any()
        assert (want == 0).any() and (want == 1).any()
    # one row of coefficients per frame: frame 0's row on every frame gives something else
    first = _coef(3, 11)[:1].expand(3, 12).contiguous()
    other = R.apply_ref(src, first, dtype == torch.uint8)
    assert np.array_equal(other[0], want[0], equal_nan=True) and not np.array_equal(other[1], want[1], equal_nan=True)


def test_apply_identity_is_the_fp32_chain_of_frames_u8():
    import frames_ref
    x = frames_ref.all_fp16()
    planes = torch.stack([x, x, x]).view(1, 3, 256, 256).to(DEV)
    ident = torch.tensor([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], dtype=torch.float32, device=DEV)
    got, _ = _check_apply(planes, ident)
    assert torch.equal(got, ops.frames_u8(planes, f32_math=True))


def _window(B, H, W, pitch_extra=11):
    """A (B, H, W, 3) window at byte offset (2, 10) of every frame of a sentinel-filled canvas with a wider, odd row pitch."""
    P = (W * 3 + 10 + pitch_extra) | 1
    canvas = torch.full((B, H + 5, P), SENTINEL, device=DEV, dtype=torch.uint8)
    return canvas, canvas.as_strided((B, H, W, 3), ((H + 5) * P, P, 3, 1), 2 * P + 10)


@pytest.mark.parametrize("size", [(3, 5, 7), (3, 16, 16)], ids=["3x5x7", "3x16x16"])
@pytest.mark.parametrize("form", ["nhwc-ld3", "nhwc-ld8", "nchw"])
def test_apply_into_a_window_of_a_canvas(form, size):
    B, H, W = size
    src = FORMS[form](*size, True)
    canvas, out = _window(B, H, W)
    got, want = _check_apply(src, _coef(B, 12), out)
    assert got.data_ptr() == out.data_ptr()
    c = canvas.cpu()
    inside = torch.zeros_like(c, dtype=torch.bool)
    inside[:, 2:2 + H, 10:10 + W * 3] = True
    assert (c[~inside] == SENTINEL).all()                                      # nothing outside the B H rows of 3 W bytes
    # the float destination inside a larger NCHW tensor: the elements around the frame stay
    big = torch.full((B, 4, H + 2, W + 3), -7.0, device=DEV)
    view = big[:, 1:, 1:1 + H, 2:2 + W]
    _check_apply(src, _coef(B, 12), view, dtype=torch.float32)
    keep = torch.ones_like(big, dtype=torch.bool)
    keep[:, 1:, 1:1 + H, 2:2 + W] = False
    assert (big[keep] == -7.0).all()
    # ... and a channels-last float destination
    nhwc = torch.full((B, H, W, 3), -7.0, device=DEV)
    _check_apply(src, _coef(B, 12), nhwc.permute(0, 3, 1, 2), dtype=torch.float32)


@pytest.mark.parametrize("form,dtype", [("nhwc-ld3", torch.uint8), ("nchw", torch.float32)])
def test_apply_past_one_grid_round(form, dtype):
    """33 frames of 256 x 256: 540 672 groups of 4 pixels, more than the 2048 x 256 threads of the capped grid: the grid-stride loop runs."""
    B = 33
    src = FORMS[form](B, 256, 256, False)
    coef = _coef(B, 13, scale=0.8)
    if dtype == torch.uint8:
        canvas, out = _window(B, 256, 256)
        a = ops.color_apply(src, coef, out).clone()
        canvas.fill_(SENTINEL)
        got, _ = _check_apply(src, coef, out)
        assert torch.equal(a, got)                                             # two calls give the same bits
        assert (canvas[:, :2] == SENTINEL).all() and (canvas[:, 258:] == SENTINEL).all() and (canvas[:, :, :10] == SENTINEL).all() and (canvas[:, :, 778:] == SENTINEL).all()
    else:
        _check_apply(src, coef, dtype=dtype)
    _check_moments(src[:2])


# ---- the refusals
def test_kernels_refuse_bad_arguments():
    B, H, W = 2, 6, 5
    lib = _lib.load()
    src = torch.zeros((B, 3, H, W), device=DEV, dtype=torch.float32)
    ws = torch.full((64,), 3.0, device=DEV)
    out = torch.full((B, 9), 5.0, device=DEV, dtype=torch.float64)
    S, st = src.data_ptr(), ops._st()
    ok = dict(src=S, f32=0, B=B, H=H, W=W, sB=3 * H * W, sC=H * W, sY=W, sX=1, ws=ws.data_ptr(), wsb=256, out=out.data_ptr())
    order = ("src", "f32", "B", "H", "W", "sB", "sC", "sY", "sX", "ws", "wsb", "out")
    for change in (dict(src=0), dict(ws=0), dict(out=0), dict(B=0), dict(H=0), dict(W=-1), dict(B=2 ** 11, H=2 ** 10, W=2 ** 10), dict(f32=2), dict(f32=-1),
                   dict(src=S + 1), dict(src=S + 2, f32=1), dict(ws=ws.data_ptr() + 2), dict(out=out.data_ptr() + 4), dict(wsb=2 * 36 - 1), dict(wsb=0)):
        args = tuple(dict(ok, **change)[k] for k in order) + (st,)
        with pytest.raises(_lib.MdanceHipError, match="md_color_moments"):
            _lib.call("md_color_moments", *args)
        assert lib.md_color_moments(*args) == -1, change                       # MD_ERR_ARG
    torch.cuda.synchronize()
    assert (ws == 3.0).all() and (out == 5.0).all()                            # nothing was launched
    coef = torch.zeros((B, 12), device=DEV)
    dst = torch.full((B, H, W * 3 + 4), SENTINEL, device=DEV, dtype=torch.uint8)
    fdst = torch.full((B, 3, H, W), -7.0, device=DEV)
    dY = W * 3 + 4
    ok = dict(src=S, f32=0, coef=coef.data_ptr(), dst=dst.data_ptr(), df32=0, B=B, H=H, W=W, sB=3 * H * W, sC=H * W, sY=W, sX=1, dB=H * dY, dC=1, dY=dY, dX=3)
    fok = dict(ok, dst=fdst.data_ptr(), df32=1, dB=3 * H * W, dC=H * W, dY=W, dX=1)
    order = ("src", "f32", "coef", "dst", "df32", "B", "H", "W", "sB", "sC", "sY", "sX", "dB", "dC", "dY", "dX")
    bad = [dict(ok, **c) for c in (dict(src=0), dict(coef=0), dict(dst=0), dict(B=0), dict(H=-1), dict(W=0), dict(B=2 ** 11, H=2 ** 10, W=2 ** 10, dB=2 ** 40, dY=2 ** 20),
                                   dict(f32=2), dict(df32=2), dict(df32=-1), dict(src=S + 1), dict(src=S + 2, f32=1), dict(coef=coef.data_ptr() + 2), dict(dC=2), dict(dX=4),
                                   dict(dY=W * 3 - 1), dict(dY=0), dict(dY=-dY), dict(dB=(H - 1) * dY + W * 3 - 1), dict(dB=0))]
    bad += [dict(fok, **c) for c in (dict(dst=fdst.data_ptr() + 2), dict(dB=0), dict(dC=0), dict(dY=-W), dict(dX=0))]
    for a in bad:
        args = tuple(a[k] for k in order) + (st,)
        with pytest.raises(_lib.MdanceHipError, match="md_color_apply"):
            _lib.call("md_color_apply", *args)
        assert lib.md_color_apply(*args) == -1, a
        assert lib.md_last_error().decode().startswith("md_color_apply"), a
    torch.cuda.synchronize()
    assert (dst == SENTINEL).all() and (fdst == -7.0).all()
    for good in (ok, fok, dict(ok, dst=dst.data_ptr() + 1, dB=H * dY - 1), dict(ok, src=S + 2), dict(ok, f32=1)):
        _lib.call("md_color_apply", *(good[k] for k in order), st)
    torch.cuda.synchronize()
    assert (dst[:, :, W * 3 + 1:] == SENTINEL).all()


def test_operators_refuse_bad_arguments():
    src = torch.zeros((2, 3, 6, 5), device=DEV, dtype=F16)
    coef = torch.zeros((2, 12), device=DEV)
    out = torch.full((2, 6, 5, 3), SENTINEL, device=DEV, dtype=torch.uint8)
    wide = torch.full((2, 6, 5, 4), SENTINEL, device=DEV, dtype=torch.uint8)
    fout = torch.full((2, 3, 6, 5), -7.0, device=DEV)
    for who, call in (("color_moments", ops.color_moments), ("color_apply", lambda s, **k: ops.color_apply(s, coef, **k))):
        for bad, msg in ((src.cpu(), "CUDA fp16/fp32"), (src.double(), "CUDA fp16/fp32"), (src[0], r"\(B, 3, H, W\)"), (src[:, :2], r"\(B, 3, H, W\)"),
                         (src.repeat(1, 2, 1, 1)[:, :4], r"\(B, 3, H, W\)"), (src[:, :, :0], "no empty")):
            with pytest.raises(_lib.MdanceHipError, match=f"{who}: src must be .*{msg}"):
                call(bad)
    for call, msg in ((lambda: ops.color_moments(src, torch.zeros((2, 9), device=DEV)), "float64"), (lambda: ops.color_moments(src, torch.zeros((3, 9), device=DEV, dtype=torch.float64)), "out must be"),
                      (lambda: ops.color_moments(src, torch.zeros((2, 18), device=DEV, dtype=torch.float64)[:, ::2]), "out must be"),
                      (lambda: ops.color_apply(src, coef.double()), "float32"), (lambda: ops.color_apply(src, coef[:1]), "coef must be"), (lambda: ops.color_apply(src, coef.cpu()), "GPU"),
                      (lambda: ops.color_apply(src, torch.zeros((2, 24), device=DEV)[:, ::2]), "coef must be"), (lambda: ops.color_apply(src, coef, dtype=torch.float16), "dtype must be"),
                      (lambda: ops.color_apply(src, coef, out.cpu()), "CUDA uint8"), (lambda: ops.color_apply(src, coef, fout), "CUDA uint8"),
                      (lambda: ops.color_apply(src, coef, out[:, :5]), "out must be"), (lambda: ops.color_apply(src, coef, wide[..., :3]), "packed pixels"),
                      (lambda: ops.color_apply(src, coef, out, dtype=torch.float32), "CUDA float32"), (lambda: ops.color_apply(src, coef, fout[:, :, :5], dtype=torch.float32), "out must be"),
                      (lambda: ops.color_apply(src, coef, fout[:, :1].expand(2, 3, 6, 5), dtype=torch.float32), "expanded")):
        with pytest.raises(_lib.MdanceHipError, match=msg):
            call()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (wide == SENTINEL).all() and (fout == -7.0).all()
    _lib.PROFILER.start()
    try:
        ops.color_moments(src)
        ops.color_apply(src, coef, out)
        ops.color_apply(src, coef, fout, dtype=torch.float32)
    finally:
        _lib.PROFILER.stop()
    torch.cuda.synchronize()
    recs = _lib.PROFILER.summary()
    n = 2 * 3 * 6 * 5
    assert sorted(r["bytes"] for r in recs.values()) == sorted([2.0 * n + 144, 3.0 * n + 96, 6.0 * n + 96]) and len(recs) == 3


# ---- the chain through the pipeline
CHANS = (64, 64, 64, 64)
W, H, F_ = 128, 96, 3


@pytest.fixture(scope="module")
def pipe():
    vae = AutoencoderKL(block_out_channels=CHANS, sample_size=128)
    vae.load_state_dict(synth_state_dict({k: tuple(v.shape) for k, v in vae.state_dict().items()}, seed=77), strict=True)
    ref, den, _, _ = build_models(keep_state_dicts=False)
    p = M.MikuDanceVideoPipeline(vae=vae.half().to(DEV).eval(), image_encoder=FakeCLIP(), reference_unet=ref, denoising_unet=den,
                                 scheduler=M.DDIMScheduler(**SCHED_KWARGS))
    p.to("cuda", dtype=F16)
    p.vae_batch = 2
    return p


@pytest.fixture(scope="module")
def clip():
    from PIL import Image
    rng = np.random.default_rng(9)
    img = lambda: Image.fromarray(rng.integers(0, 255, (120, 144, 3), dtype=np.uint8))
    return (img(), img(), [img() for _ in range(F_)], [img() for _ in range(F_)], [img() for _ in range(F_)], rng.uniform(-0.03, 0.03, (F_, 2, H // 8, W // 8)))


@pytest.fixture(scope="module")
def plain(pipe, clip):
    """The call without the keyword, float and bytes, and the latents it decodes (captured once, shared)."""
    seen = []
    decode = pipe.decode_latents
    pipe.decode_latents = lambda latents, output_type=None: (seen.append(latents.clone()), decode(latents, output_type))[1]
    try:
        f = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7)).videos
        u = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), output_type="uint8").videos
    finally:
        del pipe.decode_latents
    assert torch.equal(seen[0], seen[1])
    return f, u, seen[0]


def test_color_match_none_is_the_call_as_it_was(pipe, clip, plain):
    f, u, _ = plain
    assert torch.equal(pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), color_match=None).videos, f)
    assert torch.equal(pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), output_type="uint8", color_match=None).videos, u)
    assert torch.equal(u, torch.from_numpy((f * 255).numpy().astype(np.uint8)).permute(0, 2, 3, 4, 1))


@pytest.mark.parametrize("scope", CM.SCOPES)
@pytest.mark.parametrize("mode", CM.MODES)
def test_pipeline_bytes_are_the_restatement_on_the_device_sums(pipe, clip, plain, mode, scope):
    f, u, latents = plain
    kw = dict(color_match=mode, color_match_scope=scope, color_match_strength=0.9)
    got = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), output_type="uint8", **kw).videos
    maps = pipe.last_color_match
    flt = pipe(*clip, W, H, F_, 2, 3.5, generator=torch.manual_seed(7), **kw).videos
    assert got.dtype == torch.uint8 and not got.is_cuda and tuple(got.shape) == (1, F_, H, W, 3) and len(torch.unique(got)) > 50
    assert torch.equal(got, torch.from_numpy((flt * 255).numpy().astype(np.uint8)).permute(0, 2, 3, 4, 1)) and not torch.equal(got, u)
    # the same decode by hand: the views, the device's sums read back, the host solve, the numpy restatement
    z = (1 / 0.18215 * latents).permute(0, 2, 1, 3, 4).reshape(F_, 4, H // 8, W // 8).to(F16)
    views = [pipe.vae.decode_image_view(z[i:i + 2]) for i in range(0, F_, 2)]
    sums = np.concatenate([ops.color_moments(v).cpu().numpy() for v in views])
    from mikudance_amd.pipeline_mikudance import _pil_to_tensor
    target = CM.moments_of_image(_pil_to_tensor(clip[0], H, W, normalize=False)[0].permute(1, 2, 0).numpy())
    if scope == "clip":
        want_maps = [CM.transform(sums.sum(0), H * W * F_, *target, mode, 0.9)] * F_
    else:
        want_maps = [CM.transform(s, H * W, *target, mode, 0.9) for s in sums]
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] for a, b in zip(maps, want_maps)) and len(maps) == F_
    coef = CM.coefficients(want_maps)
    want = np.concatenate([R.apply_ref(v, coef[i:i + 2], True) for v, i in zip(views, range(0, F_, 2))])
    assert np.array_equal(got[0].numpy(), want)
