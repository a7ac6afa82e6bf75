"""GPU: shifted-tile spatial self-attention on the MI355X -- md_token_tile_f16 bitwise against the torch definition in both directions at the
smallest shapes where it can go wrong (pad rows +0, payloads a copy must keep, guard rows, repeatable bits, every refusal), one
TransformerBlock in every reference mode against tests/tile_ref.py, and the whole loop at reduced width against the restated loop.

Bounds.  Block: the tiled block's rel-L2 against its restatement is at most 1.5 x the rel-L2 of the SAME block with tile=None against its
restatement, measured in the same test (the yardstick is the untiled path's own error; 1.5 because a softmax over a quarter of the keys rounds
differently and both errors are a few 1e-4).  Loop: rel-L2 <= 3e-2 and cosine >= 0.999, the project's loop bound, and at most 2 x the plain
loop's error on the same clip.  profiles/tile_attention_tests.log holds every printed figure of a run on an MI355X."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import mikudance_amd as M  # noqa: E402
from mikudance_amd import _lib, blocks, ops  # noqa: E402
from mikudance_amd.selftest import SCHED_KWARGS, build_models, cosine, rel_l2  # noqa: E402
from mikudance_amd.synth import synth_inputs  # noqa: E402

import dpmpp_ref as R  # noqa: E402
import tile_ref as TR  # noqa: E402
import todo_ref as T  # noqa: E402

DEV = torch.device("cuda:0")
G = 3.5
SENTINEL = 12345.0
GUARD = 64                                                                 # rows in front of and behind the output that must stay untouched
# bit patterns a value-preserving copy must keep: -0, the smallest subnormal, 65504, a quiet NaN with a payload, a signalling NaN
PAYLOADS = [-32768, 1, 0x7BFF, 0x7E2A, 0x7D01]


# ---- 1. the kernel
def _tokens(B, Hh, Ww, C, seed):
    x = torch.randn((B * Hh * Ww, C), generator=torch.Generator().manual_seed(seed)).half()
    bits = x.view(torch.int16)
    for i, p in enumerate(PAYLOADS):                                       # fixed positions: rows 0, 7, 14, ..., channels 0, 3, 6, ...
        bits[(7 * i) % x.shape[0], (3 * i) % C] = p
    return x


def _bits(t):
    return t.contiguous().view(torch.int16)


def _call(x, rows_out, B, Hh, Ww, C, t, shift, tile_stride, inverse):
    """One call into the middle of a sentinel-filled buffer of GUARD + rows_out + GUARD rows -> the whole buffer on the host."""
    y = torch.full((GUARD + rows_out + GUARD, C), SENTINEL, dtype=torch.float16, device=DEV)
    _lib.call("md_token_tile_f16", x.data_ptr(), y[GUARD:].data_ptr(), B, Hh, Ww, C, t, shift[0], shift[1], tile_stride, inverse, ops._st())
    torch.cuda.synchronize()
    return y.cpu()


KERNEL_CASES = [(2, 8, 8, 64, 2, None, [(0, 0), (1, 3), (7, 7)]), (3, 6, 10, 320, 2, 15, [(0, 0), (2, 7)]), (3, 6, 10, 320, 2, 16, [(0, 0), (5, 9)]),
                (1, 8, 8, 8, 4, 8, [(0, 0), (3, 1)]), (2, 4, 4, 1280, 2, None, [(0, 0), (1, 1)]), (1, 16, 16, 64, 8, None, [(0, 0), (9, 4)])]


@pytest.mark.parametrize("B,Hh,Ww,C,t,stride,shifts", KERNEL_CASES)
def test_kernel_is_the_torch_definition_both_ways(B, Hh, Ww, C, t, stride, shifts):
    x = _tokens(B, Hh, Ww, C, seed=B + Hh * Ww + t)
    Lt = (Hh // t) * (Ww // t)
    stride = stride or Lt
    nt, rows_t, rows_f = B * t * t, B * t * t * stride, B * Hh * Ww
    xd = x.to(DEV)
    for shift in shifts:
        # forward
        y = _call(xd, rows_t, B, Hh, Ww, C, t, shift, stride, 0)
        body = y[GUARD:GUARD + rows_t].view(nt, stride, C)
        want = TR.tile(x.view(torch.int16), B, Hh, Ww, t, shift)           # the definition on the bit patterns
        assert torch.equal(_bits(body[:, :Lt]), want)
        pad = body[:, Lt:]
        assert pad.numel() == nt * (stride - Lt) * C and (_bits(pad) == 0).all()          # exact +0, sign bit included
        assert (y[:GUARD] == SENTINEL).all() and (y[GUARD + rows_t:] == SENTINEL).all()    # guard rows before and after
        assert torch.equal(_bits(y), _bits(_call(xd, rows_t, B, Hh, Ww, C, t, shift, stride, 0)))      # the same bits again
        # inverse: the exact inverse permutation, and the pad rows are never read
        tiles = body.clone()
        tiles[:, Lt:] = float("nan")
        z = _call(tiles.reshape(rows_t, C).to(DEV), rows_f, B, Hh, Ww, C, t, shift, stride, 1)
        assert torch.equal(_bits(z[GUARD:GUARD + rows_f]), _bits(x))
        assert (z[:GUARD] == SENTINEL).all() and (z[GUARD + rows_f:] == SENTINEL).all()
        assert torch.equal(_bits(z), _bits(_call(tiles.reshape(rows_t, C).to(DEV), rows_f, B, Hh, Ww, C, t, shift, stride, 1)))
        # the wrappers
        out, lt, st = ops.token_tile(xd, B, Hh, Ww, t, shift, tile_stride=stride)
        back = ops.token_untile(out, B, Hh, Ww, t, shift, tile_stride=stride)
        torch.cuda.synchronize()
        assert (lt, st) == (Lt, stride) and torch.equal(_bits(out.cpu()), _bits(body.reshape(rows_t, C))) and torch.equal(_bits(back.cpu()), _bits(x))
    print(f"\nTILE_KERNEL B{B} {Hh}x{Ww} C{C} t{t} stride {stride} shifts {shifts}: bitwise both ways, pad +0, guards untouched")


def test_kernel_covers_more_than_one_grid_round():
    """B * Hh * Ww * C / 8 items beyond 2048 workgroups of 256 lanes: the grid-stride loop runs more than once, in both directions."""
    B, Hh, Ww, C, t, shift = 2, 96, 96, 320, 2, (13, 40)
    x = torch.randn((B * Hh * Ww, C), generator=torch.Generator().manual_seed(1)).half()
    assert B * Hh * Ww * (C // 8) > 2048 * 256
    y = _call(x.to(DEV), B * Hh * Ww, B, Hh, Ww, C, t, shift, 48 * 48, 0)
    body = y[GUARD:GUARD + B * Hh * Ww]
    assert torch.equal(body.view(B * 4, 48 * 48, C), TR.tile(x, B, Hh, Ww, t, shift)) and (y[:GUARD] == SENTINEL).all() and (y[-GUARD:] == SENTINEL).all()
    z = _call(body.to(DEV), B * Hh * Ww, B, Hh, Ww, C, t, shift, 48 * 48, 1)
    assert torch.equal(z[GUARD:-GUARD], x) and (z[:GUARD] == SENTINEL).all() and (z[-GUARD:] == SENTINEL).all()


def test_bad_arguments_raise_and_leave_y_alone():
    B, Hh, Ww, C, t = 3, 6, 10, 320, 2
    x = _tokens(B, Hh, Ww, C, 3).to(DEV)
    rows = B * 4 * 16
    y = torch.full((rows + GUARD, C), SENTINEL, dtype=torch.float16, device=DEV)
    X, Y = x.data_ptr(), y.data_ptr()
    call = lambda xp=X, yp=Y, b=B, hh=Hh, ww=Ww, c=C, t=t, sy=0, sx=0, stride=16, inv=0: _lib.call("md_token_tile_f16", xp, yp, b, hh, ww, c, t, sy, sx,
                                                                                                 stride, inv, ops._st())
    cases = (dict(xp=0), dict(yp=0), dict(xp=X + 2), dict(yp=Y + 8), dict(c=324), dict(c=4), dict(c=0), dict(c=-8), dict(t=1), dict(t=9), dict(t=0),
             dict(t=-2), dict(t=4), dict(t=3), dict(t=5), dict(hh=7), dict(ww=9), dict(sy=-1), dict(sy=6), dict(sx=-1), dict(sx=10), dict(stride=14),
             dict(stride=0), dict(stride=-16), dict(yp=X), dict(yp=X + 16 * C), dict(xp=Y + 2 * C * 8), dict(b=0), dict(inv=2), dict(inv=-1),
             dict(b=1 << 30, hh=1 << 14, ww=1 << 14, t=2, stride=1 << 26), dict(inv=1, yp=X + 16 * C), dict(inv=1, stride=14))
    for kw in cases:
        with pytest.raises(_lib.MdanceHipError):
            call(**kw)
        torch.cuda.synchronize()
        assert (y == SENTINEL).all(), kw                                   # nothing was launched
    call()
    torch.cuda.synchronize()
    assert not (y[:rows] == SENTINEL).all(1).any() and (y[rows:] == SENTINEL).all()
    # the wrappers' own refusals
    with pytest.raises(_lib.MdanceHipError, match="no CPU path"):
        ops.token_tile(x.cpu(), B, Hh, Ww, 2)
    with pytest.raises(_lib.MdanceHipError, match="contiguous"):
        ops.token_tile(x, B, Hh, Ww + 2, 2)
    with pytest.raises(_lib.MdanceHipError, match="does not divide"):
        ops.token_tile(x, B, Hh, Ww, 4)
    with pytest.raises(_lib.MdanceHipError, match="contiguous"):
        ops.token_untile(x, B, Hh, Ww, 2, tile_stride=16)
    with pytest.raises(_lib.MdanceHipError):
        ops.token_tile(x.float(), B, Hh, Ww, 2)


# ---- 2. one TransformerBlock(320, 8 heads), 2 frames per clip-half, every reference mode
@pytest.fixture(scope="module")
def untiled():
    """{(Hh, Ww, pool): todo_ref-style runs of the block with tile=None}: the yardstick, computed once per grid."""
    return {}


def _yardstick(untiled, st, Hh, Ww, pool=None):
    key = (Hh, Ww, pool)
    if key not in untiled:
        untiled[key] = TR.block_runs(st, None, kv_pool=pool)
    return untiled[key]


@pytest.mark.parametrize("Hh,Ww,shift,pool", [(8, 8, (0, 0), None), (8, 8, (2, 6), None), (6, 10, (0, 0), None), (6, 10, (1, 3), None), (8, 8, (2, 2), (2, "mean"))])
def test_block_matches_restatement_in_every_reference_mode(untiled, Hh, Ww, shift, pool):
    st = T.block_setup(320, 64, Hh, Ww, 2, DEV)
    plain = _yardstick(untiled, st, Hh, Ww, pool)
    runs = TR.block_runs(st, (2, shift), kv_pool=pool)
    torch.cuda.synchronize()
    for case, (got, want) in runs.items():
        r, c, r0 = rel_l2(got, want), cosine(got, want), rel_l2(*plain[case])
        if case == "write-bank":
            assert torch.equal(got, plain[case][0])                        # the bank written is bitwise the untiled one
            continue
        print(f"\nTILE_BLOCK {Hh}x{Ww} t2 shift {shift} pool {pool} {case}: rel_l2 {r:.3e} cos {c:.7f} (tile=None, same block {r0:.3e}, ratio {r / r0:.2f}; "
              f"restated untiled vs tiled {rel_l2(plain[case][1], want):.3e})")
        assert torch.isfinite(got).all() and r <= 1.5 * r0, (case, r, r0)
        assert rel_l2(got, plain[case][0]) > 10 * r0                       # the field is not ignored
    # an unselected block is bitwise the call without the field
    h = st.x.reshape(-1, 320).to(DEV)
    other = blocks.TransformerBlock(320, 64)
    with torch.no_grad():
        a = st.blk(h.clone(), 4, Hh * Ww, st.cross)
        b = st.blk(h.clone(), 4, Hh * Ww, st.cross, sa=blocks.SelfAttnCall(tile={other: (2, shift)}), grid=(Hh, Ww))
        c = st.blk(h.clone(), 4, Hh * Ww, st.cross, sa=blocks.SelfAttnCall(tile=None))
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("shift", [(0, 0), (3, 5)])
def test_seg_block_blurs_then_tiles(untiled, shift):
    st = T.block_setup(320, 64, 8, 8, 2, DEV)
    got0, want0 = TR.block_runs(st, None, sigma=1.5)["seg"]
    got, want = TR.block_runs(st, (2, shift), sigma=1.5)["seg"]
    torch.cuda.synchronize()
    r, r0 = rel_l2(got, want), rel_l2(got0, want0)
    print(f"\nTILE_BLOCK 8x8 t2 shift {shift} seg sigma 1.5: rel_l2 {r:.3e} (tile=None, same block {r0:.3e}, ratio {r / r0:.2f})")
    assert torch.isfinite(got).all() and r <= 1.5 * r0 and rel_l2(got, got0) > 10 * r0, (r, r0)


# ---- 3. the loop on the small models, 16 x 16 latents, 4 frames, 4 steps
@pytest.fixture(scope="module")
def small():
    return build_models()


@pytest.fixture(scope="module")
def clip():
    """The inputs, and per sampler the plain loop's result on the device, the restated one and the error between them, shared by the loop tests."""
    return {}


STEPS = 4
WINDOWS2 = dict(context_frames=3, context_stride=1, context_overlap=1)     # 4 frames: [0, 1, 2] and [2, 3, 0]
PAG0 = dict(pag_scale=3.0, pag_applied_layers=("down_blocks.0",))


def _make(sampler):
    return M.DPMSolverMultistepScheduler(**SCHED_KWARGS) if sampler == "2m" else M.DDIMScheduler(**SCHED_KWARGS)


def _restated(sampler):
    return R.Restated(2, "dpmsolver++", "midpoint") if sampler == "2m" else None


def _loop(models, inputs, sampler="ddim", two_queues=False, **kw):
    ref, den, _, _ = models
    pipe = M.MikuDanceVideoPipeline(None, None, ref, den, _make(sampler))
    pipe.two_queues = two_queues
    out = pipe.denoise(*(t.half().to(DEV) for t in inputs), STEPS, G, **kw)
    torch.cuda.synchronize()
    return out.float().cpu()


def _plain(small, clip, sampler):
    if "inputs" not in clip:
        clip["inputs"] = tuple(t.half().float() for t in synth_inputs(4, 16, 16, ctx_len=5, ctx_dim=64, seed=504))
    if sampler not in clip:
        _, _, ref_sd, den_sd = small
        got = _loop(small, clip["inputs"], sampler)
        with torch.no_grad():
            want = TR.denoise_loop(ref_sd, den_sd, *clip["inputs"], STEPS, tile_attention=1, guidance_scale=G, scheduler=_restated(sampler))
        clip[sampler] = dict(got=got, want=want, err=rel_l2(got, want))
    return clip[sampler]


def test_factor_one_is_bitwise_the_plain_loop_and_a_factor_is_not_ignored(small, clip, monkeypatch):
    c = _plain(small, clip, "ddim")
    names, real = [], _lib.call

    def spy(name, *a, **k):
        names.append(name)
        return real(name, *a, **k)

    monkeypatch.setattr(_lib, "call", spy)
    a = _loop(small, clip["inputs"])
    seen_a = list(names)
    for kw in (dict(tile_attention=1), dict(tile_attention=(1, 1, 1, 1), tile_attention_shift="none")):
        del names[:]
        b = _loop(small, clip["inputs"], **kw)
        assert torch.equal(a, b) and torch.equal(a, c["got"]) and seen_a == names      # launch for launch
    assert "md_token_tile_f16" not in seen_a
    del names[:]
    d = _loop(small, clip["inputs"], tile_attention=(2,))
    assert names.count("md_token_tile_f16") == (2 * 3 + 3 * 3) * STEPS     # level 0 under CFG: 2 down + 3 up blocks, tile q / tile kv / untile each
    e = rel_l2(d, a)
    print(f"\nTILE_EFFECT rel_l2(tile_attention (2,), plain) {e:.3e}")
    assert not torch.equal(d, a) and e > 3e-2, e                           # the keyword is not silently ignored


VARIANTS = {"base": {}, "kv2": dict(kv_downsample=2), "pag": PAG0, "two-windows": WINDOWS2, "two-queues": dict(two_queues=True)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("sampler", ["ddim", "2m"])
def test_loop_vs_restatement_reduced_width(small, clip, sampler, variant):
    _, _, ref_sd, den_sd = small
    kw = dict(VARIANTS[variant])
    tq = kw.pop("two_queues", False)
    rkw = dict(guidance_scale=G, scheduler=_restated(sampler))
    if "kv_downsample" in kw:
        rkw.update(kv_downsample=kw["kv_downsample"])
    if "pag_scale" in kw:
        rkw.update(pag_scale=kw["pag_scale"], pag_layers=kw["pag_applied_layers"])
    if "context_frames" in kw:
        rkw.update(kw)
    plain_err = _plain(small, clip, sampler)["err"]
    if variant not in ("base", "two-queues"):                              # the plain loop's error on the same clip under the same keywords
        with torch.no_grad():
            plain_want = TR.denoise_loop(ref_sd, den_sd, *clip["inputs"], STEPS, tile_attention=1, **dict(rkw, scheduler=_restated(sampler)))
        plain_err = rel_l2(_loop(small, clip["inputs"], sampler, **kw), plain_want)
    with torch.no_grad():
        want = TR.denoise_loop(ref_sd, den_sd, *clip["inputs"], STEPS, tile_attention=(2,), tile_attention_shift="cycle", **rkw)
    out = _loop(small, clip["inputs"], sampler, two_queues=tq, tile_attention=(2,), tile_attention_shift="cycle", **kw)
    e, cs = rel_l2(out, want), cosine(out, want)
    print(f"\nTILE_LOOP {sampler} {variant} {STEPS} steps rel_l2 {e:.3e} cos {cs:.7f} (plain loop, same clip and keywords {plain_err:.3e}, ratio {e / plain_err:.2f})")
    assert torch.isfinite(out).all() and e <= 3e-2 and cs >= 0.999, (e, cs)
    assert e <= 2.0 * plain_err, (e, plain_err)
