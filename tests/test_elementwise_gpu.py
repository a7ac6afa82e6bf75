"""GPU: the kernels of mikudance_amd/csrc/elementwise.hip in every form the package calls them and past one grid round, on the MI355X.
pack / unpack / concat / window_accumulate are held to EXACT equality with tests/elementwise_ref.py (and with tests/fake_ops.py, whose
emulations the CPU suite runs the pipeline on); the DDIM and DPM-Solver++ step kernels under their four guides to float64 under the project's step error model,
|got - want| <= U16 |want| + 2e-6 scale + 2^-24 (tests/test_apg_gpu.py section 2), at small sizes through the plain entries and at
1 048 820 elements / 1 048 815 pixels, where every thread of the first 244 / 239 runs its grid-stride loop twice, with the elements of the
second round asserted on their own.  Section 6 takes UniPC's four past the round as well and holds all three samplers to the plain entry's
bits at pag_scale == 0.  tests/test_elementwise_ref_cpu.py shows that a correct fp32 evaluation passes the same bound on the same
inputs.  profiles/elementwise_tests.log holds every printed figure of a run on an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mikudance_amd import _lib, ops  # noqa: E402

import elementwise_ref as E  # noqa: E402
import fake_ops  # noqa: E402
import test_unipc_gpu as U  # noqa: E402  (the float64 statement and bounds of the UniPC entries: _case, _row, _kernel, _check)

DEV = torch.device("cuda:0")
put = lambda t: t.to(DEV)


# ---- 1. pack
def _pack(row, dt, b, f, hin, win, ho, wo, seed):
    """One pack call of form `row` on the device against the reference and the emulation -> the device result on the host."""
    _, src = E.strided_tensor(row["layout"], row["ctot"], b, f, hin, win, E.DTYPES[dt], torch.Generator().manual_seed(seed))
    n, F_, strides = E.call_strides(row["layout"], src)
    whole_d, src_d = E.strided_tensor(row["layout"], row["ctot"], b, f, hin, win, E.DTYPES[dt], 0.0)
    whole_d = whole_d.to(DEV)
    src_d = whole_d.as_strided(src.shape, src.stride(), src.storage_offset())      # the same view of the device copy
    src_d.copy_(src)
    got = ops.pack_nhwc(src_d, n, F_, strides, row["c_begin"], row["c_count"], row["cpad"], ho, wo, hin=hin, win=win).cpu()
    want = E.pack_reference(src, row["layout"], row["c_begin"], row["c_count"], row["cpad"], ho, wo)
    tag = (row["site"], dt, b, f, hin, win, ho, wo)
    assert got.shape == want.shape and torch.equal(E.bits(got), E.bits(want)), tag
    assert not E.bits(got[..., row["c_count"]:]).any(), tag                # padding channels exactly +0
    emu = fake_ops.pack_nhwc(src, n, F_, strides, row["c_begin"], row["c_count"], row["cpad"], ho, wo, hin=hin, win=win)
    assert torch.equal(E.bits(got), E.bits(emu)), tag
    return got


@pytest.mark.parametrize("row", E.PACK_FORMS, ids=[r["site"] for r in E.PACK_FORMS])
def test_pack_every_form_is_exact(row):
    h, w = E.ODD
    for dt in row["dtypes"]:
        _pack(row, dt, 2, 3, h, w, h, w, seed=11)
    print(f"\nELEMENTWISE_PACK {row['site']} {h} x {w}: exact in {len(row['dtypes'])} source types")


RESIZE_FORMS = [r for r in E.PACK_FORMS if r["resize"]]


@pytest.mark.parametrize("hin,win,ho,wo", E.RESIZE_CASES)
@pytest.mark.parametrize("row", RESIZE_FORMS, ids=[r["site"] for r in RESIZE_FORMS])
def test_pack_nearest_resize_is_exact(row, hin, win, ho, wo):
    """Shrinking, enlarging, the identity and H, W scaled differently, through the channel sub-range forms and the channel-innermost one."""
    for dt in row["dtypes"]:
        _pack(row, dt, 2, 3, hin, win, ho, wo, seed=hin * 100 + wo)
    print(f"\nELEMENTWISE_PACK {row['site']} {hin} x {win} -> {ho} x {wo}: exact in {len(row['dtypes'])} source types")


def test_pack_frames_of_several_clips():
    """F > 1 with sB != 0: n % F and n / F both at work (the unet_3d_mix form; 4 clips of 3 frames, n = 12)."""
    row = next(r for r in E.PACK_FORMS if r["layout"] == "NCFHW")
    for dt in row["dtypes"]:
        got = _pack(row, dt, 4, 3, 7, 5, 7, 5, seed=12)
        assert got.shape[0] == 12 and not torch.equal(got[1], got[3]) and not torch.equal(got[0], got[3])


def test_pack_past_one_grid_round():
    """n = 3, 105 x 105, Cpad = 64: 2 116 800 elements against 8192 x 256 threads; fp32 source, a channel sub-range."""
    row = next(r for r in E.PACK_FORMS if r["site"] == "unet_2d_mix.py:forward/sample")
    got = _pack(row, "f32", 3, 1, 105, 105, 105, 105, seed=13)
    assert got.numel() == 2116800 > 8192 * 256
    got = _pack(next(r for r in E.PACK_FORMS if r["layout"] == "HALVES"), "f16", 1, 2, 105, 105, 105, 105, seed=14)      # n = 4, F = 2, sB = 0
    assert got.numel() > 8192 * 256 and torch.equal(got[:2], got[2:])
    print("\nELEMENTWISE_PACK past one grid round: 2 116 800 (NCHW fp32) and 2 822 400 (both halves of packed latents) elements exact")


# ---- 2. unpack
def _unpack(row, dt, b, f, h, w, c, ldc, seed):
    layout = row["layout"]
    whole, dst = E.strided_tensor(layout, c, b, f, h, w, E.DTYPES[dt], -7.0)
    n, F_, strides = E.call_strides(layout, dst)
    src = torch.randn((n, h, w, ldc), generator=torch.Generator().manual_seed(seed)).half()
    whole_d = whole.to(DEV)
    dst_d = whole_d.as_strided(dst.shape, dst.stride(), dst.storage_offset())
    ops.unpack_nhwc(src.to(DEV), dst_d, n, F_, strides, c, h, w)
    got = whole_d.cpu()
    E.unpack_reference(src, dst, layout, c)
    tag = (row["site"], dt, b, f, h, w, c, ldc)
    assert torch.equal(got, whole), tag                                    # the view exact, every element around it still the sentinel
    assert (got[..., 0] == -7.0).all() and (got != -7.0).sum() == n * h * w * c, tag
    whole2, dst2 = E.strided_tensor(layout, c, b, f, h, w, E.DTYPES[dt], -7.0)
    fake_ops.unpack_nhwc(src, dst2, n, F_, strides, c, h, w)
    assert torch.equal(got, whole2), tag


@pytest.mark.parametrize("row", E.UNPACK_FORMS, ids=[r["site"] for r in E.UNPACK_FORMS])
def test_unpack_every_form_is_exact(row):
    h, w = E.ODD
    combos = {(row["c_count"], row["cpad"])} | {(c, ldc) for ldc in (4, 64) for c in (3, 4, 8) if c <= ldc}
    for dt in row["dtypes"]:
        for c, ldc in sorted(combos):
            _unpack(row, dt, 2, 3, h, w, c, ldc, seed=c * 100 + ldc)
    print(f"\nELEMENTWISE_UNPACK {row['site']}: exact in {len(row['dtypes'])} destination types, (C, ldc) {sorted(combos)}, sentinel intact")


def test_unpack_past_one_grid_round():
    """3 clips of 3 frames, 243 x 241, C = ldc = 4 (the unet_3d_mix form): 2 108 268 elements against 8192 x 256 threads."""
    row = next(r for r in E.UNPACK_FORMS if r["layout"] == "NCFHW")
    assert 9 * 243 * 241 * 4 > 2097152
    _unpack(row, "f32", 3, 3, 243, 241, 4, 4, seed=15)
    _unpack(row, "f16", 3, 3, 243, 241, 4, 4, seed=16)
    print("\nELEMENTWISE_UNPACK past one grid round: 2 108 268 elements exact in fp32 and fp16, sentinel intact")


@pytest.mark.parametrize("layout", ["NCHW", "NCFHW", "1CFHW"])
def test_pack_unpack_round_trip(layout):
    h, w = E.ODD
    for dt in ("f16", "f32"):
        _, x = E.strided_tensor(layout, 4, 2, 3, h, w, E.DTYPES[dt], torch.Generator().manual_seed(17))
        xd = x.to(DEV)                                                     # contiguous on the device: other strides than on the host
        n, F_, strides = E.call_strides(layout, xd)
        p = ops.pack_nhwc(xd, n, F_, strides, 0, 4, 64, h, w)
        y = torch.full(x.shape, -7.0, dtype=E.DTYPES[dt], device=DEV)
        ops.unpack_nhwc(p, y, n, F_, E.call_strides(layout, y)[2], 4, h, w)
        assert torch.equal(y.cpu(), x.half().to(E.DTYPES[dt])), (layout, dt)


# ---- 3. concat
def _concat(m, ca, cb, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = (torch.randint(-32768, 32768, (m, c), generator=g, dtype=torch.int16).view(torch.float16) for c in (ca, cb))      # any 16 bits
    got = ops.concat_channels(a.to(DEV), b.to(DEV)).cpu()
    assert got.shape == (m, ca + cb) and torch.equal(E.bits(got), E.bits(E.concat_reference(a, b))), (m, ca, cb)
    return got


@pytest.mark.parametrize("m", [1, 7, 257])
@pytest.mark.parametrize("ca,cb", [(8, 8), (64, 128), (320, 640), (1280, 8)])
def test_concat_is_exact(m, ca, cb):
    got = _concat(m, ca, cb, seed=m + ca)
    x = torch.randn((m, ca), generator=torch.Generator().manual_seed(1)).half()
    y = torch.randn((m, cb), generator=torch.Generator().manual_seed(2)).half()
    assert torch.equal(ops.concat_channels(x.to(DEV), y.to(DEV)).cpu(), fake_ops.concat_channels(x, y)) and got.dtype == torch.float16


def test_concat_past_one_grid_round():
    """M = 17 477, 1280 + 640 channels: 4 194 480 half8 vectors against 16384 x 256 threads."""
    assert 17477 * (1280 + 640) // 8 == 4194480 > 16384 * 256
    _concat(17477, 1280, 640, seed=18)
    print("\nELEMENTWISE_CONCAT past one grid round: 4 194 480 vectors exact")


def test_concat_refuses_channels_that_are_no_multiple_of_8():
    a, b = torch.ones((7, 12), dtype=torch.float16, device=DEV), torch.ones((7, 8), dtype=torch.float16, device=DEV)
    out = torch.full((7, 20), -7.0, dtype=torch.float16, device=DEV)
    for ca, cb in ((12, 8), (8, 12), (4, 4)):
        with pytest.raises(_lib.MdanceHipError):
            _lib.call("md_concat_channels_f16", a.data_ptr(), ca, b.data_ptr(), cb, out.data_ptr(), 7, ops._st())
        torch.cuda.synchronize()
        assert (out == -7.0).all()                                         # nothing was launched
    with pytest.raises(_lib.MdanceHipError):
        ops.concat_channels(a, b)


# ---- 4. window_accumulate
WINDOWS = [[5, 6, 0, 1], [2, -1, 4, 3]]                                    # a wrapping order; a skipped slot and an unordered window; f = 4 < Ftot = 7


@pytest.mark.parametrize("hw", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("halves", [1, 2])
def test_window_accumulate_is_exact(halves, hw):
    f, ftot = 4, 7
    pred, ns, cnt = E.accumulate_case(f, ftot, hw, halves, seed=hw + halves)
    for window in WINDOWS:
        want_ns, want_cnt = E.accumulate_reference(pred, ns, cnt, window, f, halves)
        runs = []
        for _ in range(2):                                                 # two identical launches from the same start
            nd, cd = ns.to(DEV), cnt.to(DEV)
            ops.window_accumulate(pred.to(DEV), nd, cd, torch.tensor(window, dtype=torch.int32, device=DEV), f, ftot, hw, halves=halves)
            runs.append((nd.cpu(), cd.cpu()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        got_ns, got_cnt = runs[0]
        assert torch.equal(got_ns.view(torch.int32), want_ns.view(torch.int32)) and torch.equal(got_cnt, want_cnt), (halves, hw, window)
        named = [fr for fr in window if fr >= 0]
        rest = [fr for fr in range(ftot) if fr not in named]
        assert rest and torch.equal(got_ns[:, rest].view(torch.int32), ns[:, rest].view(torch.int32)) and torch.equal(got_cnt[rest], cnt[rest])
        assert not torch.equal(got_ns[:, named], ns[:, named]) and torch.equal(got_cnt[named], cnt[named] + 1)


# ---- 5. the step tail against float64
def _step(tag, flavour, kind, ftot, hw, halves, second_round_from=None):
    co = E._coefficients(kind)
    case = E.step_case(flavour, ftot, hw, halves, E.step_seed(flavour, ftot, hw, halves))
    got, h_got, extra = E.run_step(ops, case, kind, co, put=put)
    if flavour == "apg":
        assert (extra[0][:, 0] < 1).any()                                  # the cap is at work
    return E.check_step(tag, case, kind, got, h_got, *E.step_want(case, kind, co, extra), second_round_from=second_round_from)


@pytest.mark.parametrize("ftot,h,w", E.SMALL_STEP_CASES)
@pytest.mark.parametrize("kind", E.KINDS)
def test_plain_step_entries_match_float64(ftot, h, w, kind):
    """md_cfg_ddim_step, md_cfg_ddim_step_eta, md_cfg_multistep_step with and without CFG.  Without CFG the counter holds NaN and a first-order
    history holds NaN: neither may be read."""
    for halves in (1, 2):
        _step("ELEMENTWISE_STEP", "plain", kind, ftot, h * w, halves)


@pytest.mark.parametrize("flavour,halves", E.LARGE_FLAVOURS)
@pytest.mark.parametrize("kind,ftot,h,w", E.LARGE_STEP_CASES)
def test_step_past_one_grid_round_matches_float64(kind, ftot, h, w, flavour, halves):
    """All eight kernels with every term live (eta > 0 / second order SDE), past 4096 x 256 threads: the threads that loop re-derive the frame,
    and with it counter[fr] and coef[2 fr], from an index of the second round."""
    per = 1 if kind.startswith("ddim") else 4                              # elements per thread
    assert ftot * h * w * 4 // per > E.ROUND
    _step("ELEMENTWISE_STEP_ROUND2", flavour, kind, ftot, h * w, halves, second_round_from=E.ROUND * per)


@pytest.mark.parametrize("ftot,h,w", E.BOUNDARY_CASES)
def test_plain_ddim_at_the_exact_round_boundary(ftot, h, w):
    total = ftot * h * w * 4
    _step("ELEMENTWISE_STEP_BOUNDARY", "plain", "ddim-eta", ftot, h * w, 2, second_round_from=E.ROUND if total > E.ROUND else None)


# ---- 6. what one step_v behind the three samplers makes natural
@pytest.mark.parametrize("flavour,halves", E.LARGE_FLAVOURS)
def test_unipc_past_one_grid_round_matches_float64(flavour, halves):
    """The four cfg_unipc_kernel instantiations at the pixel count of LARGE_STEP_CASES (5 x 459 x 457 = 1 048 815: 239 pixels loop twice, the
    round boundary inside frame 4), corrector on so that every plane is read: the float64 statement and the bounds of
    test_unipc_gpu.test_every_entry_matches_float64, the latents' bound asserted once more over the pixels of the second round."""
    _, ftot, h, w = E.LARGE_STEP_CASES[1]
    assert ftot * h * w > E.ROUND
    case, row = U._case(ftot, h * w, halves), U._row("on")
    got, st, extra = U._kernel(flavour, case, row, case.state)
    U._check("ELEMENTWISE_UNIPC_ROUND2", flavour, case, row, case.state, got, st, extra, second_round_from=E.ROUND)


def _pag_or_plain(kind, case, state, s):
    """One step on the case's inputs through the *_pag entry at pag_scale s, or through the plain entry (s None) -> (latents, history or state
    or None) on the host."""
    ftot, hw, halves, g = case.ftot, case.hw, case.halves, E.G_PAG
    ld, nd, cd, pd = put(case.lat), put(case.ns), put(case.cnt), put(case.pp)
    if kind.startswith("unipc"):
        row, kept = U._row(kind[6:]), put(state)
        if s is None:
            ops.cfg_unipc_step(ld, nd, cd, kept, ftot, hw, g, row, halves=halves)
        else:
            ops.cfg_unipc_step_pag(ld, nd, cd, kept, pd, ftot, hw, g, s, row, halves=halves)
    elif kind.startswith("ddim"):
        a_t, a_p, eta = E._coefficients(kind)
        kept, kw = None, dict(halves=halves, eta=eta, variance_noise=put(case.z) if eta else None)
        if s is None:
            ops.cfg_ddim_step(ld, nd, cd, ftot, hw, g, a_t, a_p, **kw)
        else:
            ops.cfg_ddim_step_pag(ld, nd, cd, pd, ftot, hw, g, s, a_t, a_p, **kw)
    else:
        co = E._coefficients(kind)
        kept, kw = put(case.hist), dict(halves=halves, variance_noise=put(case.z) if co[5] else None)
        if s is None:
            ops.cfg_multistep_step(ld, nd, cd, kept, ftot, hw, g, *co, **kw)
        else:
            ops.cfg_multistep_step_pag(ld, nd, cd, kept, pd, ftot, hw, g, s, *co, **kw)
    return ld.cpu(), None if kept is None else kept.cpu()


@pytest.mark.parametrize("ftot,h,w", E.SMALL_STEP_CASES[:2])
@pytest.mark.parametrize("kind", E.KINDS + ["unipc-on", "unipc-off"])
def test_pag_scale_zero_is_the_plain_entry_bitwise(kind, ftot, h, w):
    """pag_scale == 0 adds a zero to the guided v, and the update that follows must round as the plain entry's does: the same bits in the
    latents and in the history / state, for every sampler, with and without CFG, on finite planes.  At PAG_S the result differs (the term is
    there).  test_pag_gpu holds DDIM and multistep to this at (3, 13, 11) and (16, 16, 16); here also one pixel, and UniPC."""
    for halves in (1, 2):
        case = E.step_case("pag", ftot, h * w, halves, E.step_seed("pag", ftot, h * w, halves))
        state = torch.randn((4, ftot, h * w, 4), generator=torch.Generator().manual_seed(ftot + h * w + halves))
        zero, plain, live = (_pag_or_plain(kind, case, state, s) for s in (0.0, None, E.PAG_S))
        assert torch.equal(E.bits(zero[0]), E.bits(plain[0])), (kind, halves)
        assert zero[1] is None or torch.equal(zero[1].view(torch.int32), plain[1].view(torch.int32)), (kind, halves)
        assert torch.isfinite(zero[0]).all() and not torch.equal(live[0], plain[0])
