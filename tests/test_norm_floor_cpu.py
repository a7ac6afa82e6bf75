"""CPU: the dispatch of md_groupnorm_ld_nhwc_f16 / md_groupnorm_table_f16 / md_layernorm_f16 and the yardstick of
tests/test_norm_flavours_gpu.py.

md_groupnorm_plan and md_layernorm_plan run the host functions the launchers run (csrc/norm.hip gn_plan, ln_plan) without touching a
device.  The tables below are derived by hand from the rule:
  one sweep (61k / 62k, never for the table)   cpg = C / G with cpg % 4 == 0 and cpr = cpg / 4 <= 64, B G >= 256, HW <= 1024; 512 threads
      when cdiv(HW, 256 // cpr) > 24, else 256; R = threads // cpr pixel lanes; it = cdiv(HW, R) <= 24 sweeps (more: two launches);
      instance <6> (256 threads only) / <12> / <24> by it; (threads, R, slab, nslab) = (256 | 512, R, HW, 1)
  two / three launches (600 / 601)   R = max(512 // (C / 8), 1) row lanes, threads = C / 8 * R, rows = 32 halved down to 8 while
      B cdiv(HW, R rows) < 512, slab = R rows, nslab = cdiv(HW, slab); 601 when nslab > 128
  LayerNorm   720 at C = 320, else 700 + cdiv(C, 512)

The floors: rel_l2(emulation, reference) of every case of the GPU file (tests/norm_ref.py), minimum .. maximum observed on the CPU:
  GroupNorm 2.04e-4 .. 2.12e-4 over whole tensors; 1.23e-4 .. 2.81e-4 over the single (image, group) units of the marked cases (the
  planted element carries a visible share of the unit's norm: 1.23e-4 where it is 300 sigma out, and its own rounding is a draw);
  LayerNorm y 1.70e-4 .. 2.40e-4 (the ends are C = 8 with 128 and 8 elements; 1.9e-4 .. 2.2e-4 from 2048 elements up), y2 2.05e-4 (no row
  receives anything: one rounding) and 2.4e-4 .. 2.80e-4; InstanceNorm 2.03e-4 .. 2.14e-4 and exactly 0 at HW = 1, its marked (image,
  channel) units 1.2e-4 .. 3.2e-4; softmax 1.5e-4 .. 2.53e-4, peaky cases 3e-12 and 2.4e-5 (rows that are 1.0 and zeros have nothing to
  round); the fp32 table 2.6e-7 .. 9.1e-6 (about sqrt(n) 2^-25 for the n = 1000 .. 88 320 values of a group).
One fp16 rounding is 2^-12 / sqrt(3) ~ 1.4e-4 of the element's binade top, 2.0e-4 in relative L2 of a normalised tensor; y2 has two of
them.  The bands asserted below are these rounded outward."""
import ctypes

import pytest
import torch

import norm_ref as nr
from norm_ref import FACTOR, S6, S12, S24, THREE, TWO, W12, W24, rel_l2

MD_ERR_ARG = -1


def gn_plan(B, HW, C, G, ldx=None, x16=1, table=0):
    from mikudance_amd import _lib
    out = [ctypes.c_int(-7) for _ in range(4)]
    code = _lib.load().md_groupnorm_plan(B, HW, C, G, C if ldx is None else ldx, x16, table, *(ctypes.byref(o) for o in out))
    return (code,) + tuple(o.value for o in out)


def ln_plan(M, C):
    from mikudance_amd import _lib
    return _lib.load().md_layernorm_plan(M, C)


def test_groupnorm_dispatch_table():
    table = {  # (B, HW, C, G): (code, threads, R, slab, nslab)
        # The benchmark's levels (768 x 768, CFG batch 32 = 2 x 16 frames, G = 32).  96 x 96: norm1 / norm2 of the C = 320 resnets, the
        # transformer's and the motion module's entry norm, the up path's concatenated inputs (640, 960); cpg = 10 is no multiple of 4
        # and HW > 1024 in any case: two launches
        (32, 9216, 320, 32): (TWO, 480, 12, 384, 24), (32, 9216, 640, 32): (TWO, 480, 6, 192, 48), (32, 9216, 960, 32): (TWO, 480, 4, 128, 72),
        # 48 x 48: C = 640 resnets and norms, the up path's 1280 / 1920 / 960 inputs
        (32, 2304, 640, 32): (TWO, 480, 6, 96, 24), (32, 2304, 1280, 32): (TWO, 480, 3, 96, 24), (32, 2304, 1920, 32): (TWO, 480, 2, 64, 36),
        # 24 x 24: C = 1280 resnets and norms on <24,256> (cdiv(576, 25) = 24), the up path's 1920 / 2560 on <24,512>
        (32, 576, 1280, 32): (S24, 256, 25, 576, 1), (32, 576, 1920, 32): (W24, 512, 34, 576, 1), (32, 576, 2560, 32): (W24, 512, 25, 576, 1),
        (32, 576, 640, 32): (S12, 256, 51, 576, 1),
        # 12 x 12: the mid block and the lowest down / up resnets
        (32, 144, 1280, 32): (S6, 256, 25, 144, 1), (32, 144, 2560, 32): (S12, 256, 12, 144, 1), (32, 144, 1920, 32): (S12, 256, 17, 144, 1),
        # the reference UNet runs the same levels at batch 2 (B G = 64 < 256): two launches, rows = 8
        (2, 576, 1280, 32): (TWO, 480, 3, 24, 24), (2, 9216, 320, 32): (TWO, 480, 12, 96, 96),
        # the AutoencoderKL at 768 x 768, C = 128: 576 slabs per image, three launches
        (1, 589824, 128, 32): (THREE, 512, 32, 1024, 576),
        # both sides of HW = 1024
        (8, 1024, 1280, 32): (W24, 512, 51, 1024, 1), (8, 1025, 1280, 32): (TWO, 480, 3, 24, 43),
        # both sides of B G = 256
        (8, 150, 1280, 32): (S6, 256, 25, 150, 1), (7, 150, 1280, 32): (TWO, 480, 3, 24, 7),
        (4, 33, 256, 64): (S6, 256, 256, 33, 1), (3, 33, 256, 64): (TWO, 512, 16, 128, 1), (64, 20, 64, 4): (S6, 256, 64, 20, 1),
        # cpg % 4: 10 and 6 never run the one-sweep kernel
        (32, 144, 320, 32): (TWO, 480, 12, 96, 2), (8, 37, 192, 32): (TWO, 504, 21, 168, 1), (8, 37, 128, 32): (S6, 256, 256, 37, 1),
        # cpg / 4 <= 64: cpg = 256 does, cpg = 512 does not
        (8, 10, 8192, 32): (S6, 256, 4, 10, 1), (16, 10, 8192, 16): (TWO, 1024, 1, 8, 2),
        # the 256 -> 512 thread switch at cdiv(HW, 25) = 24 | 25
        (8, 600, 1280, 32): (S24, 256, 25, 600, 1), (8, 601, 1280, 32): (W12, 512, 51, 601, 1),
        # the template steps, 256 threads: it = 6 | 7, 12 | 13
        (8, 151, 1280, 32): (S12, 256, 25, 151, 1), (8, 300, 1280, 32): (S12, 256, 25, 300, 1), (8, 301, 1280, 32): (S24, 256, 25, 301, 1),
        # ... 512 threads: it = 12 | 13, and 24 | 25 (25 sweeps: two launches) at cpg = 256, 8 lanes
        (8, 612, 1280, 32): (W12, 512, 51, 612, 1), (8, 613, 1280, 32): (W24, 512, 51, 613, 1),
        (8, 192, 8192, 32): (W24, 512, 8, 192, 1), (8, 200, 8192, 32): (TWO, 1024, 1, 8, 25),
        # nslab = 128 | 129
        (1, 1024, 2560, 32): (TWO, 320, 1, 8, 128), (1, 1025, 2560, 32): (THREE, 320, 1, 8, 129),
        # the slab halving: 32 rows once B cdiv(HW, 32 R) >= 512, 16, 8
        (16, 9216, 320, 32): (TWO, 480, 12, 192, 48), (1, 9216, 320, 32): (TWO, 480, 12, 96, 96),
    }
    for key, want in table.items():
        assert gn_plan(*key) == want, (key, gn_plan(*key), want)
    # the table entry never runs the one-sweep kernel: it answers with the geometry of the two sweeps
    assert gn_plan(32, 576, 1280, 32, table=1) == (TWO, 480, 3, 24, 24) and gn_plan(8, 150, 1280, 32, table=1) == (TWO, 480, 3, 24, 7)
    assert gn_plan(1, 1025, 2560, 32, table=1) == (THREE, 320, 1, 8, 129)
    # a channel slice changes nothing
    assert gn_plan(8, 607, 1280, 32, ldx=1376) == (W12, 512, 51, 607, 1) and gn_plan(2, 100, 320, 32, ldx=392) == (TWO, 480, 12, 96, 2)


def test_layernorm_dispatch_table():
    table = {8: 701, 64: 701, 512: 701, 520: 702, 640: 702, 1024: 702, 1032: 703, 1280: 703, 1536: 703, 1544: 704, 2048: 704,
             # C = 320 (the 96 x 96 level's blocks) has its own kernel; 640 / 1280 (48 x 48, 24 x 24 and 12 x 12) run <2> / <3>
             320: 720, 312: 701, 328: 701}
    for C, want in table.items():
        for M in (1, 33, 294912):
            assert ln_plan(M, C) == want, (M, C, ln_plan(M, C), want)


@pytest.mark.parametrize("key", [(32, 9216, 320, 32), (32, 576, 1280, 32), (8, 150, 1280, 32), (1, 1025, 2560, 32), (2, 12400, 320, 32),
                                 (1, 589824, 128, 32), (2, 5, 64, 32), (4, 33, 256, 64)])
def test_workspace_matches_the_plan(key):
    from mikudance_amd import _lib
    B, HW, C, G = key
    nslab = gn_plan(*key, table=1)[4]
    assert _lib.load().md_groupnorm_workspace_bytes(B, HW, C, G) == (B * nslab * G * 2 + B * G * 3) * 4
    code, _, _, _, ns = gn_plan(*key)
    assert ns == (nslab if code in (TWO, THREE) else 1)


def test_plans_refuse_what_the_entries_refuse():
    from mikudance_amd import _lib
    lib = _lib.load()
    bad = [dict(C=324, ldx=328), dict(C=4), dict(C=520, G=65), dict(G=0), dict(G=-1), dict(G=3),               # C % 8, G outside 1 .. 64, C % G
           dict(ldx=312), dict(ldx=324), dict(x16=0), dict(C=8200, G=1)]                                       # ldx < C, ldx % 8, alignment, C > 8192
    for kw in bad:
        for table in (0, 1):
            args = dict(B=2, HW=100, C=320, G=32, table=table)
            args.update(kw)
            got = gn_plan(**args)
            assert got == (MD_ERR_ARG, -7, -7, -7, -7), (args, got)
            assert lib.md_last_error().decode().startswith("md_groupnorm_table:" if table else "md_groupnorm:")
    assert gn_plan(2, 100, 8192, 1)[0] == TWO and gn_plan(2, 100, 512, 64)[0] == TWO
    # any output pointer may be NULL
    assert lib.md_groupnorm_plan(1, 1025, 2560, 32, 2560, 1, 0, None, None, None, None) == THREE
    ns = ctypes.c_int(0)
    assert lib.md_groupnorm_plan(2, 100, 1280, 32, 1280, 1, 0, None, None, None, ctypes.byref(ns)) == TWO and ns.value == 5
    for C in (2056, 4096, 12, 324):
        assert ln_plan(16, C) == MD_ERR_ARG and lib.md_last_error().decode().startswith("md_layernorm")


def test_softmax_refuses_a_scale_that_is_not_positive():
    """The kernel scales the row maximum of x: the header asks for scale > 0 and the entry checks it before anything else (nothing is
    launched and the pointer is not looked at)."""
    from mikudance_amd import _lib
    lib = _lib.load()
    for scale in (-1.0, -1e-30, 0.0, float("nan"), float("inf")):
        assert lib.md_softmax_rows_f16(16, 8, 1, 8, scale, None) == MD_ERR_ARG
        assert "scale" in lib.md_last_error().decode()


@pytest.mark.parametrize("case", nr.GN_CASES, ids=lambda c: c.name)
def test_plan_and_floor_of_every_groupnorm_case(case):
    want = (case.code, case.threads, case.R, case.slab, case.nslab)
    assert gn_plan(case.B, case.HW, case.C, case.G, ldx=case.lead + case.C + case.tail, table=int(case.table)) == want
    if case.mark:
        assert gn_plan(case.B, case.HW, case.C, case.G)[0] == case.code, "md_groupnorm_ld_nhwc_f16 on this shape runs the form the case names"
    pr = nr.gn_problem(case)
    print(f"\nPARITY_MEASURE norm_floor_cpu:gn {case.name} floor={pr.floor:.6e}")
    assert 1.9e-4 <= pr.floor <= 2.2e-4, pr.floor
    for b, g, p, c, k in pr.marks:
        f = rel_l2(nr.unit(pr.emu, case, b, g), nr.unit(pr.ref, case, b, g))
        print(f"PARITY_MEASURE norm_floor_cpu:gn {case.name} unit ({b}, {g}) floor={f:.6e}")
        assert 1.1e-4 <= f <= 3.0e-4, f
    if case.table:
        ref, floor = nr.table_problem(case)
        print(f"PARITY_MEASURE norm_floor_cpu:gn {case.name} table floor={floor:.6e}")
        assert 1e-7 <= floor <= 1e-5, floor


@pytest.mark.parametrize("case", nr.LN_CASES, ids=lambda c: c.name)
def test_plan_and_floor_of_every_layernorm_case(case):
    assert ln_plan(case.M, case.C) == case.code
    pr = nr.ln_problem(case)
    print(f"\nPARITY_MEASURE norm_floor_cpu:ln {case.name} floor={pr.floor:.6e}" + (f" floor2={pr.floor2:.6e}" if case.add_mode else ""))
    lo, hi = (1.9e-4, 2.2e-4) if case.M * case.C >= 2048 else (1.6e-4, 2.5e-4)
    assert lo <= pr.floor <= hi, pr.floor
    if case.add_mode:
        nobody = not bool(pr.got.any())
        assert (1.9e-4 if nobody else 2.2e-4) <= pr.floor2 <= (2.2e-4 if nobody else 3.1e-4), pr.floor2


@pytest.mark.parametrize("case", nr.IN_CASES, ids=lambda c: c.name)
def test_floor_of_every_instancenorm_case(case):
    pr = nr.in_problem(case)
    print(f"\nPARITY_MEASURE norm_floor_cpu:in {case.name} floor={pr.floor:.6e}")
    if case.HW == 1:
        assert pr.floor == 0.0 and torch.equal(pr.emu, pr.gb[..., case.C:])      # y = beta: see norm_ref's docstring
    else:
        assert 1.9e-4 <= pr.floor <= 2.2e-4, pr.floor
    for b, c, p, k in pr.marks:
        f = rel_l2(pr.emu[b, :, c], pr.ref[b, :, c])
        assert 1.1e-4 <= f <= 3.4e-4, f


@pytest.mark.parametrize("case", nr.SM_CASES, ids=lambda c: c.name)
def test_floor_of_every_softmax_case(case):
    pr = nr.sm_problem(case)
    print(f"\nPARITY_MEASURE norm_floor_cpu:softmax {case.name} floor={pr.floor:.6e}")
    assert (0.0 if case.peaky else 1.4e-4) <= pr.floor <= 2.7e-4, pr.floor      # a peaky row is 1.0 and zeros: nothing to round


# ------------------------------------------------------------------------------------------------------------------ the check bites
def _case(name):
    return next(c for c in nr.GN_CASES if c.name == name)


def _sums(pr, case):
    B, HW, C, G = case.B, case.HW, case.C, case.G
    xg = pr.x.double().view(B, HW, G, C // G)
    return xg.sum(dim=(1, 3)), (xg * xg).sum(dim=(1, 3))


def _report(what, case, value, floor):
    print(f"\nPARITY_MEASURE norm_mutation:{what} [{case.name}] floor={floor:.6e} got={value:.6e} ratio={value / floor:.1f}")
    assert value > 1.4 * FACTOR * floor, (what, value, floor)


@pytest.mark.parametrize("name", ["small sentinels", "two sentinels", "three sentinels"])
def test_a_pixel_left_out_of_the_statistics_lands_above_the_factor(name):
    """Each planted element's pixel in turn is dropped from the sums (all of its channels): the element's (image, group) unit lands far
    above FACTOR x its floor -- and only because of the planted element: over the whole tensor the same mutation stays under the factor."""
    case = _case(name)
    pr = nr.gn_problem(case)
    for b, g, p, c, k in pr.marks:
        keep = torch.ones(case.HW, dtype=torch.bool)
        keep[p] = False
        stats = nr._group_stats(pr.x[:, keep], case.G, torch.float32)
        out = nr.groupnorm_emulation(pr.x, pr.gamma, pr.beta, case.G, case.eps, stats=stats)
        ref, emu = nr.unit(pr.ref, case, b, g), nr.unit(pr.emu, case, b, g)
        _report(f"pixel {p} dropped, unit ({b}, {g})", case, rel_l2(nr.unit(out, case, b, g), ref), rel_l2(emu, ref))


def test_n_from_the_slab_grid_lands_above_the_factor():
    """n = slab x nslab x cpg (120 pixels) instead of HW x cpg (97) on the case whose last slab holds one pixel."""
    case = _case("two ragged last slab of 1")
    pr = nr.gn_problem(case)
    s, q = _sums(pr, case)
    n = case.slab * case.nslab * (case.C // case.G)
    mean = s / n
    out = nr.groupnorm_emulation(pr.x, pr.gamma, pr.beta, case.G, case.eps, stats=((mean).float(), (q / n - mean * mean).float()))
    _report("n = slab * nslab * cpg", case, rel_l2(out, pr.ref), pr.floor)


@pytest.mark.parametrize("name", ["two cpg 10", "two cpg 30", "small cpg 20"])
def test_the_neighbouring_groups_mean_lands_above_the_factor(name):
    case = _case(name)
    pr = nr.gn_problem(case)
    mean, var = nr._group_stats(pr.x, case.G, torch.float32)
    out = nr.groupnorm_emulation(pr.x, pr.gamma, pr.beta, case.G, case.eps, stats=(mean.roll(1, dims=1), var))
    _report("mean of group g - 1", case, rel_l2(out, pr.ref), pr.floor)


@pytest.mark.parametrize("name", ["two cpg 10", "small <12,512> it 12", "three 129 slabs"])
def test_gamma_and_beta_one_chunk_off_land_above_the_factor(name):
    case = _case(name)
    pr = nr.gn_problem(case)
    for what, gamma, beta in (("gamma one chunk off", pr.gamma.roll(8), pr.beta), ("beta one chunk off", pr.gamma, pr.beta.roll(8))):
        out = nr.groupnorm_emulation(pr.x, gamma, beta, case.G, case.eps, silu=case.silu)
        _report(what, case, rel_l2(out, pr.ref), pr.floor)
