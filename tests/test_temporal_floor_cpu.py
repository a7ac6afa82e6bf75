"""CPU: the dispatch of md_temporal_attention_fwd_f16 and the yardstick of tests/test_temporal_flavours_gpu.py.

md_temporal_attention_plan runs the host function the launcher runs (csrc/temporal.hip temporal_plan) without touching a device: 500 = the
lane-per-query temporal_attn_kernel, 511 / 512 = temporal_attn_mfma_kernel with one / two 16-frame blocks, and the workgroup geometry
(hg heads x pb pixels).  The table is derived by hand from the launcher's rule, lds = 3 F (pb hg D 2 + 16) <= 49152 bytes with at most
16 (F <= 16) / 8 (F <= 32) units per workgroup: hg = H halved until one pixel fits, pb = units / hg lowered until it fits.

The floors: rel_l2(emulation, reference) of every case of the GPU file (tests/temporal_ref.py) lies in [1e-4, 6e-4] -- a few fp16 roundings
(2^-12 / sqrt(3) = 1.4e-4 each) per element and nothing else -- so that a kernel can pass at FACTOR x floor from the arithmetic alone.
F = 1 is the exception by arithmetic, not by measurement: softmax over one key is 1.0, emulation and reference both equal V, the floor
is exactly 0 and the kernel has to reproduce V bit for bit."""
import ctypes

import pytest

from temporal_ref import CASES, FRAME_EDGES, GEOMETRIES, LANE, MFMA1, MFMA2, problem

MD_ERR_ARG = -1


def plan(NB, F, HW, H, D, aligned16=1):
    from mikudance_amd import _lib
    hg, pb = ctypes.c_int(-7), ctypes.c_int(-7)
    code = _lib.load().md_temporal_attention_plan(NB, F, HW, H, D, aligned16, ctypes.byref(hg), ctypes.byref(pb))
    return code, hg.value, pb.value


def test_temporal_dispatch_table():
    table = {  # (H, D, F): (code, hg, pb)
        # the benchmark's motion modules (BASELINE configs[1], 16 frames: the 96 x 96 / 48 x 48 / 24 x 24 levels) ...
        (8, 40, 16): (MFMA1, 8, 1), (8, 80, 16): (MFMA1, 4, 1), (8, 160, 16): (MFMA1, 2, 1),
        # ... and the long-clip windows of 30 frames (configs[4]).  3 * 30 * (8 * 40 * 2 + 16) = 59040 > 49152: eight heads of d = 40 do
        # not fit at F = 30, four do (30240) -- the geometry tests/test_lds_layouts_cpu.py has always stated for this shape
        (8, 40, 30): (MFMA2, 4, 1), (8, 80, 30): (MFMA2, 2, 1), (8, 160, 32): (MFMA2, 1, 1),
        # more than one pixel per workgroup
        (8, 40, 7): (MFMA1, 8, 2), (2, 40, 16): (MFMA1, 2, 6), (1, 40, 17): (MFMA2, 1, 8), (8, 40, 17): (MFMA2, 8, 1), (8, 160, 3): (MFMA1, 8, 2),
        (4, 40, 8): (MFMA1, 4, 4), (4, 80, 16): (MFMA1, 4, 1), (1, 160, 16): (MFMA1, 1, 3), (1, 80, 32): (MFMA2, 1, 3),
        # both sides of the 48 KiB cap at d = 40, H = 8: 3 F 1296 <= 49152 holds up to F = 12
        (8, 40, 12): (MFMA1, 8, 2), (8, 40, 13): (MFMA1, 8, 1),
        # eight heads of d = 40 in two blocks: 3 F 656 <= 49152 holds up to F = 24
        (8, 40, 24): (MFMA2, 8, 1), (8, 40, 25): (MFMA2, 4, 1),
    }
    for (H, D, F), want in table.items():
        assert plan(2, F, 5, H, D) == want, ((H, D, F), plan(2, F, 5, H, D), want)
    # every other head dim runs the lane-per-query kernel, and so does d = 40 / 80 / 160 with an operand that is not 16-byte aligned
    for D in (8, 16, 32, 64):
        for F in (1, 4, 5, 16, 17, 32):
            assert plan(2, F, 5, 8, D)[0] == LANE, (D, F)
    for D in (40, 80, 160):
        assert plan(2, 16, 5, 8, D, aligned16=0)[0] == LANE and plan(2, 30, 5, 8, D, aligned16=0)[0] == LANE
    # its geometry: HG F <= 256 lanes and 4 F HG D <= 48 KiB per pixel, PB = min(256 / (HG F), 48 KiB / (4 F HG D))
    assert plan(2, 16, 5, 8, 40, aligned16=0) == (LANE, 8, 2) and plan(2, 32, 5, 8, 160, aligned16=0) == (LANE, 2, 1)
    assert plan(2, 32, 5, 8, 64) == (LANE, 4, 1) and plan(2, 3, 5, 8, 8) == (LANE, 8, 10) and plan(2, 32, 5, 2, 64) == (LANE, 2, 3)
    # the plan does not depend on the number of pixels
    assert plan(1, 16, 1, 8, 40) == plan(60, 16, 16384, 8, 40) == (MFMA1, 8, 1)


def test_temporal_plan_refuses_what_the_entry_point_refuses():
    from mikudance_amd import _lib
    lib = _lib.load()
    bad = [(2, 0, 5, 8, 40), (2, 33, 5, 8, 40), (2, -1, 5, 8, 40),            # F outside 1 .. 32
           (2, 16, 5, 8, 36), (2, 16, 5, 8, 4), (2, 16, 5, 8, 0),             # D no positive multiple of 8
           (2, 16, 5, 3, 40), (2, 16, 5, 16, 40), (2, 16, 5, 0, 40), (2, 16, 5, 6, 40),      # H not a power of two <= 8
           (2, 32, 5, 8, 1024), (2, 32, 5, 1, 776)]                           # one head's K + V of one pixel (4 F D bytes) beyond 96 KiB
    for args in bad:
        code, hg, pb = plan(*args)
        assert code == MD_ERR_ARG and (hg, pb) == (-7, -7), (args, code, hg, pb)
        assert lib.md_last_error().decode().startswith("md_temporal_attention_fwd")
    assert plan(2, 32, 5, 1, 768)[0] == LANE                                   # 4 * 32 * 768 = 96 KiB exactly
    # either output pointer may be NULL
    assert lib.md_temporal_attention_plan(2, 16, 5, 8, 40, 1, None, None) == MFMA1
    hg = ctypes.c_int(0)
    assert lib.md_temporal_attention_plan(2, 30, 5, 8, 40, 1, ctypes.byref(hg), None) == MFMA2 and hg.value == 4


@pytest.mark.parametrize("case", GEOMETRIES + FRAME_EDGES, ids=lambda c: c.name)
def test_plan_of_every_matrix_core_case(case):
    """The (code, hg, pb) each GPU case states, written by hand in tests/temporal_ref.py, is what the plan says."""
    assert plan(case.NB, case.F, case.HW, case.H, case.D) == (case.code, case.hg, case.pb)
    if case.pb > 1 and case in GEOMETRIES:
        assert (case.NB * case.HW) % case.pb != 0, "the geometry cases end in a partial workgroup wherever pb > 1"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_floor_of_every_gpu_case(case):
    pr = problem(case)
    print(f"\nPARITY_MEASURE temporal_floor_cpu:{case.name} floor={pr.floor:.6e}")
    if case.F == 1:
        assert pr.floor == 0.0          # 1.0 * v / 1.0: see the module docstring
    else:
        assert 1e-4 <= pr.floor <= 6e-4, pr.floor


def test_a_probability_cut_to_eight_bits_lands_above_the_factor():
    """The check bites: the matrix-core arithmetic with P truncated to 8 of its 11 significant bits exceeds FACTOR x floor."""
    import torch
    from temporal_ref import FACTOR, LOG2E, _fold, _unfold, rel_l2
    for case in (GEOMETRIES[0], GEOMETRIES[4]):
        pr, (NB, F, HW, H, D) = problem(case), case[1:6]
        qh, kh, vh = (_fold(t.float(), NB, F, HW, H, D) for t in (pr.q, pr.k, pr.v))
        s = qh @ kh.transpose(-1, -2)
        p = torch.exp2((s - s.max(dim=-1, keepdim=True).values) * (pr.scale * LOG2E))
        cut = (p.half().view(torch.int16) & ~7).view(torch.float16).float()
        out = _unfold(((cut @ vh) / p.sum(dim=-1, keepdim=True)).half(), NB, F, HW, H, D)
        assert rel_l2(out, pr.ref) > 1.4 * FACTOR * pr.floor, (rel_l2(out, pr.ref), pr.floor)
