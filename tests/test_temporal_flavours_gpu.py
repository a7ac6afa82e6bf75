"""GPU: every kernel flavour behind md_temporal_attention_fwd_f16, each at the smallest shapes that reach its code paths, in the operand
forms the pipeline uses.  The entry point chooses between the lane-per-query temporal_attn_kernel<FMAX> (500) and the matrix-core
temporal_attn_mfma_kernel<D, QB> (511 / 512), whose workgroup geometry (hg heads x pb pixels, wave w owning units w, w + 4, ...) is
computed at run time; md_temporal_attention_plan answers which, and every case here (tests/temporal_ref.py CASES)
  (a) asserts code, hg and pb from the plan BEFORE launching, so a change of the rule fails the case instead of silently moving it;
  (b) launches three times and requires identical bits;
  (c) starts O as NaN, dense or as a column slice of a wider buffer filled with 7.0 that must be untouched afterwards;
  (d) compares with float64 softmax(scale Q K^T) V on the same fp16-rounded inputs: elementwise |err| <= 1e-2 max|ref| + 1e-3 (the
      project's kernel tolerance) and relative L2 <= FACTOR x the case's floor, the relative L2 of a plain PyTorch emulation of the
      documented arithmetic (computed from the reference alone, not recorded; F = 1 has a floor of 0: the output must be V exactly).
Q, K and V come from different seeds and, like O, live in four slots of ONE device allocation, each slot large enough for its operand
at the widest pitch of the case (3 C): a kernel that addressed one operand with another's pitch reads garbage (N(0, 50)) or writes into
the 7.0 -- it fails the case, it does not leave the allocation.  After the three launches the input slots must hold their initial bits.
The misaligned fallback (D = 40 / 80 / 160 with an operand that is not 16-byte aligned) is not launched: nothing in the pipeline reaches
it; the plan reports it and tests/test_temporal_floor_cpu.py pins it.
profiles/temporal_flavour_tests.log: plan, floor and measured value of every case on MI355X, and the mutations these cases catch."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from temporal_ref import FACTOR, FRAME_EDGES, GEOMETRIES, LANE_CASES, OPERAND_FORMS, PEAKY, SCALES, problem, rel_l2, rnd  # noqa: E402

from mikudance_amd import _lib, ops  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def layout(case):
    """(pitch, first column) of q, k, v, o inside their slots, and the slot of each (q | k | v of the production form share slot 0)."""
    C = case.H * case.D
    if case.form == "dense":
        return [(C, 0)] * 4, [0, 1, 2, 3]
    if case.form == "qkv":
        return [(3 * C, 0), (3 * C, C), (3 * C, 2 * C), (C, 0)], [0, 0, 0, 3]
    assert case.form == "pitches"
    return [(C + 64, 32), (2 * C, C), (C + 8, 8), (C + 32, 16)], [0, 1, 2, 3]


def run_case(dev, case, runs=3):
    pr = problem(case)
    NB, F, HW, H, D = case.NB, case.F, case.HW, case.H, case.D
    M, C = NB * F * HW, H * D
    slot = M * 3 * C + 64                                  # a multiple of 8 elements: every slot starts 16-byte aligned
    geo, slots = layout(case)
    host = rnd(4 * slot, seed=11, scale=50.0)              # garbage wherever no operand lives
    host[3 * slot:] = 7.0

    def view(t, i):
        ld, c0 = geo[i]
        return t[slots[i] * slot: slots[i] * slot + M * ld].view(M, ld)[:, c0:c0 + C]
    for i, src in enumerate((pr.q, pr.k, pr.v)):
        view(host, i).copy_(src)
    view(host, 3).fill_(float("nan"))
    arena = host.to(dev)
    q, k, v, o = (view(arena, i) for i in range(4))
    assert all(t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 for t in (q, k, v, o))

    hg, pb = ctypes.c_int(0), ctypes.c_int(0)
    code = _lib.load().md_temporal_attention_plan(NB, F, HW, H, D, 1, ctypes.byref(hg), ctypes.byref(pb))
    assert (code, hg.value, pb.value) == (case.code, case.hg, case.pb), f"{case.name}: the plan is {(code, hg.value, pb.value)}, the case is meant for {(case.code, case.hg, case.pb)}"

    outs = []
    for _ in range(runs):
        arena[3 * slot:].copy_(host[3 * slot:])
        ops.temporal_attention(q, k, v, NB, F, HW, H, D, out=o, scale=None if case.mult == 1.0 else pr.scale)
        outs.append(arena[3 * slot:].cpu())
    assert torch.equal(arena[:3 * slot].cpu().view(torch.int16), host[:3 * slot].view(torch.int16)), f"{case.name}: an input slot was written"
    for got in outs[1:]:
        assert torch.equal(got.view(torch.int16), outs[0].view(torch.int16)), f"{case.name}: two runs on the same inputs differ"
    ld, c0 = geo[3]
    out = outs[0][:M * ld].view(M, ld)[:, c0:c0 + C].clone()
    outs[0][:M * ld].view(M, ld)[:, c0:c0 + C] = 7.0
    assert bool((outs[0] == 7.0).all()), f"{case.name}: {int((outs[0] != 7.0).sum())} elements outside O were written"

    ref = pr.ref
    assert bool(torch.isfinite(out.float()).all()), f"{case.name}: non-finite output (an element that was never written stays NaN)"
    err, bound = float((out.double() - ref).abs().max()), 1e-2 * float(ref.abs().max()) + 1e-3
    value = rel_l2(out, ref)
    print(f"\nPARITY_MEASURE temporal_flavour:{case.name} plan={code}/{hg.value}/{pb.value} floor={pr.floor:.6e} got={value:.6e} ratio={value / pr.floor if pr.floor else float(value != 0):.3f}")
    assert err <= bound, f"{case.name}: max err {err:.4g} > {bound:.4g}"
    assert value <= FACTOR * pr.floor, f"{case.name}: relative L2 {value:.3e} > {FACTOR} x the floor {pr.floor:.3e}"


def _ids(c):
    return c.name


@pytest.mark.parametrize("case", GEOMETRIES, ids=_ids)
def test_workgroup_geometries(dev, case):
    """One case per row of the plan table (tests/test_temporal_floor_cpu.py): hg x pb units dealt to four waves, a partial last workgroup
    wherever pb > 1 -- at D <= 80 through the O-through-LDS write-back loop, at D = 160 through the direct stores."""
    run_case(dev, case)


@pytest.mark.parametrize("case", FRAME_EDGES, ids=_ids)
def test_frame_count_edges(dev, case):
    """F = 1, 2 (one / two live keys, 15 / 14 masked), 15, 16 (a full block), 17 (QB = 2 with a single live key and a single live query
    in the second block), 31, 32 at every matrix-core head dim."""
    run_case(dev, case)


@pytest.mark.parametrize("case", LANE_CASES, ids=_ids)
def test_lane_per_query_kernel(dev, case):
    """The FMAX = 4 / 8 / 16 / 32 instances at F = 3, 5, 9, 17, 32 (frames past F clamped for the loads and masked), H = 2 and 8, pixel
    counts that leave a partial last workgroup and lanes past pb * hg * F."""
    run_case(dev, case)


@pytest.mark.parametrize("case", OPERAND_FORMS, ids=_ids)
def test_operand_forms(dev, case):
    """qkv: the motion module's call (q | k | v the column thirds of one GEMM output, ld = 3 C).  pitches: ldq, ldk, ldv and ldo all
    different and every operand at a column offset, so that a pitch or an offset taken from the wrong operand shows."""
    run_case(dev, case)


@pytest.mark.parametrize("case", PEAKY, ids=_ids)
def test_peaky_rows(dev, case):
    """Dominant keys (logit ~ 4 sqrt(D) >= 25: every other P underflows in fp16) in the first 16-block and in the last live frame, for
    units of the first and of the last wave: P = 1.0 exactly, the denominator 1 + the fp32 tails."""
    run_case(dev, case)


@pytest.mark.parametrize("case", SCALES, ids=_ids)
def test_scale_argument(dev, case):
    """scale = 0.5 / 3 x D^-0.5 through ops.temporal_attention(scale=): the C ABI's argument reaches both kernels."""
    run_case(dev, case)

