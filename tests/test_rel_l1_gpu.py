"""GPU: md_rel_l1_f16 (ops.rel_l1), the distance of adaptive DeepCache, against float64 sums of the same fp16 values on the MI355X.

Bound.  Every term |a - b|, |b| is >= 0, so a sum's relative error is at most depth 2^-24 to first order, depth = the largest number of fp32
additions a term passes through in the kernel's own order (mikudance_amd/csrc/rel_l1.hip states it; tests/deepcache_adaptive_ref.rel_l1_depth
restates it); one more 2^-24 for the fp32 subtraction a - b and one for the reference: |got - want| <= (depth + 2) 2^-24 want.  A sum whose
terms are all 0 must be exactly 0, and the kernel is bitwise repeatable, also after something else has written the workspace."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from mikudance_amd import ops  # noqa: E402

import deepcache_adaptive_ref as AR  # noqa: E402

DEV = torch.device("cuda:0")
U = 2.0 ** -24


def _views(rows, C, lda, ldb, offa, offb, seed, scale_b=1.0):
    """a, b: rows x C channel slices, from column offa / offb on, of wider (rows, lda) / (rows, ldb) device buffers of N(0, 1) fp16 values."""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((rows, lda), generator=g).half().to(DEV)
    B = (torch.randn((rows, ldb), generator=g) * scale_b).half().to(DEV)
    return A[:, offa:offa + C], B[:, offb:offb + C]


def _check(a, b, vector, tag):
    assert AR.vector_path(a, b) == vector, tag                             # the case runs the path it is meant for
    got = ops.rel_l1(a, b)
    again = ops.rel_l1(a, b)
    for ws in ops._workspaces["rel_l1"].values():                          # an unrelated kernel writes the workspace
        ws.fill_(float("nan"))
    third = ops.rel_l1(a, b)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and got.shape == (2,) and got.device == a.device
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)) and torch.equal(got.view(torch.int32), third.view(torch.int32)), tag
    rows, C = a.numel() // a.shape[-1], a.shape[-1]
    bound = (AR.rel_l1_depth(rows, C, vector) + 2) * U
    want = AR.rel_l1_f64(a, b)
    errs = []
    for g, w in zip(got.tolist(), want):
        if w == 0.0:
            assert g == 0.0, (tag, g)
            errs.append(0.0)
        else:
            errs.append(abs(g - w) / w)
    print(f"\nREL_L1 {tag} {rows} x {C} {'vector' if vector else 'scalar'}: rel err {errs[0]:.2e} {errs[1]:.2e}, bound {bound:.2e}")
    assert max(errs) <= bound, (tag, errs, bound)
    return got.tolist()


# rows, C, lda, ldb, offset of a, offset of b, the path
CASES = {"1x8": (1, 8, 960, 640, 640, 320, True),
         "3x320": (3, 320, 960, 640, 640, 320, True),
         "3x320-base-8-bytes": (3, 320, 960, 640, 4, 320, False),        # a's base is 8-byte aligned only: one element per access
         "7x321-odd-C": (7, 321, 960, 640, 639, 319, False),
         "round+1-scalar": (1, AR.ROUND + 1, AR.ROUND + 1, AR.ROUND + 9, 0, 8, False),      # every thread once, thread 0 twice
         "round+1-vector": (174763, 24, 24, 32, 0, 8, True)}                                # 174763 x 3 = ROUND + 1 units of 8


@pytest.mark.parametrize("case", list(CASES))
def test_against_float64(case):
    rows, C, lda, ldb, offa, offb, vector = CASES[case]
    if case.startswith("round+1"):
        assert rows * (C // 8 if vector else C) == AR.ROUND + 1
    a, b = _views(rows, C, lda, ldb, offa, offb, seed=len(case))
    num, den = _check(a, b, vector, case)
    assert num > 0 and den > 0


def test_zero_sums_are_exact():
    a, b = _views(3, 320, 960, 640, 640, 320, seed=3)
    b.zero_()
    num, den = _check(a, b, True, "b == 0")
    assert den == 0.0 and num > 0
    a2, _ = _views(7, 321, 960, 640, 639, 319, seed=4)
    num, den = _check(a2, a2, False, "a is b")
    assert num == 0.0 and den > 0
    a3, b3 = _views(3, 320, 960, 640, 640, 320, seed=5)
    b3.copy_(a3)
    num, den = _check(a3, b3, True, "a == b")
    assert num == 0.0 and den > 0


@pytest.mark.parametrize("vector", [True, False])
def test_nan_and_inf_reach_the_output(vector):
    rows, C, lda, ldb, offa, offb, _ = CASES["3x320" if vector else "7x321-odd-C"]
    a, b = _views(rows, C, lda, ldb, offa, offb, seed=6)
    want_den = AR.rel_l1_f64(a, b)[1]
    a[rows - 1, C - 1] = float("nan")
    num, den = ops.rel_l1(a, b).tolist()
    assert math.isnan(num) and abs(den - want_den) <= (AR.rel_l1_depth(rows, C, vector) + 2) * U * want_den
    a[rows - 1, C - 1] = 0.0
    b[0, 0] = float("inf")
    num, den = ops.rel_l1(a, b).tolist()
    assert num == math.inf and den == math.inf


def test_refusals():
    from mikudance_amd import _lib
    a, b = _views(3, 320, 960, 640, 640, 320, seed=7)
    with pytest.raises(_lib.MdanceHipError, match="one shape"):
        ops.rel_l1(a, b[:2])
    with pytest.raises(_lib.MdanceHipError, match="torch.float16"):
        ops.rel_l1(a.float(), b.float())
    with pytest.raises(_lib.MdanceHipError, match="uniform pixel pitch"):
        ops.rel_l1(a[:, ::2], b[:, ::2])
    with pytest.raises(_lib.MdanceHipError, match="must live on the GPU"):
        ops.rel_l1(a.cpu(), b.cpu())
