"""CPU: is the floor of tests/attention_ref.py a fair yardstick for the d = 40 kernels?  tests/test_attention_flavours_gpu.py requires
rel_l2(kernel) <= 2 x rel_l2(emulation), both against float64.  Here the kernel's place is taken by the CPU model of its softmax
bookkeeping (test_softmax_scheme_cpu.emulate: pre-scaled fp16 Q, reference four octaves above the maximum, lazy rescale by the OR test,
64-key tiles), on single-head versions of the shapes the GPU file runs.

Measured (rel L2 against float64; plain = emulation(fold=False), fold = emulation(fold=True)):
    case    plain      fold       scheme model   P cut to 8 bits
    257     2.75e-4    3.45e-4    3.50e-4        1.89e-3
    8       2.36e-4    2.75e-4    2.92e-4        1.53e-3
    320     2.75e-4    3.52e-4    3.58e-4        1.89e-3
    peaky   2.03e-4    3.73e-4    3.81e-4        1.12e-3
    q x 3   2.20e-4    4.23e-4    4.42e-4
The scheme is within 1.3 x the plain floor on N(0,1) rows but at 1.9-2.0 x on peaky ones (the fp16 rounding of the pre-scaled Q moves a
logit by ~|s| 2^-12), so the d = 8 / 40 cases of the DMA kernels take the fold floor: the scheme sits at 1.0-1.1 x of it, an 8-bit P at 3-5 x."""
import pytest
import torch

from attention_ref import FACTOR, emulation, reference, rel_l2, rnd
from test_softmax_scheme_cpu import emulate

D = 40
CASES = {"257": (257, False, 1.0), "8": (8, False, 1.0), "64": (64, False, 1.0), "72": (72, False, 1.0), "320": (320, False, 1.0),
         "peaky": (257, True, 1.0), "qx3": (257, False, 3.0)}


def _inputs(case):
    Lk, peaky, qs = CASES[case]
    Lq = 512
    q, k, v = rnd(1, Lq, D, seed=1, scale=qs), rnd(1, Lk, D, seed=2), rnd(1, Lk, D, seed=3)
    if peaky:                                   # as the GPU file's peaky case: one dominant key in tile 0, one in the last tile
        k[0, 300 % Lk] = 4 * q[0, 5]
        k[0, Lk - 1] = 5 * q[0, 500]
    return q, k, v


@pytest.mark.parametrize("case", list(CASES))
def test_scheme_model_stays_within_the_factor_of_the_fold_floor(case):
    q, k, v = _inputs(case)
    ref = reference(q, k, v, 1, D)
    floor = rel_l2(emulation(q, k, v, 1, D, fold=True), ref)
    plain = rel_l2(emulation(q, k, v, 1, D), ref)
    got, _ = emulate(q[0], k[0], v[0], D ** -0.5)
    scheme = rel_l2(got.half(), ref)
    print(f"\nPARITY_MEASURE attn_floor_cpu:{case} plain={plain:.6e} floor={floor:.6e} scheme={scheme:.6e}")
    assert 1e-4 < floor < 1e-3 and 1e-4 < plain < 1e-3     # a few fp16 roundings (2^-12 / sqrt(3) = 1.4e-4 each) per element, nothing else
    assert scheme <= FACTOR * floor, (scheme, floor)


@pytest.mark.parametrize("case", ["257", "8", "320", "peaky"])
def test_a_probability_cut_to_eight_bits_lands_above_the_factor(case):
    """The check bites: the same arithmetic with P truncated to 8 of its 11 significant bits (the degraded build of
    profiles/r06_parity_budget_degraded.log) exceeds FACTOR x floor."""
    q, k, v = _inputs(case)
    ref = reference(q, k, v, 1, D)
    floor = rel_l2(emulation(q, k, v, 1, D, fold=True), ref)
    sc2 = torch.tensor(D ** -0.5, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    s = (q[0].float() * sc2).half().float() @ k[0].float().t()
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values - 4.0).half()
    p = (p.view(torch.int16) & ~7).view(torch.float16).float()
    cut = rel_l2(((p @ v[0].float()) / p.sum(-1, keepdim=True)).half(), ref)
    assert cut > 1.4 * FACTOR * floor, (cut, floor)
