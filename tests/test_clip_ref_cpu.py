"""CPU: the yardstick of tests/test_clip_kernels_gpu.py.  tests/clip_ref.py chains the per-operator references of the kernel tests into one
CLIPEncoderLayer; here that chain is held against the layer written out with torch.nn.functional in float64 WITHOUT the intermediate fp16
roundings (so the two differ by those roundings and by nothing structural: a swapped weight, a wrong head split or the residual taken
from the wrong tensor would be orders of magnitude above the bound), the floor is in the range its docstring explains, and the patch
matrix agrees with F.unfold."""
import torch
import torch.nn.functional as F

import clip_ref
from attention_ref import rel_l2
from norm_ref import LN, ln_problem

EPS = 1e-5


def _layer_functional(x, w, heads):
    d = {k: v.double() for k, v in w.items()}
    L, C = x.shape
    x = x.double()
    n = F.layer_norm(x, (C,), d["n1w"], d["n1b"], EPS)
    split = lambda t: t.view(L, heads, C // heads).transpose(0, 1)
    q, k, v = split(F.linear(n, d["qw"], d["qb"])), split(F.linear(n, d["kw"], d["kb"])), split(F.linear(n, d["vw"], d["vb"]))
    a = torch.softmax(q @ k.transpose(1, 2) * (C // heads) ** -0.5, dim=-1) @ v
    x = x + F.linear(a.transpose(0, 1).reshape(L, C), d["ow"], d["ob"])
    h = F.linear(F.layer_norm(x, (C,), d["n2w"], d["n2b"], EPS), d["f1w"], d["f1b"])
    return x + F.linear(h * torch.sigmoid(1.702 * h), d["f2w"], d["f2b"])


def test_layer_restatement_is_a_clip_encoder_layer_and_its_floor_is_a_few_flipped_roundings():
    dim, inner, heads, L = 128, 256, 4, 17
    w = clip_ref.layer_weights(dim, inner, seed=9100 + dim)
    x = ln_problem(LN("clip layer input", L, dim, 0, EPS)).x
    ref = clip_ref.layer(x, w, heads, EPS, exact=True)
    plain = _layer_functional(x, w, heads)
    floor = rel_l2(clip_ref.layer(x, w, heads, EPS, exact=False), ref)
    print(f"\nPARITY_MEASURE clip_ref_cpu:layer dim={dim} L={L} roundings={rel_l2(ref, plain):.6e} floor={floor:.6e}")
    assert ref.dtype == torch.float64 and ref.shape == plain.shape
    assert rel_l2(ref, plain) < 2e-3                       # seven fp16 roundings of O(1) tensors; a structural slip is > 1e-1
    assert torch.equal(ref, ref.half().double())           # the final sum is rounded to fp16 too
    # value and floor consist of the elements whose last rounding fell the other way (measured: 40 % of them, floor 3.2e-4): one whole ulp
    # each, sqrt(12) x the 2.07e-4 of a plain output rounding if EVERY element flipped
    assert 0 < floor < 12 ** 0.5 * 2.07e-4


def test_patches_are_unfold():
    px = torch.randn(1, 3, 56, 56, generator=torch.Generator().manual_seed(5)).half()
    assert torch.equal(clip_ref.patches(px, 14), F.unfold(px.float(), kernel_size=14, stride=14)[0].t().half())
