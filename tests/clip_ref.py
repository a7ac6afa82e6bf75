"""Restatement of the CLIP vision tower's kernel-level pieces for tests/test_clip_kernels_gpu.py: plain PyTorch on the CPU, built from the
per-operator references of the other kernel tests (tests/norm_ref.py, tests/gemm_ref.py, tests/attention_ref.py) and nothing of
mikudance_amd/clip_vision.py.

`layer(x, w, heads, eps, exact)`  one CLIPEncoderLayer, x + attn(LN1(x)) then x + fc2(quick_gelu(fc1(LN2(x)))), on fp16-rounded weights and
input.  ROUNDING PLACEMENT: the product materialises an fp16 tensor after every operator, and each of them is an input of the next, so the
restatement rounds to fp16 at exactly those points -- the LayerNorm outputs, q | k, V, the attention output, the attention residual sum,
the fc1 output (after QuickGELU), the final sum -- and nowhere else.  A float64 chain without those roundings would differ from ANY
correct fp16 product by the seven intermediate roundings (about 3e-4 each, amplified by the LayerNorms), and a bound wide enough for
that would measure them and not the kernels.
    exact=True   every operator is its float64 reference (layernorm_reference, gemm_ref.reference, attention_ref.reference).
    exact=False  every operator is the fp32 emulation of the arithmetic include/mdance_hip.h documents for it (layernorm_emulation,
                 gemm_ref.emulation: fp32 accumulation and epilogue, one rounding; attention_ref.emulation: fp32 scores, P rounded to fp16
                 as the matrix core takes it, fp32 accumulation).  Its relative L2 against exact=True is the FLOOR of a layer case: what
                 a correct fp16 product costs on these very operands, computed from the references alone.
Both return the fp16 result as float64 / fp16 [L, C].

`patches(px, p)`  (1, 3, S, S) -> [grid^2, 3 p^2] rows (gy, gx), columns (c, ky, kx): the A operand of the patch embedding, written as a
reshape of the image and not through F.unfold (which the product uses)."""
import torch

import attention_ref
import gemm_ref
from norm_ref import layernorm_emulation, layernorm_reference

WEIGHTS = ("n1w", "n1b", "qw", "qb", "kw", "kb", "vw", "vb", "ow", "ob", "n2w", "n2b", "f1w", "f1b", "f2w", "f2b")


def layer_weights(dim, inner, seed):
    """fp16 CPU weights of one layer: Linear weights N(0, 1 / fan_in), biases N(0, 0.1^2), LayerNorm gamma 1 + 0.3 N, beta 0.5 N (as
    norm_ref.ln_problem)."""
    g = torch.Generator().manual_seed(seed)
    lin = lambda n, k: ((torch.randn(n, k, generator=g) * k ** -0.5).half(), (0.1 * torch.randn(n, generator=g)).half())
    w = {}
    for name, (n, k) in dict(q=(dim, dim), k=(dim, dim), v=(dim, dim), o=(dim, dim), f1=(inner, dim), f2=(dim, inner)).items():
        w[name + "w"], w[name + "b"] = lin(n, k)
    for name in ("n1", "n2"):
        w[name + "w"], w[name + "b"] = (1.0 + 0.3 * torch.randn(dim, generator=g)).half(), (0.5 * torch.randn(dim, generator=g)).half()
    assert sorted(w) == sorted(WEIGHTS)
    return w


def layer(x, w, heads, eps, exact):
    C = x.shape[1]
    D = C // heads
    ln = (lambda t, g, b: layernorm_reference(t, g, b, eps).half()) if exact else (lambda t, g, b: layernorm_emulation(t, g, b, eps))
    gemm = (lambda *a, **k: gemm_ref.reference(*a, **k).half()) if exact else gemm_ref.emulation
    attn = (lambda q, k, v: attention_ref.reference(q, k, v, heads, D).half()) if exact else (lambda q, k, v: attention_ref.emulation(q, k, v, heads, D))
    n = ln(x, w["n1w"], w["n1b"])
    q, k, v = gemm(n, w["qw"], bias=w["qb"]), gemm(n, w["kw"], bias=w["kb"]), gemm(n, w["vw"], bias=w["vb"])
    a = attn(q[None], k[None], v[None])
    x1 = gemm(a, w["ow"], bias=w["ob"], residual=x)
    n = ln(x1, w["n2w"], w["n2b"])
    h = gemm(n, w["f1w"], bias=w["f1b"], act=gemm_ref.ACT_QUICKGELU)
    out = gemm(h, w["f2w"], bias=w["f2b"], residual=x1)
    assert out.dtype == torch.float16
    return out.double() if exact else out


def patches(px, p):
    _, c, S, _ = px.shape
    g = S // p
    return px[0].reshape(c, g, p, g, p).permute(1, 3, 0, 2, 4).reshape(g * g, c * p * p)
