"""References for the kernel-level attention tests (tests/test_attention_flavours_gpu.py, tests/test_attention_floor_cpu.py); CPU only.

`reference`   float64 softmax(scale * Q K^T) V per (batch, head) on the fp16-rounded inputs, the kv_index gather applied here.
`emulation`   the arithmetic md_attention_fwd_f16 documents, in plain PyTorch and nothing of the kernels' structure: scores in fp32, P =
              exp(s - rowmax) rounded to fp16, P V and the denominator accumulated in fp32 from that fp16 P, output rounded to fp16.
`rel_l2`      relative L2 against the float64 reference.

rel_l2(emulation) is the FLOOR of a case: what a correct kernel of this arithmetic costs on these very inputs (about 2.8e-4: the output
rounding and the rounding of P, each ~2^-12 / sqrt(3) per element).  It is computed from the reference alone, never recorded from a
build, so a wrong kernel cannot bless itself.  A kernel passes with rel_l2 <= FACTOR x floor; FACTOR = 2.0 is parity_budget.FACTOR, the
project's allowance for accumulation-order noise.

fold=True models what attention_v2.h documents for the head dims with D % 16 == 8 (8, 40) on the DMA kernels: Q is multiplied by
scale * log2(e) and rounded to fp16 ONCE MORE before the matrix core, the exponential is base 2, and the softmax reference sits four
octaves above the row maximum (P <= 2^-4).  Measured on the CPU scheme model of tests/test_softmax_scheme_cpu.py against the plain floor
(tests/test_attention_floor_cpu.py has the figures): the four octaves cost nothing visible (2.744e-4 either way at Lk = 257), the extra
rounding of Q moves every logit by ~|s| 2^-12 and takes a correct kernel to 1.3 x the plain floor on N(0,1) rows and to 1.9-2.5 x on
peaky rows -- past the factor.  So those cases take their floor from this model; it still has nothing of the kernels' tiling, lazy
rescale or key order in it, and P cut to 8 significant bits lands at 3-5 x this floor."""
import torch

FACTOR = 2.0


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def _heads(x, H, D):                       # [n, L, H*D] -> [n, H, L, D]
    n, L, _ = x.shape
    return x.view(n, L, H, D).transpose(1, 2)


def reference(q, k, v, H, D, kv_index=None, scale=None):
    """q [B, Lq, H*D], k / v [nkv, Lk, H*D] fp16 -> float64 [B*Lq, H*D]."""
    B, Lq, C = q.shape
    scale = D ** -0.5 if scale is None else scale
    out = torch.empty(B, Lq, C, dtype=torch.float64)
    for b in range(B):
        kb = b if kv_index is None else int(kv_index[b])
        qh, kh, vh = _heads(q[b:b + 1].double(), H, D)[0], _heads(k[kb:kb + 1].double(), H, D)[0], _heads(v[kb:kb + 1].double(), H, D)[0]
        a = torch.softmax((qh @ kh.transpose(1, 2)) * scale, dim=-1)
        out[b] = (a @ vh).transpose(0, 1).reshape(Lq, C)
    return out.view(B * Lq, C)


def emulation(q, k, v, H, D, kv_index=None, scale=None, fold=False):
    """Same operands -> fp16 [B*Lq, H*D] by the documented arithmetic (see the module docstring)."""
    B, Lq, C = q.shape
    scale = D ** -0.5 if scale is None else scale
    sc2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)    # fp32 product, as the library forms it
    out = torch.empty(B, Lq, C, dtype=torch.float16)
    for b in range(B):
        kb = b if kv_index is None else int(kv_index[b])
        qh, kh, vh = _heads(q[b:b + 1].float(), H, D)[0], _heads(k[kb:kb + 1].float(), H, D)[0], _heads(v[kb:kb + 1].float(), H, D)[0]
        if fold:
            s = (qh * sc2).half().float() @ kh.transpose(1, 2)                  # Q pre-scaled and rounded to fp16, scores in fp32 (base 2)
            p = torch.exp2(s - s.max(dim=-1, keepdim=True).values - 4.0).half().float()
        else:
            s = (qh @ kh.transpose(1, 2)) * scale                               # fp32
            p = torch.exp(s - s.max(dim=-1, keepdim=True).values).half().float()    # P rounded to fp16
        o = (p @ vh) / p.sum(dim=-1, keepdim=True)                              # fp32 accumulation, the denominator from the same P
        out[b] = o.half().transpose(0, 1).reshape(Lq, C)
    return out.view(B * Lq, C)


def rel_l2(got, ref64):
    g, r = got.detach().double().cpu(), ref64.double()
    return float((g - r).norm() / r.norm())
