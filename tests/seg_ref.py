"""TEST INFRASTRUCTURE: smoothed-energy guidance (SEG; Hong, arXiv 2408.00760) as this project defines it -- the float64 definition of the query
blur, a float32 restatement of the separable algorithm the kernel runs, the perturbed block and the loop stated in torch on top of
oracle/cpu_ref.py, and a CPU emulation of ops.token_blur, which tests/fake_ops.py installs with its own.

    kernel_size(sigma, n), taps(sigma, n), reflect(i, n)    the clamp rule, the normalised Gaussian (float64), torch's "reflect" index
    blur64(x, B, Hh, Ww, sigma)                             the definition: a direct 2-D reflect-padded convolution with the outer-product
                                                            kernel (the official gaussian_blur_2d's literal form, NOT separable); inf: the mean
    blur32(x, B, Hh, Ww, sigma)                             float32, separable, x axis first, taps added in ascending order, fp32 between the axes
    block_read(sd, p, x, ctx, bank, Hh, Ww, sigma, kv_pool) the perturbed conditional read block with blurred queries
    perturbed_forward(...), denoise_loop(..., seg_scale=, seg_blur_sigma=, seg_layers=)   tests/pag_ref.denoise_loop with SEG's perturbation
    token_blur                                              the operator's emulation (installed by fake_ops.install)
The oracle is not edited: the perturbed block and the patcher that swaps it in for the selected prefixes are tests/selfattn_ref.py's.
"""
import math

import torch

from oracle import cpu_ref as O

import fake_ops
import pag_ref as P
import selfattn_ref as SA
import todo_ref as T


# ---- the definition
def kernel_size(sigma, n):
    """ceil(6 sigma) + 1 - ceil(6 sigma) % 2 (the official rule), clamped to n if n is odd else n + 1 (what reflect padding of n allows)."""
    c = math.ceil(6.0 * sigma)
    return min(c + 1 - c % 2, n if n % 2 else n + 1)


def taps(sigma, n):
    """float64 tensor of kernel_size(sigma, n) taps, exp(-(j / sigma)^2 / 2) over j = -r..r, normalised."""
    r = kernel_size(sigma, n) // 2
    j = torch.arange(-r, r + 1, dtype=torch.float64)
    w = torch.exp(-0.5 * (j / sigma) ** 2)
    return w / w.sum()


def reflect(i, n):
    """torch's "reflect" padding index (the edge is not repeated)."""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    assert 0 <= i < n, (i, n)
    return i


def blur64(x, B, Hh, Ww, sigma):
    """x [B*Hh*Ww, C] (any dtype) -> float64 [B*Hh*Ww, C]."""
    C = x.shape[-1]
    g = x.double().reshape(B, Hh, Ww, C)
    if math.isinf(sigma):
        return g.mean(dim=(1, 2), keepdim=True).expand(B, Hh, Ww, C).reshape(B * Hh * Ww, C)
    wy, wx = taps(sigma, Hh), taps(sigma, Ww)
    ry, rx = len(wy) // 2, len(wx) // 2
    k2 = wy[:, None] * wx[None, :]                                         # the outer-product kernel
    iy = torch.tensor([[reflect(y + j - ry, Hh) for j in range(len(wy))] for y in range(Hh)])      # [Hh, ky]
    ix = torch.tensor([[reflect(x_ + j - rx, Ww) for j in range(len(wx))] for x_ in range(Ww)])    # [Ww, kx]
    out = torch.zeros_like(g)
    for a in range(len(wy)):
        rows = g[:, iy[:, a]]                                              # (B, Hh, Ww, C)
        for b in range(len(wx)):
            out += k2[a, b] * rows[:, :, ix[:, b]]
    return out.reshape(B * Hh * Ww, C)


def blur32(x, B, Hh, Ww, sigma):
    """The algorithm of md_token_blur_f16 / md_token_mean_f16 in float32 (before the final rounding): fp16 in, x axis first, taps in
    ascending order, fp32 between the axes.  The mean: a float32 sum over the tokens times fp32(1 / L)."""
    C = x.shape[-1]
    g = x.float().reshape(B, Hh, Ww, C)
    if math.isinf(sigma):
        m = g.sum(dim=(1, 2), keepdim=True) * torch.tensor(1.0 / (Hh * Ww), dtype=torch.float32)
        return m.expand(B, Hh, Ww, C).reshape(B * Hh * Ww, C)
    wy, wx = taps(sigma, Hh).float(), taps(sigma, Ww).float()
    ry, rx = len(wy) // 2, len(wx) // 2
    t = torch.zeros_like(g)
    for j in range(len(wx)):
        t = t + wx[j] * g[:, :, [reflect(x_ + j - rx, Ww) for x_ in range(Ww)]]
    out = torch.zeros_like(g)
    for j in range(len(wy)):
        out = out + wy[j] * t[:, [reflect(y + j - ry, Hh) for y in range(Hh)]]
    return out.reshape(B * Hh * Ww, C)


def ulp16(v):
    """The spacing of fp16 at |v| (float64 tensor), subnormal spacing below 2^-14."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return 2.0 ** (e - 10)


def bound(x, B, Hh, Ww, sigma):
    """(ref64, per-element bound): half an fp16 ulp of the reference plus 4 x the largest error of the float32 restatement over the tensor
    (the rule of tests/test_free_init_gpu.py for the DFT mix; the 4 allows another summation order)."""
    ref = blur64(x, B, Hh, Ww, sigma)
    e32 = float((blur32(x, B, Hh, Ww, sigma).double() - ref).abs().max())
    return ref, 0.5 * ulp16(ref) + 4.0 * e32


# ---- the perturbed block
def block_read(sd, p, x, ctx, bank, Hh, Ww, sigma, kv_pool=None):
    """oracle transformer_block_read(cfg=False) with the QUERIES blurred over the Hh x Ww grid: q = blur(to_q(norm1(x))), k / v from
    norm1(x) + bank (pooled by kv_pool = (s, mode) AFTER the add, when given)."""
    return SA.block_read(sd, p, x, ctx, bank, False, (Hh, Ww), sigma=sigma, pool=kv_pool)


def perturbed(selected, sigma):
    """Within the block, the oracle's read blocks whose key prefix is in `selected` blur their queries (selfattn_ref.modified)."""
    return SA.modified(blur=selected, sigma=sigma)


def perturbed_forward(den_sd, x, t, ctx, banks, names, sigma):
    sel = P.select(P.block_prefixes(den_sd), names)
    with perturbed(sel, sigma) as seen:
        out = O.denoising_unet_forward(den_sd, x, t, ctx, banks, cfg=False)
    assert sorted(s[0] for s in seen) == sorted(p + ".transformer_blocks.0." for p in sel), (seen, sel)
    return out


def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, seg_scale=0.0, seg_blur_sigma=100.0, seg_layers=("mid",),
                 kv_downsample=1, **kw):
    """tests/pag_ref.denoise_loop with SEG's perturbed evaluation in place of PAG's (the combination rule, the extra plane and the step are
    PAG's with s = seg_scale at every step); seg_scale = 0 is tests/fusion_ref.denoise_loop op for op.  kv_downsample: tests/todo_ref.pooled
    around it (the selected blocks must lie on levels whose factor is 1)."""
    orig = P.perturbed_forward
    P.perturbed_forward = lambda den_sd_, x, t, ctx, banks, names: perturbed_forward(den_sd_, x, t, ctx, banks, names, seg_blur_sigma)
    try:
        run = lambda: P.denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, pag_scale=seg_scale, pag_layers=seg_layers, **kw)
        factors = T.check_factors(kv_downsample)
        if all(v == 1 for v in factors):
            return run()
        with T.pooled(den_sd, factors, "nearest"):
            return run()
    finally:
        P.perturbed_forward = orig


# ------------------------------------------------------------------ the operator, emulated like tests/fake_ops.py emulates the others
def token_blur(x, B, Hh, Ww, sigma, out=None):
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float16 and x.shape[0] == B * Hh * Ww and x.shape[1] % 8 == 0
    assert isinstance(sigma, (int, float)) and sigma > 0
    y = blur32(x, B, Hh, Ww, float(sigma)).to(torch.float16)
    fake_ops.CALLS.append(("token_blur", (B, Hh, Ww, x.shape[1], float(sigma))))
    if out is None:
        return y
    assert out.is_contiguous() and out.shape == x.shape and out.data_ptr() != x.data_ptr()
    out.copy_(y)
    return out
