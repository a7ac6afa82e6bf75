"""TEST INFRASTRUCTURE: K / V token downsampling in spatial self-attention (ToDo: Token Downsampling, Smith et al., arXiv 2402.13573) as this
project defines it, stated in torch at the caller's dtype on top of oracle/cpu_ref.py, and a CPU emulation of the operator the feature adds
to mikudance_amd.ops, which tests/fake_ops.py installs with its own.

    pool(tokens, B, Hh, Ww, s, mode)                       the definition: F.interpolate(nearest) / F.avg_pool2d on the token grid
    level_of(prefix, levels), factor_of(...)               which resolution level a block's key prefix belongs to, on strings
    pooled(den_sd, factors, mode)                          context: the oracle's read blocks of the selected levels take K / V from the pooled source
    block_read(sd, p, x, ctx, bank, cfg, Hh, Ww, s, mode)  one read block with pooled K / V
    unet_forward(den_sd, x, t, ctx, banks, factors, mode, cfg)
    denoise_loop(..., kv_downsample=, mode=)               tests/fusion_ref.denoise_loop (tests/pag_ref.denoise_loop when pag_scale > 0);
                                                           with every factor 1 it is that loop op for op
    token_pool                                             the operator's emulation (installed by fake_ops.install)
    block_setup(...), block_runs(st, kv_pool)              one product TransformerBlock in every reference mode beside its restatement
The oracle is not edited: the pooled block and the patcher that swaps it in on the selected levels are tests/selfattn_ref.py's.
"""
import re

import torch
import torch.nn.functional as F

from oracle import cpu_ref as O

import fake_ops
import fusion_ref as FR
import selfattn_ref as SA


# ---- the definition
def pool(tokens, B, Hh, Ww, s, mode):
    """tokens (B, Hh*Ww, C) or [B*Hh*Ww, C] -> (B, (Hh // s) * (Ww // s), C): the token grid reduced by s per axis."""
    C = tokens.shape[-1]
    grid = tokens.reshape(B, Hh, Ww, C).permute(0, 3, 1, 2)
    if mode == "nearest":
        g = F.interpolate(grid, scale_factor=1.0 / s, mode="nearest")
    else:
        assert mode == "mean", mode
        g = F.avg_pool2d(grid, kernel_size=s, stride=s)
    assert tuple(g.shape[2:]) == (Hh // s, Ww // s), (tuple(g.shape), Hh, Ww, s)
    return g.permute(0, 2, 3, 1).reshape(B, -1, C)


def check_factors(factors):
    factors = (factors,) if isinstance(factors, int) else tuple(factors)
    assert all(isinstance(v, int) and 1 <= v <= 8 for v in factors), factors
    return factors


# ---- levels, on strings
def level_of(prefix, levels):
    """Resolution level of a block key prefix: down_blocks.I -> I, up_blocks.J -> levels - 1 - J, mid_block -> levels - 1."""
    m = re.match(r"^(down_blocks|up_blocks)\.(\d+)\.", prefix)
    if m:
        return int(m.group(2)) if m.group(1) == "down_blocks" else levels - 1 - int(m.group(2))
    assert prefix.startswith("mid_block."), prefix
    return levels - 1


def factor_of(prefix, factors, levels):
    lvl = level_of(prefix, levels)
    return factors[lvl] if lvl < len(factors) else 1


# ---- one block
def block_read(sd, p, x, ctx, bank, cfg, Hh, Ww, s, mode):
    """oracle transformer_block_read with the self-attention K / V source pooled: q from every token of norm1(x), k / v from
    pool(norm1(x) + bank) -- pooled AFTER the add -- and, under cfg, from pool(norm1(x)) on the unconditional first half."""
    return SA.block_read(sd, p, x, ctx, bank, cfg, (Hh, Ww), pool=(s, mode))


def pooled(den_sd, factors, mode="nearest"):
    """Within the block, the oracle's read blocks on a level with a factor > 1 take K / V from the pooled source (selfattn_ref.modified)."""
    return SA.modified(den_sd, pool=(factors, mode))


def unet_forward(den_sd, x, t, ctx, banks, factors, mode="nearest", cfg=True):
    """oracle.cpu_ref.denoising_unet_forward with K / V token downsampling."""
    with pooled(den_sd, factors, mode):
        return O.denoising_unet_forward(den_sd, x, t, ctx, banks, cfg=cfg)


# ---- the loop
def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, kv_downsample=1, mode="nearest", pag_scale=0.0, **kw):
    """tests/fusion_ref.denoise_loop (reduced=True) -- tests/pag_ref.denoise_loop when pag_scale > 0, where the unselected blocks of the
    perturbed evaluation pool like the main one -- with K / V token downsampling.  Every factor 1: that loop op for op."""
    factors = check_factors(kv_downsample)
    if pag_scale > 0:
        import pag_ref as P
        loop = lambda: P.denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, pag_scale=pag_scale, **kw)
    else:
        loop = lambda: FR.denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, reduced=True, **kw)
    if all(v == 1 for v in factors):
        return loop()
    with pooled(den_sd, factors, mode) as seen:
        out = loop()
    assert seen, "no block was pooled"
    return out


# ------------------------------------------------------------------ the operator, emulated like tests/fake_ops.py emulates the others
# Written from the entry point's contract in include/mdance_hip.h with slices, not with the two torch calls of pool() above: fp32 sum of the
# block in the order (dy, dx) ascending, times fp32(1 / s^2), ONE rounding; zero pad rows.
def token_pool(x, B, Hh, Ww, s, mode="nearest", out=None):
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float16 and x.shape[0] == B * Hh * Ww and mode in ("nearest", "mean")
    C = x.shape[1]
    assert 2 <= s <= 8 and C % 8 == 0
    Ho, Wo = Hh // s, Ww // s
    assert Ho >= 1 and Wo >= 1
    Lk = Ho * Wo
    stride = (Lk + 7) // 8 * 8
    g = x.view(B, Hh, Ww, C)[:, :Ho * s, :Wo * s]
    if mode == "nearest":
        y = g[:, ::s, ::s]
    else:
        acc = torch.zeros((B, Ho, Wo, C), dtype=torch.float32)
        for dy in range(s):
            for dx in range(s):
                acc = acc + g[:, dy::s, dx::s].float()
        y = (acc * torch.tensor(1.0 / (s * s), dtype=torch.float32)).to(torch.float16)
    if out is None:
        out = torch.empty((B * stride, C), dtype=torch.float16)
    assert out.is_contiguous() and tuple(out.shape) == (B * stride, C)
    o = out.view(B, stride, C)
    o[:, :Lk] = y.reshape(B, Lk, C)
    o[:, Lk:] = 0
    fake_ops.CALLS.append(("token_pool", (B, Hh, Ww, C, s, mode)))
    return out, Lk, stride


# ------------------------------------------------------------------ one TransformerBlock in every reference mode (CPU-emulated and GPU tests)
def block_setup(dim, dctx, Hh, Ww, f, device, seed=21):
    """One mikudance_amd TransformerBlock with seeded weights on `device`, and the inputs of a CFG batch of 2f frames on an Hh x Ww grid:
    -> namespace(blk, sd (fp32, fp16-rounded), x (2f, L, dim), bank (f, L, dim), ctx_f (2f, lk, dctx) per-frame context, cross, f, L)."""
    import types
    from mikudance_amd import blocks
    from mikudance_amd.synth import synth_state_dict
    L, lk, lpad = Hh * Ww, 5, 8
    blk = blocks.TransformerBlock(dim, dctx)
    sd = synth_state_dict({k: tuple(v.shape) for k, v in blk.state_dict().items()}, seed=seed)
    blk.load_state_dict(sd, strict=True)
    blk = blk.half().to(device).eval()
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn((2 * f, L, dim), generator=g).half()
    bank = (torch.randn((f, L, dim), generator=g) * 0.5).half()
    ctx = torch.randn((1, lk, dctx), generator=g).half()
    buf = torch.zeros((2, lpad, dctx), dtype=torch.float16)
    buf[1, :lk] = ctx[0]
    from mikudance_amd.blocks import CrossContext
    cross = CrossContext(buf.view(2 * lpad, dctx).to(device), torch.tensor([0] * f + [1] * f, dtype=torch.int32, device=device), lk, lpad, zero_frames=f)
    ctx_f = torch.cat([torch.zeros((f, lk, dctx)), ctx.float().repeat(f, 1, 1)])
    return types.SimpleNamespace(blk=blk, sd={k: v.half().float() for k, v in sd.items()}, x=x, bank=bank, ctx_f=ctx_f, cross=cross, f=f, L=L,
                                 Hh=Hh, Ww=Ww, dim=dim, device=device)


def block_runs(st, kv_pool):
    """selfattn_ref.block_runs of the block of block_setup with `kv_pool` ((Hh, Ww, s, mode) or None)."""
    return SA.block_runs(st) if kv_pool is None else SA.block_runs(st, tuple(kv_pool[:2]), pool=tuple(kv_pool[2:]))
