"""TEST INFRASTRUCTURE: shifted-tile spatial self-attention (tile_attention=; MSW-MSA of HiDiffusion, Zhang et al., arXiv 2311.17528) as this
project defines it, stated in torch at the caller's dtype on top of oracle/cpu_ref.py, and a CPU emulation of the operator the feature adds
to mikudance_amd.ops.  The tests that need them install the emulations themselves (install / install_process), on top of fake_ops.install or
after loop_helpers.worker_setup in a spawned worker.

    tile(tokens, B, Hh, Ww, t, shift), untile(...)         the definition: torch.roll(grid, (-sy, -sx), (1, 2)) and a plain partition
    shift_at(mode, k, th, tw)                              the step's shift: "cycle": q = k mod 4, (q th // 4, q tw // 4); "none": (0, 0)
    block_read(sd, p, x, ctx, bank, cfg, Hh, Ww, t, shift, pool, sigma)   one read block attending per shifted tile
    tiled(den_sd, factors, shift, first_step, kv)          context: the oracle's read blocks of the selected levels attend per shifted tile
    unet_forward(den_sd, x, t, ctx, banks, factors, shift=(mode, k), cfg)
    denoise_loop(..., tile_attention=, tile_attention_shift=)   the restated loops of tests/*_ref.py under tiled(); every factor 1: that loop op for op
    token_tile, token_untile                               the operator's emulation, from the contract in include/mdance_hip.h, with slices
    install(monkeypatch), install_process()                the emulations over mikudance_amd.ops; every attention / token_tile / token_untile call is
                                                           also noted with the TransformerBlock that made it (BLOCK_CALLS)
    block_runs(st, tile, ...)                              todo_ref.block_runs with the tile field
The oracle is not edited: the tiled block and the patcher that swaps it in on the selected levels are tests/selfattn_ref.py's.
"""
import torch

from oracle import cpu_ref as O

import fake_ops
import fusion_ref as FR
import selfattn_ref as SA
import todo_ref as T


# ---- the definition
def tile(tokens, B, Hh, Ww, t, shift=(0, 0)):
    """tokens (B, Hh*Ww, C) or [B*Hh*Ww, C] -> (B*t*t, th*tw, C): tile (b, j, i) is item (b*t + j)*t + i of the rolled grid's partition."""
    C = tokens.shape[-1]
    th, tw = Hh // t, Ww // t
    g = torch.roll(tokens.reshape(B, Hh, Ww, C), (-shift[0], -shift[1]), (1, 2))
    return g.reshape(B, t, th, t, tw, C).permute(0, 1, 3, 2, 4, 5).reshape(B * t * t, th * tw, C)


def untile(tiles, B, Hh, Ww, t, shift=(0, 0)):
    """The inverse of tile: (B*t*t, th*tw, C) -> (B, Hh*Ww, C)."""
    C = tiles.shape[-1]
    th, tw = Hh // t, Ww // t
    g = tiles.reshape(B, t, t, th, tw, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hh, Ww, C)
    return torch.roll(g, (shift[0], shift[1]), (1, 2)).reshape(B, Hh * Ww, C)


def shift_at(mode, k, th, tw):
    assert mode in ("cycle", "none"), mode
    q = k % 4 if mode == "cycle" else 0
    return (q * th // 4, q * tw // 4)


# ---- one block
def block_read(sd, p, x, ctx, bank, cfg, Hh, Ww, t, shift, pool=None, sigma=None):
    """oracle transformer_block_read with the self-attention run inside every shifted tile: q from tile(norm1(x)) -- with sigma, from
    tile(blur(to_q(norm1(x)))), blurred over the whole frame grid first -- k / v from tile(norm1(x) + bank), pooled per tile by
    pool = (s, mode) when given; the output goes back to frame order in front of to_out.  Under cfg the unconditional first half attends
    to tile(norm1(x)) alone."""
    return SA.block_read(sd, p, x, ctx, bank, cfg, (Hh, Ww), sigma=sigma, pool=pool, tile=(t, shift))


def tiled(den_sd, factors, shift="cycle", first_step=0, kv=None, step=None):
    """Within the block, the oracle's read blocks on a level with a factor > 1 attend per shifted tile (selfattn_ref.modified, which states
    the step index); kv = (factors, mode): those levels' K / V are pooled inside each tile."""
    return SA.modified(den_sd, pool=kv, tile=factors, shift=shift, first_step=first_step, step=step)


def unet_forward(den_sd, x, t, ctx, banks, factors, shift=("none", 0), cfg=True):
    """oracle.cpu_ref.denoising_unet_forward with shifted-tile self-attention at step shift[1] of mode shift[0]."""
    with tiled(den_sd, factors, shift[0], step=shift[1]):
        return O.denoising_unet_forward(den_sd, x, t, ctx, banks, cfg=cfg)


def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, tile_attention=1, tile_attention_shift="cycle", kv_downsample=1,
                 kv_mode="nearest", pag_scale=0.0, pag_layers=("mid",), seg_scale=0.0, seg_blur_sigma=100.0, seg_layers=("mid",),
                 init_latents=None, strength=1.0, free_init_iters=1, **kw):
    """The restated loop of the feature the keywords ask for -- tests/fusion_ref.denoise_loop (reduced=True), tests/pag_ref.denoise_loop
    (pag_scale / seg_scale > 0; a PAG-selected block has no attention to tile, a SEG-selected one blurs then tiles, the unselected blocks
    of the perturbed evaluation tile like the main one), tests/v2v_ref.denoise_loop (init_latents; the step index starts at the first kept
    step), tests/free_init_ref.denoise_loop (free_init_iters > 1; every pass starts over) -- with shifted-tile self-attention and kv_downsample's
    pooling in one selfattn_ref.modified block around it.  Every tile factor 1: that loop op for op."""
    import pag_ref as P
    factors, kvf = T.check_factors(tile_attention), T.check_factors(kv_downsample)
    first = 0
    if free_init_iters > 1:
        import free_init_ref as FI
        gen = kw.pop("generator")
        mk = kw.pop("make_scheduler", None)
        loop = lambda: FI.denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, free_init_iters, gen, make_scheduler=mk, reduced=True, **kw)
    elif init_latents is not None:
        import v2v_ref as V
        first = num_steps - V.kept_steps(num_steps, strength)
        loop = lambda: V.denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, init_latents, strength, reduced=True, **kw)
    elif seg_scale > 0:
        loop = lambda: P.denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, pag_scale=seg_scale, pag_layers=seg_layers, **kw)
    elif pag_scale > 0:
        loop = lambda: P.denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, pag_scale=pag_scale, pag_layers=pag_layers, **kw)
    else:
        loop = lambda: FR.denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, reduced=True, **kw)
    orig = P.perturbed_forward
    if seg_scale > 0:                                                 # a selected block blurs over the whole frame, then tiles
        import seg_ref as S
        P.perturbed_forward = lambda sd, x, t, ctx, banks, names: S.perturbed_forward(sd, x, t, ctx, banks, names, seg_blur_sigma)
    try:
        with SA.modified(den_sd, pool=(kvf, kv_mode), tile=factors, shift=tile_attention_shift, first_step=first) as seen:
            out = loop()
        assert all(v == 1 for v in factors) or any("tile" in s[3] for s in seen), "no block was tiled"
        return out
    finally:
        P.perturbed_forward = orig


# ------------------------------------------------------------------ the operator, emulated like tests/fake_ops.py emulates the others
# Written from the entry point's contract in include/mdance_hip.h with slices, not with the roll / reshape of tile() above: tile (b, j, i)
# row r * tw + c holds the token at ((j th + r + sy) mod Hh, (i tw + c + sx) mod Ww); an axis run that crosses the frame edge is two slices.
def _runs(start, length, n):
    """[(offset inside the run, first source index, count)] of the `length` indices (start + k) mod n, k = 0.., as at most two slices."""
    start %= n
    first = min(length, n - start)
    return [(0, start, first)] + ([(first, 0, length - first)] if first < length else [])


def _tile_copy(frame, tiles, B, Hh, Ww, t, shift, inverse):
    """frame (B, Hh, Ww, C), tiles (B*t*t, tile_stride, C): copy the tokens tile by tile, frame -> tiles or (inverse) tiles -> frame."""
    th, tw = Hh // t, Ww // t
    for j in range(t):
        for i in range(t):
            item = tiles[j * t + i::t * t][:, :th * tw].unflatten(1, (th, tw))          # tile (., j, i) of every frame, (B, th, tw, C)
            for ry, y0, ny in _runs(j * th + shift[0], th, Hh):
                for rx, x0, nx in _runs(i * tw + shift[1], tw, Ww):
                    a, b = frame[:, y0:y0 + ny, x0:x0 + nx], item[:, ry:ry + ny, rx:rx + nx]
                    if inverse:
                        a.copy_(b)
                    else:
                        b.copy_(a)


def _tile_args(x, B, Hh, Ww, t, shift, tile_stride, rows_of):
    assert x.dim() == 2 and x.is_contiguous() and x.dtype == torch.float16 and x.shape[1] % 8 == 0
    assert 2 <= t <= 8 and Hh % t == 0 and Ww % t == 0 and 0 <= shift[0] < Hh and 0 <= shift[1] < Ww, (Hh, Ww, t, shift)
    Lt = (Hh // t) * (Ww // t)
    tile_stride = Lt if tile_stride is None else tile_stride
    assert tile_stride >= Lt and x.shape[0] == rows_of(tile_stride), (tuple(x.shape), tile_stride)
    return Lt, tile_stride


def token_tile(x, B, Hh, Ww, t, shift=(0, 0), tile_stride=None, out=None):
    Lt, tile_stride = _tile_args(x, B, Hh, Ww, t, shift, tile_stride, lambda s: B * Hh * Ww)
    C = x.shape[1]
    if out is None:
        out = torch.empty((B * t * t * tile_stride, C), dtype=torch.float16)
    assert out.is_contiguous() and tuple(out.shape) == (B * t * t * tile_stride, C)
    o = out.view(B * t * t, tile_stride, C)
    o[:, Lt:] = 0
    _tile_copy(x.view(B, Hh, Ww, C), o, B, Hh, Ww, t, shift, False)
    _note("token_tile", (B, Hh, Ww, C, t, tuple(shift), tile_stride))
    return out, Lt, tile_stride


def token_untile(x, B, Hh, Ww, t, shift=(0, 0), tile_stride=None, out=None):
    Lt, tile_stride = _tile_args(x, B, Hh, Ww, t, shift, tile_stride, lambda s: B * t * t * s)
    C = x.shape[1]
    if out is None:
        out = torch.empty((B * Hh * Ww, C), dtype=torch.float16)
    assert out.is_contiguous() and tuple(out.shape) == (B * Hh * Ww, C)
    _tile_copy(out.view(B, Hh, Ww, C), x.view(B * t * t, tile_stride, C), B, Hh, Ww, t, shift, True)
    _note("token_untile", (B, Hh, Ww, C, t, tuple(shift), tile_stride))
    return out


# ---- installing them, and noting which TransformerBlock called what
BLOCK_CALLS = []        # (TransformerBlock or None, name, detail) of every attention / token_tile / token_untile call
_CURRENT = []


def _note(name, detail):
    fake_ops.CALLS.append((name, detail))
    BLOCK_CALLS.append((_CURRENT[-1] if _CURRENT else None, name, detail))


def _wrappers(ops, blocks):
    real_attention, real_forward = ops.attention, blocks.TransformerBlock.forward

    def attention(q, k, vt, B, H, D, Lq, Lk, kv_stride=None, kv_index=None, **kw):
        _note("attention", (B, Lq, Lk, kv_stride, kv_index is not None, tuple(k.shape), tuple(vt.shape)))
        return real_attention(q, k, vt, B, H, D, Lq, Lk, kv_stride=kv_stride, kv_index=kv_index, **kw)

    def forward(self, *a, **kw):
        _CURRENT.append(self)
        try:
            return real_forward(self, *a, **kw)
        finally:
            _CURRENT.pop()

    return attention, forward


def install(monkeypatch):
    """After fake_ops.install(monkeypatch): the two emulations, and attention / TransformerBlock.forward wrapped so that every call is noted."""
    from mikudance_amd import blocks, ops
    attention, forward = _wrappers(ops, blocks)
    monkeypatch.setattr(ops, "token_tile", token_tile, raising=False)
    monkeypatch.setattr(ops, "token_untile", token_untile, raising=False)
    monkeypatch.setattr(ops, "attention", attention)
    monkeypatch.setattr(blocks.TransformerBlock, "forward", forward)
    del BLOCK_CALLS[:], fake_ops.CALLS[:]


def install_process():
    """The same for a whole (spawned worker) process, after loop_helpers.worker_setup."""
    from mikudance_amd import blocks, ops
    attention, forward = _wrappers(ops, blocks)
    ops.token_tile, ops.token_untile, ops.attention = token_tile, token_untile, attention
    blocks.TransformerBlock.forward = forward
    del BLOCK_CALLS[:], fake_ops.CALLS[:]


def clear():
    del BLOCK_CALLS[:], fake_ops.CALLS[:]


# ------------------------------------------------------------------ one TransformerBlock in every reference mode (CPU-emulated and GPU tests)
def block_runs(st, tile_spec, kv_pool=None, sigma=None):
    """selfattn_ref.block_runs of the block of todo_ref.block_setup with tile_spec = (t, (sy, sx)) or None and kv_pool = (s, mode) or None."""
    return SA.block_runs(st, (st.Hh, st.Ww), pool=kv_pool, tile=tile_spec, sigma=sigma)
