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
The oracle is not edited: inside `tiled(...)`, and in this process only, its denoising_unet_forward is wrapped to note the timestep, its
transformer_3d to note the grid, and its transformer_block_read is swapped for block_read on the selected prefixes.
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import cpu_ref as O

import fake_ops
import fusion_ref as FR
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
def block_read(sd, p, x, ctx, bank, cfg, Hh, Ww, t, shift, pool=None, sigma=None, heads=O.HEADS):
    """oracle transformer_block_read with the self-attention run inside every shifted tile: q from tile(norm1(x)) -- with sigma, from
    tile(blur(to_q(norm1(x)))), blurred over the whole frame grid first -- k / v from tile(norm1(x) + bank), pooled per tile by
    pool = (s, mode) when given; the output goes back to frame order in front of to_out.  Under cfg the unconditional first half attends
    to tile(norm1(x)) alone."""
    B, L, C = x.shape
    th, tw = Hh // t, Ww // t
    a = p + "attn1."
    d = C // heads
    n = O.layer_norm(sd, p + "norm1.", x)

    def attend(nq, kv):
        b = nq.shape[0]
        q = F.linear(nq, sd[a + "to_q.weight"])
        if sigma is not None:
            import seg_ref
            q = seg_ref.blur64(q.reshape(b * L, C), b, Hh, Ww, sigma).to(q.dtype).reshape(b, L, C)
        q, kv = tile(q, b, Hh, Ww, t, shift), tile(kv, b, Hh, Ww, t, shift)
        if pool is not None:
            kv = T.pool(kv, b * t * t, th, tw, *pool)
        k, v = F.linear(kv, sd[a + "to_k.weight"]), F.linear(kv, sd[a + "to_v.weight"])
        q, k, v = (z.view(b * t * t, -1, heads, d).transpose(1, 2) for z in (q, k, v))
        o = O._sdpa(q, k, v).transpose(1, 2).reshape(b * t * t, th * tw, C)
        return F.linear(untile(o, b, Hh, Ww, t, shift), sd[a + "to_out.0.weight"], sd[a + "to_out.0.bias"])

    h = attend(n, n + bank if bank is not None else n) + x
    if cfg:
        half = B // 2
        h = h.clone()
        h[:half] = attend(n[:half], n[:half]) + x[:half]
    x = h
    x = O.attention(sd, p + "attn2.", O.layer_norm(sd, p + "norm2.", x), ctx) + x
    x = O.feed_forward(sd, p + "ff.", O.layer_norm(sd, p + "norm3.", x)) + x
    return x


@contextlib.contextmanager
def tiled(den_sd, factors, shift="cycle", first_step=0, kv=None, step=None):
    """Within the block, the oracle's read blocks on a level with a factor > 1 attend per shifted tile.  The step index of an evaluation is
    first_step + the position of its timestep among the distinct timesteps seen so far (a FreeInit pass sees the same ones again), or
    `step` where given (one forward outside a loop).  kv = (factors, mode): those levels' K / V are pooled inside each tile.  Yields the list
    of (prefix, Hh, Ww, t, (sy, sx)) of every block evaluated that way."""
    factors = T.check_factors(factors)
    levels = O._n_levels(den_sd)
    assert len(factors) <= levels, (factors, levels)
    kv_factors, kv_mode = (T.check_factors(kv[0]), kv[1]) if kv is not None else ((), "nearest")
    orig_fwd, orig_t3d, orig_read = O.denoising_unet_forward, O.transformer_3d, O.transformer_block_read
    grid, seen, order, now = [], [], {}, []

    def forward(sd, sample, t, *a, **kw):
        key = float(torch.as_tensor(t).reshape(-1)[0])
        now.append(step if step is not None else first_step + order.setdefault(key, len(order)))
        try:
            return orig_fwd(sd, sample, t, *a, **kw)
        finally:
            now.pop()

    def transformer_3d(sd, p, x, ctx_per_frame, bank, cfg):
        grid.append(tuple(x.shape[2:]))
        try:
            return orig_t3d(sd, p, x, ctx_per_frame, bank, cfg)
        finally:
            grid.pop()

    def read(sd, p, x, ctx, bank, cfg=True, sigma=None):
        t = T.factor_of(p, factors, levels)
        if t == 1:
            assert sigma is None
            return orig_read(sd, p, x, ctx, bank, cfg)
        Hh, Ww = grid[-1]
        s = T.factor_of(p, kv_factors, levels) if kv_factors else 1
        sh = shift_at(shift, now[-1], Hh // t, Ww // t)
        seen.append((p, Hh, Ww, t, sh))
        return block_read(sd, p, x, ctx, bank, cfg, Hh, Ww, t, sh, pool=(s, kv_mode) if s > 1 else None, sigma=sigma)

    read.grid = grid
    O.denoising_unet_forward, O.transformer_3d, O.transformer_block_read = forward, transformer_3d, read
    try:
        yield seen
    finally:
        O.denoising_unet_forward, O.transformer_3d, O.transformer_block_read = orig_fwd, orig_t3d, orig_read


def unet_forward(den_sd, x, t, ctx, banks, factors, shift=("none", 0), cfg=True):
    """oracle.cpu_ref.denoising_unet_forward with shifted-tile self-attention at step shift[1] of mode shift[0]."""
    with tiled(den_sd, factors, shift[0], step=shift[1]):
        return O.denoising_unet_forward(den_sd, x, t, ctx, banks, cfg=cfg)


def _seg_forward(den_sd, x, t, ctx, banks, names, sigma, factors):
    """seg_ref.perturbed_forward under tiled(): a selected block on a tiled level blurs over the whole frame, then tiles."""
    import pag_ref as P
    import seg_ref as S
    sel = P.select(P.block_prefixes(den_sd), names)
    keys = {p + ".transformer_blocks.0." for p in sel}
    levels = O._n_levels(den_sd)
    outer = O.transformer_block_read                                  # tiled()'s read

    def read(sd, p, x_, ctx_, bank, cfg=True):
        if p not in keys:
            return outer(sd, p, x_, ctx_, bank, cfg)
        assert not cfg, "the perturbed evaluation is conditional-only"
        if T.factor_of(p, factors, levels) > 1:
            return outer(sd, p, x_, ctx_, bank, cfg, sigma=sigma)
        Hh, Ww = outer.grid[-1]
        return S.block_read(sd, p, x_, ctx_, bank, Hh, Ww, sigma)

    O.transformer_block_read = read
    try:
        return O.denoising_unet_forward(den_sd, x, t, ctx, banks, cfg=False)
    finally:
        O.transformer_block_read = outer


def denoise_loop(ref_sd, den_sd, latents, ref_latents, embeds, num_steps, tile_attention=1, tile_attention_shift="cycle", kv_downsample=1,
                 kv_mode="nearest", pag_scale=0.0, pag_layers=("mid",), seg_scale=0.0, seg_blur_sigma=100.0, seg_layers=("mid",),
                 init_latents=None, strength=1.0, free_init_iters=1, **kw):
    """The restated loop of the feature the keywords ask for -- tests/fusion_ref.denoise_loop (reduced=True), tests/pag_ref.denoise_loop
    (pag_scale / seg_scale > 0; a PAG-selected block has no attention to tile, a SEG-selected one blurs then tiles, the unselected blocks
    of the perturbed evaluation tile like the main one), tests/v2v_ref.denoise_loop (init_latents; the step index starts at the first kept
    step), tests/free_init_ref.denoise_loop (free_init_iters > 1; every pass starts over) -- with shifted-tile self-attention, and with
    tests/todo_ref.pooled around it for kv_downsample.  Every tile factor 1: that loop op for op."""
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
    if seg_scale > 0:
        P.perturbed_forward = lambda sd, x, t, ctx, banks, names: _seg_forward(sd, x, t, ctx, banks, names, seg_blur_sigma, factors)
    try:
        with contextlib.ExitStack() as stack:
            if any(v > 1 for v in kvf):
                stack.enter_context(T.pooled(den_sd, kvf, kv_mode))
            if all(v == 1 for v in factors):
                if seg_scale > 0:                                     # no tiled() to note the grid: seg_ref's own restatement
                    import seg_ref as S
                    P.perturbed_forward = lambda sd, x, t, ctx, banks, names: S.perturbed_forward(sd, x, t, ctx, banks, names, seg_blur_sigma)
                return loop()
            seen = stack.enter_context(tiled(den_sd, factors, tile_attention_shift, first, kv=(kvf, kv_mode)))
            out = loop()
        assert seen, "no block was tiled"
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
    """todo_ref.block_runs with the tile field: the block of todo_ref.block_setup in every reference mode with tile_spec = (t, (sy, sx)) or
    None, kv_pool = (s, mode) or None on the same block -> {case: (got, want)} on the host, fp32: plain, write (with the bank it wrote), read
    + ref_cfg on the whole batch, and its two clip-halves as SelfAttnCall(half=0 / 1).  sigma: the block blurs its queries (a perturbed
    evaluation: only the conditional frames, every row reads the bank) -> {"seg": (got, want)}."""
    from mikudance_amd import blocks
    blk, f, L, dim, dev, Hh, Ww = st.blk, st.f, st.L, st.dim, st.device, st.Hh, st.Ww
    h = st.x.reshape(2 * f * L, dim).to(dev)
    xf, bankf = st.x.float(), st.bank.float()
    grid = (Hh, Ww)
    tile_f = None if tile_spec is None else {blk: tile_spec}
    pool_f = None if kv_pool is None else {blk: kv_pool}

    def ref(x, ctx, bank, cfg, sg=None):
        if tile_spec is not None:
            return block_read(st.sd, "", x, ctx, bank, cfg, Hh, Ww, tile_spec[0], tile_spec[1], pool=kv_pool, sigma=sg)
        if sg is not None:
            import seg_ref
            return seg_ref.block_read(st.sd, "", x, ctx, bank, Hh, Ww, sg, kv_pool=kv_pool)
        if kv_pool is not None:
            return T.block_read(st.sd, "", x, ctx, bank, cfg, Hh, Ww, *kv_pool)
        return O.transformer_block_read(st.sd, "", x, ctx, bank, cfg=cfg)

    out = {}
    with torch.no_grad():
        if sigma is not None:
            blk.ref_mode, blk.ref_cfg, blk.bank = "read", True, [st.bank.to(dev)]
            got = blk(h[f * L:].clone(), f, L, st.cross.rows(f, 2 * f), sa=blocks.SelfAttnCall(blur=((blk,), sigma), pool=pool_f, tile=tile_f), grid=grid)
            out["seg"] = (got, ref(xf[f:], st.ctx_f[f:], bankf, False, sigma))
            blk.ref_mode, blk.ref_cfg, blk.bank = None, False, []
            return {k: (g.float().cpu().reshape(w.shape), w) for k, (g, w) in out.items()}
        kw = dict(sa=blocks.SelfAttnCall(pool=pool_f, tile=tile_f), grid=grid)
        want_plain = ref(xf, st.ctx_f, None, False)
        want_read = ref(xf, st.ctx_f, torch.cat([torch.zeros_like(bankf), bankf]), True)
        blk.ref_mode, blk.ref_cfg, blk.bank = None, False, []
        out["plain"] = (blk(h.clone(), 2 * f, L, st.cross, **kw), want_plain)
        blk.ref_mode = "write"
        out["write"] = (blk(h.clone(), 2 * f, L, st.cross, **kw), want_plain)
        out["write-bank"] = (blk.bank[0].reshape(2 * f, L, dim), O.layer_norm(st.sd, "norm1.", xf))
        blk.ref_mode, blk.ref_cfg, blk.bank = "read", True, [st.bank.to(dev)]
        out["read-cfg"] = (blk(h.clone(), 2 * f, L, st.cross, **kw), want_read)
        for c in (0, 1):
            got = blk(h[c * f * L:(c + 1) * f * L].clone(), f, L, st.cross.rows(c * f, (c + 1) * f),
                      sa=blocks.SelfAttnCall(half=c, pool=pool_f, tile=tile_f), grid=grid)
            out[f"read-cfg-chain{c}"] = (got, want_read[c * f:(c + 1) * f])
        blk.ref_mode, blk.ref_cfg, blk.bank = None, False, []
    return {k: (g.float().cpu().reshape(w.shape), w) for k, (g, w) in out.items()}
