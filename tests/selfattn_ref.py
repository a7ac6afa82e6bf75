"""TEST INFRASTRUCTURE: the ONE restatement of a "read" transformer block whose spatial self-attention is modified the ways
mikudance_amd.blocks.SelfAttnCall describes -- identity map (PAG), blurred queries (SEG), pooled K / V (kv_downsample), shifted tiles
(tile_attention) and their combinations -- stated in torch at the caller's dtype on top of oracle/cpu_ref.py, and the ONE patcher that makes
the oracle's denoising UNet evaluate selected blocks that way.  The definitions of the four modifications stay beside their features
(pag_ref, seg_ref.blur64, todo_ref.pool, tile_ref.tile / untile), whose public names call this module.

    block_read(sd, p, x, ctx, bank, cfg, grid, identity, sigma, pool, tile)   one read block
    modified(den_sd, identity=, blur=, pool=, tile=, ...)                      context: which blocks of the oracle are evaluated that way
    block_runs(st, grid, pool, tile, sigma)                                    one product TransformerBlock in every reference mode beside block_read
The oracle is not edited: inside `modified(...)`, and in this process only, its denoising_unet_forward is wrapped to note the timestep, its
transformer_3d to note the grid, and its transformer_block_read is swapped for block_read on the blocks a modification applies to.
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import cpu_ref as O

import seg_ref
import tile_ref
import todo_ref


def block_read(sd, p, x, ctx, bank, cfg, grid=None, identity=False, sigma=None, pool=None, tile=None, heads=O.HEADS):
    """oracle transformer_block_read with the self-attention of SelfAttnCall: q from norm1(x), k / v from norm1(x) + bank.
    identity: softmax(q k^T d^-1/2) is the identity, attn1 = to_out(to_v(norm1(x) + bank)); nothing else applies then.
    sigma: q = blur(to_q(norm1(x))) over the whole frame grid (Hh, Ww) = grid.
    tile = (t, (sy, sx)): q and the K / V source are cut into shifted tiles (after the blur), attention runs inside every tile and the output
    goes back to frame order in front of to_out.
    pool = (s, mode): the K / V source is pooled AFTER the bank add, per tile where tiled.
    Under cfg the unconditional first half of the batch runs without the bank."""
    B, L, C = x.shape
    a = p + "attn1."
    d = C // heads
    t, shift = tile or (1, (0, 0))
    n = O.layer_norm(sd, p + "norm1.", x)

    def attend(nq, kv):
        if identity:
            return F.linear(F.linear(kv, sd[a + "to_v.weight"]), sd[a + "to_out.0.weight"], sd[a + "to_out.0.bias"])
        b = nq.shape[0]
        q = F.linear(nq, sd[a + "to_q.weight"])
        if sigma is not None:
            q = seg_ref.blur64(q.reshape(b * L, C), b, grid[0], grid[1], sigma).to(q.dtype).reshape(b, L, C)
        if tile is not None:
            q, kv = tile_ref.tile(q, b, grid[0], grid[1], t, shift), tile_ref.tile(kv, b, grid[0], grid[1], t, shift)
        if pool is not None:
            kv = todo_ref.pool(kv, b * t * t, grid[0] // t, grid[1] // t, *pool)
        k, v = F.linear(kv, sd[a + "to_k.weight"]), F.linear(kv, sd[a + "to_v.weight"])
        q, k, v = (z.view(b * t * t, -1, heads, d).transpose(1, 2) for z in (q, k, v))
        o = O._sdpa(q, k, v).transpose(1, 2).reshape(b * t * t, L // (t * t), C)
        if tile is not None:
            o = tile_ref.untile(o, b, grid[0], grid[1], t, shift)
        return F.linear(o, sd[a + "to_out.0.weight"], sd[a + "to_out.0.bias"])

    h = attend(n, n + bank if bank is not None else n) + x
    if cfg:
        half = B // 2
        h = h.clone()
        h[:half] = attend(n[:half], n[:half]) + x[:half]
    x = h
    x = O.attention(sd, p + "attn2.", O.layer_norm(sd, p + "norm2.", x), ctx) + x
    x = O.feed_forward(sd, p + "ff.", O.layer_norm(sd, p + "norm3.", x)) + x
    return x


# ---- the oracle's denoising UNet with some blocks evaluated by block_read
_LAYERS = []        # the settings of the enclosing `modified` blocks, outermost first; the oracle is patched while there is one
_STATE = {}         # the oracle's own three functions, the grid of the transformer_3d being evaluated and the timestep of the forward


def _forward(sd, sample, t, *a, **kw):
    _STATE["t"].append(float(torch.as_tensor(t).reshape(-1)[0]))
    try:
        return _STATE["forward"](sd, sample, t, *a, **kw)
    finally:
        _STATE["t"].pop()


def _transformer_3d(sd, p, x, ctx_per_frame, bank, cfg):
    _STATE["grid"].append(tuple(x.shape[2:]))
    try:
        return _STATE["t3d"](sd, p, x, ctx_per_frame, bank, cfg)
    finally:
        _STATE["grid"].pop()


def _read(sd, p, x, ctx, bank, cfg=True):
    """Per block prefix, what the enclosing `modified` blocks ask for: an identity map has no attention to blur, shorten or tile."""
    Hh, Ww = _STATE["grid"][-1]
    kw, by = {}, []
    for lay in _LAYERS:
        if p in lay["identity"]:
            kw, by = dict(identity=True), [lay]
            break
        if p in lay["blur"]:
            kw["sigma"] = lay["sigma"]
        s = todo_ref.factor_of(p, lay["pool"][0], lay["levels"]) if lay["pool"] else 1
        if s > 1:
            kw["pool"] = (s, lay["pool"][1])
        t = todo_ref.factor_of(p, lay["tile"], lay["levels"]) if lay["tile"] else 1
        if t > 1:
            k = lay["step"] if lay["step"] is not None else lay["first_step"] + lay["order"].setdefault(_STATE["t"][-1], len(lay["order"]))
            kw["tile"] = (t, tile_ref.shift_at(lay["shift"], k, Hh // t, Ww // t))
        if p in lay["blur"] or s > 1 or t > 1:
            by.append(lay)
    if not kw:
        return _STATE["read"](sd, p, x, ctx, bank, cfg)
    assert not cfg or not ("identity" in kw or "sigma" in kw), "the perturbed evaluation is conditional-only"
    for lay in by:
        lay["seen"].append((p, Hh, Ww, dict(kw)))
    return block_read(sd, p, x, ctx, bank, cfg, (Hh, Ww), **kw)


@contextlib.contextmanager
def modified(den_sd=None, identity=(), blur=(), sigma=None, pool=None, tile=None, shift="cycle", first_step=0, step=None):
    """Within the block, the oracle's read blocks are evaluated by block_read where a modification applies to them:
    identity, blur: key prefixes "....attentions.J" of the blocks with the identity map / with queries blurred by `sigma`;
    pool = (factors, mode), tile = factors: per resolution level of den_sd, as kv_downsample / tile_attention; shift, first_step, step: the
    tiling's shift mode and step index -- first_step + the position of the evaluation's timestep among the distinct timesteps seen so far
    (a FreeInit pass sees the same ones again), or `step` where given (one forward outside a loop).
    Blocks nest: an inner one adds its modifications to the outer ones' (the perturbed evaluation of a loop that pools or tiles).  Yields the
    list of (prefix, Hh, Ww, {the block_read keywords}) of every block evaluation that one of ITS modifications applied to."""
    lay = dict(identity={q + ".transformer_blocks.0." for q in identity}, blur={q + ".transformer_blocks.0." for q in blur}, sigma=sigma,
               pool=pool and (todo_ref.check_factors(pool[0]), pool[1]), tile=tile and todo_ref.check_factors(tile), shift=shift,
               first_step=first_step, step=step, order={}, seen=[], levels=den_sd and O._n_levels(den_sd))
    assert all(len(f) <= lay["levels"] for f in (lay["pool"] and lay["pool"][0], lay["tile"]) if f), (pool, tile, lay["levels"])
    if not _LAYERS:
        _STATE.update(forward=O.denoising_unet_forward, t3d=O.transformer_3d, read=O.transformer_block_read, grid=[], t=[])
        O.denoising_unet_forward, O.transformer_3d, O.transformer_block_read = _forward, _transformer_3d, _read
    _LAYERS.append(lay)
    try:
        yield lay["seen"]
    finally:
        _LAYERS.pop()
        if not _LAYERS:
            O.denoising_unet_forward, O.transformer_3d, O.transformer_block_read = _STATE["forward"], _STATE["t3d"], _STATE["read"]


# ------------------------------------------------------------------ one TransformerBlock in every reference mode (CPU-emulated and GPU tests)
def block_runs(st, grid=None, pool=None, tile=None, sigma=None):
    """The block of todo_ref.block_setup in every reference mode with pool = (s, mode) and tile = (t, (sy, sx)), or None, on that block ->
    {case: (got, want)} on the host, fp32: plain, write (with the bank it wrote), read + ref_cfg on the whole batch, and its two clip-halves as
    SelfAttnCall(half=0 / 1).  sigma: the block blurs its queries (a perturbed evaluation: only the conditional frames, every row reads the
    bank) -> {"seg": (got, want)}."""
    from mikudance_amd import blocks
    blk, f, L, dim, dev = st.blk, st.f, st.L, st.dim, st.device
    h = st.x.reshape(2 * f * L, dim).to(dev)
    xf, bankf = st.x.float(), st.bank.float()
    opts = dict(pool=None if pool is None else {blk: pool}, tile=None if tile is None else {blk: tile})
    ref = lambda x, ctx, bank, cfg, sg=None: block_read(st.sd, "", x, ctx, bank, cfg, grid, sigma=sg, pool=pool, tile=tile)
    out = {}
    with torch.no_grad():
        if sigma is not None:
            blk.ref_mode, blk.ref_cfg, blk.bank = "read", True, [st.bank.to(dev)]
            got = blk(h[f * L:].clone(), f, L, st.cross.rows(f, 2 * f), sa=blocks.SelfAttnCall(blur=((blk,), sigma), **opts), grid=grid)
            out["seg"] = (got, ref(xf[f:], st.ctx_f[f:], bankf, False, sigma))
            blk.ref_mode, blk.ref_cfg, blk.bank = None, False, []
            return {k: (g.float().cpu().reshape(w.shape), w) for k, (g, w) in out.items()}
        kw = dict(sa=blocks.SelfAttnCall(**opts), grid=grid)
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
            got = blk(h[c * f * L:(c + 1) * f * L].clone(), f, L, st.cross.rows(c * f, (c + 1) * f), sa=blocks.SelfAttnCall(half=c, **opts), grid=grid)
            out[f"read-cfg-chain{c}"] = (got, want_read[c * f:(c + 1) * f])
        blk.ref_mode, blk.ref_cfg, blk.bank = None, False, []
    return {k: (g.float().cpu().reshape(w.shape), w) for k, (g, w) in out.items()}
