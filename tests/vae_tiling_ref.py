"""TEST INFRASTRUCTURE of tiled / sliced VAE encode and decode (AutoencoderKL.enable_tiling / enable_slicing): the float64 restatement of
md_tile_blend_f16 and of the tile loop around it, the bound both are held to, and the emulation of ops.tile_blend for the CPU tests.

A literal transcription of the rules (diffusers 0.24 tiled_encode / tiled_decode, restated from the published algorithm):

    blend_ref(cur, above, left, ev, eh)   one tile, (B, Th, Tw, C) fp16 -> float64: vertical first over ev' = min(Ah, Th, ev) rows,
                                          v = above[Ah - ev' + y] (1 - y / ev') + v (y / ev'), then horizontal over eh' = min(Lw, Tw, eh)
                                          columns on the result; `above` / `left` are the neighbours AFTER their own blends (in place)
    axis_ref(n, tile, factor, out_tile, f, encode)   tiles along one axis: [(start, size, out_start, keep)]; start = 0, overlap, 2 overlap ..
                                          with overlap = int(tile (1 - factor)), size = min(tile, n - start), keep = min(limit, output size
                                          of the tile), limit = out_tile - int(out_tile factor), out_start = the kept sizes before it
    tiled_ref(x, run_tile, ...)           the whole loop: every tile through run_tile (-> (B, th, tw, C) fp16 NHWC), blended with the blended
                                          tile above and the blended tile to its left, each blended tile ROUNDED to fp16 where it is stored
                                          (the tiles below and to the right read that), the kept corners assembled -> (B, C, H, W) float64
    within_one_ulp                        tests/hires_ref.py's: |y - ref| <= 2^-10 max(|ref|, 2^-14), every element
"""
import torch

from hires_ref import within_one_ulp  # noqa: F401  (the bound md_latent_resize_f16 is held to)

F16 = torch.float16


def blend_ref(cur, above=None, left=None, ev=0, eh=0):
    assert cur.dim() == 4                                             # fp16 tiles, or an fp32 oracle's
    v = cur.double().clone()
    Th, Tw = cur.shape[1:3]
    if above is not None:
        Ah = above.shape[1]
        e = min(Ah, Th, ev)
        for y in range(e):
            v[:, y] = above[:, Ah - e + y].double() * (1 - y / e) + v[:, y] * (y / e)
    if left is not None:
        Lw = left.shape[2]
        e = min(Lw, Tw, eh)
        for x in range(e):
            v[:, :, x] = left[:, :, Lw - e + x].double() * (1 - x / e) + v[:, :, x] * (x / e)
    return v


def sizes_ref(tile_sample, tile_latent, factor, encode):
    """(tile, overlap, extent, limit) of tiled_encode / tiled_decode."""
    if encode:
        overlap, extent = int(tile_sample * (1 - factor)), int(tile_latent * factor)
        return tile_sample, overlap, extent, tile_latent - extent
    overlap, extent = int(tile_latent * (1 - factor)), int(tile_sample * factor)
    return tile_latent, overlap, extent, tile_sample - extent


def axis_ref(n, tile_sample, tile_latent, factor, f, encode):
    tile, overlap, extent, limit = sizes_ref(tile_sample, tile_latent, factor, encode)
    out, tiles = 0, []
    for start in range(0, n, overlap):
        size = min(tile, n - start)
        keep = min(limit, size // f if encode else size * f)           # tile[:, :, :limit, :limit] of a tile that may be smaller
        tiles.append((start, size, out, keep))
        out += keep
    return tiles


def tiled_ref(x, run_tile, tile_sample, tile_latent, factor, f, encode):
    """x (B, C, H, W).  run_tile(view) -> (B, th, tw, C_out) fp16 NHWC, the tile's own untiled result."""
    _, _, extent, _ = sizes_ref(tile_sample, tile_latent, factor, encode)
    rows = axis_ref(x.shape[2], tile_sample, tile_latent, factor, f, encode)
    cols = axis_ref(x.shape[3], tile_sample, tile_latent, factor, f, encode)
    blended = []                                                      # diffusers' `rows`, holding the tiles as blended (in place)
    out_rows = []
    for i, (y0, th, _, kh) in enumerate(rows):
        blended.append([])
        out_row = []
        for j, (x0, tw, _, kw) in enumerate(cols):
            cur = run_tile(x[:, :, y0:y0 + th, x0:x0 + tw])
            v = blend_ref(cur, blended[i - 1][j] if i else None, blended[i][j - 1] if j else None, extent, extent)
            blended[i].append(v.to(F16) if cur.dtype == F16 else v)   # stored as the path stores it: fp16 tiles are rounded
            out_row.append(v[:, :kh, :kw])
        out_rows.append(torch.cat(out_row, dim=2))
    return torch.cat(out_rows, dim=1).permute(0, 3, 1, 2).contiguous()


def tile_blend(cur, dst, c, above=None, left=None, extent=(0, 0)):
    """The emulation of mikudance_amd.ops.tile_blend: the float64 rule, one rounding, logged in fake_ops.CALLS."""
    import fake_ops
    B, Th, Tw, ldc = cur.shape
    assert cur.dtype == F16 and cur.is_contiguous() and c <= ldc
    assert above is None or (above.is_contiguous() and (above.shape[0], above.shape[2], above.shape[3]) == (B, Tw, ldc))
    assert left is None or (left.is_contiguous() and (left.shape[0], left.shape[1], left.shape[3]) == (B, Th, ldc))
    kh, kw = dst.shape[2:]
    assert dst.shape[:2] == (B, c) and 1 <= kh <= Th and 1 <= kw <= Tw
    fake_ops.CALLS.append(("tile_blend", dict(B=B, Th=Th, Tw=Tw, c=c, ldc=ldc, Ah=None if above is None else above.shape[1],
                                             Lw=None if left is None else left.shape[2], extent=tuple(extent), keep=(kh, kw))))
    v = blend_ref(cur[..., :c], None if above is None else above[..., :c], None if left is None else left[..., :c], *extent)
    cur[..., :c] = v.to(F16)
    dst.copy_((v[:, :kh, :kw].permute(0, 3, 1, 2) if dst.dtype != F16 else cur[:, :kh, :kw, :c].permute(0, 3, 1, 2)).to(dst.dtype))
    return cur


def install(monkeypatch):
    """fake_ops.install and this operator on top of it."""
    import fake_ops
    from mikudance_amd import ops
    fake_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "tile_blend", tile_blend, raising=False)
