// Shifted-tile reorder of a token matrix for tiled spatial self-attention (MSW-MSA of HiDiffusion, Zhang et al., arXiv 2311.17528; the
// pipeline's tile_attention=): every frame's Hh x Ww token grid is cut into t x t tiles of th x tw tokens (th = Hh / t, tw = Ww / t) after a
// cyclic shift by (sy, sx), and every tile becomes one batch item of md_attention_fwd_f16.
//
//   frame-major [B * Hh * Ww][C] fp16: row = (b * Hh + yy) * Ww + xx (the layout of md_token_pool_f16)
//   tile-major  [B * t * t * tile_stride][C]: tile (b, j, i), j, i < t, is batch item (b t + j) t + i; its row r tw + c holds the token at
//               (yy, xx) = ((j th + r + sy) mod Hh, (i tw + c + sx) mod Ww): torch.roll(grid, (-sy, -sx), (1, 2)) and a plain partition.
//   inverse = 0: x frame-major -> y tile-major; rows [Lt, tile_stride) of every tile = +0 (Lt = th tw): the pad that md_attention_fwd_f16
//                reads and masks, the contract of md_token_pool_f16.
//   inverse = 1: x tile-major -> y frame-major, the exact inverse permutation; the pad rows of x are never read.
// The wrap-around is not masked (the paper's code does not mask it either): on a shifted step a tile may hold tokens of opposite frame edges.
//
// Memory-bound, one pass: one lane moves eight channels of one OUTPUT row with a 16-byte load and a 16-byte store, lanes run over the
// channels of the output row fastest (a wave writes 1 KiB of consecutive output and reads whole token rows), a capped grid strides over the
// rest.  No atomics, no LDS, no cross-lane traffic, no arithmetic on the values: a copy keeps every bit pattern, two calls give the same bits.
#include "common.h"

#define TT_THREADS 256
#define TT_MAX_BLOCKS 2048

// total = output rows * C8.  Both directions walk the OUTPUT rows: the forward one decodes a tile-major row into its frame-major source, the
// inverse one decodes a frame-major row into its tile-major source.  Every source row lies inside x: (yy, xx) < (Hh, Ww) after the modulo,
// tile < t * t and r tw + c < Lt <= tile_stride.
__global__ void __launch_bounds__(TT_THREADS) token_tile_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, long total, int Hh, int Ww,
                                                                 int C8, int t, int th, int tw, int sy, int sx, int tile_stride, int inverse) {
  const long xrow = (long)C8 * 8;                                  // elements per token row
  const int Lt = th * tw;
  for (long i = (long)blockIdx.x * TT_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * TT_THREADS) {
    const int c8 = (int)(i % C8);
    const long row = i / C8;                                       // output row
    half8_t o = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!inverse) {
      const int r = (int)(row % tile_stride);
      if (r < Lt) {
        const long tile = row / tile_stride;                       // (b t + j) t + i
        const int ti = (int)(tile % t), tj = (int)((tile / t) % t);
        const long b = tile / ((long)t * t);
        const int rr = r / tw, cc = r - rr * tw;
        int yy = tj * th + rr + sy, xx = ti * tw + cc + sx;        // < 2 Hh, < 2 Ww: one conditional subtraction is the modulo
        yy -= yy >= Hh ? Hh : 0;
        xx -= xx >= Ww ? Ww : 0;
        o = *reinterpret_cast<const half8_t*>(x + ((b * Hh + yy) * Ww + xx) * xrow + (long)c8 * 8);
      }
    } else {
      const int xx = (int)(row % Ww), yy = (int)((row / Ww) % Hh);
      const long b = row / ((long)Hh * Ww);
      int ry = yy - sy, rx = xx - sx;                              // position in the rolled grid, > -Hh, > -Ww
      ry += ry < 0 ? Hh : 0;
      rx += rx < 0 ? Ww : 0;
      const int tj = ry / th, ti = rx / tw;
      const long src = ((b * t + tj) * t + ti) * tile_stride + (long)(ry - tj * th) * tw + (rx - ti * tw);
      o = *reinterpret_cast<const half8_t*>(x + src * xrow + (long)c8 * 8);
    }
    *reinterpret_cast<half8_t*>(y + row * xrow + (long)c8 * 8) = o;
  }
}

extern "C" int md_token_tile_f16(const void* x, void* y, int B, int Hh, int Ww, int C, int t, int sy, int sx, int tile_stride, int inverse,
                                 void* stream) {
  MD_CHECK_ARG(x && y, "md_token_tile_f16: NULL pointer");
  MD_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, "md_token_tile_f16: x / y need 16-byte alignment");
  MD_CHECK_ARG(B > 0 && Hh > 0 && Ww > 0 && C > 0 && C % 8 == 0, "md_token_tile_f16: B, Hh, Ww, C must be positive and C a multiple of 8 (C=%d)", C);
  MD_CHECK_ARG(t >= 2 && t <= 8, "md_token_tile_f16: t must be 2..8, got %d", t);
  MD_CHECK_ARG(Hh % t == 0 && Ww % t == 0, "md_token_tile_f16: t = %d does not divide the %d x %d grid", t, Hh, Ww);
  MD_CHECK_ARG(sy >= 0 && sy < Hh && sx >= 0 && sx < Ww, "md_token_tile_f16: shift (%d, %d) outside the %d x %d grid", sy, sx, Hh, Ww);
  MD_CHECK_ARG(inverse == 0 || inverse == 1, "md_token_tile_f16: inverse must be 0 or 1, got %d", inverse);
  const int th = Hh / t, tw = Ww / t;
  const long Lt = (long)th * tw;
  MD_CHECK_ARG(tile_stride >= Lt, "md_token_tile_f16: tile_stride %d must be >= Lt = %ld", tile_stride, Lt);
  const long rows_frame = (long)B * Hh * Ww, rows_tile = (long)B * t * t * tile_stride;
  MD_CHECK_ARG(rows_frame <= (1L << 40) / C && rows_tile <= (1L << 40) / C, "md_token_tile_f16: problem too large");
  const long rows_in = inverse ? rows_tile : rows_frame, rows_out = inverse ? rows_frame : rows_tile;
  const uintptr_t xb = (uintptr_t)x, xe = xb + (uintptr_t)(rows_in * C * 2), yb = (uintptr_t)y, ye = yb + (uintptr_t)(rows_out * C * 2);
  MD_CHECK_ARG(xe <= yb || ye <= xb, "md_token_tile_f16: x and y overlap");
  const long total = rows_out * (C / 8);
  const long blocks = (total + TT_THREADS - 1) / TT_THREADS;
  hipLaunchKernelGGL(token_tile_kernel, dim3((unsigned)(blocks < TT_MAX_BLOCKS ? blocks : TT_MAX_BLOCKS)), dim3(TT_THREADS), 0, (hipStream_t)stream,
                     (const half_t*)x, (half_t*)y, total, Hh, Ww, C / 8, t, th, tw, sy, sx, tile_stride, inverse);
  MD_CHECK_LAUNCH("md_token_tile_f16");
  return MD_OK;
}
