// Token downsampling of the K / V source of spatial self-attention (ToDo: Token Downsampling, Smith et al., arXiv 2402.13573): the token
// grid of every frame is reduced by a factor s per axis before to_k / to_v, Q keeps every token.
//
//   x [B * Hh * Ww][C] fp16, the tokens of B frames (row = (b * Hh + y) * Ww + x)
//   y [B * out_stride][C]: frame b writes rows b * out_stride + oy * Wo + ox, Ho = Hh / s, Wo = Ww / s (what does not fill a block is dropped)
//     mode 0 (nearest, the paper's): y = x[b, oy s, ox s]                       F.interpolate(scale_factor = 1 / s, mode = "nearest")
//     mode 1 (mean):                 y = fp16(sum of the s x s block / s^2)      F.avg_pool2d(kernel = s, stride = s)
//   rows [Ho * Wo, out_stride) of every frame = +0: the pad that md_attention_fwd_f16 reads and masks.
//
// Memory-bound and small (one pass over kv, or 1 / s^2 of it): one lane moves eight channels of one output row with a 16-byte load and a
// 16-byte store, lanes run over the channels fastest (a wave writes 1 KiB of consecutive output and reads whole token rows or 16-byte-aligned
// runs of them), a capped grid strides over the rest.  The mean adds the s^2 values in fp32 in the order (dy, dx) ascending, multiplies by fp32(1 / s^2) and rounds ONCE.
// No atomics, no LDS, no cross-lane traffic: the same inputs give the same bits.
#include "common.h"

#define TP_THREADS 256
#define TP_MAX_BLOCKS 2048

__global__ void __launch_bounds__(TP_THREADS) token_pool_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, long total, int Hh, int Ww,
                                                                 int C8, int s, int Wo, int Lk, int out_stride, int mean, float inv) {
  const long xrow = (long)C8 * 8;                                  // elements per token row
  for (long i = (long)blockIdx.x * TP_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * TP_THREADS) {
    const int c8 = (int)(i % C8);
    const long row = i / C8;                                       // output row, < B * out_stride
    const int r = (int)(row % out_stride);
    const long b = row / out_stride;
    half8_t o = {0, 0, 0, 0, 0, 0, 0, 0};
    if (r < Lk) {
      const int oy = r / Wo, ox = r - oy * Wo;
      // top-left token of the block: oy s + s <= Hh and ox s + s <= Ww, so every token read below lies inside frame b
      const half_t* src = x + ((b * Hh + (long)oy * s) * Ww + (long)ox * s) * xrow + (long)c8 * 8;
      if (!mean) {
        o = *reinterpret_cast<const half8_t*>(src);
      } else {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int dy = 0; dy < s; ++dy) {
          for (int dx = 0; dx < s; ++dx) {
            const half8_t v = *reinterpret_cast<const half8_t*>(src + ((long)dy * Ww + dx) * xrow);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += (float)v[j];
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)(acc[j] * inv);
      }
    }
    *reinterpret_cast<half8_t*>(y + row * xrow + (long)c8 * 8) = o;
  }
}

extern "C" int md_token_pool_f16(const void* x, void* y, int B, int Hh, int Ww, int C, int s, int mode, int out_stride, void* stream) {
  MD_CHECK_ARG(x && y, "md_token_pool_f16: NULL pointer");
  MD_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0, "md_token_pool_f16: x / y need 16-byte alignment");
  MD_CHECK_ARG(B > 0 && Hh > 0 && Ww > 0 && C > 0 && C % 8 == 0, "md_token_pool_f16: B, Hh, Ww, C must be positive and C a multiple of 8 (C=%d)", C);
  MD_CHECK_ARG(s >= 2 && s <= 8, "md_token_pool_f16: s must be 2..8, got %d", s);
  MD_CHECK_ARG(mode == 0 || mode == 1, "md_token_pool_f16: mode must be 0 (nearest) or 1 (mean), got %d", mode);
  const int Ho = Hh / s, Wo = Ww / s;
  MD_CHECK_ARG(Ho >= 1 && Wo >= 1, "md_token_pool_f16: a %d x %d grid has no %d x %d block", Hh, Ww, s, s);
  const long Lk = (long)Ho * Wo;
  MD_CHECK_ARG(out_stride >= Lk && out_stride % 8 == 0, "md_token_pool_f16: out_stride %d must be a multiple of 8 and >= Lk = %ld", out_stride, Lk);
  const long rows_in = (long)B * Hh * Ww, rows_out = (long)B * out_stride;
  MD_CHECK_ARG(rows_in <= (1L << 40) / C && rows_out <= (1L << 40) / C, "md_token_pool_f16: problem too large");
  const uintptr_t xb = (uintptr_t)x, xe = xb + (uintptr_t)(rows_in * C * 2), yb = (uintptr_t)y, ye = yb + (uintptr_t)(rows_out * C * 2);
  MD_CHECK_ARG(xe <= yb || ye <= xb, "md_token_pool_f16: x and y overlap");
  const long total = rows_out * (C / 8);
  const long blocks = (total + TP_THREADS - 1) / TP_THREADS;
  hipLaunchKernelGGL(token_pool_kernel, dim3((unsigned)(blocks < TP_MAX_BLOCKS ? blocks : TP_MAX_BLOCKS)), dim3(TP_THREADS), 0, (hipStream_t)stream,
                     (const half_t*)x, (half_t*)y, total, Hh, Ww, C / 8, s, Wo, (int)Lk, out_stride, mode, 1.0f / (float)(s * s));
  MD_CHECK_LAUNCH("md_token_pool_f16");
  return MD_OK;
}
