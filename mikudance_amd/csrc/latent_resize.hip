// Resampling of the loop's packed latents for two-pass high-resolution sampling (the pipeline's hires_scale=): the clip sampled at the low size
// is enlarged to the target size here, re-noised (md_add_noise_f16) and the tail of the schedule runs on it.
//
//   x (F, Hi, Wi, 4) fp16 -> y (F, Ho, Wo, 4) fp16, both contiguous, the layout of md_pack_nhwc_f16 with cpad = 4 (8 bytes per pixel).
//   mode 0 nearest-exact, 1 bilinear, 2 bicubic (A = -0.75): torch.nn.functional.interpolate(size=(Ho, Wo), align_corners=False, antialias=False).
//   Along an axis of ni inputs and no outputs, output o sits at the source coordinate (o + 0.5) ni / no - 0.5 = num / den with the integers
//   num = (2 o + 1) ni - no and den = 2 no.  nearest-exact reads floor((o + 0.5) ni / no) = (num + no) / den, clamped; bilinear clamps the
//   coordinate at 0 and blends floor and floor + 1 (clamped); bicubic blends floor - 1 .. floor + 2, the tap indices clamped to the border.
//   Any ratio, up or down.  NO antialiasing on the way down: a ratio below 1 skips input pixels, exactly like antialias=False.
//
// Arithmetic: fp32 operations only, ONE rounding to fp16 at the store.  A resampled value is a signed sum; where it cancels, its error is that of
// the weights times the operands, not times the result, and plain fp32 weights (2^-24 relative) leave more than an fp16 ulp of a result 2^-13 of its
// operands.  So floor and fraction come from the integer division num / den, not from a rounded coordinate, and the fraction, the weights and the
// sums are unevaluated pairs of floats hi + lo (two_sum / fma error terms: about 2^-45 relative).  nearest-exact and every size-preserving call
// (fraction 0: the weights are exactly 0 and 1) return x bit for bit, up to the sign of a zero.  Non-finite inputs give non-finite outputs, as
// 0 * Inf does in torch.
//
// Runs once per clip on a few MB: one thread per output pixel, one 8-byte load per tap and one 8-byte store, weights per thread, a capped grid
// striding over F Ho Wo.  No atomics, no LDS: two calls give the same bits.
#include "common.h"
#include <limits.h>

#define LR_THREADS 256
#define LR_MAX_BLOCKS 2048

// The pair arithmetic below names every rounding it relies on: p = a * b must be the ROUNDED product both where it is added and where fmaf(a, b, -p)
// takes its error.  The compiler's own fusing of a * b + c (hipcc's default for device code) would hand the addition the exact product and count
// that error twice, so it is switched off for this file; the fmaf calls stay fused.
#pragma clang fp contract(off)

#include "ff_pair.h"

// The taps of output o along one axis: TAPS input indices, all inside [0, ni), and their weights.  rem and den are exact as floats while
// no < 2^23 (beyond that the fraction is an fp32 quotient, no worse than a rounded coordinate); q (den) - rem is then exact too.
template <int MODE>
__host__ __device__ __forceinline__ void axis_taps(int o, int ni, int no, int* idx, ff_t* w) {
  const long den = 2L * no;
  const long num = (2L * o + 1) * ni - no;                         // > -den
  const int last = ni - 1;
  if (MODE == 0) {
    const long i = (num + no) / den;
    idx[0] = (int)(i < last ? i : last);
    w[0] = {1.f, 0.f};
    return;
  }
  long i0 = num / den, rem = num - i0 * den;
  if (num < 0) {                                                   // bilinear: the coordinate is clamped at 0; bicubic: floor = -1
    i0 = MODE == 1 ? 0 : -1;
    rem = MODE == 1 ? 0 : num + den;
  }
  const float rf = (float)rem, df = (float)den;
  const float th = rf / df;
  const ff_t t = ff_fast_sum(th, fmaf(-th, df, rf) / df);          // rem / den in [0, 1)
  const ff_t u = ff_add(ff_t{-t.h, -t.l}, 1.f);                    // 1 - t
  if (MODE == 1) {
    idx[0] = (int)i0;                                              // <= last: the coordinate stays below ni - 0.5
    idx[1] = (int)(i0 < last ? i0 + 1 : last);
    w[0] = u;
    w[1] = t;
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long i = i0 - 1 + k;
    idx[k] = (int)(i < 0 ? 0 : i > last ? last : i);
  }
  // the cubic convolution kernel with A = -0.75 at distances t + 1, t, 1 - t, 2 - t: A s (1 - s)^2 outside and (A + 2) s^3 - (A + 3) s^2 + 1 inside
  w[0] = ff_mul(ff_mul(ff_mul(t, u), u), -0.75f);
  w[1] = ff_add(ff_mul(ff_mul(ff_add(ff_mul(t, 1.25f), -2.25f), t), t), 1.f);
  w[2] = ff_add(ff_mul(ff_mul(ff_add(ff_mul(u, 1.25f), -2.25f), u), u), 1.f);
  w[3] = ff_mul(ff_mul(ff_mul(u, t), t), -0.75f);
}

// Output pixel i of F * Ho * Wo.  Every tap index lies inside its axis (axis_taps), f < F: nothing outside x is read, nothing outside y written.
// Host-callable, so that the arithmetic can be run and checked without a device.
template <int MODE>
__host__ __device__ __forceinline__ void resize_pixel(const half_t* __restrict__ x, half_t* __restrict__ y, long i, int Hi, int Wi, int Ho, int Wo) {
  constexpr int TAPS = MODE == 0 ? 1 : MODE == 1 ? 2 : 4;
  const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
  const long f = i / ((long)Wo * Ho);
  int iy[TAPS], ix[TAPS];
  ff_t wy[TAPS], wx[TAPS];
  axis_taps<MODE>(oy, Hi, Ho, iy, wy);
  axis_taps<MODE>(ox, Wi, Wo, ix, wx);
  if (MODE == 0) {                                                 // a copy: every bit pattern survives
    *reinterpret_cast<half4_t*>(y + i * 4) = *reinterpret_cast<const half4_t*>(x + ((f * Hi + iy[0]) * Wi + ix[0]) * 4);
    return;
  }
  ff_t acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
  for (int j = 0; j < TAPS; ++j) {
    ff_t row[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
    for (int k = 0; k < TAPS; ++k) {
      const half4_t v = *reinterpret_cast<const half4_t*>(x + ((f * Hi + iy[j]) * Wi + ix[k]) * 4);
#pragma unroll
      for (int c = 0; c < 4; ++c) row[c] = ff_add(row[c], ff_mul(wx[k], (float)v[c]));
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = ff_add(acc[c], ff_mul(wy[j], row[c]));
  }
  half4_t o;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = (half_t)(acc[c].h + acc[c].l);
  *reinterpret_cast<half4_t*>(y + i * 4) = o;
}

template <int MODE>
__global__ void __launch_bounds__(LR_THREADS) latent_resize_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, long total, int Hi, int Wi,
                                                                    int Ho, int Wo) {
  for (long i = (long)blockIdx.x * LR_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * LR_THREADS) resize_pixel<MODE>(x, y, i, Hi, Wi, Ho, Wo);
}

extern "C" int md_latent_resize_f16(const void* x, void* y, int F, int Hi, int Wi, int Ho, int Wo, int mode, void* stream) {
  MD_CHECK_ARG(x && y, "md_latent_resize_f16: NULL pointer");
  MD_CHECK_ARG(((uintptr_t)x % 8) == 0 && ((uintptr_t)y % 8) == 0, "md_latent_resize_f16: x / y need 8-byte alignment");
  MD_CHECK_ARG(F > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "md_latent_resize_f16: F, Hi, Wi, Ho, Wo must be positive (%d, %d, %d, %d, %d)", F, Hi, Wi,
               Ho, Wo);
  MD_CHECK_ARG(mode >= 0 && mode <= 2, "md_latent_resize_f16: mode must be 0 (nearest-exact), 1 (bilinear) or 2 (bicubic), got %d", mode);
  const long rows_in = (long)F * Hi, rows_out = (long)F * Ho;
  MD_CHECK_ARG(rows_in <= INT_MAX / Wi && rows_out <= INT_MAX / Wo, "md_latent_resize_f16: F*Hi*Wi and F*Ho*Wo must fit an int (F=%d, %d x %d -> %d x %d)",
               F, Hi, Wi, Ho, Wo);
  const long n_in = rows_in * Wi, total = rows_out * Wo;
  const uintptr_t xb = (uintptr_t)x, xe = xb + (uintptr_t)(n_in * 8), yb = (uintptr_t)y, ye = yb + (uintptr_t)(total * 8);
  MD_CHECK_ARG(xe <= yb || ye <= xb, "md_latent_resize_f16: x and y overlap");
  const long blocks = (total + LR_THREADS - 1) / LR_THREADS;
  const dim3 grid((unsigned)(blocks < LR_MAX_BLOCKS ? blocks : LR_MAX_BLOCKS)), block(LR_THREADS);
  const half_t* xp = (const half_t*)x;
  half_t* yp = (half_t*)y;
  if (mode == 0)
    hipLaunchKernelGGL(latent_resize_kernel<0>, grid, block, 0, (hipStream_t)stream, xp, yp, total, Hi, Wi, Ho, Wo);
  else if (mode == 1)
    hipLaunchKernelGGL(latent_resize_kernel<1>, grid, block, 0, (hipStream_t)stream, xp, yp, total, Hi, Wi, Ho, Wo);
  else
    hipLaunchKernelGGL(latent_resize_kernel<2>, grid, block, 0, (hipStream_t)stream, xp, yp, total, Hi, Wi, Ho, Wo);
  MD_CHECK_LAUNCH("md_latent_resize_f16");
  return MD_OK;
}
