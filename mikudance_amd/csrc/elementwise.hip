// Small HBM-bound kernels around the two UNets: layout packing at the API boundary, channel concat for the decoder
// skip connections, window accumulation + classifier-free guidance + DDIM step (reference
// src/pipelines/pipeline_mikudance.py:577-589, 662-678 and diffusers DDIMScheduler.step, v-prediction, eta = 0) or DPM-Solver++
// multistep step (the same call site's scheduler.step with a DPMSolverMultistepScheduler).
#include "common.h"
#include <stdarg.h>
#include <initializer_list>

static thread_local char g_err[512] = "";
void md_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
extern "C" const char* md_last_error(void) { return g_err; }
extern "C" int md_version(void) { return 100; }

// ---- strided gather -> NHWC fp16 with zero channel padding and optional nearest sub-sampling --------------------------
// dst[n][y][x][c] = c < c_count ? src[(n / F)*sB + (n % F)*sF + (c_begin + c)*sC + ny(y)*sY + nx(x)*sX] : 0
// with ny(y) = min(floor(y * Hin / Ho), Hin - 1)  (PyTorch 'nearest' rule; identity when Hin == Ho)
template <typename T>
__global__ void pack_nhwc_kernel(const T* __restrict__ src, half_t* __restrict__ dst, long total, int F, long sB, long sF, long sC, long sY, long sX,
                                 int c_begin, int c_count, int Cpad, int Ho, int Wo, int Hin, int Win) {
  const float fy = (float)Hin / (float)Ho, fx = (float)Win / (float)Wo;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % Cpad);
    long r = idx / Cpad;
    const int x = (int)(r % Wo);
    r /= Wo;
    const int y = (int)(r % Ho);
    const long n = r / Ho;
    float v = 0.f;
    if (c < c_count) {
      const int sy = min((int)floorf(y * fy), Hin - 1), sx = min((int)floorf(x * fx), Win - 1);
      v = (float)src[(n / F) * sB + (n % F) * sF + (long)(c_begin + c) * sC + (long)sy * sY + (long)sx * sX];
    }
    dst[idx] = (half_t)v;
  }
}

extern "C" int md_pack_nhwc_f16(const void* src, int src_is_f32, void* dst, int N, int F, long sB, long sF, long sC, long sY, long sX, int c_begin,
                                int c_count, int Cpad, int Ho, int Wo, int Hin, int Win, void* stream) {
  MD_CHECK_ARG(N > 0 && F > 0 && c_count <= Cpad && Hin >= 1 && Win >= 1, "md_pack_nhwc: bad arguments");
  const long total = (long)N * Ho * Wo * Cpad;
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  if (src_is_f32)
    hipLaunchKernelGGL(pack_nhwc_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)src, (half_t*)dst, total, F, sB, sF, sC, sY, sX,
                       c_begin, c_count, Cpad, Ho, Wo, Hin, Win);
  else
    hipLaunchKernelGGL(pack_nhwc_kernel<half_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const half_t*)src, (half_t*)dst, total, F, sB, sF, sC, sY, sX,
                       c_begin, c_count, Cpad, Ho, Wo, Hin, Win);
  MD_CHECK_LAUNCH("md_pack_nhwc");
  return MD_OK;
}

// ---- channel concat of two token-major matrices ------------------------------------------------------------------------
__global__ void concat_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, half_t* __restrict__ o, long M, int ca8, int cb8) {
  const int ct = ca8 + cb8;
  const long total = M * ct;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const long m = idx / ct;
    const int c = (int)(idx - m * ct);
    const half8_t v = c < ca8 ? reinterpret_cast<const half8_t*>(a)[m * ca8 + c] : reinterpret_cast<const half8_t*>(b)[m * cb8 + (c - ca8)];
    reinterpret_cast<half8_t*>(o)[idx] = v;
  }
}

extern "C" int md_concat_channels_f16(const void* a, int Ca, const void* b, int Cb, void* out, long M, void* stream) {
  MD_CHECK_ARG(Ca % 8 == 0 && Cb % 8 == 0, "md_concat_channels: channel counts must be multiples of 8");
  const long total = M * ((Ca + Cb) / 8);
  const int grid = (int)((total + 255) / 256 < 16384 ? (total + 255) / 256 : 16384);
  hipLaunchKernelGGL(concat_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const half_t*)a, (const half_t*)b, (half_t*)out, M, Ca / 8, Cb / 8);
  MD_CHECK_LAUNCH("md_concat_channels");
  return MD_OK;
}

// ---- window accumulate: noise_sum[half][win[i]] += pred[half*f + i], counter[win[i]] += 1 -------------------------------
// Frame slots of one window must be unique or -1 (skipped): blocks of different slots update disjoint rows without atomics.
// pred: [(2 f) HW][4] fp16 (conv_out output, NHWC with 4 channels); noise_sum: [2][Ftot][HW][4] fp32; counter [Ftot] fp32
__global__ void window_accumulate_kernel(const half_t* __restrict__ pred, float* __restrict__ noise_sum, float* __restrict__ counter,
                                         const int* __restrict__ win, int f, int Ftot, int HW4, int halves) {
  const int i = blockIdx.y;  // frame slot inside the window
  const int fr = win[i];
  if (fr < 0) return;  // an earlier duplicate of a frame named twice by this window (host marks it: last occurrence wins)
  if (blockIdx.x == 0 && threadIdx.x == 0) counter[fr] += 1.f;
  for (int h = 0; h < halves; ++h) {
    const half_t* src = pred + (size_t)(h * f + i) * HW4;
    float* dst = noise_sum + ((size_t)h * Ftot + fr) * HW4;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < HW4; e += gridDim.x * blockDim.x) dst[e] += (float)src[e];
  }
}

extern "C" int md_window_accumulate(const void* pred, void* noise_sum, void* counter, const int* window, int f, int Ftot, int HW, int halves, void* stream) {
  MD_CHECK_ARG(f > 0 && Ftot >= f && (halves == 1 || halves == 2), "md_window_accumulate: bad arguments");
  hipLaunchKernelGGL(window_accumulate_kernel, dim3(cdiv(HW * 4, 256 * 4), f), dim3(256), 0, (hipStream_t)stream, (const half_t*)pred, (float*)noise_sum,
                     (float*)counter, window, f, Ftot, HW * 4, halves);
  MD_CHECK_LAUNCH("md_window_accumulate");
  return MD_OK;
}

// ---- weighted window accumulate: noise_sum[half][win[i]] += w[i] * pred[half*f + i], counter[win[i]] += w[i] ------------------
// The pyramid fuse (context_fuse="pyramid"): w[i] is slot i's triangular weight already divided by the frame's total over every window
// of the step (the host normalises, float64 -> fp32), so noise_sum ends up as the weighted MEAN and counter as 1 up to rounding.
// Same buffers, same slot rule (unique or -1) and therefore the same no-atomics argument as window_accumulate_kernel.
// One thread owns one pixel of one slot: 4 fp16 = one 8-byte load per clip-half, 4 fp32 = one 16-byte load and one 16-byte store per
// clip-half, block row blockIdx.y = slot; the loads of both halves are issued before the first store.
// The product and the sum are rounded SEPARATELY (fp contraction is switched off in the kernel body: no fma): a window's share w * p then has
// the same fp32 value whether it lands on this rank's accumulator or arrives through WindowParallel's all-reduce, so a frame that lies in
// at most two windows gets the same bits on one rank and on many (a + b is commutative; fma(w2, p2, w1 p1) is not fl(w1 p1) + fl(w2 p2)).
// With w == 1 the product is exact and the update is window_accumulate_kernel's s + p, bit for bit.
template <int HALVES>
__global__ __launch_bounds__(256) void window_accumulate_weighted_kernel(const half4_t* __restrict__ pred, floatx4* __restrict__ noise_sum,
                                                                         float* __restrict__ counter, const int* __restrict__ win,
                                                                         const float* __restrict__ weights, int f, int Ftot, int HW) {
#pragma clang fp contract(off)
  const int i = blockIdx.y;  // frame slot inside the window
  const int fr = win[i];
  if (fr < 0 || fr >= Ftot) return;  // -1: an earlier duplicate (last occurrence wins); >= Ftot never leaves the host, and is not followed
  const float w = weights[i];
  if (blockIdx.x == 0 && threadIdx.x == 0) counter[fr] += w;
  const int px = blockIdx.x * blockDim.x + threadIdx.x;
  if (px >= HW) return;
  half4_t p[HALVES];
  floatx4 s[HALVES];
#pragma unroll
  for (int h = 0; h < HALVES; ++h) {
    p[h] = pred[(size_t)(h * f + i) * HW + px];
    s[h] = noise_sum[((size_t)h * Ftot + fr) * HW + px];
  }
#pragma unroll
  for (int h = 0; h < HALVES; ++h) {
    floatx4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float share = w * (float)p[h][c];
      o[c] = s[h][c] + share;
    }
    noise_sum[((size_t)h * Ftot + fr) * HW + px] = o;
  }
}

extern "C" int md_window_accumulate_weighted(const void* pred, void* noise_sum, void* counter, const int* window, const float* weights, int f,
                                             int Ftot, int HW, int halves, void* stream) {
  MD_CHECK_ARG(pred && noise_sum && counter && window && weights, "md_window_accumulate_weighted: null pointer");
  MD_CHECK_ARG(f > 0 && f <= 65535 && Ftot >= f && HW > 0 && (halves == 1 || halves == 2), "md_window_accumulate_weighted: bad arguments");
  MD_CHECK_ARG((uintptr_t)pred % 8 == 0 && (uintptr_t)noise_sum % 16 == 0 && (uintptr_t)counter % 4 == 0 && (uintptr_t)window % 4 == 0 &&
                   (uintptr_t)weights % 4 == 0,
               "md_window_accumulate_weighted: pred must be 8-byte, noise_sum 16-byte, counter / window / weights 4-byte aligned");
  const dim3 grid(cdiv(HW, 256), f);
  if (halves == 2)
    hipLaunchKernelGGL(window_accumulate_weighted_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, (const half4_t*)pred, (floatx4*)noise_sum,
                       (float*)counter, window, weights, f, Ftot, HW);
  else
    hipLaunchKernelGGL(window_accumulate_weighted_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const half4_t*)pred, (floatx4*)noise_sum,
                       (float*)counter, window, weights, f, Ftot, HW);
  MD_CHECK_LAUNCH("md_window_accumulate_weighted");
  return MD_OK;
}

// ---- the guided v every kernel of the step tail forms ----------------------------------------------------------------------------
//   u = sum_u / cnt, c = sum_c / cnt, v = u + s (c - u)                              pipeline_mikudance.py:670-674
// as  inv = 1 / cnt;  v = sum_u inv;  c = sum_c inv;  v = v + s (c - v)  in exactly this order.  Without guidance (halves == 1) the
// reference takes the window SUM as it is: its division by the counter sits inside `if do_classifier_free_guidance:`, so neither the
// counter nor the second half is read.  T = float (one element at index i of `total`) or floatx4 (one pixel).  c_out, where given,
// receives c (the rescale statistics; halves == 2 only).
// SCALED in the step kernels (guidance rescale): they multiply this v by *vscale, the factor md_cfg_guidance_rescale left in device
// memory; the unscaled instantiation has neither the load nor the multiply.
template <typename T>
__device__ __forceinline__ T guided_v(const T* __restrict__ ns, const float* __restrict__ counter, long i, long total, int fr, int halves,
                                      float guidance, T* c_out = nullptr) {
  const float inv = halves == 2 ? 1.f / counter[fr] : 1.f;
  T v = ns[i] * inv;
  if (halves == 2) {
    const T c = ns[total + i] * inv;
    v = v + guidance * (c - v);
    if (c_out) *c_out = c;
  }
  return v;
}

// The argument rules all five step entry points share.  Alignment and a kernel's own buffers are its launcher's business.
// noise_coeff: the factor of variance_noise (eta / c_z).  scaled: the *_scaled entries, which need CFG and the factor.
static int cfg_step_check(const char* who, const void* latents, const void* noise_sum, const void* counter, const void* variance_noise,
                          bool scaled, const float* vscale, int Ftot, int HW, int halves, float noise_coeff, std::initializer_list<float> coeffs) {
  MD_CHECK_ARG(Ftot > 0 && HW > 0 && (halves == 1 || halves == 2), "%s: bad arguments", who);
  MD_CHECK_ARG(latents && noise_sum && (halves == 1 || counter), "%s: null pointer", who);
  MD_CHECK_ARG(!scaled || (halves == 2 && vscale && ((uintptr_t)vscale % 4) == 0),
               "%s: guidance rescale needs halves == 2 and a 4-byte aligned vscale", who);
  for (const float c : coeffs) MD_CHECK_ARG(__builtin_isfinite(c), "%s: non-finite coefficient", who);
  MD_CHECK_ARG(noise_coeff == 0.f || variance_noise, "%s: a non-zero noise coefficient needs variance_noise", who);
  return MD_OK;
}

// ---- CFG combine + DDIM v-prediction step -------------------------------------------------------------------------------
//   v   = guided_v
//   x0  = sqrt(a_t) x - sqrt(1-a_t) v ;  eps = sqrt(a_t) v + sqrt(1-a_t) x
//   x'  = sqrt(a_prev) x0 + sqrt(1-a_prev) eps                                      DDIMScheduler.step
// latents: [Ftot][HW][4] fp16, updated in place (fp32 arithmetic, one rounding).
template <bool SCALED>
__global__ void cfg_ddim_kernel(half_t* __restrict__ lat, const float* __restrict__ noise_sum, const float* __restrict__ counter,
                                const half_t* __restrict__ variance_noise, int Ftot, int HW4, int halves, float guidance, float sa, float sb, float sap,
                                float sdir, float sigma, const float* __restrict__ vscale) {
  const long total = (long)Ftot * HW4;
  const float vs = SCALED ? *vscale : 1.f;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    float v = guided_v(noise_sum, counter, idx, total, (int)(idx / HW4), halves, guidance);
    if constexpr (SCALED) v *= vs;
    const float x = (float)lat[idx];
    const float x0 = sa * x - sb * v;
    const float ep = sa * v + sb * x;
    float out = sap * x0 + sdir * ep;                              // sdir = sqrt(1 - alpha_prev - sigma^2)
    if (variance_noise) out += sigma * (float)variance_noise[idx];  // eta > 0: + sigma_t * z
    lat[idx] = (half_t)out;
  }
}

static int cfg_ddim_launch(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, int Ftot, int HW, int halves,
                           float guidance, float alpha_t, float alpha_prev, float eta, void* stream, bool scaled, const float* vscale,
                           const char* who) {
  if (cfg_step_check(who, latents, noise_sum, counter, variance_noise, scaled, vscale, Ftot, HW, halves, eta, {guidance, alpha_t, alpha_prev, eta}))
    return MD_ERR_ARG;
  MD_CHECK_ARG(eta >= 0.f, "%s: eta must be >= 0", who);
  // diffusers DDIMScheduler._get_variance: sigma_t^2 = eta^2 (1 - a_prev) / (1 - a_t) (1 - a_t / a_prev); a_t == 1 never occurs (t >= 0 of a
  // zero-terminal-SNR table has a_t < 1)
  const float var = eta > 0.f ? (1.f - alpha_prev) / (1.f - alpha_t) * (1.f - alpha_t / alpha_prev) : 0.f;
  const float sigma = eta * sqrtf(var > 0.f ? var : 0.f);
  const float dir2 = 1.f - alpha_prev - sigma * sigma;
  const long total = (long)Ftot * HW * 4;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(scaled ? cfg_ddim_kernel<true> : cfg_ddim_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (half_t*)latents,
                     (const float*)noise_sum, (const float*)counter, eta > 0.f ? (const half_t*)variance_noise : nullptr, Ftot, HW * 4, halves,
                     guidance, sqrtf(alpha_t), sqrtf(1.f - alpha_t), sqrtf(alpha_prev), sqrtf(dir2 > 0.f ? dir2 : 0.f), sigma, vscale);
  MD_CHECK_LAUNCH(who);
  return MD_OK;
}

extern "C" int md_cfg_ddim_step(void* latents, const void* noise_sum, const void* counter, int Ftot, int HW, int halves, float guidance, float alpha_t,
                                float alpha_prev, void* stream) {
  return cfg_ddim_launch(latents, noise_sum, counter, nullptr, Ftot, HW, halves, guidance, alpha_t, alpha_prev, 0.f, stream, false, nullptr,
                         "md_cfg_ddim_step");
}

extern "C" int md_cfg_ddim_step_eta(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, int Ftot, int HW, int halves,
                                    float guidance, float alpha_t, float alpha_prev, float eta, void* stream) {
  return cfg_ddim_launch(latents, noise_sum, counter, variance_noise, Ftot, HW, halves, guidance, alpha_t, alpha_prev, eta, stream, false, nullptr,
                         "md_cfg_ddim_step_eta");
}

extern "C" int md_cfg_ddim_step_scaled(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, const float* vscale,
                                       int Ftot, int HW, int halves, float guidance, float alpha_t, float alpha_prev, float eta, void* stream) {
  return cfg_ddim_launch(latents, noise_sum, counter, variance_noise, Ftot, HW, halves, guidance, alpha_t, alpha_prev, eta, stream, true, vscale,
                         "md_cfg_ddim_step_scaled");
}

// ---- CFG combine + DPM-Solver++ multistep step (orders 1 / 2, ODE or SDE; Lu et al., arXiv 2211.01095) ------------------
//   v   = guided_v
//   m0  = alpha_s x - sigma_s v                    data prediction (x0) of this step
//   x'  = c_x x + c_m0 m0 + c_m1 m1 + c_z z        m1 = the previous step's m0 (history), z = variance noise
// The coefficients are host scalars (DPMSolverMultistepScheduler.multistep_coefficients): every solver variant is this one update.
// One thread per pixel (4 channels): 8-byte latents / noise, 16-byte noise_sum / history.  history is read (only when c_m1 != 0: on
// the first step it is uninitialised) and then overwritten with m0 by the same thread at the same index.
template <bool SCALED>
__global__ void cfg_multistep_kernel(half_t* __restrict__ lat, const float* __restrict__ noise_sum, const float* __restrict__ counter,
                                     float* __restrict__ history, const half_t* __restrict__ variance_noise, int Ftot, int HW, int halves,
                                     float guidance, float alpha_s, float sigma_s, float c_x, float c_m0, float c_m1, float c_z,
                                     const float* __restrict__ vscale) {
  const long total = (long)Ftot * HW;  // pixels
  const floatx4* ns = reinterpret_cast<const floatx4*>(noise_sum);
  floatx4* hist = reinterpret_cast<floatx4*>(history);
  half4_t* lat4 = reinterpret_cast<half4_t*>(lat);
  const float vs = SCALED ? *vscale : 1.f;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    floatx4 v = guided_v(ns, counter, p, total, (int)(p / HW), halves, guidance);
    if constexpr (SCALED) v *= vs;
    const floatx4 x = __builtin_convertvector(lat4[p], floatx4);
    const floatx4 m0 = alpha_s * x - sigma_s * v;
    floatx4 out = c_x * x + c_m0 * m0;
    if (c_m1 != 0.f) out += c_m1 * hist[p];
    hist[p] = m0;
    if (variance_noise) out += c_z * __builtin_convertvector(reinterpret_cast<const half4_t*>(variance_noise)[p], floatx4);
    lat4[p] = __builtin_convertvector(out, half4_t);
  }
}

static int cfg_multistep_launch(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise, int Ftot, int HW,
                                int halves, float guidance, float alpha_s, float sigma_s, float c_x, float c_m0, float c_m1, float c_z, void* stream,
                                bool scaled, const float* vscale, const char* who) {
  if (cfg_step_check(who, latents, noise_sum, counter, variance_noise, scaled, vscale, Ftot, HW, halves, c_z,
                     {guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z}))
    return MD_ERR_ARG;
  MD_CHECK_ARG(history, "%s: null history", who);
  MD_CHECK_ARG(((uintptr_t)latents % 8) == 0 && ((uintptr_t)noise_sum % 16) == 0 && ((uintptr_t)history % 16) == 0 &&
                   ((uintptr_t)variance_noise % 8) == 0,
               "%s: latents / variance_noise need 8-byte, noise_sum / history 16-byte alignment", who);
  const long total = (long)Ftot * HW;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(scaled ? cfg_multistep_kernel<true> : cfg_multistep_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream,
                     (half_t*)latents, (const float*)noise_sum, (const float*)counter, (float*)history,
                     c_z != 0.f ? (const half_t*)variance_noise : nullptr, Ftot, HW, halves, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z, vscale);
  MD_CHECK_LAUNCH(who);
  return MD_OK;
}

extern "C" int md_cfg_multistep_step(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise, int Ftot,
                                     int HW, int halves, float guidance, float alpha_s, float sigma_s, float c_x, float c_m0, float c_m1, float c_z,
                                     void* stream) {
  return cfg_multistep_launch(latents, noise_sum, counter, history, variance_noise, Ftot, HW, halves, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z,
                              stream, false, nullptr, "md_cfg_multistep_step");
}

extern "C" int md_cfg_multistep_step_scaled(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise,
                                            const float* vscale, int Ftot, int HW, int halves, float guidance, float alpha_s, float sigma_s, float c_x,
                                            float c_m0, float c_m1, float c_z, void* stream) {
  return cfg_multistep_launch(latents, noise_sum, counter, history, variance_noise, Ftot, HW, halves, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z,
                              stream, true, vscale, "md_cfg_multistep_step_scaled");
}

// ---- guidance rescale factor (Lin et al., arXiv 2305.08891 section 3.4; diffusers rescale_noise_cfg) ----------------------------------
//   c = sum_c / cnt, v = u + s (c - u)              formed on the fly by guided_v, the step kernels' own code (never materialised)
//   out_scale = 1 - phi + phi std(c) / std(v)      std over all Ftot HW 4 elements; the (N - 1) of torch.std cancels in the ratio
//   std(v) == 0 -> out_scale = 1                  (diffusers would give inf / NaN; NaN / Inf inputs still propagate)
// Deterministic, no float atomics, no host sync: rescale_blocks(Ftot, HW) <= 512 workgroups, each over a FIXED contiguous slice of
// pixels, reduce shifted sums in fp64 (pilot = element 0 of c and of v, so that a large common offset does not cancel; differences and
// squares are formed in fp64) through a fixed butterfly and a fixed wave order into workspace partials; ONE small launch then adds the
// partials in a fixed order and writes the factor.  A separate finalize launch (~2 us) instead of a combine in every workgroup of the step
// kernel's prologue: the step kernels run up to 4096 workgroups, each would re-read all partials, and the factor would never exist on its own
// (the tests compare it against float64 directly).
#define RS_THREADS 256
#define RS_MAX_BLOCKS 512

static int rescale_blocks(int Ftot, int HW) {
  const long b = ((long)Ftot * HW + RS_THREADS - 1) / RS_THREADS;
  return (int)(b < RS_MAX_BLOCKS ? b : RS_MAX_BLOCKS);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// part[b] = (sum dc, sum dc^2, sum dv, sum dv^2) of workgroup b's slice, dc = c - c[0], dv = v - v[0]
__global__ void __launch_bounds__(RS_THREADS) cfg_rescale_partials_kernel(const float* __restrict__ noise_sum, const float* __restrict__ counter,
                                                                          double* __restrict__ part, int Ftot, int HW, float guidance, long chunk) {
  const long total = (long)Ftot * HW;
  const floatx4* ns = reinterpret_cast<const floatx4*>(noise_sum);
  floatx4 c;
  floatx4 v = guided_v(ns, counter, 0, total, 0, 2, guidance, &c);
  const double kc = c.x, kv = v.x;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  const long p1 = min(((long)blockIdx.x + 1) * chunk, total);
  for (long p = (long)blockIdx.x * chunk + threadIdx.x; p < p1; p += RS_THREADS) {
    v = guided_v(ns, counter, p, total, (int)(p / HW), 2, guidance, &c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double dc = (double)c[e] - kc, dv = (double)v[e] - kv;
      s[0] += dc;
      s[1] += dc * dc;
      s[2] += dv;
      s[3] += dv * dv;
    }
  }
  __shared__ double red[RS_THREADS / 64][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    s[q] = wave_sum_f64(s[q]);
    if (lane == 0) red[wave][q] = s[q];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    double a = 0.0;
    for (int w = 0; w < RS_THREADS / 64; ++w) a += red[w][threadIdx.x];
    part[(size_t)blockIdx.x * 4 + threadIdx.x] = a;
  }
}

// One wave: lane l adds partials l, l + 64, ... in that order, then the fixed butterfly; lane 0 writes the factor.
__global__ void __launch_bounds__(64) cfg_rescale_finalize_kernel(const double* __restrict__ part, int nblocks, double n, float phi,
                                                                  float* __restrict__ out_scale) {
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblocks; b += 64)
#pragma unroll
    for (int q = 0; q < 4; ++q) s[q] += part[(size_t)b * 4 + q];
#pragma unroll
  for (int q = 0; q < 4; ++q) s[q] = wave_sum_f64(s[q]);
  if (threadIdx.x == 0) {
    double m2c = s[1] - s[0] * s[0] / n, m2v = s[3] - s[2] * s[2] / n;  // n * biased variance; NaN stays NaN
    m2c = m2c < 0.0 ? 0.0 : m2c;
    m2v = m2v < 0.0 ? 0.0 : m2v;
    const double phid = (double)phi;
    out_scale[0] = m2v == 0.0 ? 1.f : (float)(1.0 - phid + phid * sqrt(m2c / m2v));
  }
}

extern "C" size_t md_cfg_rescale_workspace_bytes(int Ftot, int HW) {
  return Ftot > 0 && HW > 0 ? (size_t)rescale_blocks(Ftot, HW) * 4 * sizeof(double) : 0;
}

extern "C" int md_cfg_guidance_rescale(const void* noise_sum, const void* counter, int Ftot, int HW, int halves, float guidance, float phi,
                                       void* workspace, size_t workspace_bytes, void* out_scale, void* stream) {
  MD_CHECK_ARG(noise_sum && counter && workspace && out_scale && Ftot > 0 && HW > 0 && halves == 2,
               "md_cfg_guidance_rescale: bad arguments (guidance rescale needs halves == 2)");
  MD_CHECK_ARG(((uintptr_t)noise_sum % 16) == 0 && ((uintptr_t)counter % 4) == 0 && ((uintptr_t)workspace % 8) == 0 &&
                   ((uintptr_t)out_scale % 4) == 0,
               "md_cfg_guidance_rescale: noise_sum needs 16-byte, workspace 8-byte, counter / out_scale 4-byte alignment");
  MD_CHECK_ARG(__builtin_isfinite(guidance) && __builtin_isfinite(phi) && phi >= 0.f && phi <= 1.f,
               "md_cfg_guidance_rescale: guidance must be finite and phi finite in [0, 1]");
  MD_CHECK_ARG(workspace_bytes >= md_cfg_rescale_workspace_bytes(Ftot, HW), "md_cfg_guidance_rescale: workspace too small");
  const long total = (long)Ftot * HW;
  const int nb = rescale_blocks(Ftot, HW);
  const long chunk = (total + nb - 1) / nb;
  hipLaunchKernelGGL(cfg_rescale_partials_kernel, dim3(nb), dim3(RS_THREADS), 0, (hipStream_t)stream, (const float*)noise_sum, (const float*)counter,
                     (double*)workspace, Ftot, HW, guidance, chunk);
  MD_CHECK_LAUNCH("md_cfg_guidance_rescale");
  hipLaunchKernelGGL(cfg_rescale_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, nb, (double)total * 4.0, phi,
                     (float*)out_scale);
  MD_CHECK_LAUNCH("md_cfg_guidance_rescale");
  return MD_OK;
}

// ---- forward noising of a clean latent (video-to-video start; diffusers DDIMScheduler.add_noise) ----------------------------------
//   latents = fp16(a x0 + b latents)      a = sqrt(abar_t), b = sqrt(1 - abar_t) from the host; fp32 arithmetic, one rounding
// latents holds the noise on entry and is updated in place.  a == 0 (t = 999 of the zero-terminal-SNR table) never reads x0: the output is
// then b * noise exactly, whatever x0 holds (0 * Inf would be NaN).  Runs once per clip: a plain grid-stride loop over fp16 elements.
__global__ void add_noise_kernel(half_t* __restrict__ lat, const half_t* __restrict__ x0, long n, float a, float b) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float z = (float)lat[i];
    lat[i] = (half_t)(a != 0.f ? a * (float)x0[i] + b * z : b * z);
  }
}

extern "C" int md_add_noise_f16(void* latents, const void* x0, long n, float a, float b, void* stream) {
  MD_CHECK_ARG(latents && x0 && n > 0, "md_add_noise_f16: bad arguments");
  MD_CHECK_ARG(((uintptr_t)latents % 2) == 0 && ((uintptr_t)x0 % 2) == 0, "md_add_noise_f16: latents / x0 need 2-byte alignment");
  MD_CHECK_ARG(__builtin_isfinite(a) && __builtin_isfinite(b) && a >= 0.f && b >= 0.f, "md_add_noise_f16: a and b must be finite and >= 0");
  const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(add_noise_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (half_t*)latents, (const half_t*)x0, n, a, b);
  MD_CHECK_LAUNCH("md_add_noise_f16");
  return MD_OK;
}

// ---- generic strided scatter of NHWC fp16 -> any layout/dtype (API boundary: UNet.forward returns NCFHW) ---------------
template <typename T>
__global__ void unpack_nhwc_kernel(const half_t* __restrict__ src, T* __restrict__ dst, long total, int F, long sB, long sF, long sC, long sY, long sX,
                                   int C, int ldc, int Ho, int Wo) {
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int c = (int)(idx % C);
    long r = idx / C;
    const int x = (int)(r % Wo);
    r /= Wo;
    const int y = (int)(r % Ho);
    const long n = r / Ho;
    dst[(n / F) * sB + (n % F) * sF + (long)c * sC + (long)y * sY + (long)x * sX] = (T)(float)src[((n * Ho + y) * Wo + x) * ldc + c];
  }
}

extern "C" int md_unpack_nhwc_f16(const void* src, int ldc, void* dst, int dst_is_f32, int N, int F, long sB, long sF, long sC, long sY, long sX, int C,
                                  int Ho, int Wo, void* stream) {
  MD_CHECK_ARG(N > 0 && F > 0 && C <= ldc, "md_unpack_nhwc: bad arguments");
  const long total = (long)N * Ho * Wo * C;
  const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
  if (dst_is_f32)
    hipLaunchKernelGGL(unpack_nhwc_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const half_t*)src, (float*)dst, total, F, sB, sF, sC, sY,
                       sX, C, ldc, Ho, Wo);
  else
    hipLaunchKernelGGL(unpack_nhwc_kernel<half_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const half_t*)src, (half_t*)dst, total, F, sB, sF, sC, sY,
                       sX, C, ldc, Ho, Wo);
  MD_CHECK_LAUNCH("md_unpack_nhwc");
  return MD_OK;
}
