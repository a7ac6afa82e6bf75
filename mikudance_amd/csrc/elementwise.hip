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
template <typename T>
__device__ __forceinline__ T guided_v(const T* __restrict__ ns, const float* __restrict__ counter, long i, long total, int fr, int halves,
                                      float guidance, T* c_out = nullptr) {
  const float inv = halves == 2 ? 1.f / counter[fr] : 1.f;
  T v = ns[i] * inv;
  if (halves == 2) {
    const T c = ns[total + i] * inv;
    T d;
    {
      // c is a finished (rounded) value when it is subtracted, as the order above says: contracted, c - v became fma(sum_c, inv, -v), which
      // leaves the rounding error of one product where sum_c == sum_u bit for bit (md_cfg_uncond_cache, mode 1 with scale 0), and the
      // guided v of a step without guidance would not be the conditional mean exactly
#pragma clang fp contract(off)
      d = c - v;
    }
    v = v + guidance * d;
    if (c_out) *c_out = c;
  }
  return v;
}

// APG in the step kernels (adaptive projected guidance, the *_apg entries): the guided v is replaced by
//   D_c = a x - s c ;  v_g = c - (g - 1) (S m - K D_c) / s
// with c formed by guided_v, m the momentum buffer and (S, K) = coef[fr] as md_cfg_apg_prepare left them in device memory, a / s the
// step's sqrt(abar_t) / sqrt(1 - abar_t), x the latent and gs = (g - 1) / s from the caller.  T as in guided_v.
template <typename T>
__device__ __forceinline__ T apg_v(const T* __restrict__ ns, const float* __restrict__ counter, const T* __restrict__ mom,
                                   const float* __restrict__ coef, long i, long total, int fr, float guidance, float a, float s, float gs, T x) {
  T c;
  guided_v(ns, counter, i, total, fr, 2, guidance, &c);
  const float S = coef[2 * fr], K = coef[2 * fr + 1];
  const T dc = a * x - s * c;
  return c - gs * (S * mom[i] - K * dc);
}

// PAG in the step kernels (perturbed-attention guidance, the *_pag entries; Ahn et al., arXiv 2403.17377, diffusers PAGMixin): the guided v
// gains the step away from a second conditional prediction p, made with the self-attention map of a few blocks replaced by the identity:
//   v = guided_v + s (c - p)  =  guided_v + s inv (sum_c - sum_p)
// inv as guided_v has it (1 / cnt under CFG, 1 without: the window SUM), sum_c the conditional plane of ns (plane halves - 1), sum_p the
// perturbed plane `pp`, accumulated like the others.  s == 0 adds a zero: the bits of guided_v, for finite planes.  T as in guided_v.
template <typename T>
__device__ __forceinline__ T pag_v(const T* __restrict__ ns, const T* __restrict__ pp, const float* __restrict__ counter, long i, long total, int fr,
                                   int halves, float guidance, float pag_scale) {
  const T v = guided_v(ns, counter, i, total, fr, halves, guidance);
  const float inv = halves == 2 ? 1.f / counter[fr] : 1.f;
  const T d = ns[(halves == 2 ? total : 0) + i] - pp[i];
  return v + (pag_scale * inv) * d;
}

// ---- the guide of a step: what an entry adds to the plain one -------------------------------------------------------------------
//   guide          entries     aux0                           aux1                auxs
//   GUIDE_PLAIN    (plain)     -                              -                   -
//   GUIDE_SCALED   *_scaled    vscale, one fp32 (the factor   -                   -
//                              md_cfg_guidance_rescale left)
//   GUIDE_APG      *_apg       momentum buffer [Ftot][HW][4]  coef [Ftot][2]      gs = (guidance - 1) / sigma_s, formed by the launcher
//   GUIDE_PAG      *_pag       perturbed plane [Ftot][HW][4]  -                   pag_scale
// all fp32 in device memory, as md_cfg_guidance_rescale / md_cfg_apg_prepare / the window accumulation left them.
enum { GUIDE_PLAIN = 0, GUIDE_SCALED, GUIDE_APG, GUIDE_PAG };

struct StepExtra {
  int guide = GUIDE_PLAIN;
  const float* aux0 = nullptr;
  const float* aux1 = nullptr;
  float auxs = 0.f;
};

static StepExtra step_scaled(const float* vscale) { return {GUIDE_SCALED, vscale, nullptr, 0.f}; }
static StepExtra step_apg(const void* momentum_buf, const float* coef) { return {GUIDE_APG, (const float*)momentum_buf, coef, 0.f}; }
static StepExtra step_pag(const void* perturbed_sum, float pag_scale) { return {GUIDE_PAG, (const float*)perturbed_sum, nullptr, pag_scale}; }

// The v a step kernel updates with, for the element or pixel i (T as in guided_v): the one place that chooses between guided_v, apg_v and
// pag_v.  aux0 / aux1: the guide's buffers; sc: its scalar, which for GUIDE_SCALED is *vscale as the kernel read it once ahead of its loop
// (the plain instantiation has neither the load nor the multiply).  a, s, x: the step's alpha_s / sigma_s and the latent, which APG reads.
// The fence: under PAG v leaves as a finished value, opaque to the compiler.  pag_scale == 0 must give the plain entry's bits, and without
// the fence the update that follows is free to fuse its products with other sums than in the plain instantiation (DDIM's did, while its
// update was left to contraction: sb x + sa v instead of sa v + sb x).  It is unconditional: UniPC's PAG instantiation, written without
// one, gives the same bits with it (50 of 50 cases on an MI355X, profiles/step_kernels_refactor.log), so no sampler needs to opt out.
// The other guides promise no bits of another entry and have none.
template <int GUIDE, typename T>
__device__ __forceinline__ T step_v(const T* __restrict__ ns, const float* __restrict__ counter, const T* __restrict__ aux0,
                                    const float* __restrict__ aux1, float sc, long i, long total, int fr, int halves, float guidance, float a,
                                    float s, T x) {
  T v;
  if constexpr (GUIDE == GUIDE_APG)
    v = apg_v(ns, counter, aux0, aux1, i, total, fr, guidance, a, s, sc, x);
  else if constexpr (GUIDE == GUIDE_PAG)
    v = pag_v(ns, aux0, counter, i, total, fr, halves, guidance, sc);
  else
    v = guided_v(ns, counter, i, total, fr, halves, guidance);
  if constexpr (GUIDE == GUIDE_SCALED) v *= sc;
  if constexpr (GUIDE == GUIDE_PAG) asm volatile("" : "+v"(v));
  return v;
}

// Launches the instantiation of a step kernel that ex.guide names, one thread per element or pixel up to one grid round of 4096 x 256.
// k: the four instantiations in the enum's order; args: the kernel's arguments up to the guide's three, which follow from ex.
template <typename K, typename... Args>
static void step_launch(K* const (&k)[4], const StepExtra& ex, float apg_gs, long threads, void* stream, Args... args) {
  const int grid = (int)((threads + 255) / 256 < 4096 ? (threads + 255) / 256 : 4096);
  hipLaunchKernelGGL(k[ex.guide], dim3(grid), dim3(256), 0, (hipStream_t)stream, args..., ex.aux0, ex.aux1,
                     ex.guide == GUIDE_APG ? apg_gs : ex.auxs);
}

// The argument rules all step entry points share.  Alignment and a kernel's own buffers are its launcher's business.
// noise_coeff: the factor of variance_noise (eta / c_z).  The *_scaled entries need CFG and the factor; the *_apg entries CFG, the momentum
// buffer and the coefficients; the *_pag entries the perturbed plane and a finite scale >= 0, with or without CFG.
static int cfg_step_check(const char* who, const void* latents, const void* noise_sum, const void* counter, const void* variance_noise,
                          const StepExtra& ex, int Ftot, int HW, int halves, float noise_coeff, std::initializer_list<float> coeffs) {
  MD_CHECK_ARG(Ftot > 0 && HW > 0 && (halves == 1 || halves == 2), "%s: bad arguments", who);
  MD_CHECK_ARG(latents && noise_sum && (halves == 1 || counter), "%s: null pointer", who);
  MD_CHECK_ARG(ex.guide != GUIDE_SCALED || (halves == 2 && ex.aux0 && ((uintptr_t)ex.aux0 % 4) == 0),
               "%s: guidance rescale needs halves == 2 and a 4-byte aligned vscale", who);
  MD_CHECK_ARG(ex.guide != GUIDE_APG || (halves == 2 && ex.aux0 && ex.aux1), "%s: APG needs halves == 2, the momentum buffer and coef", who);
  MD_CHECK_ARG(ex.guide != GUIDE_PAG || (ex.aux0 && __builtin_isfinite(ex.auxs) && ex.auxs >= 0.f),
               "%s: PAG needs the perturbed plane and a finite pag_scale >= 0", who);
  for (const float c : coeffs) MD_CHECK_ARG(__builtin_isfinite(c), "%s: non-finite coefficient", who);
  MD_CHECK_ARG(noise_coeff == 0.f || variance_noise, "%s: a non-zero noise coefficient needs variance_noise", who);
  return MD_OK;
}

// The alignment md_cfg_multistep_step asks for (one pixel = 4 channels per access), which the *_apg and *_pag entries ask for as well.
static int cfg_pixel_alignment_check(const char* who, const void* latents, const void* noise_sum, const void* history,
                                     const void* variance_noise, const StepExtra& ex) {
  MD_CHECK_ARG(((uintptr_t)latents % 8) == 0 && ((uintptr_t)noise_sum % 16) == 0 && ((uintptr_t)history % 16) == 0 &&
                   ((uintptr_t)variance_noise % 8) == 0,
               "%s: latents / variance_noise need 8-byte, noise_sum / history 16-byte alignment", who);
  MD_CHECK_ARG(ex.guide != GUIDE_APG || (((uintptr_t)ex.aux0 % 16) == 0 && ((uintptr_t)ex.aux1 % 4) == 0),
               "%s: the momentum buffer needs 16-byte, coef 4-byte alignment", who);
  MD_CHECK_ARG(ex.guide != GUIDE_PAG || ((uintptr_t)ex.aux0 % 16) == 0, "%s: the perturbed plane needs 16-byte alignment", who);
  return MD_OK;
}

// ---- CFG combine + DDIM v-prediction step -------------------------------------------------------------------------------
//   v   = step_v                                                                     the guided v under the entry's guide
//   x0  = sqrt(a_t) x - sqrt(1-a_t) v ;  eps = sqrt(a_t) v + sqrt(1-a_t) x
//   x'  = sqrt(a_prev) x0 + sqrt(1-a_prev) eps                                      DDIMScheduler.step
// latents: [Ftot][HW][4] fp16, updated in place (fp32 arithmetic, one rounding).
// ddim_update is the update every guide of the kernel shares, from v on.  x0 and eps are spelled out as one rounded product and one fma
// each: left to contraction, which product is rounded follows from where the kernel happens to load x, and the entries' bits with it.
// x0 under APG rounds sa x, the product its D_c already holds, and under every other guide sb v; both are the bits each entry has always
// given, so both stay.
template <int GUIDE>
__device__ __forceinline__ void ddim_update(half_t* __restrict__ lat, const half_t* __restrict__ variance_noise, long idx, float x, float v, float sa,
                                            float sb, float sap, float sdir, float sigma) {
  const float x0 = GUIDE == GUIDE_APG ? __builtin_fmaf(-sb, v, sa * x) : __builtin_fmaf(sa, x, -(sb * v));
  const float ep = __builtin_fmaf(sa, v, sb * x);
  float out = sap * x0 + sdir * ep;                              // sdir = sqrt(1 - alpha_prev - sigma^2)
  if (variance_noise) out += sigma * (float)variance_noise[idx];  // eta > 0: + sigma_t * z
  lat[idx] = (half_t)out;
}

// One element per thread.  APG's mom / coef are md_cfg_apg_prepare's at THIS step's (sa, sb).
template <int GUIDE>
__global__ void cfg_ddim_kernel(half_t* __restrict__ lat, const float* __restrict__ noise_sum, const float* __restrict__ counter,
                                const half_t* __restrict__ variance_noise, int Ftot, int HW4, int halves, float guidance, float sa, float sb, float sap,
                                float sdir, float sigma, const float* __restrict__ aux0, const float* __restrict__ aux1, float auxs) {
  const long total = (long)Ftot * HW4;
  const float sc = GUIDE == GUIDE_SCALED ? *aux0 : auxs;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const float x = (float)lat[idx];
    const float v = step_v<GUIDE>(noise_sum, counter, aux0, aux1, sc, idx, total, (int)(idx / HW4), halves, guidance, sa, sb, x);
    ddim_update<GUIDE>(lat, variance_noise, idx, x, v, sa, sb, sap, sdir, sigma);
  }
}

static int cfg_ddim_launch(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, int Ftot, int HW, int halves,
                           float guidance, float alpha_t, float alpha_prev, float eta, void* stream, const StepExtra& ex, const char* who) {
  if (cfg_step_check(who, latents, noise_sum, counter, variance_noise, ex, Ftot, HW, halves, eta, {guidance, alpha_t, alpha_prev, eta}))
    return MD_ERR_ARG;
  MD_CHECK_ARG(eta >= 0.f, "%s: eta must be >= 0", who);
  // single-element accesses under every guide: the *_pag entry asks for natural alignment only, like the plain one, and the *_apg entry
  // keeps the contract it was published with, md_cfg_multistep_step's
  if (ex.guide == GUIDE_APG) {
    if (cfg_pixel_alignment_check(who, latents, noise_sum, nullptr, variance_noise, ex)) return MD_ERR_ARG;
    MD_CHECK_ARG(alpha_t >= 0.f && alpha_t < 1.f, "%s: APG divides by sqrt(1 - alpha_t): alpha_t must be in [0, 1)", who);
  }
  MD_CHECK_ARG(ex.guide != GUIDE_PAG || (((uintptr_t)latents % 2) == 0 && ((uintptr_t)variance_noise % 2) == 0 &&
                                         ((uintptr_t)noise_sum % 4) == 0 && ((uintptr_t)counter % 4) == 0 && ((uintptr_t)ex.aux0 % 4) == 0),
               "%s: latents / variance_noise need 2-byte, noise_sum / counter / the perturbed plane 4-byte alignment", who);
  // diffusers DDIMScheduler._get_variance: sigma_t^2 = eta^2 (1 - a_prev) / (1 - a_t) (1 - a_t / a_prev); a_t == 1 never occurs (t >= 0 of a
  // zero-terminal-SNR table has a_t < 1)
  const float var = eta > 0.f ? (1.f - alpha_prev) / (1.f - alpha_t) * (1.f - alpha_t / alpha_prev) : 0.f;
  const float sigma = eta * sqrtf(var > 0.f ? var : 0.f);
  const float dir2 = 1.f - alpha_prev - sigma * sigma;
  const half_t* z = eta > 0.f ? (const half_t*)variance_noise : nullptr;
  const float sa = sqrtf(alpha_t), sb = sqrtf(1.f - alpha_t), sap = sqrtf(alpha_prev), sdir = sqrtf(dir2 > 0.f ? dir2 : 0.f);
  step_launch({cfg_ddim_kernel<GUIDE_PLAIN>, cfg_ddim_kernel<GUIDE_SCALED>, cfg_ddim_kernel<GUIDE_APG>, cfg_ddim_kernel<GUIDE_PAG>}, ex,
              (guidance - 1.f) / sb, (long)Ftot * HW * 4, stream, (half_t*)latents, (const float*)noise_sum, (const float*)counter, z, Ftot, HW * 4,
              halves, guidance, sa, sb, sap, sdir, sigma);
  MD_CHECK_LAUNCH(who);
  return MD_OK;
}

extern "C" int md_cfg_ddim_step(void* latents, const void* noise_sum, const void* counter, int Ftot, int HW, int halves, float guidance, float alpha_t,
                                float alpha_prev, void* stream) {
  return cfg_ddim_launch(latents, noise_sum, counter, nullptr, Ftot, HW, halves, guidance, alpha_t, alpha_prev, 0.f, stream, StepExtra(),
                         "md_cfg_ddim_step");
}

extern "C" int md_cfg_ddim_step_eta(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, int Ftot, int HW, int halves,
                                    float guidance, float alpha_t, float alpha_prev, float eta, void* stream) {
  return cfg_ddim_launch(latents, noise_sum, counter, variance_noise, Ftot, HW, halves, guidance, alpha_t, alpha_prev, eta, stream, StepExtra(),
                         "md_cfg_ddim_step_eta");
}

extern "C" int md_cfg_ddim_step_scaled(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, const float* vscale,
                                       int Ftot, int HW, int halves, float guidance, float alpha_t, float alpha_prev, float eta, void* stream) {
  return cfg_ddim_launch(latents, noise_sum, counter, variance_noise, Ftot, HW, halves, guidance, alpha_t, alpha_prev, eta, stream,
                         step_scaled(vscale), "md_cfg_ddim_step_scaled");
}

extern "C" int md_cfg_ddim_step_apg(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, const void* momentum_buf,
                                    const float* coef, int Ftot, int HW, int halves, float guidance, float alpha_t, float alpha_prev, float eta,
                                    void* stream) {
  return cfg_ddim_launch(latents, noise_sum, counter, variance_noise, Ftot, HW, halves, guidance, alpha_t, alpha_prev, eta, stream,
                         step_apg(momentum_buf, coef), "md_cfg_ddim_step_apg");
}

extern "C" int md_cfg_ddim_step_pag(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, const void* perturbed_sum,
                                    int Ftot, int HW, int halves, float guidance, float pag_scale, float alpha_t, float alpha_prev, float eta,
                                    void* stream) {
  return cfg_ddim_launch(latents, noise_sum, counter, variance_noise, Ftot, HW, halves, guidance, alpha_t, alpha_prev, eta, stream,
                         step_pag(perturbed_sum, pag_scale), "md_cfg_ddim_step_pag");
}

// ---- CFG combine + DPM-Solver++ multistep step (orders 1 / 2, ODE or SDE; Lu et al., arXiv 2211.01095) ------------------
//   v   = step_v                                   the guided v under the entry's guide
//   m0  = alpha_s x - sigma_s v                    data prediction (x0) of this step
//   x'  = c_x x + c_m0 m0 + c_m1 m1 + c_z z        m1 = the previous step's m0 (history), z = variance noise
// The coefficients are host scalars (DPMSolverMultistepScheduler.multistep_coefficients): every solver variant is this one update.
// One thread per pixel (4 channels): 8-byte latents / noise, 16-byte noise_sum / history.  history is read (only when c_m1 != 0: on
// the first step it is uninitialised) and then overwritten with m0 by the same thread at the same index.
// multistep_update is the update every flavour of the kernel shares, from v on.
__device__ __forceinline__ void multistep_update(half4_t* __restrict__ lat4, floatx4* __restrict__ hist, const half_t* __restrict__ variance_noise,
                                                 long p, floatx4 x, floatx4 v, float alpha_s, float sigma_s, float c_x, float c_m0, float c_m1,
                                                 float c_z) {
  const floatx4 m0 = alpha_s * x - sigma_s * v;
  floatx4 out = c_x * x + c_m0 * m0;
  if (c_m1 != 0.f) out += c_m1 * hist[p];
  hist[p] = m0;
  if (variance_noise) out += c_z * __builtin_convertvector(reinterpret_cast<const half4_t*>(variance_noise)[p], floatx4);
  lat4[p] = __builtin_convertvector(out, half4_t);
}

// APG's mom / coef are md_cfg_apg_prepare's at THIS step's (alpha_s, sigma_s).
template <int GUIDE>
__global__ void cfg_multistep_kernel(half_t* __restrict__ lat, const float* __restrict__ noise_sum, const float* __restrict__ counter,
                                     float* __restrict__ history, const half_t* __restrict__ variance_noise, int Ftot, int HW, int halves,
                                     float guidance, float alpha_s, float sigma_s, float c_x, float c_m0, float c_m1, float c_z,
                                     const float* __restrict__ aux0, const float* __restrict__ aux1, float auxs) {
  const long total = (long)Ftot * HW;  // pixels
  const floatx4* ns = reinterpret_cast<const floatx4*>(noise_sum);
  const floatx4* a4 = reinterpret_cast<const floatx4*>(aux0);
  floatx4* hist = reinterpret_cast<floatx4*>(history);
  half4_t* lat4 = reinterpret_cast<half4_t*>(lat);
  const float sc = GUIDE == GUIDE_SCALED ? *aux0 : auxs;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const floatx4 x = __builtin_convertvector(lat4[p], floatx4);
    const floatx4 v = step_v<GUIDE>(ns, counter, a4, aux1, sc, p, total, (int)(p / HW), halves, guidance, alpha_s, sigma_s, x);
    multistep_update(lat4, hist, variance_noise, p, x, v, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z);
  }
}

static int cfg_multistep_launch(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise, int Ftot, int HW,
                                int halves, float guidance, float alpha_s, float sigma_s, float c_x, float c_m0, float c_m1, float c_z, void* stream,
                                const StepExtra& ex, const char* who) {
  if (cfg_step_check(who, latents, noise_sum, counter, variance_noise, ex, Ftot, HW, halves, c_z,
                     {guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z}))
    return MD_ERR_ARG;
  MD_CHECK_ARG(history, "%s: null history", who);
  if (cfg_pixel_alignment_check(who, latents, noise_sum, history, variance_noise, ex)) return MD_ERR_ARG;
  MD_CHECK_ARG(ex.guide != GUIDE_APG || sigma_s > 0.f, "%s: APG divides by sigma_s: it must be > 0", who);
  const half_t* z = c_z != 0.f ? (const half_t*)variance_noise : nullptr;
  step_launch({cfg_multistep_kernel<GUIDE_PLAIN>, cfg_multistep_kernel<GUIDE_SCALED>, cfg_multistep_kernel<GUIDE_APG>,
               cfg_multistep_kernel<GUIDE_PAG>},
              ex, (guidance - 1.f) / sigma_s, (long)Ftot * HW, stream, (half_t*)latents, (const float*)noise_sum, (const float*)counter,
              (float*)history, z, Ftot, HW, halves, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z);
  MD_CHECK_LAUNCH(who);
  return MD_OK;
}

extern "C" int md_cfg_multistep_step(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise, int Ftot,
                                     int HW, int halves, float guidance, float alpha_s, float sigma_s, float c_x, float c_m0, float c_m1, float c_z,
                                     void* stream) {
  return cfg_multistep_launch(latents, noise_sum, counter, history, variance_noise, Ftot, HW, halves, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z,
                              stream, StepExtra(), "md_cfg_multistep_step");
}

extern "C" int md_cfg_multistep_step_scaled(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise,
                                            const float* vscale, int Ftot, int HW, int halves, float guidance, float alpha_s, float sigma_s, float c_x,
                                            float c_m0, float c_m1, float c_z, void* stream) {
  return cfg_multistep_launch(latents, noise_sum, counter, history, variance_noise, Ftot, HW, halves, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z,
                              stream, step_scaled(vscale), "md_cfg_multistep_step_scaled");
}

extern "C" int md_cfg_multistep_step_apg(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise,
                                         const void* momentum_buf, const float* coef, int Ftot, int HW, int halves, float guidance, float alpha_s,
                                         float sigma_s, float c_x, float c_m0, float c_m1, float c_z, void* stream) {
  return cfg_multistep_launch(latents, noise_sum, counter, history, variance_noise, Ftot, HW, halves, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z,
                              stream, step_apg(momentum_buf, coef), "md_cfg_multistep_step_apg");
}

extern "C" int md_cfg_multistep_step_pag(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise,
                                         const void* perturbed_sum, int Ftot, int HW, int halves, float guidance, float pag_scale, float alpha_s,
                                         float sigma_s, float c_x, float c_m0, float c_m1, float c_z, void* stream) {
  return cfg_multistep_launch(latents, noise_sum, counter, history, variance_noise, Ftot, HW, halves, guidance, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z,
                              stream, step_pag(perturbed_sum, pag_scale), "md_cfg_multistep_step_pag");
}

// ---- CFG combine + UniPC correct-then-predict step (orders 1 - 3; Zhao et al., arXiv 2302.04867, data-prediction form) -----------------
//   v    = step_v                                            the guided v under the entry's guide
//   m_t  = alpha_s x - sigma_s v                             data prediction at this step's point, x the fp16 latent the UNet saw
//   x^c  = cc_x x_last + cc_m m_t + cc_0 H0 + cc_1 H1 + cc_2 H2      UniC from the previous point to this one; corrector off: x^c = x
//   x'   = pc_x x^c + pc_m m_t + pc_0 H0 + pc_1 H1                   UniP from this point to the next, stored as the fp16 latent
//   x_last <- x^c;  H0 <- m_t;  H1 <- H0;  H2 <- H1
// Every solver variant is this one update: the weights are host scalars (UniPCMultistepScheduler.unipc_coefficients, the <= 3 x 3 systems
// solved there in float64).  state: fp32 planes [x_last, H0, H1, H2], each [Ftot][HW][4].  One thread owns one pixel: an 8-byte latent
// access and 16-byte plane accesses, the rotation a register move.  A plane is read only where one of its weights is non-zero (x_last only
// with the corrector on) and only a plane that was read moves down a slot, so the first step runs on an uninitialised state; the scheduler's
// docstring shows that no later step misses a plane that was left behind.
struct UniPCRow {
  float alpha_s, sigma_s;
  float cc_x, cc_m, cc_0, cc_1, cc_2;
  float pc_x, pc_m, pc_0, pc_1;
  int correct;
};

template <int GUIDE>
__global__ __launch_bounds__(256) void cfg_unipc_kernel(half_t* __restrict__ lat, const float* __restrict__ noise_sum,
                                                        const float* __restrict__ counter, float* __restrict__ state, int Ftot, int HW, int halves,
                                                        float guidance, UniPCRow r, const float* __restrict__ aux0, const float* __restrict__ aux1,
                                                        float auxs) {
  const long total = (long)Ftot * HW;  // pixels
  const floatx4* ns = reinterpret_cast<const floatx4*>(noise_sum);
  const floatx4* a4 = reinterpret_cast<const floatx4*>(aux0);
  half4_t* lat4 = reinterpret_cast<half4_t*>(lat);
  floatx4* xl = reinterpret_cast<floatx4*>(state);
  floatx4 *H0 = xl + total, *H1 = H0 + total, *H2 = H1 + total;
  const bool rd0 = r.cc_0 != 0.f || r.pc_0 != 0.f, rd1 = r.cc_1 != 0.f || r.pc_1 != 0.f, rd2 = r.cc_2 != 0.f;
  const float sc = GUIDE == GUIDE_SCALED ? *aux0 : auxs;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const floatx4 x = __builtin_convertvector(lat4[p], floatx4);
    const floatx4 v = step_v<GUIDE>(ns, counter, a4, aux1, sc, p, total, (int)(p / HW), halves, guidance, r.alpha_s, r.sigma_s, x);
    const floatx4 mt = r.alpha_s * x - r.sigma_s * v;
    floatx4 h0, h1, h2;
    if (rd0) h0 = H0[p];
    if (rd1) h1 = H1[p];
    if (rd2) h2 = H2[p];
    floatx4 xc = x;
    if (r.correct) {
      xc = r.cc_x * xl[p] + r.cc_m * mt;
      if (r.cc_0 != 0.f) xc += r.cc_0 * h0;
      if (r.cc_1 != 0.f) xc += r.cc_1 * h1;
      if (r.cc_2 != 0.f) xc += r.cc_2 * h2;
    }
    floatx4 out = r.pc_x * xc + r.pc_m * mt;
    if (r.pc_0 != 0.f) out += r.pc_0 * h0;
    if (r.pc_1 != 0.f) out += r.pc_1 * h1;
    lat4[p] = __builtin_convertvector(out, half4_t);
    xl[p] = xc;
    H0[p] = mt;
    if (rd0) H1[p] = h0;
    if (rd1) H2[p] = h1;
  }
}

// row: 12 host floats, (alpha_s, sigma_s, cc_x, cc_m, cc_0, cc_1, cc_2, pc_x, pc_m, pc_0, pc_1, corrector on: 0 or 1)
static int cfg_unipc_launch(void* latents, const void* noise_sum, const void* counter, void* state, int Ftot, int HW, int halves, float guidance,
                            const float* row, void* stream, const StepExtra& ex, const char* who) {
  MD_CHECK_ARG(row, "%s: null coefficient row", who);
  if (cfg_step_check(who, latents, noise_sum, counter, nullptr, ex, Ftot, HW, halves, 0.f,
                     {guidance, row[0], row[1], row[2], row[3], row[4], row[5], row[6], row[7], row[8], row[9], row[10]}))
    return MD_ERR_ARG;
  MD_CHECK_ARG(row[11] == 0.f || row[11] == 1.f, "%s: the corrector flag must be 0 or 1", who);
  MD_CHECK_ARG(state, "%s: null state", who);
  if (cfg_pixel_alignment_check(who, latents, noise_sum, state, nullptr, ex)) return MD_ERR_ARG;
  MD_CHECK_ARG(((uintptr_t)counter % 4) == 0, "%s: counter needs 4-byte alignment", who);
  MD_CHECK_ARG(ex.guide != GUIDE_APG || row[1] > 0.f, "%s: APG divides by sigma_s: it must be > 0", who);
  const UniPCRow r = {row[0], row[1], row[2], row[3], row[4], row[5], row[6], row[7], row[8], row[9], row[10], row[11] != 0.f};
  step_launch({cfg_unipc_kernel<GUIDE_PLAIN>, cfg_unipc_kernel<GUIDE_SCALED>, cfg_unipc_kernel<GUIDE_APG>, cfg_unipc_kernel<GUIDE_PAG>}, ex,
              (guidance - 1.f) / r.sigma_s, (long)Ftot * HW, stream, (half_t*)latents, (const float*)noise_sum, (const float*)counter,
              (float*)state, Ftot, HW, halves, guidance, r);
  MD_CHECK_LAUNCH(who);
  return MD_OK;
}

extern "C" int md_cfg_unipc_step(void* latents, const void* noise_sum, const void* counter, void* state, int Ftot, int HW, int halves, float guidance,
                                 const float* row, void* stream) {
  return cfg_unipc_launch(latents, noise_sum, counter, state, Ftot, HW, halves, guidance, row, stream, StepExtra(), "md_cfg_unipc_step");
}

extern "C" int md_cfg_unipc_step_scaled(void* latents, const void* noise_sum, const void* counter, void* state, const float* vscale, int Ftot, int HW,
                                        int halves, float guidance, const float* row, void* stream) {
  return cfg_unipc_launch(latents, noise_sum, counter, state, Ftot, HW, halves, guidance, row, stream, step_scaled(vscale),
                          "md_cfg_unipc_step_scaled");
}

extern "C" int md_cfg_unipc_step_apg(void* latents, const void* noise_sum, const void* counter, void* state, const void* momentum_buf,
                                     const float* coef, int Ftot, int HW, int halves, float guidance, const float* row, void* stream) {
  return cfg_unipc_launch(latents, noise_sum, counter, state, Ftot, HW, halves, guidance, row, stream, step_apg(momentum_buf, coef),
                          "md_cfg_unipc_step_apg");
}

extern "C" int md_cfg_unipc_step_pag(void* latents, const void* noise_sum, const void* counter, void* state, const void* perturbed_sum, int Ftot,
                                     int HW, int halves, float guidance, float pag_scale, const float* row, void* stream) {
  return cfg_unipc_launch(latents, noise_sum, counter, state, Ftot, HW, halves, guidance, row, stream, step_pag(perturbed_sum, pag_scale),
                          "md_cfg_unipc_step_pag");
}

// ---- the unconditional plane of a step that did not evaluate it (guidance_interval=, uncond_cache_interval=) ---------------------------
// A step that runs the conditional evaluation only leaves plane 0 (u) of the accumulator empty.  This kernel fills it so that every
// consumer of the planes (guided_v and with it both steps, the rescale, APG, PAG / SEG) works unchanged:
//   mode 0 (store, after a full step's windows):  delta = c_sum / cnt - u_sum / cnt, the guidance direction c - u as guided_v forms it
//   mode 1 (restore, after a conditional-only step's windows):  u_sum = c_sum - scale delta cnt, so that guided_v's c - u is scale delta
// Rounding order (fp32, no fma: fp contraction is switched off in the kernel body, every line below is rounded once, in this order, so every
// rank of a window-parallel run, which holds the same planes after the all-reduce, gets the same bits):
//   store:    inv = 1 / cnt;  u = u_sum inv;  c = c_sum inv;  delta = c - u            (inv, u, c exactly as guided_v writes them)
//   restore:  t = delta cnt;  t = scale t  (exact for scale == 1);  u_sum = c_sum - t
// scale == 0 (a step outside the guidance interval): the product is not formed and delta is not read; u_sum = c_sum bit for bit, so c - u
// is exactly 0 and the guided v is the conditional mean, whatever delta holds (it may be NULL).
// A frame whose counter is 0 gets no special case, as in the step kernels: guided_v forms inv = 1 / 0 = Inf and 0 * Inf = NaN for such a
// frame; here store writes the same NaN into delta, restore with scale != 0 hands it on (NaN * 0) and restore with scale == 0 copies the
// (zero) c_sum, which the step then turns into NaN itself.  The loop never produces such a frame: every frame lies in a window.
// Streaming, HBM-bound: one thread owns one pixel per round (16-byte loads and stores), grid-stride with the step kernels' grid cap.
// Every element is written by exactly one thread: deterministic, no atomics.
template <int MODE>
__global__ __launch_bounds__(256) void cfg_uncond_cache_kernel(floatx4* __restrict__ ns, const float* __restrict__ counter,
                                                               floatx4* __restrict__ delta, int Ftot, int HW, float scale) {
#pragma clang fp contract(off)
  const long total = (long)Ftot * HW;  // pixels
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
    const float cnt = counter[(int)(p / HW)];
    if constexpr (MODE == 0) {
      const float inv = 1.f / cnt;
      const floatx4 u = ns[p] * inv;
      const floatx4 c = ns[total + p] * inv;
      delta[p] = c - u;
    } else {
      floatx4 c = ns[total + p];
      if (scale != 0.f) {
        floatx4 t = delta[p] * cnt;
        t = scale * t;
        c = c - t;
      }
      ns[p] = c;
    }
  }
}

extern "C" int md_cfg_uncond_cache(void* noise_sum, const void* counter, void* delta, int Ftot, int HW, int mode, float scale, void* stream) {
  MD_CHECK_ARG(Ftot > 0 && HW > 0 && (mode == 0 || mode == 1), "md_cfg_uncond_cache: bad arguments (Ftot, HW > 0, mode 0 = store or 1 = restore)");
  MD_CHECK_ARG(__builtin_isfinite(scale), "md_cfg_uncond_cache: non-finite scale");
  MD_CHECK_ARG(noise_sum && counter && (delta || (mode == 1 && scale == 0.f)),
               "md_cfg_uncond_cache: null pointer (delta may be NULL for mode 1 with scale == 0 only)");
  MD_CHECK_ARG(((uintptr_t)noise_sum % 16) == 0 && ((uintptr_t)delta % 16) == 0 && ((uintptr_t)counter % 4) == 0,
               "md_cfg_uncond_cache: noise_sum / delta need 16-byte, counter 4-byte alignment");
  const long total = (long)Ftot * HW;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  if (mode == 0)
    hipLaunchKernelGGL(cfg_uncond_cache_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (floatx4*)noise_sum, (const float*)counter,
                       (floatx4*)delta, Ftot, HW, scale);
  else
    hipLaunchKernelGGL(cfg_uncond_cache_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (floatx4*)noise_sum, (const float*)counter,
                       (floatx4*)delta, Ftot, HW, scale);
  MD_CHECK_LAUNCH("md_cfg_uncond_cache");
  return MD_OK;
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

// ---- adaptive projected guidance: momentum update and per-frame coefficients (Sadat et al., arXiv 2410.02416, Algorithm 1) -------------
// On the data prediction, per frame fr over its HW 4 elements (one frame = one sample of the paper):
//   u, c as guided_v forms them;  D_c = a x - s c;  m = s (u - c) + beta m_prev        m: fp32, updated in place; beta == 0 never reads it
//   N2 = sum m^2, P = sum m D_c, Q = sum D_c^2                                        fp64
//   S = r == 0 || N2 == 0 ? 1 : min(1, r / sqrt(N2));  proj = Q == 0 ? 0 : P / Q;  coef[fr] = (S, (1 - eta) S proj)
// The discipline of md_cfg_guidance_rescale, per frame: apg_blocks_per_frame(HW) <= 16 workgroups per frame, each over a FIXED contiguous
// slice of that frame's pixels, reduce in fp64 through the fixed butterfly and a fixed wave order into workspace partials; ONE small launch
// of one wave per frame then adds that frame's partials in a fixed order and writes coef[fr].  No float atomics, no host sync.
#define APG_MAX_BPF 16

static int apg_blocks_per_frame(int HW) {
  const int b = (HW + RS_THREADS - 1) / RS_THREADS;
  return b < APG_MAX_BPF ? b : APG_MAX_BPF;
}

// part[fr * bpf + b] = (N2, P, Q) of workgroup b's slice of frame fr.  Grid: Ftot * bpf workgroups.
__global__ void __launch_bounds__(RS_THREADS) cfg_apg_partials_kernel(const half_t* __restrict__ lat, const float* __restrict__ noise_sum,
                                                                      const float* __restrict__ counter, float* __restrict__ mom,
                                                                      double* __restrict__ part, int Ftot, int HW, int bpf, int chunk, float a,
                                                                      float s, float beta) {
  // u and c are rounded before they are subtracted (no fma across u - c: contracted, fl(ns_u inv) - ns_c inv leaves the rounding error of one
  // product where u == c, and that frame's N2 would not be the exact 0 the S = 1 rule tests for)
#pragma clang fp contract(off)
  const long total = (long)Ftot * HW;
  const floatx4* ns = reinterpret_cast<const floatx4*>(noise_sum);
  const half4_t* lat4 = reinterpret_cast<const half4_t*>(lat);
  floatx4* mom4 = reinterpret_cast<floatx4*>(mom);
  const int fr = blockIdx.x / bpf, b = blockIdx.x - fr * bpf;
  const int p0 = b * chunk, p1 = min(p0 + chunk, HW);
  const float inv = 1.f / counter[fr];
  double acc[3] = {0.0, 0.0, 0.0};
  for (int q = p0 + threadIdx.x; q < p1; q += RS_THREADS) {
    const long p = (long)fr * HW + q;
    const floatx4 u = ns[p] * inv, c = ns[total + p] * inv;  // guided_v's u and c
    const floatx4 x = __builtin_convertvector(lat4[p], floatx4);
    const floatx4 dc = a * x - s * c;
    floatx4 m = s * (u - c);
    if (beta != 0.f) m += beta * mom4[p];
    mom4[p] = m;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double md = (double)m[e], dd = (double)dc[e];
      acc[0] += md * md;
      acc[1] += md * dd;
      acc[2] += dd * dd;
    }
  }
  __shared__ double red[RS_THREADS / 64][3];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    acc[q] = wave_sum_f64(acc[q]);
    if (lane == 0) red[wave][q] = acc[q];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    double t = 0.0;
    for (int w = 0; w < RS_THREADS / 64; ++w) t += red[w][threadIdx.x];
    part[(size_t)blockIdx.x * 3 + threadIdx.x] = t;
  }
}

// One wave per frame: lane l takes partial l of its frame (bpf <= 16 < 64), then the fixed butterfly; lane 0 writes (S, K).
__global__ void __launch_bounds__(64) cfg_apg_finalize_kernel(const double* __restrict__ part, int bpf, float eta, float r, float* __restrict__ coef) {
  const int fr = blockIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < bpf; b += 64)
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q] += part[((size_t)fr * bpf + b) * 3 + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) acc[q] = wave_sum_f64(acc[q]);
  if (threadIdx.x == 0) {
    const double N2 = acc[0], P = acc[1], Q = acc[2];
    double S = 1.0;
    if (r != 0.f && N2 != 0.0) {
      const double t = (double)r / sqrt(N2);
      S = t < 1.0 ? t : 1.0;
    }
    const double proj = Q == 0.0 ? 0.0 : P / Q;
    coef[2 * fr] = (float)S;
    coef[2 * fr + 1] = (float)((1.0 - (double)eta) * S * proj);
  }
}

extern "C" size_t md_cfg_apg_workspace_bytes(int Ftot, int HW) {
  return Ftot > 0 && HW > 0 ? (size_t)Ftot * apg_blocks_per_frame(HW) * 3 * sizeof(double) : 0;
}

extern "C" int md_cfg_apg_prepare(const void* latents, const void* noise_sum, const void* counter, void* momentum_buf, int Ftot, int HW, int halves,
                                  float alpha_s, float sigma_s, float momentum, float eta, float norm_threshold, void* workspace,
                                  size_t workspace_bytes, void* coef, void* stream) {
  MD_CHECK_ARG(Ftot > 0 && HW > 0 && halves == 2 && (long)Ftot * APG_MAX_BPF <= 0x7fffffffL, "md_cfg_apg_prepare: bad arguments (APG needs halves == 2)");
  MD_CHECK_ARG(latents && noise_sum && counter && momentum_buf && workspace && coef, "md_cfg_apg_prepare: null pointer");
  MD_CHECK_ARG(((uintptr_t)latents % 8) == 0 && ((uintptr_t)noise_sum % 16) == 0 && ((uintptr_t)momentum_buf % 16) == 0 &&
                   ((uintptr_t)workspace % 8) == 0 && ((uintptr_t)counter % 4) == 0 && ((uintptr_t)coef % 4) == 0,
               "md_cfg_apg_prepare: latents need 8-byte, noise_sum / momentum_buf 16-byte, workspace 8-byte, counter / coef 4-byte alignment");
  MD_CHECK_ARG(__builtin_isfinite(alpha_s) && __builtin_isfinite(sigma_s), "md_cfg_apg_prepare: non-finite coefficient");
  MD_CHECK_ARG(__builtin_isfinite(momentum) && momentum > -1.f && momentum < 1.f && __builtin_isfinite(eta) && eta >= 0.f && eta <= 1.f &&
                   __builtin_isfinite(norm_threshold) && norm_threshold >= 0.f,
               "md_cfg_apg_prepare: momentum must be finite in (-1, 1), eta in [0, 1], norm_threshold >= 0");
  MD_CHECK_ARG(workspace_bytes >= md_cfg_apg_workspace_bytes(Ftot, HW), "md_cfg_apg_prepare: workspace too small");
  const int bpf = apg_blocks_per_frame(HW);
  const int chunk = (HW + bpf - 1) / bpf;
  hipLaunchKernelGGL(cfg_apg_partials_kernel, dim3(Ftot * bpf), dim3(RS_THREADS), 0, (hipStream_t)stream, (const half_t*)latents,
                     (const float*)noise_sum, (const float*)counter, (float*)momentum_buf, (double*)workspace, Ftot, HW, bpf, chunk, alpha_s, sigma_s,
                     momentum);
  MD_CHECK_LAUNCH("md_cfg_apg_prepare");
  hipLaunchKernelGGL(cfg_apg_finalize_kernel, dim3(Ftot), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, bpf, eta, norm_threshold,
                     (float*)coef);
  MD_CHECK_LAUNCH("md_cfg_apg_prepare");
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
