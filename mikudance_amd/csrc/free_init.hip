// FreeInit noise re-initialisation (Wu et al., arXiv 2312.07537; diffusers FreeInitMixin): the 3-D frequency-domain mix of the re-noised
// sample with fresh noise, on the packed (F, H, W, 4) fp16 latents of the sampling loop.
//
//   out = fp16( z + IDFT3( lpf * DFT3( a x0 + b noise0 - z ) ) )          per channel, transforms over (F, H, W)
//
// which is diffusers' real(ifftn(ifftshift(fftshift(fftn(z_t)) LPF + fftshift(fftn(z)) (1 - LPF)))) for lpf = the symmetrised, unshifted
// table that mikudance_amd/free_init.py builds (the mix is linear; .real discards exactly the antisymmetric part of the table).
//
// A dense separable DFT, one axis per launch, in place on an fp32 complex workspace laid out like the latents ([F][H][W][4] float2):
//   W forward (forms a x0 + b noise0 - z on load) -> H forward -> F forward (times lpf / (F H W)) -> F inverse -> H inverse
//   -> W inverse (real part only, adds z, ONE rounding to fp16).
// Any length 1..256 per axis: no radix, n complex multiply-adds per output.  About 2 GFLOP at 16 x 96 x 96 and once per FreeInit iteration,
// so neither the matrix core nor an FFT is worth their index arithmetic here.
//
// Twiddles: one table of n entries per axis, (cos, sin)(2 pi m / n) from the double-precision sincospi rounded once to fp32, copied to LDS
// by every workgroup and indexed by (j k) mod n kept as a running integer -- j k / n is never formed in floating point.
// Every output is the sum of four interleaved partial sums (j mod 4), in a fixed order: two calls give the same bits.
//
// Coalescing: a line along W is contiguous.  Lines along H and F are strided, so a workgroup takes P adjacent pixels (P x 32 bytes of
// complex fp32, P >= 4: whole 128-byte segments) and all n positions of their lines; lanes run over (pixel, channel) fastest.
#include "common.h"

#define FI_MAX 256       // longest supported axis
#define FI_THREADS 256
#define FI_TW_BYTES ((size_t)3 * FI_MAX * sizeof(float2))

// lines per workgroup: the largest power of two with n * P <= 1024 (32 KiB of LDS for the lines), between 4 and 64
static inline int fi_tile(int n) {
  int p = 64;
  while (p > 4 && n * p > 1024) p >>= 1;
  return p;
}

__global__ void __launch_bounds__(FI_THREADS) fi_twiddle_kernel(float2* __restrict__ tw, int nF, int nH, int nW) {
  const int n = blockIdx.x == 0 ? nF : blockIdx.x == 1 ? nH : nW;
  for (int m = threadIdx.x; m < n; m += FI_THREADS) {
    double s, c;
    sincospi(2.0 * (double)m / (double)n, &s, &c);
    tw[blockIdx.x * FI_MAX + m] = make_float2((float)c, (float)s);
  }
}

// table -> LDS with the sine signed for the direction: forward e^{-i t} = (c, -s), inverse (c, +s)
__device__ __forceinline__ void fi_load_table(float2* __restrict__ twl, const float2* __restrict__ tw, int n, float sgn) {
  for (int m = threadIdx.x; m < n; m += FI_THREADS) {
    const float2 t = tw[m];
    twl[m] = make_float2(t.x, sgn * t.y);
  }
}

// acc += x * t (complex)
__device__ __forceinline__ void fi_cmac(float2& acc, const float2 x, const float2 t) {
  acc.x = fmaf(x.x, t.x, acc.x);
  acc.x = fmaf(-x.y, t.y, acc.x);
  acc.y = fmaf(x.y, t.x, acc.y);
  acc.y = fmaf(x.x, t.y, acc.y);
}

__device__ __forceinline__ int fi_next(int idx, int k, int n) {
  idx += k;
  return idx >= n ? idx - n : idx;
}

// sum_j x[j * stride] * twl[(j k) mod n]: four partial sums over j mod 4, combined (0 + 1) + (2 + 3)
__device__ __forceinline__ float2 fi_line_dft(const float2* __restrict__ x, int stride, const float2* __restrict__ twl, int k, int n) {
  float2 s0 = make_float2(0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
  int idx = 0, j = 0;
  for (; j + 4 <= n; j += 4) {
    fi_cmac(s0, x[(size_t)j * stride], twl[idx]);
    idx = fi_next(idx, k, n);
    fi_cmac(s1, x[(size_t)(j + 1) * stride], twl[idx]);
    idx = fi_next(idx, k, n);
    fi_cmac(s2, x[(size_t)(j + 2) * stride], twl[idx]);
    idx = fi_next(idx, k, n);
    fi_cmac(s3, x[(size_t)(j + 3) * stride], twl[idx]);
    idx = fi_next(idx, k, n);
  }
  if (j < n) {
    fi_cmac(s0, x[(size_t)j * stride], twl[idx]);
    idx = fi_next(idx, k, n);
  }
  if (j + 1 < n) {
    fi_cmac(s1, x[(size_t)(j + 1) * stride], twl[idx]);
    idx = fi_next(idx, k, n);
  }
  if (j + 2 < n) fi_cmac(s2, x[(size_t)(j + 2) * stride], twl[idx]);
  return make_float2((s0.x + s1.x) + (s2.x + s3.x), (s0.y + s1.y) + (s2.y + s3.y));
}

// ---- W forward: rows [r0, r0 + P) of the R = F * H rows; d = a x0 + b noise0 - z formed on load (a == 0 never reads x0) ------------------
// LDS: d as float2 (imaginary part 0) [P][n][4], then the table.  Outputs in memory order (row, k, channel): contiguous stores.
__global__ void __launch_bounds__(FI_THREADS) fi_rows_forward_kernel(const half_t* __restrict__ x0, const half_t* __restrict__ noise0,
                                                                     const half_t* __restrict__ z, float2* __restrict__ buf,
                                                                     const float2* __restrict__ tw, int R, int n, int P, float a, float b) {
  extern __shared__ float4 fi_smem[];
  float2* lds = reinterpret_cast<float2*>(fi_smem);
  float2* twl = lds + (size_t)P * n * 4;
  const int r0 = blockIdx.x * P;
  const int rows = min(P, R - r0);
  const int count = rows * n * 4;                                   // <= 64 * 1024 / 64 * 4 = 4096
  const size_t base = (size_t)r0 * n * 4;
  fi_load_table(twl, tw, n, -1.f);
  for (int e = threadIdx.x; e < count; e += FI_THREADS) {
    const float zz = (float)z[base + e];
    const float nn = b * (float)noise0[base + e];
    const float d = a != 0.f ? a * (float)x0[base + e] + nn - zz : nn - zz;
    lds[e] = make_float2(d, 0.f);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < count; e += FI_THREADS) {
    const int c = e & 3, k = (e >> 2) % n, p = (e >> 2) / n;
    buf[base + e] = fi_line_dft(lds + (size_t)p * n * 4 + c, 4, twl, k, n);
  }
}

// ---- W inverse: real part only, + z, one rounding, fp16 store -----------------------------------------------------------------------------
__global__ void __launch_bounds__(FI_THREADS) fi_rows_inverse_kernel(const float2* __restrict__ buf, const half_t* __restrict__ z,
                                                                     half_t* __restrict__ out, const float2* __restrict__ tw, int R, int n,
                                                                     int P) {
  extern __shared__ float4 fi_smem[];
  float2* lds = reinterpret_cast<float2*>(fi_smem);
  float2* twl = lds + (size_t)P * n * 4;
  const int r0 = blockIdx.x * P;
  const int rows = min(P, R - r0);
  const int count = rows * n * 4;
  const size_t base = (size_t)r0 * n * 4;
  fi_load_table(twl, tw, n, 1.f);
  for (int e = threadIdx.x; e < count; e += FI_THREADS) lds[e] = buf[base + e];
  __syncthreads();
  for (int e = threadIdx.x; e < count; e += FI_THREADS) {
    const int c = e & 3, k = (e >> 2) % n, p = (e >> 2) / n;
    const float2 v = fi_line_dft(lds + (size_t)p * n * 4 + c, 4, twl, k, n);
    out[base + e] = (half_t)((float)z[base + e] + v.x);
  }
}

// ---- a strided axis (H or F), in place: line (o, i) = buf[((o n + j) I + i)][4], j < n; the workgroup owns pixels i0 .. i0 + P - 1 of
// outer index o = blockIdx.y.  LDS [n][P][4] float2, lanes over (pixel, channel) fastest: P * 32 contiguous bytes per position, and a
// wave shares at most 64 / (4 P) ... 16 twiddle addresses.  scale != NULL: output (k, pixel) is multiplied by scale[(o n + k) I + i] * gain.
__global__ void __launch_bounds__(FI_THREADS) fi_axis_kernel(float2* __restrict__ buf, const float2* __restrict__ tw,
                                                             const float* __restrict__ scale, float gain, int I, int n, int P, int logP,
                                                             float sgn) {
  extern __shared__ float4 fi_smem[];
  float2* lds = reinterpret_cast<float2*>(fi_smem);
  float2* twl = lds + (size_t)P * n * 4;
  const int i0 = blockIdx.x * P;
  const size_t obase = (size_t)blockIdx.y * n * I;
  const int count = n * P * 4;                                      // <= 4096
  fi_load_table(twl, tw, n, sgn);
  for (int e = threadIdx.x; e < count; e += FI_THREADS) {
    const int c = e & 3, p = (e >> 2) & (P - 1), j = e >> (2 + logP);
    lds[e] = i0 + p < I ? buf[(obase + (size_t)j * I + i0 + p) * 4 + c] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < count; e += FI_THREADS) {
    const int c = e & 3, p = (e >> 2) & (P - 1), k = e >> (2 + logP);
    if (i0 + p >= I) continue;
    float2 v = fi_line_dft(lds + p * 4 + c, P * 4, twl, k, n);
    const size_t g = obase + (size_t)k * I + i0 + p;
    if (scale) {
      const float s = scale[g] * gain;
      v.x *= s;
      v.y *= s;
    }
    buf[g * 4 + c] = v;
  }
}

extern "C" int md_free_init_plan(int F, int H, int W) {
  return F >= 1 && F <= FI_MAX && H >= 1 && H <= FI_MAX && W >= 1 && W <= FI_MAX ? 1 : 0;
}

extern "C" size_t md_free_init_workspace_bytes(int F, int H, int W) {
  return md_free_init_plan(F, H, W) ? FI_TW_BYTES + (size_t)F * H * W * 4 * sizeof(float2) : 0;
}

static inline int fi_log2(int p) {
  int l = 0;
  while ((1 << l) < p) ++l;
  return l;
}

extern "C" int md_free_init_mix_f16(void* out, const void* x0, const void* noise0, const void* z, const float* lpf, int F, int H, int W,
                                    float a, float b, void* workspace, size_t workspace_bytes, void* stream) {
  MD_CHECK_ARG(out && x0 && noise0 && z && lpf && workspace, "md_free_init_mix_f16: null pointer");
  MD_CHECK_ARG(md_free_init_plan(F, H, W), "md_free_init_mix_f16: no kernel for F=%d H=%d W=%d (every axis must be 1..%d)", F, H, W, FI_MAX);
  MD_CHECK_ARG(((uintptr_t)out % 8) == 0 && ((uintptr_t)x0 % 8) == 0 && ((uintptr_t)noise0 % 8) == 0 && ((uintptr_t)z % 8) == 0 &&
                   ((uintptr_t)lpf % 4) == 0 && ((uintptr_t)workspace % 16) == 0,
               "md_free_init_mix_f16: out / x0 / noise0 / z need 8-byte, lpf 4-byte, workspace 16-byte alignment");
  MD_CHECK_ARG(__builtin_isfinite(a) && __builtin_isfinite(b) && a >= 0.f && b >= 0.f, "md_free_init_mix_f16: a and b must be finite and >= 0");
  MD_CHECK_ARG(workspace_bytes >= md_free_init_workspace_bytes(F, H, W), "md_free_init_mix_f16: workspace too small (%zu < %zu bytes)",
               workspace_bytes, md_free_init_workspace_bytes(F, H, W));
  hipStream_t st = (hipStream_t)stream;
  float2* tw = (float2*)workspace;
  float2* buf = (float2*)((char*)workspace + FI_TW_BYTES);
  const float2 *twF = tw, *twH = tw + FI_MAX, *twW = tw + 2 * FI_MAX;
  const float gain = (float)(1.0 / ((double)F * H * W));
  const int R = F * H, HW = H * W;
  const int pW = fi_tile(W), pH = fi_tile(H), pF = fi_tile(F);
  auto lds = [](int n, int p) { return (size_t)(n * p * 4 + n) * sizeof(float2); };      // <= 32 KiB + 2 KiB
  hipLaunchKernelGGL(fi_twiddle_kernel, dim3(3), dim3(FI_THREADS), 0, st, tw, F, H, W);
  MD_CHECK_LAUNCH("md_free_init_mix_f16");
  hipLaunchKernelGGL(fi_rows_forward_kernel, dim3(cdiv(R, pW)), dim3(FI_THREADS), lds(W, pW), st, (const half_t*)x0, (const half_t*)noise0,
                     (const half_t*)z, buf, twW, R, W, pW, a, b);
  MD_CHECK_LAUNCH("md_free_init_mix_f16");
  hipLaunchKernelGGL(fi_axis_kernel, dim3(cdiv(W, pH), F), dim3(FI_THREADS), lds(H, pH), st, buf, twH, (const float*)nullptr, 1.f, W, H, pH,
                     fi_log2(pH), -1.f);
  MD_CHECK_LAUNCH("md_free_init_mix_f16");
  hipLaunchKernelGGL(fi_axis_kernel, dim3(cdiv(HW, pF), 1), dim3(FI_THREADS), lds(F, pF), st, buf, twF, lpf, gain, HW, F, pF, fi_log2(pF), -1.f);
  MD_CHECK_LAUNCH("md_free_init_mix_f16");
  hipLaunchKernelGGL(fi_axis_kernel, dim3(cdiv(HW, pF), 1), dim3(FI_THREADS), lds(F, pF), st, buf, twF, (const float*)nullptr, 1.f, HW, F, pF,
                     fi_log2(pF), 1.f);
  MD_CHECK_LAUNCH("md_free_init_mix_f16");
  hipLaunchKernelGGL(fi_axis_kernel, dim3(cdiv(W, pH), F), dim3(FI_THREADS), lds(H, pH), st, buf, twH, (const float*)nullptr, 1.f, W, H, pH,
                     fi_log2(pH), 1.f);
  MD_CHECK_LAUNCH("md_free_init_mix_f16");
  hipLaunchKernelGGL(fi_rows_inverse_kernel, dim3(cdiv(R, pW)), dim3(FI_THREADS), lds(W, pW), st, buf, (const half_t*)z, (half_t*)out, twW, R, W,
                     pW);
  MD_CHECK_LAUNCH("md_free_init_mix_f16");
  return MD_OK;
}
