// Query blur of smoothed-energy guidance (SEG, Hong, arXiv 2408.00760): the token matrix of B frames is filtered along the two axes of its
// Hh x Ww grid, every channel on its own.
//
//   x [B * Hh * Ww][C] fp16, the tokens of B frames (row = (b * Hh + y) * Ww + x, the layout of md_token_pool_f16); y the same shape.
//   md_token_blur_f16: separable Gaussian with reflect padding (the official gaussian_blur_2d, per axis): kx taps wx along x, ky taps wy
//                      along y, fp32 tables made by the host; tap j of output position p reads position reflect(p + j - k / 2),
//                      reflect(i) = -i below 0 and 2 (n - 1) - i from n on (torch "reflect": the edge is not repeated).
//   md_token_mean_f16: sigma = infinity, the reference's inf_blur: every token of frame b becomes the frame's per-channel mean.
//
// Blur = two launches of one kernel: x -> fp32 workspace along the grid's x axis, workspace -> y along its y axis, so what passes between the
// axes is never rounded to fp16.  A workgroup owns ONE line (the n positions of one grid row or column) of up to 64 channels: the line goes
// through LDS as fp32 (each input element leaves HBM once per pass, not k times), lanes run over the channels fastest with 16-byte
// (fp16) / 2 x 16-byte (fp32) loads and stores of eight channels, and every lane then forms FOUR consecutive output positions of its eight
// channels from a sliding window of k + 3 LDS reads, so an LDS read feeds up to 32 FMAs; the taps are wave-uniform reads of the table.  Each output
// adds its taps in ascending tap order into an fp32 accumulator that starts at -0 (a one-tap filter, weight 1, returns x bit for bit, -0 too);
// one rounding to fp16 at the end of the second pass.
// Mean = two launches: per-slice partial sums in a fixed order (lanes over fixed token subsets, then the 32 position slots of the workgroup
// in ascending order through LDS) into the workspace, then every output workgroup adds the slices in ascending order, multiplies by
// fp32(1 / L), rounds once and writes its rows.  No atomics anywhere: the same inputs give the same bits.
#include "common.h"

#define TB_CH 8                                    // channel groups (of eight channels) per workgroup: 64 channels, 128 B of fp16 per position
#define TB_P 4                                     // consecutive output positions per lane
#define TB_ROW (TB_CH * 8 + 8)                     // floats per LDS row: 64 channels + 32 B of pad, so position slots 4 rows apart miss each other's banks
#define TB_MAX_N 224                               // longest line: TB_MAX_N * TB_ROW * 4 = 64,512 B of LDS
#define TB_MEAN_SLICES 32                          // token slices per frame of the mean's first launch (fewer for short frames)

__device__ __forceinline__ void tb_load8(const half_t* p, float* v) {
  const half8_t h = *reinterpret_cast<const half8_t*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (float)h[j];
}
__device__ __forceinline__ void tb_load8(const float* p, float* v) {
  const floatx4 a = *reinterpret_cast<const floatx4*>(p), b = *reinterpret_cast<const floatx4*>(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
}
__device__ __forceinline__ void tb_store8(half_t* p, const float* v) {
  half8_t h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (half_t)v[j];
  *reinterpret_cast<half8_t*>(p) = h;
}
__device__ __forceinline__ void tb_store8(float* p, const float* v) {
  floatx4 a, b;
#pragma unroll
  for (int j = 0; j < 4; ++j) { a[j] = v[j]; b[j] = v[4 + j]; }
  *reinterpret_cast<floatx4*>(p) = a;
  *reinterpret_cast<floatx4*>(p + 4) = b;
}

// A position's 64 channels in LDS: the first four channels of every lane (16 B each, 128 B), then the second four.  One ds_read_b128 of a wave
// then covers 128 consecutive bytes per position slot, and with rows of 288 B the slots of a lane group (4 rows apart) fall on different banks.
__device__ __forceinline__ void tb_lds_load8(const float* p, float* v) {
  const floatx4 a = *reinterpret_cast<const floatx4*>(p), b = *reinterpret_cast<const floatx4*>(p + TB_CH * 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { v[j] = a[j]; v[4 + j] = b[j]; }
}
__device__ __forceinline__ void tb_lds_store8(float* p, const float* v) {
  floatx4 a, b;
#pragma unroll
  for (int j = 0; j < 4; ++j) { a[j] = v[j]; b[j] = v[4 + j]; }
  *reinterpret_cast<floatx4*>(p) = a;
  *reinterpret_cast<floatx4*>(p + TB_CH * 4) = b;
}

// One axis pass.  Line `line` = (outer, inner) = (line / inner_n, line % inner_n) starts at element outer * outer_stride + inner * inner_stride;
// its n positions are pos_stride elements apart; all strides in elements, multiples of 8.  Along x: inner_n = 1 (outer = b * Hh + y);
// along y: inner_n = Ww (outer = b, inner = x).  blockIdx.x = line * chunks + chunk, a chunk = TB_CH channel groups; C8 = C / 8.
// blockDim.x = TB_CH * slots; lane (slot, cl) = (threadIdx.x / TB_CH, threadIdx.x % TB_CH).
template <typename TIn, typename TOut>
__global__ void __launch_bounds__(256) token_blur_axis_kernel(const TIn* __restrict__ in, TOut* __restrict__ out, const float* __restrict__ w,
                                                             int k, int n, int inner_n, long outer_stride, long inner_stride, long pos_stride,
                                                             int C8, int chunks) {
  extern __shared__ __attribute__((aligned(16))) float tb_line[];                 // [n][TB_ROW]
  const int slots = blockDim.x / TB_CH;
  const int cl = threadIdx.x % TB_CH, slot = threadIdx.x / TB_CH;
  const long line = blockIdx.x / chunks;
  const int c8 = (blockIdx.x % chunks) * TB_CH + cl;
  const bool live = c8 < C8;                                                      // the last chunk of a C that is no multiple of 64
  const long base = (line / inner_n) * outer_stride + (line % inner_n) * inner_stride + (long)c8 * 8;
  if (live) {
    for (int p = slot; p < n; p += slots) {
      float v[8];
      tb_load8(in + base + p * pos_stride, v);
      tb_lds_store8(tb_line + p * TB_ROW + cl * 4, v);
    }
  }
  __syncthreads();
  if (!live) return;
  const int r = k >> 1;
  for (int p0 = slot * TB_P; p0 < n; p0 += slots * TB_P) {
    float acc[TB_P][8];
#pragma unroll
    for (int i = 0; i < TB_P; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = -0.0f;
    // window step tt reads position p0 - r + tt; it is tap tt - i of output p0 + i
    for (int tt = 0; tt < k + TB_P - 1; ++tt) {
      int t = p0 - r + tt;
      t = t < 0 ? -t : t;
      t = t >= n ? 2 * (n - 1) - t : t;
      // outputs p0 + i >= n of the last group are computed and dropped: their window may leave the reflected range, keep it inside the line
      t = t < 0 ? 0 : (t >= n ? n - 1 : t);
      float v[8];
      tb_lds_load8(tb_line + t * TB_ROW + cl * 4, v);
#pragma unroll
      for (int i = 0; i < TB_P; ++i) {
        const int j = tt - i;                                                     // the same in every lane: a scalar branch and a scalar tap
        if (j >= 0 && j < k) {
          const float wj = w[j];
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[i][c] = fmaf(wj, v[c], acc[i][c]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < TB_P; ++i)
      if (p0 + i < n) tb_store8(out + base + (p0 + i) * pos_stride, acc[i]);
  }
}

// Mean, first launch: blockIdx.x = (b * slices + s) * chunks + chunk; slice s owns tokens [s * per, min(L, (s + 1) * per)).
// part[(b * slices + s) * C + c] = the slice's fp32 sum.  256 threads = 32 slots x TB_CH.
__global__ void __launch_bounds__(256) token_mean_partial_kernel(const half_t* __restrict__ x, float* __restrict__ part, int L, int C8, int chunks,
                                                                int slices, int per) {
  __shared__ __attribute__((aligned(16))) float red[32][TB_CH * 8];
  const int cl = threadIdx.x % TB_CH, slot = threadIdx.x / TB_CH;
  const int chunk = blockIdx.x % chunks;
  const long bs = blockIdx.x / chunks;                                            // b * slices + s
  const int s = (int)(bs % slices);
  const long b = bs / slices;
  const int c8 = chunk * TB_CH + cl;
  const bool live = c8 < C8;
  const long C = (long)C8 * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    const int end = min(L, (s + 1) * per);
    for (int t = s * per + slot; t < end; t += 32) {
      float v[8];
      tb_load8(x + (b * L + t) * C + (long)c8 * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
  }
  tb_store8(&red[slot][cl * 8], acc);
  __syncthreads();
  if (slot == 0 && live) {
    for (int q = 1; q < 32; ++q) {
      float v[8];
      tb_load8(&red[q][cl * 8], v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
    tb_store8(part + bs * C + (long)c8 * 8, acc);
  }
}

// Mean, second launch: the same grid; every workgroup adds the frame's slices in ascending order and writes its own slice of token rows.
__global__ void __launch_bounds__(256) token_mean_write_kernel(const float* __restrict__ part, half_t* __restrict__ y, int L, int C8, int chunks,
                                                              int slices, int per, float inv) {
  const int cl = threadIdx.x % TB_CH, slot = threadIdx.x / TB_CH;
  const int chunk = blockIdx.x % chunks;
  const long bs = blockIdx.x / chunks;
  const int s = (int)(bs % slices);
  const long b = bs / slices;
  const int c8 = chunk * TB_CH + cl;
  if (c8 >= C8) return;
  const long C = (long)C8 * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int q = 0; q < slices; ++q) {
    float v[8];
    tb_load8(part + (b * slices + q) * C + (long)c8 * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += v[j];
  }
  half8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (half_t)(acc[j] * inv);
  const int end = min(L, (s + 1) * per);
  for (int t = s * per + slot; t < end; t += 32) *reinterpret_cast<half8_t*>(y + (b * L + t) * C + (long)c8 * 8) = o;
}

static inline int tb_mean_slices(long L) { return (int)(L < 32 * TB_MEAN_SLICES ? (L + 31) / 32 : TB_MEAN_SLICES); }

extern "C" size_t md_token_blur_workspace_bytes(int B, int Hh, int Ww, int C) {
  if (B <= 0 || Hh <= 0 || Ww <= 0 || C <= 0) return 0;
  const size_t L = (size_t)Hh * Ww;
  const size_t blur = (size_t)B * L * C * 4, mean = (size_t)B * tb_mean_slices((long)L) * C * 4;
  return blur > mean ? blur : mean;
}

static int tb_check(const char* who, const void* x, const void* y, long B, long L, int C, const void* workspace) {
  MD_CHECK_ARG(x && y && workspace, "%s: NULL pointer", who);
  MD_CHECK_ARG(((uintptr_t)x % 16) == 0 && ((uintptr_t)y % 16) == 0 && ((uintptr_t)workspace % 16) == 0,
               "%s: x / y / workspace need 16-byte alignment", who);
  MD_CHECK_ARG(B > 0 && L > 0 && C > 0 && C % 8 == 0, "%s: sizes must be positive and C a multiple of 8 (C=%d)", who, C);
  MD_CHECK_ARG(B * L <= (1L << 38) / C, "%s: problem too large", who);
  const uintptr_t bytes = (uintptr_t)(B * L * C * 2);
  const uintptr_t xb = (uintptr_t)x, yb = (uintptr_t)y, wb = (uintptr_t)workspace;
  MD_CHECK_ARG(xb + bytes <= yb || yb + bytes <= xb, "%s: x and y overlap", who);
  MD_CHECK_ARG(wb + 2 * bytes <= xb || xb + bytes <= wb, "%s: the workspace overlaps x", who);
  MD_CHECK_ARG(wb + 2 * bytes <= yb || yb + bytes <= wb, "%s: the workspace overlaps y", who);
  return MD_OK;
}

extern "C" int md_token_blur_f16(const void* x, void* y, int B, int Hh, int Ww, int C, const float* wy, int ky, const float* wx, int kx,
                                 void* workspace, void* stream) {
  MD_CHECK_ARG(Hh > 0 && Ww > 0, "md_token_blur_f16: the grid must be positive, got %d x %d", Hh, Ww);
  if (int e = tb_check("md_token_blur_f16", x, y, B, (long)Hh * Ww, C, workspace)) return e;
  MD_CHECK_ARG(wy && wx, "md_token_blur_f16: NULL tap table");
  MD_CHECK_ARG(ky >= 1 && ky % 2 == 1 && ky <= Hh + 1, "md_token_blur_f16: ky must be odd and in 1..Hh + 1, got %d for Hh=%d", ky, Hh);
  MD_CHECK_ARG(kx >= 1 && kx % 2 == 1 && kx <= Ww + 1, "md_token_blur_f16: kx must be odd and in 1..Ww + 1, got %d for Ww=%d", kx, Ww);
  MD_CHECK_ARG(Hh <= TB_MAX_N && Ww <= TB_MAX_N, "md_token_blur_f16: a grid axis is limited to %d tokens, got %d x %d", TB_MAX_N, Hh, Ww);
  const int C8 = C / 8, chunks = (C8 + TB_CH - 1) / TB_CH;
  const long lines_x = (long)B * Hh, lines_y = (long)B * Ww;
  MD_CHECK_ARG(lines_x * chunks < (1L << 31) && lines_y * chunks < (1L << 31), "md_token_blur_f16: problem too large");
  // position slots of a workgroup: enough for the groups of TB_P outputs of one line, whole waves, at most 256 threads
  auto slots = [](int n) { const int g = (n + TB_P - 1) / TB_P; return g >= 32 ? 32 : (g + 7) / 8 * 8; };
  const long row = (long)Ww * C;
  hipLaunchKernelGGL((token_blur_axis_kernel<half_t, float>), dim3((unsigned)(lines_x * chunks)), dim3(TB_CH * slots(Ww)),
                     (size_t)Ww * TB_ROW * 4, (hipStream_t)stream, (const half_t*)x, (float*)workspace, wx, kx, Ww, 1, row, 0L, (long)C, C8, chunks);
  hipLaunchKernelGGL((token_blur_axis_kernel<float, half_t>), dim3((unsigned)(lines_y * chunks)), dim3(TB_CH * slots(Hh)),
                     (size_t)Hh * TB_ROW * 4, (hipStream_t)stream, (const float*)workspace, (half_t*)y, wy, ky, Hh, Ww, (long)Hh * row, (long)C, row,
                     C8, chunks);
  MD_CHECK_LAUNCH("md_token_blur_f16");
  return MD_OK;
}

extern "C" int md_token_mean_f16(const void* x, void* y, int B, int L, int C, void* workspace, void* stream) {
  if (int e = tb_check("md_token_mean_f16", x, y, B, L, C, workspace)) return e;
  const int C8 = C / 8, chunks = (C8 + TB_CH - 1) / TB_CH;
  const int slices = tb_mean_slices(L), per = (L + slices - 1) / slices;
  const long blocks = (long)B * slices * chunks;
  MD_CHECK_ARG(blocks < (1L << 31), "md_token_mean_f16: problem too large");
  hipLaunchKernelGGL(token_mean_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (float*)workspace, L,
                     C8, chunks, slices, per);
  hipLaunchKernelGGL(token_mean_write_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, (half_t*)y, L,
                     C8, chunks, slices, per, 1.0f / (float)L);
  MD_CHECK_LAUNCH("md_token_mean_f16");
  return MD_OK;
}
