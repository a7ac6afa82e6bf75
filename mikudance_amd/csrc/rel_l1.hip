// The distance of adaptive DeepCache (forward_nhwc(deep_cache=slot.auto(...))): how far skip d - 1 of this step lies from the one of the step
// before, the relative-L1 criterion of TeaCache (arXiv 2411.19108) / first-block cache on the tensor a shallow step computes anyway.
//
//   a, b  fp16, rows x C each, row r of a at a + r lda, of b at b + r ldb (elements): channel slices of wider concat buffers, lda, ldb >= C
//   out   2 fp32 on the device: out[0] = sum |a - b|, out[1] = sum |b|, every term formed and added in fp32
//
// Two launches, no atomics, nothing read that this call has not written:
//   1. rel_l1_partial_kernel: P = min(ceil(units / 256), 2048) workgroups of 256 threads, a function of the shape alone.  A unit is eight
//      consecutive channels of one row (two 16-byte loads) where C, lda, ldb are multiples of 8 and a, b are 16-byte aligned ("vector path"),
//      one element otherwise ("scalar path"); unit i belongs to thread i mod (256 P) and a thread takes its units in ascending order.
//      One partial (sum |a - b|, sum |b|) per workgroup goes to workspace[block] with one 8-byte vector store.
//   2. rel_l1_final_kernel: one workgroup of 256 threads adds the P partials and writes out with one 8-byte vector store.
//
// THE SUMMATION ORDER (tests/test_rel_l1_gpu.py computes its bound from it).  Every term is >= 0, so the relative error of a sum is at most
// depth 2^-24 to first order, depth = the largest number of inexact fp32 additions a term passes through:
//   vector path only: the 8 terms of a unit are added in channel order into a fresh accumulator                        7
//   a thread adds its units (scalar path: its terms) in ascending order, iters = ceil(units / (256 P)) of them      iters
//   the 64 lanes of a wave: xor butterfly, offsets 32, 16, ..., 1 (every lane ends with the same bits)                6
//   thread 0 adds the 4 wave sums in wave order                                                                       3
//   final launch: thread t adds partials t, t + 256, ... in ascending order                                     ceil(P / 256)
//   the same butterfly and the same 4-wave sum                                                                      6 + 3
//   depth = (vector ? 7 : 0) + iters + ceil(P / 256) + 18
// (an addition to the initial 0 is exact and counted all the same: the bound errs on the wide side by at most 3).  |a - b| itself is one fp32
// subtraction of two exactly converted fp16 values: one more rounding per term.  NaN and Inf are ordinary operands of these additions: a NaN
// in a or b, or Inf - Inf, reaches out as NaN, an Inf as Inf (or NaN).
//
// HBM-bound: 4 rows C bytes read, 16 KiB written.  Lanes run over the channels of a row fastest, so a wave reads 1 KiB runs of each operand;
// 2048 workgroups are 8 per CU, the loop is unrolled so that a thread has 8 loads in flight.  Same inputs, same bits, whatever ran before:
// the grid, the unit-to-thread map and every order above depend on (rows, C, path) only.
#include "common.h"
#include "rel_l1.h"

#define RL_THREADS 256
#define RL_MAX_BLOCKS 2048

typedef float float2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float2_t rl_block_sum(float sd, float sb) {
  __shared__ float2_t waves[RL_THREADS / 64];
  sd = wave_sum(sd);
  sb = wave_sum(sb);
  if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = float2_t{sd, sb};
  __syncthreads();
  float2_t r = waves[0];
#pragma unroll
  for (int w = 1; w < RL_THREADS / 64; ++w) r += waves[w];
  return r;                                                        // (every thread holds it; thread 0 stores it)
}

template <bool VEC>
__global__ void __launch_bounds__(RL_THREADS) rel_l1_partial_kernel(const half_t* __restrict__ a, long lda, const half_t* __restrict__ b, long ldb,
                                                                     long units, int per_row, float2_t* __restrict__ partial) {
  float sd = 0.f, sb = 0.f;
#pragma unroll 4
  for (long i = (long)blockIdx.x * RL_THREADS + threadIdx.x; i < units; i += (long)gridDim.x * RL_THREADS) {
    const long row = i / per_row;                                  // < rows
    const long c = i - row * per_row;                              // < per_row: the unit's last channel is < C <= lda, ldb
    if (VEC) {
      const half8_t va = *reinterpret_cast<const half8_t*>(a + row * lda + c * 8);
      const half8_t vb = *reinterpret_cast<const half8_t*>(b + row * ldb + c * 8);
      float td = 0.f, tb = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float fa = (float)va[j], fb = (float)vb[j];
        td += fabsf(fa - fb);
        tb += fabsf(fb);
      }
      sd += td;
      sb += tb;
    } else {
      const float fa = (float)a[row * lda + c], fb = (float)b[row * ldb + c];
      sd += fabsf(fa - fb);
      sb += fabsf(fb);
    }
  }
  const float2_t r = rl_block_sum(sd, sb);
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ void __launch_bounds__(RL_THREADS) rel_l1_final_kernel(const float2_t* __restrict__ partial, int P, float2_t* __restrict__ out) {
  float sd = 0.f, sb = 0.f;
  for (int i = threadIdx.x; i < P; i += RL_THREADS) {
    const float2_t p = partial[i];
    sd += p.x;
    sb += p.y;
  }
  const float2_t r = rl_block_sum(sd, sb);
  if (threadIdx.x == 0) out[0] = r;
}

static inline bool rl_vector_path(const void* a, int lda, const void* b, int ldb, int C) {
  return C % 8 == 0 && lda % 8 == 0 && ldb % 8 == 0 && ((uintptr_t)a % 16) == 0 && ((uintptr_t)b % 16) == 0;
}

static inline long rl_blocks(long units) {
  const long blocks = (units + RL_THREADS - 1) / RL_THREADS;
  return blocks < RL_MAX_BLOCKS ? blocks : RL_MAX_BLOCKS;
}

// One 8-byte partial per workgroup of the first launch.  The scalar path has the most units, so its count covers both paths.
extern "C" size_t md_rel_l1_workspace_bytes(int rows, int C) {
  if (rows <= 0 || C <= 0) return 0;
  return (size_t)rl_blocks((long)rows * C) * sizeof(float2_t);
}

extern "C" int md_rel_l1_f16(const void* a, int lda, const void* b, int ldb, int rows, int C, void* workspace, size_t workspace_bytes, void* out,
                             void* stream) {
  MD_CHECK_ARG(a && b && workspace && out, "md_rel_l1_f16: NULL pointer");
  MD_CHECK_ARG(rows > 0 && C > 0, "md_rel_l1_f16: rows and C must be positive, got %d x %d", rows, C);
  MD_CHECK_ARG(lda >= C && ldb >= C, "md_rel_l1_f16: lda = %d and ldb = %d must be >= C = %d", lda, ldb, C);
  MD_CHECK_ARG((long)rows * C <= (1L << 40), "md_rel_l1_f16: problem too large");
  MD_CHECK_ARG(((uintptr_t)a % 2) == 0 && ((uintptr_t)b % 2) == 0, "md_rel_l1_f16: a / b need 2-byte alignment");
  MD_CHECK_ARG(((uintptr_t)workspace % 8) == 0 && ((uintptr_t)out % 8) == 0, "md_rel_l1_f16: workspace / out need 8-byte alignment");
  MD_CHECK_ARG(workspace_bytes >= md_rel_l1_workspace_bytes(rows, C), "md_rel_l1_f16: workspace of %zu bytes, %zu needed", workspace_bytes,
               md_rel_l1_workspace_bytes(rows, C));
  const bool vec = rl_vector_path(a, lda, b, ldb, C);
  const int per_row = vec ? C / 8 : C;
  const long units = (long)rows * per_row;
  const int P = (int)rl_blocks(units);                             // <= the workspace's count: units <= rows C
  if (vec)
    hipLaunchKernelGGL(rel_l1_partial_kernel<true>, dim3((unsigned)P), dim3(RL_THREADS), 0, (hipStream_t)stream, (const half_t*)a, (long)lda,
                       (const half_t*)b, (long)ldb, units, per_row, (float2_t*)workspace);
  else
    hipLaunchKernelGGL(rel_l1_partial_kernel<false>, dim3((unsigned)P), dim3(RL_THREADS), 0, (hipStream_t)stream, (const half_t*)a, (long)lda,
                       (const half_t*)b, (long)ldb, units, per_row, (float2_t*)workspace);
  MD_CHECK_LAUNCH("md_rel_l1_f16");
  hipLaunchKernelGGL(rel_l1_final_kernel, dim3(1), dim3(RL_THREADS), 0, (hipStream_t)stream, (const float2_t*)workspace, P, (float2_t*)out);
  MD_CHECK_LAUNCH("md_rel_l1_f16");
  return MD_OK;
}
