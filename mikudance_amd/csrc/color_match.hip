// Colour matching of the decoded frames (color_match=): a per-frame 3 x 3 affine colour transfer toward a target image, the stock post-process
// of the SD-1.5 front ends (A1111 "apply color correction", Deforum "color coherence", ComfyUI ColorMatch), at the output boundary and on the
// device.  Two entry points around a small host solve (mikudance_amd/color_match.py):
//
//   md_color_moments   frames -> B x 9 fp64 colour moments (sums of s_c and of s_c s_c' over a frame's pixels), deterministic
//   md_color_apply     frames, B x 12 fp32 coefficients -> clamp(M s + t), as the writers' bytes or as fp32
//
//   src   frame_io.h's source with 3 channels, read by its load rule: md_color_moments in units of NPIX = 8 pixels with 16-byte vectors,
//         md_color_apply in md_frames_u8's units (NPIX = 4, vectors of 4 elements)
//   s     frame_io.h's display colour (fio_display); md_color_apply's bytes are its byte and its byte writer
//
// THE SUMMATION ORDER of md_color_moments (tests/color_match_ref.py restates the depth, tests/test_color_match_gpu.py takes its bound from it).
// A unit is 8 consecutive pixels of a row; a frame has U = H ceil(W / 8) units and P = ceil(U / 1024) workgroups of 256 threads, workgroup
// b P + j works on frame b; unit i of the frame belongs to thread i mod (256 P) of the frame's 256 P threads.  Every term is >= 0, so the
// relative error of a sum is at most (roundings in a term + d) 2^-24 to first order, d = the largest number of fp32 additions a term passes:
//   the (up to) 8 pixels of a unit are added in pixel order into a fresh accumulator                                   7
//   a thread adds its units in ascending order, iters = ceil(U / (256 P)) <= 4 of them                              iters
//   the 64 lanes of a wave: xor butterfly, offsets 32, 16, ..., 1 (every lane ends with the same bits)                6
//   thread k < 9 adds the 4 wave sums of moment k in wave order                                                       3
//   d = iters + 16 <= 20
// (an addition to the initial 0 is exact and counted all the same).  A term holds at most three roundings: the sum in s_i, the one in s_j and
// their product (0.5 v is exact but for subnormal results).  One partial of 9 fp32 per workgroup goes to workspace[9 (b P + j) ...]; the
// second launch, one workgroup of 256 threads per frame, adds them in fp64: thread t takes partials t, t + 256, ... in ascending order, then
// the same butterfly and the same 4-wave sum -- all exact to fp64's 2^-53, which the bound does not notice.  No atomics; every workspace word
// read was written by the first launch of the same call; the grid and every order above depend on (B, H, W) only: same inputs, same bits.
// NaN is an ordinary operand: a NaN in channel c of one pixel reaches the five sums s_c is a term of.
//
// Both kernels are HBM-bound streams (2 or 4 bytes read per element once; 1 or 4 written by apply).  Lanes run along a row, so a wave
// reads one run of its row; the moments kernel's unit loop is unrolled so that a thread has several units' loads in flight.
#include "frame_io.h"
#include "color_match.h"

#define CM_THREADS FIO_THREADS
#define CM_UNITS_PER_BLOCK 1024                                      // 4 units of 8 pixels per thread

// ---------------------------------------------------------------------------------------------------------------- md_color_moments
template <typename T>
__global__ void __launch_bounds__(CM_THREADS) color_moments_partial_kernel(fio_src_t a, int G, long U, int P, float* __restrict__ partial) {
  constexpr int VE = 16 / sizeof(T);
  __shared__ float waves[CM_THREADS / 64][9];
  const int b = blockIdx.x / P, j = blockIdx.x - b * P;              // b < B: the grid is B P
  float acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.f;
#pragma unroll 2
  for (long i = (long)j * CM_THREADS + threadIdx.x; i < U; i += (long)P * CM_THREADS) {
    const int y = (int)(i / G), xg = (int)(i - (long)y * G);         // y < H: i < U = H G
    const fio_unit_t un = fio_unit_at<8>(b, y, xg, a.W);             // 1 <= np: xg < G = ceil(W / 8)
    FIO_PIXELS(v, 8, 3);
    fio_load<T, 3, 8, VE>(fio_src_at<T>(a, un), a.sC, a.sX, un.np, un.inner, v);
    float u[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) u[k] = 0.f;
#pragma unroll
    for (int p = 0; p < 8; ++p)
      if (p < un.np) {
        const float s0 = fio_display(v[p][0]), s1 = fio_display(v[p][1]), s2 = fio_display(v[p][2]);
        u[0] = fio_add(u[0], s0);
        u[1] = fio_add(u[1], s1);
        u[2] = fio_add(u[2], s2);
        u[3] = fio_add(u[3], fio_mul(s0, s0));
        u[4] = fio_add(u[4], fio_mul(s1, s1));
        u[5] = fio_add(u[5], fio_mul(s2, s2));
        u[6] = fio_add(u[6], fio_mul(s0, s1));
        u[7] = fio_add(u[7], fio_mul(s0, s2));
        u[8] = fio_add(u[8], fio_mul(s1, s2));
      }
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = fio_add(acc[k], u[k]);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const float w = wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6][k] = w;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    float r = waves[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < CM_THREADS / 64; ++w) r = fio_add(r, waves[w][threadIdx.x]);
    partial[(long)blockIdx.x * 9 + threadIdx.x] = r;                 // < 9 B P floats: the workspace's count
  }
}

__device__ __forceinline__ double cm_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(CM_THREADS) color_moments_final_kernel(const float* __restrict__ partial, int P, double* __restrict__ out) {
  __shared__ double waves[CM_THREADS / 64][9];
  const float* pf = partial + (long)blockIdx.x * P * 9;              // frame b = blockIdx.x: partials 9 b P .. 9 (b + 1) P - 1
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < P; i += CM_THREADS)
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] += (double)pf[(long)i * 9 + k];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double w = cm_wave_sum_f64(acc[k]);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6][k] = w;
  }
  __syncthreads();
  if (threadIdx.x < 9) {
    double r = waves[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < CM_THREADS / 64; ++w) r += waves[w][threadIdx.x];
    out[(long)blockIdx.x * 9 + threadIdx.x] = r;
  }
}

static inline long cm_blocks_per_frame(int H, int W) {
  const long U = (long)H * ((W + 7) / 8);
  return (U + CM_UNITS_PER_BLOCK - 1) / CM_UNITS_PER_BLOCK;
}

extern "C" size_t md_color_moments_workspace_bytes(int B, int H, int W) {
  if (!fio_shape_ok(B, H, W)) return 0;
  return (size_t)B * (size_t)cm_blocks_per_frame(H, W) * 9 * sizeof(float);
}

extern "C" int md_color_moments(const void* src, int src_is_f32, int B, int H, int W, long sB, long sC, long sY, long sX, void* workspace,
                                size_t workspace_bytes, void* out, void* stream) {
  MD_CHECK_ARG(src && workspace && out, "md_color_moments: NULL pointer");
  if (int e = fio_check_src("md_color_moments", src, src_is_f32, B, H, W)) return e;
  MD_CHECK_ARG(((uintptr_t)workspace % 4) == 0 && ((uintptr_t)out % 8) == 0, "md_color_moments: workspace needs 4-byte, out 8-byte alignment");
  MD_CHECK_ARG(workspace_bytes >= md_color_moments_workspace_bytes(B, H, W), "md_color_moments: workspace of %zu bytes, %zu needed", workspace_bytes,
               md_color_moments_workspace_bytes(B, H, W));
  const long P = cm_blocks_per_frame(H, W);                          // <= B H W / 8192 + 1
  MD_CHECK_ARG((long)B * P <= INT_MAX, "md_color_moments: %d frames of %ld workgroups exceed the grid", B, P);
  const fio_src_t a = {src, B, H, W, sB, sC, sY, sX};
  const int G = (W + 7) / 8;
  const long U = (long)H * G;
  const dim3 grid((unsigned)((long)B * P)), block(CM_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  if (src_is_f32)
    hipLaunchKernelGGL(color_moments_partial_kernel<float>, grid, block, 0, st, a, G, U, (int)P, (float*)workspace);
  else
    hipLaunchKernelGGL(color_moments_partial_kernel<half_t>, grid, block, 0, st, a, G, U, (int)P, (float*)workspace);
  MD_CHECK_LAUNCH("md_color_moments");
  hipLaunchKernelGGL(color_moments_final_kernel, dim3((unsigned)B), block, 0, st, (const float*)workspace, (int)P, (double*)out);
  MD_CHECK_LAUNCH("md_color_moments");
  return MD_OK;
}

// ------------------------------------------------------------------------------------------------------------------ md_color_apply
struct cm_dst_t {
  void* dst;
  const float* coef;
  long dB, dC, dY, dX;
};

// One thread per unit of 4 pixels, md_frames_u8's map (fio_unit).
template <typename T, bool F32D>
__global__ void __launch_bounds__(CM_THREADS) color_apply_kernel(fio_src_t a, cm_dst_t d, long total, int G) {
  for (long i = (long)blockIdx.x * CM_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * CM_THREADS) {
    const fio_unit_t un = fio_unit<4>((unsigned)i, G, a.H, a.W);     // b < B: i < total = B H G
    const int b = un.b, y = un.y, x0 = un.x0, np = un.np;
    FIO_PIXELS(v, 4, 3);
    fio_load<T, 3, 4, 4>(fio_src_at<T>(a, un), a.sC, a.sX, np, un.inner, v);
    float m[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) m[k] = d.coef[(long)b * 12 + k];    // row-major M, then t
    float o[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const float s0 = fio_display(v[p][0]), s1 = fio_display(v[p][1]), s2 = fio_display(v[p][2]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float r = fio_add(m[9 + c], fio_mul(m[3 * c], s0));
        r = fio_add(r, fio_mul(m[3 * c + 1], s1));
        r = fio_add(r, fio_mul(m[3 * c + 2], s2));
        o[p][c] = fio_clamp01(r);                                    // NaN kept
      }
    }
    if (F32D) {
      float* pd = (float*)d.dst + (long)b * d.dB + (long)y * d.dY + (long)x0 * d.dX;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float* pc = pd + (long)c * d.dC;
        if (np == 4 && d.dX == 1 && ((uintptr_t)pc % 16) == 0) {
          *reinterpret_cast<floatx4*>(pc) = floatx4{o[0][c], o[1][c], o[2][c], o[3][c]};
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (p < np) pc[(long)p * d.dX] = o[p][c];
        }
      }
    } else {
      fio_store_bytes<3>((unsigned char*)d.dst + (long)b * d.dB + (long)y * d.dY + (long)x0 * 3, np, o);
    }
  }
}

extern "C" int md_color_apply(const void* src, int src_is_f32, const void* coef, void* dst, int dst_is_f32, int B, int H, int W, long sB, long sC,
                              long sY, long sX, long dB, long dC, long dY, long dX, void* stream) {
  MD_CHECK_ARG(src && coef && dst, "md_color_apply: NULL src, coef or dst");
  if (int e = fio_check_src("md_color_apply", src, src_is_f32, B, H, W)) return e;
  MD_CHECK_ARG(dst_is_f32 == 0 || dst_is_f32 == 1, "md_color_apply: dst_is_f32 must be 0 or 1, got %d", dst_is_f32);
  MD_CHECK_ARG(((uintptr_t)coef % 4) == 0, "md_color_apply: coef needs 4-byte alignment");
  if (dst_is_f32) {
    MD_CHECK_ARG(((uintptr_t)dst % 4) == 0, "md_color_apply: an fp32 dst needs 4-byte alignment");
    MD_CHECK_ARG(dB > 0 && dC > 0 && dY > 0 && dX > 0, "md_color_apply: the strides of an fp32 dst must be positive (%ld, %ld, %ld, %ld)", dB, dC, dY, dX);
  } else {
    MD_CHECK_ARG(dC == 1 && dX == 3, "md_color_apply: a byte dst has packed pixels, dC = 1 and dX = 3, got %ld and %ld", dC, dX);
    if (int e = fio_check_bytes("md_color_apply", B, H, W, 3, dB, dY)) return e;
  }
  const fio_src_t a = {src, B, H, W, sB, sC, sY, sX};
  const cm_dst_t d = {dst, (const float*)coef, dB, dC, dY, dX};
  const int G = (W + 3) / 4;
  const long total = (long)B * H * G;
  const dim3 grid = fio_grid(total), block(CM_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  if (src_is_f32) {
    if (dst_is_f32)
      hipLaunchKernelGGL((color_apply_kernel<float, true>), grid, block, 0, st, a, d, total, G);
    else
      hipLaunchKernelGGL((color_apply_kernel<float, false>), grid, block, 0, st, a, d, total, G);
  } else {
    if (dst_is_f32)
      hipLaunchKernelGGL((color_apply_kernel<half_t, true>), grid, block, 0, st, a, d, total, G);
    else
      hipLaunchKernelGGL((color_apply_kernel<half_t, false>), grid, block, 0, st, a, d, total, G);
  }
  MD_CHECK_LAUNCH("md_color_apply");
  return MD_OK;
}
