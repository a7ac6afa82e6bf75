// The output boundary of the pipeline: decoded frames -> the bytes every writer takes (MJPEG, GIF, PIL, a preview), in one launch in the place of
// the reference's `(video / 2 + 0.5).clamp(0, 1)` (three torch passes), the permuted copy, the fp32 host array and the writer's own
// `(x * 255).astype(uint8)`.
//
//   src   fp16 or fp32 (src_is_f32), element (b, c, y, x) at b sB + c sC + y sY + x sX in elements: the decoders' own NHWC result (sC = 1,
//         sX = ldc >= C) or a finished NCHW tensor (sX = 1), or any other strided view
//   dst   bytes, (b, y, x, c) at b dB + y dY + x C + c: packed H x W x C frames; the row pitch dY and the frame pitch dB are the caller's, so a
//         frame can be written straight into a larger canvas (a grid of clips).  No alignment is asked of dst: canvas offsets are odd.
//
// Arithmetic: the reference's chain restated operation by operation, NOT the one expression trunc(clamp(127.5 v + 127.5)) (which differs from
// the fp16 chain at 544 of the 63 490 non-NaN fp16 inputs):
//   f32_math = 0 (what fp16 tensors do):  a = fp16(v / 2);  s = fp16(a + 0.5), ONE round-to-nearest-even (the fp32 sum of two fp16 numbers of
//                                         which one is 0.5 and the other at most 2^15 is exact);  s clamped to [0, 1];  q = fp32(s) * 255
//                                         rounded to fp32;  the byte is q truncated toward zero
//   f32_math = 1 (an fp32 VAE boundary):  the same steps with every intermediate in fp32; an fp16 source converts exactly
// v / 2 is v * 0.5: a scaling by a power of two, the same rounding where the result is subnormal.  +Inf gives 255, -Inf gives 0.  NaN gives 0:
// the float path's cast of a NaN to uint8 is undefined in C and in numpy, so this is a CHOICE, made here.  No contraction: a + 0.5 is not
// fused with the product before it.
//
// One thread per 4 consecutive pixels of a row (4 C bytes of dst): 8- / 16-byte loads where the 4 pixels are contiguous and aligned in the source
// (sX = 1: 4 elements per channel; sC = 1 and sX = C: all 4 C elements), plain strided loads otherwise (ldc = 8 with C = 3, odd offsets, a row
// tail); 4-byte stores where the thread's 4 C bytes start on a 4-byte boundary, byte stores otherwise.  256 threads, at most 2048 blocks, a
// grid-stride loop past that.  No atomics, no LDS: two calls give the same bits.  Nothing outside the B H rows of W C bytes is written.
#include "common.h"
#include <limits.h>

#define FU_THREADS 256
#define FU_MAX_BLOCKS 2048

#pragma clang fp contract(off)

struct fu_args_t {
  const void* src;
  unsigned char* dst;
  int B, H, W;
  long sB, sC, sY, sX, dB, dY;
};

template <bool F32M>
__device__ __forceinline__ unsigned fu_quant(float v) {
  float s;
  if (F32M) {
    const float a = v * 0.5f;
    s = a + 0.5f;
  } else {
    const half_t a = (half_t)(v * 0.5f);                            // v is an fp16 number: the product is exact, the cast rounds once
    s = (float)(half_t)((float)a + 0.5f);                           // the sum is exact in fp32, the cast rounds once
  }
  if (s != s) return 0u;                                            // NaN -> 0
  s = s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
  return (unsigned)(s * 255.f);
}

// Thread i of B * H * G, G = ceil(W / 4): pixels x0 = 4 (i % G) .. x0 + np - 1 of row (i / G) % H of frame i / G / H.
template <typename T, int C, bool F32M>
__global__ void __launch_bounds__(FU_THREADS) frames_u8_kernel(fu_args_t a, long total, int G) {
  typedef T vec_t __attribute__((ext_vector_type(4)));
  const bool planar = a.sX == 1, packed = C > 1 && a.sC == 1 && a.sX == C;
  for (long i = (long)blockIdx.x * FU_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * FU_THREADS) {
    const int xg = (int)(i % G);
    const long row = i / G;
    const int y = (int)(row % a.H), b = (int)(row / a.H);
    const int x0 = xg * 4, np = a.W - x0 < 4 ? a.W - x0 : 4;
    const T* ps = (const T*)a.src + (long)b * a.sB + (long)y * a.sY + (long)x0 * a.sX;
    float v[4][C];                                                   // [pixel][channel]
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < C; ++c) v[p][c] = 0.f;
    if (np == 4 && packed && ((uintptr_t)ps % (4 * sizeof(T))) == 0) {
#pragma unroll
      for (int k = 0; k < C; ++k) {                                  // elements 4 k .. 4 k + 3 of the 4 C contiguous ones, pixel-major
        const vec_t in = *reinterpret_cast<const vec_t*>(ps + 4 * k);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[(4 * k + j) / C][(4 * k + j) % C] = (float)in[j];
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const T* pc = ps + (long)c * a.sC;
        if (np == 4 && planar && ((uintptr_t)pc % (4 * sizeof(T))) == 0) {
          const vec_t in = *reinterpret_cast<const vec_t*>(pc);
#pragma unroll
          for (int p = 0; p < 4; ++p) v[p][c] = (float)in[p];
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (p < np) v[p][c] = (float)pc[(long)p * a.sX];
        }
      }
    }
    unsigned w[C];                                                   // the 4 C bytes, little-endian in C words
#pragma unroll
    for (int k = 0; k < C; ++k) w[k] = 0u;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < C; ++c) w[(p * C + c) / 4] |= fu_quant<F32M>(v[p][c]) << (8 * ((p * C + c) % 4));
    unsigned char* pd = a.dst + (long)b * a.dB + (long)y * a.dY + (long)x0 * C;
    if (np == 4 && ((uintptr_t)pd % 4) == 0) {
#pragma unroll
      for (int k = 0; k < C; ++k) reinterpret_cast<unsigned*>(pd)[k] = w[k];
    } else {
#pragma unroll
      for (int j = 0; j < 4 * C; ++j)
        if (j < np * C) pd[j] = (unsigned char)(w[j / 4] >> (8 * (j % 4)));
    }
  }
}

template <typename T, bool F32M>
static void fu_launch(int C, dim3 grid, dim3 block, hipStream_t st, const fu_args_t& a, long total, int G) {
  switch (C) {
    case 1: hipLaunchKernelGGL((frames_u8_kernel<T, 1, F32M>), grid, block, 0, st, a, total, G); break;
    case 2: hipLaunchKernelGGL((frames_u8_kernel<T, 2, F32M>), grid, block, 0, st, a, total, G); break;
    case 3: hipLaunchKernelGGL((frames_u8_kernel<T, 3, F32M>), grid, block, 0, st, a, total, G); break;
    default: hipLaunchKernelGGL((frames_u8_kernel<T, 4, F32M>), grid, block, 0, st, a, total, G); break;
  }
}

extern "C" int md_frames_u8(const void* src, int src_is_f32, int f32_math, void* dst, int B, int H, int W, int C, long sB, long sC, long sY, long sX,
                            long dB, long dY, void* stream) {
  MD_CHECK_ARG(src && dst, "md_frames_u8: NULL src or dst");
  MD_CHECK_ARG(C >= 1 && C <= 4, "md_frames_u8: C must be 1..4, got %d", C);
  MD_CHECK_ARG(B > 0 && H > 0 && W > 0, "md_frames_u8: B, H, W must be positive (%d, %d, %d)", B, H, W);
  MD_CHECK_ARG((long)B * H <= INT_MAX / W, "md_frames_u8: B*H*W must fit an int (B=%d, %d x %d)", B, H, W);
  MD_CHECK_ARG((src_is_f32 == 0 || src_is_f32 == 1) && (f32_math == 0 || f32_math == 1), "md_frames_u8: src_is_f32 and f32_math must be 0 or 1, got %d, %d",
               src_is_f32, f32_math);
  MD_CHECK_ARG(!src_is_f32 || f32_math, "md_frames_u8: an fp32 source (src_is_f32 = 1) needs f32_math = 1");
  const long wc = (long)W * C;
  MD_CHECK_ARG(dY >= wc && dY <= (LONG_MAX - wc) / H, "md_frames_u8: the row pitch dY = %ld must be at least W*C = %ld (and (H-1)*dY + W*C within long)", dY, wc);
  MD_CHECK_ARG(dB >= (long)(H - 1) * dY + wc && dB <= LONG_MAX / B, "md_frames_u8: the frame pitch dB = %ld must be at least (H-1)*dY + W*C = %ld (and B*dB within long)",
               dB, (long)(H - 1) * dY + wc);
  MD_CHECK_ARG(((uintptr_t)src % (src_is_f32 ? 4 : 2)) == 0, "md_frames_u8: src must be aligned to its element (%d bytes)", src_is_f32 ? 4 : 2);
  const fu_args_t a = {src, (unsigned char*)dst, B, H, W, sB, sC, sY, sX, dB, dY};
  const int G = (W + 3) / 4;
  const long total = (long)B * H * G;
  const long blocks = (total + FU_THREADS - 1) / FU_THREADS;
  const dim3 grid((unsigned)(blocks < FU_MAX_BLOCKS ? blocks : FU_MAX_BLOCKS)), block(FU_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  if (src_is_f32)
    fu_launch<float, true>(C, grid, block, st, a, total, G);
  else if (f32_math)
    fu_launch<half_t, true>(C, grid, block, st, a, total, G);
  else
    fu_launch<half_t, false>(C, grid, block, st, a, total, G);
  MD_CHECK_LAUNCH("md_frames_u8");
  return MD_OK;
}
