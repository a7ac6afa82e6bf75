// The output boundary of the pipeline: decoded frames -> the bytes every writer takes (MJPEG, GIF, PIL, a preview), in one launch in the place of
// the reference's `(video / 2 + 0.5).clamp(0, 1)` (three torch passes), the permuted copy, the fp32 host array and the writer's own
// `(x * 255).astype(uint8)`.  The source, the destination, the thread map (one thread per 4 consecutive pixels of a row), the load rule and
// the byte writer are frame_io.h's, stated there.
//
// Arithmetic: the reference's chain restated operation by operation, NOT the one expression trunc(clamp(127.5 v + 127.5)) (which differs from
// the fp16 chain at 544 of the 63 490 non-NaN fp16 inputs):
//   f32_math = 0 (what fp16 tensors do):  a = fp16(v / 2);  s = fp16(a + 0.5), ONE round-to-nearest-even (the fp32 sum of two fp16 numbers of
//                                         which one is 0.5 and the other at most 2^15 is exact);  s clamped to [0, 1];  q = fp32(s) * 255
//                                         rounded to fp32;  the byte is q truncated toward zero
//   f32_math = 1 (an fp32 VAE boundary):  the same steps with every intermediate in fp32 (frame_io.h's display colour and byte); an fp16
//                                         source converts exactly
// v / 2 is v * 0.5: a scaling by a power of two, the same rounding where the result is subnormal.  +Inf gives 255, -Inf gives 0, NaN gives 0.
// No contraction: a + 0.5 is not fused with the product before it.
//
// 256 threads, at most 2048 blocks, a grid-stride loop past that.  No atomics, no LDS: two calls give the same bits.  Nothing outside the B H
// rows of W C bytes is written.
#include "frame_io.h"

// The fp16 chain's display colour; its clamp and its byte are the fp32 chain's.
__device__ __forceinline__ float fu_display_f16(float v) {
  const half_t a = (half_t)(v * 0.5f);                                // v is an fp16 number: the product is exact, the cast rounds once
  return fio_clamp01((float)(half_t)((float)a + 0.5f));               // the sum is exact in fp32, the cast rounds once
}

template <typename T, int C, bool F32M>
__global__ void __launch_bounds__(FIO_THREADS) frames_u8_kernel(fio_src_t a, unsigned char* dst, long dB, long dY, long total, int G) {
  for (long i = (long)blockIdx.x * FIO_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * FIO_THREADS) {
    const fio_unit_t u = fio_unit<4>((unsigned)i, G, a.H, a.W);
    FIO_PIXELS(v, 4, C);
    fio_load<T, C, 4, 4>(fio_src_at<T>(a, u), a.sC, a.sX, u.np, u.inner, v);
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < C; ++c) v[p][c] = F32M ? fio_display(v[p][c]) : fu_display_f16(v[p][c]);
    fio_store_bytes<C>(dst + (long)u.b * dB + (long)u.y * dY + (long)u.x0 * C, u.np, v);
  }
}

template <typename T, bool F32M>
static void fu_launch(int C, hipStream_t st, const fio_src_t& a, unsigned char* dst, long dB, long dY) {
  const int G = (a.W + 3) / 4;
  const long total = (long)a.B * a.H * G;
  const dim3 grid = fio_grid(total), block(FIO_THREADS);
  switch (C) {
    case 1: hipLaunchKernelGGL((frames_u8_kernel<T, 1, F32M>), grid, block, 0, st, a, dst, dB, dY, total, G); break;
    case 2: hipLaunchKernelGGL((frames_u8_kernel<T, 2, F32M>), grid, block, 0, st, a, dst, dB, dY, total, G); break;
    case 3: hipLaunchKernelGGL((frames_u8_kernel<T, 3, F32M>), grid, block, 0, st, a, dst, dB, dY, total, G); break;
    default: hipLaunchKernelGGL((frames_u8_kernel<T, 4, F32M>), grid, block, 0, st, a, dst, dB, dY, total, G); break;
  }
}

extern "C" int md_frames_u8(const void* src, int src_is_f32, int f32_math, void* dst, int B, int H, int W, int C, long sB, long sC, long sY, long sX,
                            long dB, long dY, void* stream) {
  MD_CHECK_ARG(src && dst, "md_frames_u8: NULL src or dst");
  MD_CHECK_ARG(C >= 1 && C <= 4, "md_frames_u8: C must be 1..4, got %d", C);
  if (int e = fio_check_src("md_frames_u8", src, src_is_f32, B, H, W)) return e;
  MD_CHECK_ARG(f32_math == 0 || f32_math == 1, "md_frames_u8: f32_math must be 0 or 1, got %d", f32_math);
  MD_CHECK_ARG(!src_is_f32 || f32_math, "md_frames_u8: an fp32 source (src_is_f32 = 1) needs f32_math = 1");
  if (int e = fio_check_bytes("md_frames_u8", B, H, W, C, dB, dY)) return e;
  const fio_src_t a = {src, B, H, W, sB, sC, sY, sX};
  const hipStream_t st = (hipStream_t)stream;
  if (src_is_f32)
    fu_launch<float, true>(C, st, a, (unsigned char*)dst, dB, dY);
  else if (f32_math)
    fu_launch<half_t, true>(C, st, a, (unsigned char*)dst, dB, dY);
  else
    fu_launch<half_t, false>(C, st, a, (unsigned char*)dst, dB, dY);
  MD_CHECK_LAUNCH("md_frames_u8");
  return MD_OK;
}
