// The output boundary's shared parts: how md_frames_u8, md_color_moments and md_color_apply (frames_u8.hip, color_match.hip) read a frame and
// how the first and the last write its bytes.  Included by those two files only.
//
//   src   fp16 or fp32, element (b, c, y, x) of a (B, C, H, W)-shaped view at b sB + c sC + y sY + x sX in elements: the decoders' NHWC image
//         (sC = 1, sX = the pixel pitch >= C), a finished NCHW tensor (sX = 1) or any other strided view.  Aligned to its element, no more.
//   dst   bytes, (b, y, x, c) at b dB + y dY + x C + c: packed H x W x C frames; the row pitch dY and the frame pitch dB are the caller's, so a
//         frame can be written straight into a larger canvas.  No alignment is asked of dst: canvas offsets are odd.
//
// A UNIT is NPIX consecutive pixels of a row (the last unit of a row has np < NPIX of them), one thread's work.
//
// THE LOAD RULE (fio_load), the same for all three kernels.  A unit is read with vectors of VE elements if it is whole (np = NPIX), its first
// element lies on a vector boundary, and it is
//   packed   channels last (sC = 1; with C = 1 the stride of the one channel says nothing) at a pixel pitch sX of
//              C          the NPIX C elements are contiguous, every one a value of the unit;
//              4 or 8 > C the NPIX sX elements are contiguous, padding channels come along and are dropped (a vector of padding alone is not
//                         read) -- but ONLY IF A PIXEL OF THE SAME ROW FOLLOWS THE UNIT (`inner`);
//   planar   sX = 1: NPIX contiguous elements per channel.
// Everything else takes element loads, of the C channels of the unit's np pixels and nothing more: a row's tail, the last unit of a row at
// pitch 4 / 8 > C, an odd base or offset, any other pitch or stride.
// THE INVARIANT: nothing outside the view's own span is read; a padding read always lies below a later pixel of the same row.  With e the
// row's last valid element, (W - 1) sX + C - 1: at pitch C a vector unit ends at (x0 + NPIX) C - 1 <= e; at pitch 4 / 8 > C it ends at or
// before (x0 + NPIX) sX - 1 <= (W - 1) sX - 1 = e - C, below pixel x0 + NPIX <= W - 1; planar and element loads read values of the view only.
// (The last pixel's padding need not exist: it is never read.)  Every (C, pitch) with pitch = C or pitch in {4, 8} has a vector form under
// this rule -- NPIX pitch is a multiple of VE for the widths in use, asserted below -- so none is sent to element loads as a pair.
//
// Arithmetic: fp32, every operation rounded on its own.  This header switches contraction off for itself and for the file that includes it;
// functions defined in a header are compiled under the HEADER's contraction mode, which is why the display colour is written with the plain
// operators below and not with the toolkit's __fmul_rn / __fadd_rn (plain operators too, but in a header that contracts: after inlining, a
// product and the sum that takes it become one fma).
#pragma once
#include "common.h"
#include <limits.h>

#pragma clang fp contract(off)

#define FIO_THREADS 256
#define FIO_MAX_BLOCKS 2048

struct fio_src_t {
  const void* src;
  int B, H, W;
  long sB, sC, sY, sX;
};

// ---- the thread map: unit xg of row y of frame b -> pixels x0 .. x0 + np - 1; `inner`: a pixel of the row follows the unit
struct fio_unit_t {
  int b, y, x0, np;
  bool inner;
};

template <int NPIX>
__device__ __forceinline__ fio_unit_t fio_unit_at(int b, int y, int xg, int W) {
  const int x0 = xg * NPIX;
  return {b, y, x0, W - x0 < NPIX ? W - x0 : NPIX, x0 + NPIX < W};
}

// Unit i of B H G, G = ceil(W / NPIX): unit i % G of row (i / G) % H of frame i / G / H.  B H W fits an int (fio_check_src), so i does.
template <int NPIX>
__device__ __forceinline__ fio_unit_t fio_unit(unsigned i, int G, int H, int W) {
  const unsigned row = i / (unsigned)G;
  return fio_unit_at<NPIX>((int)(row / (unsigned)H), (int)(row % (unsigned)H), (int)(i % (unsigned)G), W);
}

template <typename T>
__device__ __forceinline__ const T* fio_src_at(const fio_src_t& a, const fio_unit_t& u) {
  return (const T*)a.src + (long)u.b * a.sB + (long)u.y * a.sY + (long)u.x0 * a.sX;
}

// ---- the loader
// A unit's values, v[pixel][channel], all 0: what fio_load fills.  A macro, so that the loops stand in the kernel's own body: zeroed inside a
// function (or with = {}) the moments kernel takes 96 VGPRs in the place of 68 and loses two waves per SIMD.
#define FIO_PIXELS(v, NPIX, C)                                                  \
  float v[NPIX][C];                                                             \
  _Pragma("unroll") for (int p_ = 0; p_ < NPIX; ++p_)                           \
  _Pragma("unroll") for (int c_ = 0; c_ < C; ++c_) v[p_][c_] = 0.f

template <typename T, int C, int NPIX, int VE, int PITCH>
__device__ __forceinline__ void fio_load_packed(const T* ps, float (&v)[NPIX][C]) {
  typedef T vec_t __attribute__((ext_vector_type(VE)));
  static_assert(PITCH >= C && NPIX * PITCH % VE == 0, "a unit is a whole number of vectors");
#pragma unroll
  for (int k = 0; k < NPIX * PITCH / VE; ++k) {
    if (VE * k % PITCH >= C && VE * k % PITCH + VE <= PITCH) continue;          // padding only
    const vec_t in = *reinterpret_cast<const vec_t*>(ps + VE * k);
#pragma unroll
    for (int j = 0; j < VE; ++j)
      if ((VE * k + j) % PITCH < C) v[(VE * k + j) / PITCH][(VE * k + j) % PITCH] = (float)in[j];
  }
}

// The np <= NPIX pixels that start at ps -> v[pixel][channel]; pixels np .. NPIX - 1 are left as they are.
template <typename T, int C, int NPIX, int VE>
__device__ __forceinline__ void fio_load(const T* ps, long sC, long sX, int np, bool inner, float (&v)[NPIX][C]) {
  typedef T vec_t __attribute__((ext_vector_type(VE)));
  static_assert(C >= 1 && C <= 4 && NPIX % VE == 0, "1..4 channels, whole vectors per channel");
  const bool whole = np == NPIX;
  if (whole && (C == 1 || sC == 1) && (sX == C || ((sX == 4 || sX == 8) && inner)) && ((uintptr_t)ps % (VE * sizeof(T))) == 0) {
    if (sX == C)
      fio_load_packed<T, C, NPIX, VE, C>(ps, v);
    else if (sX == 4)
      fio_load_packed<T, C, NPIX, VE, 4>(ps, v);
    else
      fio_load_packed<T, C, NPIX, VE, 8>(ps, v);
    return;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const T* pc = ps + (long)c * sC;
    if (whole && sX == 1 && ((uintptr_t)pc % (VE * sizeof(T))) == 0) {
#pragma unroll
      for (int k = 0; k < NPIX / VE; ++k) {
        const vec_t in = *reinterpret_cast<const vec_t*>(pc + VE * k);
#pragma unroll
        for (int j = 0; j < VE; ++j) v[VE * k + j][c] = (float)in[j];
      }
    } else {
#pragma unroll
      for (int p = 0; p < NPIX; ++p)
        if (p < np) v[p][c] = (float)pc[(long)p * sX];
    }
  }
}

// ---- the display colour and its byte: s = clamp(0.5 v + 0.5, 0, 1), the product and the sum rounded separately, NaN kept; the byte is 0 for a
// NaN (the cast of a NaN is undefined in C and in numpy: a CHOICE, made here), otherwise fp32(s * 255) truncated toward zero
__device__ __forceinline__ float fio_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float fio_add(float a, float b) { return a + b; }
__device__ __forceinline__ float fio_clamp01(float s) { return s < 0.f ? 0.f : (s > 1.f ? 1.f : s); }      // a NaN fails both comparisons and stays
__device__ __forceinline__ float fio_display(float v) { return fio_clamp01(fio_add(fio_mul(0.5f, v), 0.5f)); }
__device__ __forceinline__ unsigned fio_byte(float s) { return s != s ? 0u : (unsigned)fio_mul(s, 255.f); }  // s in [0, 1]: the product is in [0, 255]

// ---- the byte writer: the colours s[pixel][channel] of a unit of 4 pixels -> its np C bytes at pd, little-endian in C words; 4-byte stores
// where the unit is whole and pd on a 4-byte boundary, byte stores otherwise.  Nothing past the np C bytes is written.
template <int C>
__device__ __forceinline__ void fio_store_bytes(unsigned char* pd, int np, const float (&s)[4][C]) {
  unsigned w[C];
#pragma unroll
  for (int k = 0; k < C; ++k) w[k] = 0u;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < C; ++c) w[(p * C + c) / 4] |= fio_byte(s[p][c]) << (8 * ((p * C + c) % 4));
  if (np == 4 && ((uintptr_t)pd % 4) == 0) {
#pragma unroll
    for (int k = 0; k < C; ++k) reinterpret_cast<unsigned*>(pd)[k] = w[k];
  } else {
#pragma unroll
    for (int j = 0; j < 4 * C; ++j)
      if (j < np * C) pd[j] = (unsigned char)(w[j / 4] >> (8 * (j % 4)));
  }
}

// ---- the host side of the three entry points (`who`: the entry point's name, the start of every md_last_error text)
static inline bool fio_shape_ok(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (long)B * H <= INT_MAX / W; }

static inline int fio_check_src(const char* who, const void* src, int src_is_f32, int B, int H, int W) {
  MD_CHECK_ARG(B > 0 && H > 0 && W > 0, "%s: B, H, W must be positive (%d, %d, %d)", who, B, H, W);
  MD_CHECK_ARG(fio_shape_ok(B, H, W), "%s: B*H*W must fit an int (B=%d, %d x %d)", who, B, H, W);
  MD_CHECK_ARG(src_is_f32 == 0 || src_is_f32 == 1, "%s: src_is_f32 must be 0 or 1, got %d", who, src_is_f32);
  MD_CHECK_ARG(((uintptr_t)src % (src_is_f32 ? 4 : 2)) == 0, "%s: src must be aligned to its element (%d bytes)", who, src_is_f32 ? 4 : 2);
  return MD_OK;
}

static inline int fio_check_bytes(const char* who, int B, int H, int W, int C, long dB, long dY) {
  const long wc = (long)W * C;
  MD_CHECK_ARG(dY >= wc && dY <= (LONG_MAX - wc) / H, "%s: the row pitch dY = %ld must be at least W*C = %ld (and (H-1)*dY + W*C within long)", who, dY, wc);
  MD_CHECK_ARG(dB >= (long)(H - 1) * dY + wc && dB <= LONG_MAX / B, "%s: the frame pitch dB = %ld must be at least (H-1)*dY + W*C = %ld (and B*dB within long)", who,
               dB, (long)(H - 1) * dY + wc);
  return MD_OK;
}

// The grid of the "4 pixels per thread" kernels: 256 threads, at most 2048 blocks, a grid-stride loop past that.
static inline dim3 fio_grid(long units) {
  const long blocks = (units + FIO_THREADS - 1) / FIO_THREADS;
  return dim3((unsigned)(blocks < FIO_MAX_BLOCKS ? blocks : FIO_MAX_BLOCKS));
}
