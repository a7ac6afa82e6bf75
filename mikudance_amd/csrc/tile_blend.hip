// Seam blending of tiled VAE encode / decode (AutoencoderKL.enable_tiling(), the rules of diffusers 0.24's tiled_encode / tiled_decode): one launch
// per tile does what diffusers spells as blend_v -> blend_h -> crop -> torch.cat -> layout change.
//
//   cur   (B, Th, Tw, ldc) fp16 NHWC, C <= ldc valid channels: the tile as the encoder + quant_conv or the decoder left it; updated IN PLACE
//   above (B, Ah, Tw, ldc) or NULL: the tile above, as it stands after its own call;  left (B, Th, Lw, ldc) or NULL: the tile to the left, likewise
//   dst   fp16 or fp32, element (b, c, y, x) at b sB + c sC + y sY + x sX: the caller's final tensor, already offset to this tile's corner
//
//   v = cur[y][x]
//   if above and y < ev':  v = above[Ah - ev' + y][x] (1 - y / ev') + v (y / ev')        ev' = min(Ah, Th, ev)
//   if left  and x < eh':  v = left[y][Lw - eh' + x]  (1 - x / eh') + v (x / eh')        eh' = min(Lw, Tw, eh)
//   cur[y][x] = fp16(v)                                   the whole tile: the tiles below and to the right read it
//   if y < keep_h and x < keep_w:  dst[b, c, y, x] = v    the cropped part
//
// Vertical first, then horizontal, both on the neighbour as blended, the weights from the CLAMPED extents: diffusers' order and in-place dependence.
// In place is safe: element (y, x) of cur depends on itself and on other buffers only.
//
// Arithmetic: fp32 operations only, ONE rounding to fp16 at the store (diffusers rounds after every operation).  A blend is a signed sum; where the
// two tiles cancel, plain fp32 weights would leave an error relative to the operands, not to the result, so the weights and the sums are pairs of
// floats (ff_pair.h) and the result is within an fp16 ulp of the float64 value whatever cancels.  Weight 0 (y = 0, x = 0) returns the neighbour
// exactly; non-finite inputs give non-finite outputs (0 * Inf, as in torch).
//
// A tile is a few MB once per tile of a VAE pass that runs a hundred convolutions on it: one thread per 8 bytes of channels (ldc % 4 == 0 and 8-byte
// aligned tiles: the moments, ldc = 64) or per pixel (the decoder's 3-channel image, 6 bytes per pixel), x fastest, so that a wave's stores to a
// destination row are contiguous.  No atomics, no LDS: two calls give the same bits.
#include "common.h"
#include <limits.h>

#define TB_THREADS 256
#define TB_MAX_BLOCKS 2048

#pragma clang fp contract(off)

#include "ff_pair.h"

struct tb_args_t {
  half_t* cur;
  const half_t* above;
  const half_t* left;
  void* dst;
  int B, Th, Tw, C, ldc, Ah, Lw, ev, eh, keep_h, keep_w;
  long sB, sC, sY, sX;
};

// n / d for integers 0 <= n < d < 2^24 (exact as floats): the quotient and its remainder term.
__host__ __device__ __forceinline__ ff_t tb_ratio(int n, int d) {
  const float nf = (float)n, df = (float)d;
  const float th = nf / df;
  return ff_fast_sum(th, fmaf(-th, df, nf) / df);
}

// a (1 - t) + v t
__host__ __device__ __forceinline__ ff_t tb_lerp(float a, ff_t v, ff_t t) {
  const ff_t u = ff_add(ff_t{-t.h, -t.l}, 1.f);
  return ff_add(ff_mul(u, a), ff_mul(v, t));
}

// The pair as ONE float that rounds to fp16 like the pair itself: h + l rounded to odd (the fp32 sum, moved one step towards the part it lost
// when its last bit is even).  fp32 keeps 13 bits more than fp16, so the second rounding sees on which side of an fp16 midpoint the pair lies;
// a plain h + l lands exactly on such a midpoint where one operand is many binades below the other (the rest of it lost in the fp32 sum) and
// would then go to the even neighbour whatever side the value is on.  The tile is stored for its neighbours to blend with: one ulp off there adds
// up to (1 - t) ulp to their half.
__host__ __device__ __forceinline__ float tb_round_odd(ff_t v) {
  const float s = v.h + v.l, e = v.l - (s - v.h);                  // e: what s lost, exact (|h| >= |l|)
  unsigned bits = __builtin_bit_cast(unsigned, s);
  if (__builtin_isfinite(s) && e != 0.f && !(bits & 1u)) bits += ((e > 0.f) == (s > 0.f)) ? 1u : ~0u;
  return __builtin_bit_cast(float, bits);
}

// Channels [c0, c0 + VEC) of pixel (b, y, x); the first nv of them are valid (stored).  VEC = 4: one 8-byte load per buffer, c0 + 4 <= ldc.
// y < Th, x < Tw; the neighbour rows Ah - ev + y < Ah and columns Lw - eh + x < Lw: nothing outside the three tiles is read.  Host-callable.
template <typename T, int VEC>
__host__ __device__ __forceinline__ void tb_pixel(const tb_args_t& a, int b, int y, int x, int c0, int nv) {
  const int ev = a.ev, eh = a.eh;                                     // clamped by the launcher; 0 without the neighbour
  typedef _Float16 vec_t __attribute__((ext_vector_type(VEC)));
  half_t* pc = a.cur + (((long)b * a.Th + y) * a.Tw + x) * a.ldc + c0;
  ff_t v[VEC];
  {
    const vec_t in = *reinterpret_cast<const vec_t*>(pc);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = {(float)in[k], 0.f};
  }
  if (a.above && y < ev) {
    const vec_t in = *reinterpret_cast<const vec_t*>(a.above + (((long)b * a.Ah + (a.Ah - ev + y)) * a.Tw + x) * a.ldc + c0);
    const ff_t t = tb_ratio(y, ev);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = tb_lerp((float)in[k], v[k], t);
  }
  if (a.left && x < eh) {
    const vec_t in = *reinterpret_cast<const vec_t*>(a.left + (((long)b * a.Th + y) * a.Lw + (a.Lw - eh + x)) * a.ldc + c0);
    const ff_t t = tb_ratio(x, eh);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = tb_lerp((float)in[k], v[k], t);
  }
  float r[VEC];
  vec_t o;
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    r[k] = v[k].h + v[k].l;
    o[k] = (half_t)tb_round_odd(v[k]);
  }
  if (nv == VEC) {
    *reinterpret_cast<vec_t*>(pc) = o;
  } else {                                                          // the channels behind C keep their bits
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      if (k < nv) pc[k] = o[k];
  }
  if (y < a.keep_h && x < a.keep_w) {
    T* pd = (T*)a.dst + (long)b * a.sB + (long)y * a.sY + (long)x * a.sX;
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      if (k < nv) pd[(long)(c0 + k) * a.sC] = sizeof(T) == 2 ? (T)o[k] : (T)r[k];
  }
}

// Thread i of B * Th * G * Tw: x fastest, then the channel group (VEC = 4: G = ceil(C / 4) groups of 4; VEC = 1: G = 1 and the thread walks the
// C channels of its pixel).
template <typename T, int VEC>
__global__ void __launch_bounds__(TB_THREADS) tile_blend_kernel(tb_args_t a, long total, int G) {
  for (long i = (long)blockIdx.x * TB_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * TB_THREADS) {
    const int x = (int)(i % a.Tw);
    long r = i / a.Tw;
    const int g = (int)(r % G);
    r /= G;
    const int y = (int)(r % a.Th), b = (int)(r / a.Th);
    if (VEC == 1) {
      for (int c = 0; c < a.C; ++c) tb_pixel<T, 1>(a, b, y, x, c, 1);
    } else {
      const int c0 = g * VEC, left = a.C - c0;
      tb_pixel<T, VEC>(a, b, y, x, c0, left < VEC ? left : VEC);
    }
  }
}

static inline bool tb_overlap(const void* p, long n, const void* q, long m) {      // n, m fp16 elements
  const uintptr_t pb = (uintptr_t)p, pe = pb + (uintptr_t)n * 2, qb = (uintptr_t)q, qe = qb + (uintptr_t)m * 2;
  return !(pe <= qb || qe <= pb);
}

extern "C" int md_tile_blend_f16(void* cur, int ldc, const void* above, int Ah, const void* left, int Lw, void* dst, int dst_is_f32, int B, int Th, int Tw,
                                 int C, int ev, int eh, int keep_h, int keep_w, long sB, long sC, long sY, long sX, void* stream) {
  MD_CHECK_ARG(cur && dst, "md_tile_blend_f16: NULL cur or dst");
  MD_CHECK_ARG(B > 0 && Th > 0 && Tw > 0 && C > 0 && ldc > 0, "md_tile_blend_f16: B, Th, Tw, C, ldc must be positive (%d, %d, %d, %d, %d)", B, Th, Tw, C, ldc);
  MD_CHECK_ARG(C <= ldc, "md_tile_blend_f16: C = %d valid channels exceed the pixel pitch ldc = %d", C, ldc);
  MD_CHECK_ARG(ev >= 0 && eh >= 0, "md_tile_blend_f16: blend extents must not be negative (ev %d, eh %d)", ev, eh);
  MD_CHECK_ARG(keep_h > 0 && keep_h <= Th && keep_w > 0 && keep_w <= Tw, "md_tile_blend_f16: the kept window %d x %d must lie in the %d x %d tile", keep_h,
               keep_w, Th, Tw);
  MD_CHECK_ARG((!above || Ah > 0) && (!left || Lw > 0), "md_tile_blend_f16: a neighbour needs a positive size (Ah %d, Lw %d)", Ah, Lw);
  MD_CHECK_ARG(dst_is_f32 == 0 || dst_is_f32 == 1, "md_tile_blend_f16: dst_is_f32 must be 0 or 1, got %d", dst_is_f32);
  MD_CHECK_ARG(((uintptr_t)cur % 2) == 0 && ((uintptr_t)above % 2) == 0 && ((uintptr_t)left % 2) == 0 && ((uintptr_t)dst % (dst_is_f32 ? 4 : 2)) == 0,
               "md_tile_blend_f16: cur / above / left need 2-byte alignment, dst that of its element");
  const long rows = (long)B * Th, arows = above ? (long)B * Ah : 0, lcols = left ? Lw : 0;
  MD_CHECK_ARG(rows <= INT_MAX / Tw && rows * Tw <= INT_MAX / ldc && arows <= INT_MAX / Tw && arows * Tw <= INT_MAX / ldc &&
                   (lcols == 0 || (rows <= INT_MAX / lcols && rows * lcols <= INT_MAX / ldc)),
               "md_tile_blend_f16: every tile must have fewer than 2^31 elements (B=%d, %d x %d, above %d rows, left %d columns, ldc=%d)", B, Th, Tw, Ah, Lw,
               ldc);
  const long n_cur = rows * Tw * ldc, n_above = arows * Tw * ldc, n_left = rows * lcols * ldc;
  MD_CHECK_ARG(!(above && tb_overlap(cur, n_cur, above, n_above)) && !(left && tb_overlap(cur, n_cur, left, n_left)),
               "md_tile_blend_f16: cur overlaps a neighbour");
  int evc = 0, ehc = 0;                                              // the clamped extents; 0 without the neighbour
  if (above) evc = ev < Ah ? (ev < Th ? ev : Th) : (Ah < Th ? Ah : Th);
  if (left) ehc = eh < Lw ? (eh < Tw ? eh : Tw) : (Lw < Tw ? Lw : Tw);
  const tb_args_t a = {(half_t*)cur, evc ? (const half_t*)above : nullptr, ehc ? (const half_t*)left : nullptr, dst, B, Th, Tw, C, ldc, Ah, Lw, evc, ehc,
                       keep_h, keep_w, sB, sC, sY, sX};
  const bool vec = ldc % 4 == 0 && ((uintptr_t)cur % 8) == 0 && ((uintptr_t)above % 8) == 0 && ((uintptr_t)left % 8) == 0;
  const int G = vec ? (C + 3) / 4 : 1;
  const long total = rows * Tw * G;
  const long blocks = (total + TB_THREADS - 1) / TB_THREADS;
  const dim3 grid((unsigned)(blocks < TB_MAX_BLOCKS ? blocks : TB_MAX_BLOCKS)), block(TB_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  if (vec && dst_is_f32)
    hipLaunchKernelGGL((tile_blend_kernel<float, 4>), grid, block, 0, st, a, total, G);
  else if (vec)
    hipLaunchKernelGGL((tile_blend_kernel<half_t, 4>), grid, block, 0, st, a, total, G);
  else if (dst_is_f32)
    hipLaunchKernelGGL((tile_blend_kernel<float, 1>), grid, block, 0, st, a, total, G);
  else
    hipLaunchKernelGGL((tile_blend_kernel<half_t, 1>), grid, block, 0, st, a, total, G);
  MD_CHECK_LAUNCH("md_tile_blend_f16");
  return MD_OK;
}
