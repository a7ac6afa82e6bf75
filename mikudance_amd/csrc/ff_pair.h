// Pairs of floats hi + lo (two_sum / fma error terms: about 2^-45 relative) for the kernels whose result is a signed sum that may cancel:
// where it does, plain fp32 weights (2^-24 relative to the OPERANDS) leave more than an fp16 ulp of a result 2^-13 of its operands
// (md_latent_resize_f16, md_tile_blend_f16).  fp32 operations only; host-callable, so that the arithmetic can be checked without a device.
//
// Every rounding is named: p = a * b must be the ROUNDED product both where it is added and where fmaf(a, b, -p) takes its error.  The compiler's
// own fusing of a * b + c (hipcc's default for device code) would hand the addition the exact product and count that error twice, so a file
// that includes this header switches it off for itself (#pragma clang fp contract(off)); the fmaf calls stay fused.
#pragma once

struct ff_t {                                                     // the value h + l, |l| <= ulp(h) / 2
  float h, l;
};

__host__ __device__ __forceinline__ ff_t ff_fast_sum(float a, float b) {    // |a| >= |b| or a == 0
  const float s = a + b;
  return {s, b - (s - a)};
}
__host__ __device__ __forceinline__ ff_t ff_sum(float a, float b) {
  const float s = a + b, bb = s - a;
  return {s, (a - (s - bb)) + (b - bb)};
}
__host__ __device__ __forceinline__ ff_t ff_add(ff_t a, ff_t b) {
  const ff_t s = ff_sum(a.h, b.h);
  return ff_fast_sum(s.h, s.l + (a.l + b.l));
}
__host__ __device__ __forceinline__ ff_t ff_add(ff_t a, float b) {
  const ff_t s = ff_sum(a.h, b);
  return ff_fast_sum(s.h, s.l + a.l);
}
__host__ __device__ __forceinline__ ff_t ff_mul(ff_t a, ff_t b) {
  const float p = a.h * b.h;
  return ff_fast_sum(p, fmaf(a.h, b.h, -p) + (a.h * b.l + a.l * b.h));
}
__host__ __device__ __forceinline__ ff_t ff_mul(ff_t a, float b) {
  const float p = a.h * b;
  return ff_fast_sum(p, fmaf(a.h, b, -p) + a.l * b);
}
