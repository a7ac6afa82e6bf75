// C ABI of mikudance_amd/csrc/color_match.hip, exported from libmdance_hip.so beside the entry points of include/mdance_hip.h and typed by
// mikudance_amd/_lib.py from its EXTENSION_SIGNATURES table (tests/test_rel_l1_abi_cpu.py holds the three together).  It lives here and not in
// include/mdance_hip.h because that header's set of entry points is fixed at 62 by tests/test_frames_u8_cpu.py.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Colour matching of decoded frames (color_match=): the colour moments of every frame, and the per-frame affine colour map in front of the
 * output quantisation.  Both read the source md_frames_u8 reads: fp16, or fp32 with src_is_f32 = 1, element (b, c, y, x) at
 * b sB + c sC + y sY + x sX (elements), 3 channels: the decoders' NHWC image at pixel pitch 3, 4 or 8 (sC = 1, sX = the pitch), a finished NCHW
 * tensor (sX = 1) or any other strided view, one code path.  The displayed colour of a value v is, in fp32 with the product and the sum
 * rounded separately,  s = min(max(0.5f * v + 0.5f, 0), 1)  (a NaN stays a NaN; +-Inf are clamped like every value outside [-1, 1]).
 *
 * md_color_moments: out = B x 9 fp64 in device memory (never read back by the library), per frame over its H W pixels
 *     sum s0, sum s1, sum s2, sum s0^2, sum s1^2, sum s2^2, sum s0 s1, sum s0 s2, sum s1 s2
 * fp32 terms (every one >= 0), fp32 sums inside a workgroup, one partial of 9 fp32 per workgroup in the workspace, and a second launch that
 * adds a frame's partials in fp64.  THE ORDER (csrc/color_match.hip restates it next to the code): a unit is 8 consecutive pixels of a row,
 * a frame has U = H ceil(W / 8) of them and P = ceil(U / 1024) workgroups of 256 threads; unit i of the frame belongs to thread i mod (256 P)
 * of the frame, which takes its iters = ceil(U / (256 P)) <= 4 units in ascending order.  A term passes through at most
 *     7      the 8 pixels of a unit, added in pixel order into a fresh accumulator
 *     iters  the thread's units, in ascending order
 *     6      the 64 lanes of a wave, xor butterfly with offsets 32, 16, ..., 1
 *     3      the 4 wave sums, added in wave order
 * fp32 additions:  d = iters + 16 <= 20  (an addition to the initial 0 is exact and counted all the same).  With at most three roundings in a
 * term (s_i, s_j, their product) and every term >= 0, a sum is within (d + 3) 2^-24 of the exact one, relatively, to first order.  The second launch: one workgroup
 * per frame, thread t adds partials t, t + 256, ... in ascending order, then the same butterfly and the same 4-wave sum, all in fp64.
 * Deterministic: the grid (B P workgroups) depends on the shape alone, no atomics, every workspace word that is read has been written by the
 * same call, two calls give the same bits.  A NaN in the source reaches every sum it is a term of.  Loads: csrc/frame_io.h's rule
 * with 16-byte vectors.
 * B, H, W positive with B H W <= INT_MAX; src aligned to its element, workspace to 4 and out to 8 bytes; workspace_bytes >=
 * md_color_moments_workspace_bytes(B, H, W) = 36 B P (0 for a shape that is refused); MD_ERR_ARG otherwise, with nothing launched. */
size_t md_color_moments_workspace_bytes(int B, int H, int W);
int md_color_moments(const void* src, int src_is_f32, int B, int H, int W, long sB, long sC, long sY, long sX, void* workspace,
                     size_t workspace_bytes, void* out, void* stream);

/* md_color_apply: y = M s + t per pixel, frame b's row-major 3 x 3 matrix M and offset t at coef + 12 b (B x 12 fp32 in device memory,
 * 4-byte aligned), every operation rounded on its own in fp32 (no contraction: numpy float32 reproduces it bit for bit):
 *     y_c = ((t_c + M_c0 s_0) + M_c1 s_1) + M_c2 s_2,  clamped to [0, 1] (a NaN stays a NaN)
 * dst_is_f32 = 0: dst is bytes, (b, y, x, c) at b dB + y dY + 3 x + c with dC = 1 and dX = 3 -- md_frames_u8's destination, its rules for
 *     dB and dY, no alignment asked; the byte is fp32(y * 255) truncated toward zero, 0 for a NaN (md_frames_u8's choice)
 * dst_is_f32 = 1: dst is fp32, 4-byte aligned, (b, c, y, x) at b dB + c dC + y dY + x dX (elements, all four positive): y itself
 * One thread per 4 consecutive pixels of a row; md_frames_u8's loads and byte writer (csrc/frame_io.h), 16-byte stores per channel where dX = 1 and the 4 floats start on a 16-byte boundary (element stores otherwise); 256
 * threads, at most 2048 workgroups, a grid-stride loop past that.  No atomics, no LDS.  Nothing outside the B H rows of the destination is
 * written.  B, H, W positive with B H W <= INT_MAX; MD_ERR_ARG otherwise, with nothing launched. */
int md_color_apply(const void* src, int src_is_f32, const void* coef, void* dst, int dst_is_f32, int B, int H, int W, long sB, long sC, long sY,
                   long sX, long dB, long dC, long dY, long dX, void* stream);

#ifdef __cplusplus
}
#endif
