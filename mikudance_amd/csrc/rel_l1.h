// C ABI of mikudance_amd/csrc/rel_l1.hip, exported from libmdance_hip.so beside the entry points of include/mdance_hip.h and typed by
// mikudance_amd/_lib.py from its EXTENSION_SIGNATURES table (tests/test_rel_l1_abi_cpu.py holds the three together).  It lives here and not in
// include/mdance_hip.h because that header's set of entry points is fixed at 62 by tests/test_frames_u8_cpu.py.
#pragma once
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The distance of adaptive DeepCache (deep_cache_threshold=): out[0] = sum |a - b|, out[1] = sum |b| over two fp16 operands of rows x C
 * elements, row r of a at a + r lda and of b at b + r ldb (elements; lda, ldb >= C: channel slices of wider NHWC buffers), fp32 terms and
 * fp32 sums, out = 2 fp32 in device memory (never read back by the library).  The caller divides: the relative-L1 criterion of TeaCache
 * (arXiv 2411.19108) between the skip tensor of this step and of the step before.
 * Deterministic: a grid that depends on the shape alone, one partial per workgroup in the workspace, a second launch that adds the partials
 * in a fixed order (csrc/rel_l1.hip states the whole order and the error bound that follows from it); no atomics; every workspace word that
 * is read has been written by the same call.  16-byte loads where C, lda, ldb are multiples of 8 and a, b 16-byte aligned, one element per
 * access otherwise.  NaN / Inf in either operand reach out as NaN / Inf.  a and b may overlap or be the same tensor.
 * rows, C positive with rows C <= 2^40; a, b 2-byte, workspace and out 8-byte aligned; workspace_bytes >= md_rel_l1_workspace_bytes(rows, C)
 * (at most 16 KiB); MD_ERR_ARG otherwise, with nothing launched. */
size_t md_rel_l1_workspace_bytes(int rows, int C);
int md_rel_l1_f16(const void* a, int lda, const void* b, int ldb, int rows, int C, void* workspace, size_t workspace_bytes, void* out,
                  void* stream);

#ifdef __cplusplus
}
#endif
