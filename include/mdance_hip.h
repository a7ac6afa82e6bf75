/* libmdance_hip.so -- C ABI of the MI355X (gfx950) denoising-loop kernels.
 *
 * The reference (Kebii/MikuDance) has NO FFI on this path: every hot-path FLOP is a stock PyTorch/ATen call made
 * from Python.  The boundary is therefore op-level: each entry point below replaces the
 * ATen dispatches of the cited reference call sites (paths relative to the reference repository root).  The
 * reference-side binding is a ctypes stub; mikudance_amd/_lib.py is that stub in this repo.
 *
 * Conventions: all device pointers are raw addresses owned by the caller (PyTorch-ROCm allocates them); nothing is
 * allocated, freed or retained; kernels are enqueued on `stream` (a hipStream_t passed as void*) and the call
 * returns immediately.  Activations are fp16, token-major / NHWC: a (B,H,W,C) image batch IS the row-major matrix
 * [B*H*W][C].  Weights are fp16 [N][K] with K contiguous (nn.Linear layout; 3x3 conv weights as
 * [Cout][ky][kx][Cin]).  Return value: 0 on success, negative on error (md_last_error() has the message, per thread).
 *
 * Threading / devices: entry points may be called concurrently from several host threads on distinct streams, and one
 * process may drive several GPUs (hipSetDevice before the call): the library keeps no per-call state, its one-time kernel
 * attribute setup (> 64 KiB dynamic LDS) is done per device behind an atomic mask, and the MD_* tuning knobs are read from
 * the environment once per process (thread-safe initialisation).  Two calls on the SAME stream are ordered by the stream.
 *
 * Aliasing: outputs must not overlap inputs, with ONE exception that the callers rely on: `residual` may be exactly the
 * output (same pointer, same pitch) of md_gemm_f16 / md_conv3x3*_nhwc_f16 -- every kernel flavour reads a residual element
 * in the thread that later writes the same output element (or, in the streaming kernel, reads whole rows that no workgroup
 * has written yet); a partially overlapping residual is rejected.  md_groupnorm_nhwc_f16 and md_softmax_rows_f16 may run in
 * place (y == x).
 */
#ifndef MDANCE_HIP_H
#define MDANCE_HIP_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MD_ACT_NONE 0
#define MD_ACT_SILU 1
#define MD_ACT_RELU 2
#define MD_ACT_GEGLU 3 /* W rows packed as alternating blocks of 32 'h' rows and 32 'g' rows; C gets N/2 columns */
#define MD_ACT_QUICKGELU 4 /* x * sigmoid(1.702 x): CLIP vision tower MLP (src/pipelines/pipeline_mikudance.py:406-416) */

int md_version(void);
const char* md_last_error(void);

/* C[M,N] = epi(A[M,K] . W[N,K]^T): bias[N], act, rowadd[(m / rows_per_group)][n] (time-embedding broadcast),
 * residual[M,N] (added last), or transpose_out (C is [N][ldc], used for V^T).  K % 64 == 0.
 * act is one of MD_ACT_*: any other value is MD_ERR_ARG with nothing launched (the conv entries likewise, which also refuse
 * MD_ACT_GEGLU).  The transposed store writes columns [0, M) of each of the N rows and leaves columns [M, ldc) untouched.
 * Replaces nn.Linear / 1x1 Conv2d: diffusers Attention.to_q/to_k/to_v/to_out.0 and FeedForward
 * (src/models/attention.py:109-157,323-364), proj_in/proj_out (src/models/transformer_3d.py:66-68,96-98;
 * src/models/transformer_2d.py:152-154,186-188; src/models/motion_module.py:124,146), conv_shortcut and
 * time_emb_proj (src/models/resnet.py:179-181,213-215), TimestepEmbedding (src/models/unet_3d_mix.py:99-102). */
int md_gemm_f16(const void* A, int lda, const void* W, void* C, int ldc, int M, int N, int K, const void* bias,
                const void* residual, int ldr, const void* rowadd, int ldra, int rows_per_group, int act,
                int transpose_out, void* stream);

/* Y = epi(conv3x3(X)) on NHWC, zero padding 1, stride 1|2, upsample=1 folds a nearest-2x upsample into the input
 * addressing.  Cin % 64 == 0 (zero-pad when packing).  Output (B, Hout, Wout, Cout) with row pitch ldy.
 * Replaces InflatedConv3d / Conv2d 3x3: src/models/resnet.py:9-17,71-88,106-120,165-167,194-196;
 * src/models/unet_3d_mix.py:94-96,267-269; src/models/unet_2d_mix.py:321-326; src/models/man_module.py:18-21. */
int md_conv3x3_nhwc_f16(const void* X, const void* W, void* Y, int ldy, int B, int Hin, int Win, int Cin, int Cout,
                        int stride, int upsample, const void* bias, const void* residual, int ldr,
                        const void* rowadd, int ldra, int rows_per_group, int act, void* stream);

/* Same, with pad_lo = 0: the zero padding is (0,1,0,1) (right / bottom only) and stride 2, i.e. F.pad(x, (0,1,0,1)) +
 * Conv2d(3x3, stride 2, padding 0): the downsampler of the third-party AutoencoderKL encoder (diffusers 0.24.0
 * Downsample2D(padding=0)) that src/pipelines/pipeline_mikudance.py:456-549 calls through self.vae.encode. */
int md_conv3x3_pad_nhwc_f16(const void* X, const void* W, void* Y, int ldy, int B, int Hin, int Win, int Cin, int Cout,
                            int stride, int upsample, int pad_lo, const void* bias, const void* residual, int ldr,
                            const void* rowadd, int ldra, int rows_per_group, int act, void* stream);

/* The general form of the two entries above: X may be a channel slice of a wider NHWC tensor (pixel pitch ldx >= Cin elements:
 * the skip connections of the UNets are produced straight into the concat buffer of the up-block resnet that consumes them, so
 * torch.cat([hidden, skip], 1) of src/models/unet_3d_blocks.py:736,877 / unet_2d_blocks.py never runs as a copy), and kw = 1 selects
 * a 3 x 1 filter (taps along H only, K = 3 Cin, stride 1, pad 1): nn.Conv3d(C, C, (3,1,1), padding (1,0,0)) of the third-party
 * AutoencoderKLTemporalDecoder (src/pipelines/pipeline_mikudance.py:132-150) on the (clips, frames, h*w, C) view, ONE launch and one
 * rounding instead of three accumulating GEMMs. */
int md_conv_nhwc_f16(const void* X, int ldx, const void* W, void* Y, int ldy, int B, int Hin, int Win, int Cin, int Cout, int kw,
                     int stride, int upsample, int pad_lo, const void* bias, const void* residual, int ldr, const void* rowadd,
                     int ldra, int rows_per_group, int act, void* stream);

/* In-place softmax(scale * x) over the rows of a row-major fp16 matrix [rows][ldx] (cols valid, cols % 8 == 0).
 * The score matrix of the single 512-channel head of the AutoencoderKL mid-block attention (QK^T and PV run on
 * md_gemm_f16): src/pipelines/pipeline_mikudance.py:115-130 (decode_latents), :456-549 (vae.encode).
 * scale must be positive and finite (the kernel scales the row maximum of x, which is the maximum of scale * x only for scale > 0):
 * MD_ERR_ARG otherwise, with nothing launched. */
int md_softmax_rows_f16(void* x, int ldx, int rows, int cols, float scale, void* stream);

/* GroupNorm(G, eps) [+SiLU] over (B, HW, C) NHWC.  src/models/resnet.py:20-28,220-221,231,237;
 * src/models/transformer_3d.py:60-62,130; src/models/motion_module.py:121-123,164; unet_3d_mix.py:591-592.
 * Alignment (all md_groupnorm_* entries): x, y, gamma and beta must be 16-byte aligned and C % 8 == 0 (the apply sweep loads gamma /
 * beta eight channels at a time); MD_ERR_ARG otherwise.  md_groupnorm_table_f16 reads gamma / beta as scalars but keeps the same rule
 * so that a caller can switch between the fused and the literal pair without re-packing. */
size_t md_groupnorm_workspace_bytes(int B, int HW, int C, int G);
int md_groupnorm_nhwc_f16(const void* x, void* y, const void* gamma, const void* beta, int B, int HW, int C, int G,
                          float eps, int silu, void* workspace, size_t ws_bytes, void* stream);

/* Same with an input pixel pitch ldx >= C (x a channel slice of a wider NHWC tensor; y stays contiguous; in place only if ldx == C). */
int md_groupnorm_ld_nhwc_f16(const void* x, int ldx, void* y, const void* gamma, const void* beta, int B, int HW, int C, int G,
                             float eps, int silu, void* workspace, size_t ws_bytes, void* stream);

/* LayerNorm over rows of C.  add_mode 0: y only.  add_mode 1: y2[row] = y[row] + add[row - add_row_begin] for
 * rows >= add_row_begin (reference-attention bank ADD, src/models/mutual_mix_attention.py:169-170), y2 = y
 * below.  add_mode 2: y2[row] = y[row] + add[(row / rows_per_frame) % frames] (temporal positional encoding on the
 * query input only, src/models/motion_module.py:404-417).  src/models/attention.py:105-107,331-365. */
int md_layernorm_f16(const void* x, void* y, void* y2, const void* gamma, const void* beta, const void* add, int M,
                     int C, float eps, int add_mode, int add_row_begin, int rows_per_frame, int frames, void* stream);

/* Which kernels md_groupnorm_ld_nhwc_f16 (table = 0) / md_groupnorm_table_f16 (table = 1) run, and their launch geometry; no device
 * access, nothing launched; the launchers run the same function.  x_align16: whether x is 16-byte aligned.  Returns
 *   600  two launches: the statistics sweep, then the apply sweep (or the table kernel);
 *   601  three launches: more than 128 slabs per image, one small launch reduces the partial sums in between;
 *   61k / 62k  the one-sweep kernel that keeps an (image, group) in the registers of 256 / 512 threads, k = 1, 2, 4 for its 6 / 12 / 24
 *        sweeps-per-thread instances (611 612 614 622 624; never with table = 1): (C / G) % 4 == 0, C / G <= 256, B * G >= 256, HW <= 1024;
 * or MD_ERR_ARG for what the entries refuse from these arguments (C % 8, G outside 1..64, C % G, ldx < C, ldx % 8, x not 16-byte
 * aligned, C > 8192).  *threads: threads per workgroup; *R: pixel lanes per workgroup; *slab: pixels per workgroup; *nslab: workgroups
 * per image (600 / 601) -- HW and 1 for the one-sweep kernel, whose workgroup owns a whole (image, group).  Any of them may be NULL; all
 * stay untouched on error.  md_groupnorm_workspace_bytes is (B * nslab * G * 2 + B * G * 3) floats of the table = 1 plan. */
int md_groupnorm_plan(int B, int HW, int C, int G, int ldx, int x_align16, int table, int* threads, int* R, int* slab, int* nslab);

/* Which kernel md_layernorm_f16 runs: 700 + MAXC for the kernel instance that holds rows of up to 512 * MAXC channels (701 .. 704), 720
 * the C = 320 kernel, or MD_ERR_ARG as the entry (C % 8, C > 2048).  No device access; the launcher runs the same function. */
int md_layernorm_plan(int M, int C);

/* LayerNorm FOLDED into the Linear that consumes it: C = LayerNorm(A; gamma, beta, eps) . W^T + bias [+ rowadd] computed from the RAW rows
 * of A, the normalised tensor never touching HBM.  The caller folds once per layer (mikudance_amd/packing.py ln_fold):
 *   Wf[n][k] = fp16(gamma[k] W[n][k]),   sc = fp32 [2][N]:  sc[0][n] = sum_k Wf[n][k],  sc[1][n] = sum_k beta[k] W[n][k] + bias[n]
 * and the kernel evaluates rstd_m * (A[m] . Wf[n] - mu_m * sc[0][n]) + sc[1][n] with the exact two-pass (mu, rstd) of each row taken
 * from the rows as they stream through LDS.  rowadd / rows_per_group as in md_gemm_f16 (the motion module's query-only positional
 * encoding as a per-frame row term); act must be MD_ACT_NONE.  Only shapes of the W-stationary streaming kernel exist (K = 320, N a
 * multiple of 320, >= 32768 rows: the 96 x 96 level): md_gemm_ln_plan(M, N, K, act, epi) returns 1 when this entry point has a kernel for
 * the problem (epi as md_gemm_plan), 0 when the caller has to run md_layernorm_f16 + md_gemm_f16 on the unfolded weights;
 * md_gemm_ln_f16 itself fails (MD_ERR_ARG) on anything else -- there is no silent fallback.  Replaces norm2 -> attn2.to_q
 * (src/models/attention.py:131-141,339-347; src/models/mutual_mix_attention.py:203-263) and norms[i] -> to_q / to_k / to_v of the
 * motion module (src/models/motion_module.py:245-268, 364-439). */
int md_gemm_ln_plan(int M, int N, int K, int act, int epi);
int md_gemm_ln_f16(const void* A, int lda, const void* Wf, const float* sc, void* C, int ldc, int M, int N, int K, float eps,
                   const void* rowadd, int ldra, int rows_per_group, int act, void* stream);

/* GroupNorm in front of a Linear / 1x1 conv without materialising the normalised tensor.  md_groupnorm_table_f16 runs the statistics
 * sweep only and writes table = fp32 [B][2][C]: scale[b][c] = rstd * gamma[c], shift[b][c] = beta[c] - mean * scale;
 * md_gemm_affine_f16 computes C = (A * scale[image] + shift[image], rounded to fp16) . W^T + bias, image = row / rows_per_image,
 * applying the affine to the rows as they stream through LDS: bit-identical to md_groupnorm_ld_nhwc_f16 (silu = 0, two-sweep form)
 * followed by md_gemm_f16.  A may be a channel slice (lda >= K).  md_gemm_affine_plan: 1 when the kernel exists for the shape (K = 320,
 * N a multiple of 320, >= 32768 rows, rows_per_image % 16 == 0).  Replaces norm -> proj_in of Transformer3DModel / Transformer2DModel
 * (src/models/transformer_3d.py:60-68,121-137; src/models/transformer_2d.py:296-321) and of the motion module's
 * TemporalTransformer3DModel (src/models/motion_module.py:121-124,159-170). */
int md_groupnorm_table_f16(const void* x, int ldx, const void* gamma, const void* beta, int B, int HW, int C, int G, float eps,
                           float* table, void* workspace, size_t ws_bytes, void* stream);
int md_gemm_affine_plan(int M, int N, int K, int rows_per_image);
int md_gemm_affine_f16(const void* A, int lda, const float* table, int rows_per_image, const void* W, void* C, int ldc, int M, int N,
                       int K, const void* bias, void* stream);

/* MAN: y = InstanceNorm(x) * (1 + gamma) + beta; gamma_beta is (B, HW, 2C) = [gamma | beta].
 * src/models/man_module.py:23-33. */
int md_instnorm_spade_f16(const void* x, const void* gamma_beta, void* y, int B, int HW, int C, float eps,
                          void* stream);

int md_instnorm_spade_ld_f16(const void* x, int ldx, const void* gamma_beta, void* y, int B, int HW, int C, float eps,
                             void* stream);                      /* x with a pixel pitch ldx >= C (a channel slice) */

/* O = softmax(Q K^T * scale) V per (batch, head); Vt is V transposed ([H*D][ldvt], md_gemm_f16 transpose_out);
 * kv_index (device int[B], may be NULL) maps a query batch to its K/V batch; kv_stride = tokens between K/V batches.
 * D in {8,16,32,40,64,80,160}.  Replaces F.scaled_dot_product_attention under diffusers AttnProcessor2_0 as
 * called at src/models/mutual_mix_attention.py:141-148,173-200,213-220,257-263.
 * The pad: with ldvt, kv_stride multiples of 8, Vt 16-byte aligned and roundup8(Lk) <= kv_stride (the fast kernels), rows [Lk, roundup8(Lk))
 * of every K batch and the same columns of Vt must be readable; the V^T columns are fetched.  Pad contents may be any FINITE values and do
 * not influence the result (the scores of keys >= Lk are masked, P is exactly +0 there and 0 x finite = 0: two runs that differ only in
 * the pad give the same bits, tests/test_attention_flavours_gpu.py).  Non-finite pad values are not supported: 0 x Inf is NaN in the
 * matrix core.  The pipeline's pad is exact zeros (zero context rows through a bias-free to_v: V = 0 . W).
 * The generic kernel (plan 400: any of those conditions missing, e.g. kv_stride = Lk = 257 with ldvt = 264 as the CLIP vision tower calls
 * it) has NO pad: it reads rows [0, Lk) of every K batch and columns [kb kv_stride, kb kv_stride + Lk) of Vt and nothing else -- whole
 * 16-byte chunks only where all 8 keys are < Lk, single elements under `key < Lk` otherwise.  Columns of Vt beyond Lk (the slack of a
 * row pitch ldvt > kv_stride that md_gemm_f16's transposed store leaves unwritten) may hold anything, NaN and Inf included, and need
 * not be initialised: a NaN-filled slack gives the bits of a zero one (tests/test_attention_flavours_gpu.py). */
int md_attention_fwd_f16(const void* Q, int ldq, const void* K, int ldk, const void* Vt, int ldvt, void* O, int ldo,
                         const int* kv_index, int B, int H, int D, int Lq, int Lk, int kv_stride, float scale,
                         void* stream);

/* Which kernel md_attention_fwd_f16 selects; no device access, nothing launched.  vt_align16: whether Vt is 16-byte aligned (the other
 * operands are taken as valid: the choice does not depend on them).  Returns 400 the generic kernel (ldvt % 8, kv_stride % 8, Vt not
 * 16-byte aligned or roundup8(Lk) > kv_stride), 414 / 418 the DMA ring kernel with 4 / 8 waves per workgroup (8: D <= 40 and Lq >= 1024),
 * 420 the kernel that keeps K / V^T of a (batch, head) pair resident in LDS (D = 40, Lq >= 2048, 8 <= Lk <= 320), or MD_ERR_ARG
 * (unsupported D, empty problem, kv_stride < Lk).  Pins the dispatch in CPU tests and lets a GPU test state which kernel it runs. */
int md_attention_plan(int D, int Lq, int Lk, int kv_stride, int ldvt, int vt_align16);

/* Attention over FRAMES for every (clip-half, pixel, head); rows are (b*F + frame)*HW + pixel.  F <= 32.  O must not overlap Q, K or V
 * (column-sliced siblings of one wider row-major buffer, e.g. q | k | v of one GEMM, are fine): checked, MD_ERR_ARG otherwise.
 * src/models/motion_module.py:364-439 (VersatileAttention, Temporal mode). */
int md_temporal_attention_fwd_f16(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, void* O,
                                  int ldo, int NB, int F, int HW, int H, int D, float scale, void* stream);

/* Which kernel and workgroup geometry md_temporal_attention_fwd_f16 selects; no device access, nothing launched.  aligned16: whether Q, K,
 * V and O are all 16-byte aligned.  Returns 500 the lane-per-query kernel (every D other than 40 / 80 / 160, or an operand that is not
 * 16-byte aligned), 511 / 512 the matrix-core kernel with one / two 16-frame blocks (F <= 16 / F <= 32), or MD_ERR_ARG for what the
 * entry point refuses (F outside 1..32, D no positive multiple of 8, H not a power of two <= 8, F*D too large for LDS).  *hg / *pb
 * receive the heads and pixels one workgroup owns (either may be NULL; untouched on error).  The launcher runs the same function. */
int md_temporal_attention_plan(int NB, int F, int HW, int H, int D, int aligned16, int* hg, int* pb);

/* Layout packing at the API boundary (any strided fp16/fp32 source -> NHWC fp16 with zero channel padding and
 * nearest resize (Hin,Win)->(Ho,Wo); and back).  src/models/unet_2d_mix.py:1208-1210 (22-channel split),
 * src/models/man_module.py:27 (nearest resize), einops rearranges of src/models/resnet.py:12-16. */
int md_pack_nhwc_f16(const void* src, int src_is_f32, void* dst, int N, int F, long sB, long sF, long sC, long sY,
                     long sX, int c_begin, int c_count, int Cpad, int Ho, int Wo, int Hin, int Win, void* stream);
int md_unpack_nhwc_f16(const void* src, int ldc, void* dst, int dst_is_f32, int N, int F, long sB, long sF, long sC,
                       long sY, long sX, int C, int Ho, int Wo, void* stream);

/* torch.cat([hidden, skip], dim=channel) on token-major matrices.  src/models/unet_3d_blocks.py:736,877. */
int md_concat_channels_f16(const void* a, int Ca, const void* b, int Cb, void* out, long M, void* stream);

/* noise_pred[:, :, window] += pred; counter[window] += 1.  src/pipelines/pipeline_mikudance.py:662-664. */
int md_window_accumulate(const void* pred, void* noise_sum, void* counter, const int* window, int f, int Ftot, int HW,
                         int halves, void* stream);

/* Weighted window fusion (context_fuse="pyramid"; the triangular per-slot weights of diffusers' FreeNoise weighting_scheme="pyramid" and
 * AnimateDiff-Evolved's pyramid fuse): noise_pred[:, :, window[i]] += weights[i] * pred[:, :, i]; counter[window[i]] += weights[i].
 * weights: f fp32 in device memory, one per slot, already divided by the frame's total weight over every window of the step, so that
 * noise_sum ends as the weighted mean and counter as 1 up to rounding; every consumer of md_window_accumulate's buffers works unchanged.
 * Buffers and slot rule as md_window_accumulate (slots unique or -1 = skipped; a slot >= Ftot is skipped too).  fp32 arithmetic, the
 * product and the sum rounded separately (no fma), so a window's share is the same number on every rank of a window-parallel run; with
 * every weight 1.0 the result is md_window_accumulate's bit for bit.  No pointer may be NULL; pred 8-byte, noise_sum 16-byte, counter /
 * window / weights 4-byte aligned; f > 0, Ftot >= f, HW > 0, halves 1 or 2; MD_ERR_ARG otherwise.
 * The place of src/pipelines/pipeline_mikudance.py:662-664 when the caller asks for weighted fusion (an addition). */
int md_window_accumulate_weighted(const void* pred, void* noise_sum, void* counter, const int* window, const float* weights, int f,
                                  int Ftot, int HW, int halves, void* stream);

/* ---- The step family: md_cfg_<sampler>_step<guide>, 13 entries ---------------------------------------------------------------------
 * (noise_pred / counter) -> guided v -> one step of the sampler, the fp16 latents [Ftot][HW][4] updated in place (fp32 arithmetic, one
 * rounding).  src/pipelines/pipeline_mikudance.py:670-678 (CFG, then self.scheduler.step; :45-52 types the scheduler).
 *
 * Every entry takes latents, noise_sum (fp32 [halves][Ftot][HW][4], the window sums, planes [u, c] under CFG), counter (fp32 [Ftot]), Ftot, HW,
 * halves and guidance.  halves == 2: inv = 1 / counter, u = sum_u inv, c = sum_c inv, v = u + guidance (c - u).  halves == 1: v is the window SUM
 * and neither the counter nor a second plane is read.  latents / noise_sum (and counter when halves == 2) must not be NULL, Ftot > 0, HW > 0,
 * halves 1 or 2, guidance and every coefficient finite; MD_ERR_ARG otherwise, with nothing launched and the latents untouched.
 *
 * What the sampler adds
 *   ddim       alpha_t, alpha_prev (and eta, variance_noise in every entry but md_cfg_ddim_step, which is eta == 0): diffusers DDIMScheduler.step,
 *              v-prediction.  sigma_t = eta sqrt((1 - a_prev) / (1 - a_t) (1 - a_t / a_prev)), x' = sqrt(a_prev) x0 + sqrt(1 - a_prev - sigma_t^2)
 *              eps + sigma_t z, z = variance_noise, fp16, laid out like the latents: the caller draws it from ITS generator (`eta` of
 *              MikuDanceVideoPipeline.__call__, pipeline_mikudance.py:152-171,375).  eta >= 0; variance_noise not NULL when eta != 0.
 *              One element per access: the buffers need their natural alignment only (md_cfg_ddim_step_apg: as multistep).
 *   multistep  history, variance_noise, alpha_s, sigma_s, c_x, c_m0, c_m1, c_z: one DPM-Solver++ update (orders 1 / 2, ODE or SDE),
 *              m0 = alpha_s x - sigma_s v, x' = c_x x + c_m0 m0 + c_m1 m1 + c_z z, with m1 = history (fp32 [Ftot][HW][4], the previous step's m0)
 *              read only when c_m1 != 0 and then overwritten with m0.  The coefficients are DPMSolverMultistepScheduler.multistep_coefficients;
 *              variance_noise may be NULL when c_z == 0.  One pixel per access: latents / variance_noise 8-byte, noise_sum / history 16-byte aligned.
 *   unipc      state, row: the corrector of the step that produced these latents and the predictor to the next point in ONE pass per pixel (Zhao et
 *              al., arXiv 2302.04867; diffusers UniPCMultistepScheduler, data prediction, orders 1 - 3; not among the reference's schedulers):
 *                m_t = alpha_s x - sigma_s v
 *                x^c = cc_x x_last + cc_m m_t + cc_0 H0 + cc_1 H1 + cc_2 H2       corrector on; off: x^c = x
 *                x'  = pc_x x^c + pc_m m_t + pc_0 H0 + pc_1 H1                    -> latents
 *                x_last <- x^c;  H0 <- m_t;  H1 <- H0;  H2 <- H1
 *              state: fp32 [4][Ftot][HW][4], the planes x_last, H0, H1, H2, kept by the caller between steps.  A plane is read only where one of
 *              its weights is non-zero (x_last only with the corrector on) and only a plane that was read moves down a slot: a first step
 *              (corrector off, pc_0 = pc_1 = 0) may be given uninitialised memory.  row: 12 floats in HOST memory, read before the call returns:
 *              alpha_s, sigma_s, cc_x, cc_m, cc_0, cc_1, cc_2, pc_x, pc_m, pc_0, pc_1 and the corrector flag (0 or 1), as
 *              UniPCMultistepScheduler.unipc_coefficients gives them.  Latents 8-byte, noise_sum / state 16-byte, counter 4-byte aligned.
 *
 * What the guide adds
 *   _scaled    vscale: v is multiplied by *vscale, the out_scale of md_cfg_guidance_rescale, read on the device (diffusers rescale_noise_cfg
 *              followed by scheduler.step; arXiv 2305.08891 section 3.4).  halves must be 2; vscale 4-byte aligned.
 *   _apg       momentum_buf, coef: v_g = c - (guidance - 1) (S m - K D_c) / s in place of v, D_c = a x - s c, (S, K) = coef[frame], m = momentum_buf
 *              as md_cfg_apg_prepare left them for THIS step (a, s: sqrt(alpha_t), sqrt(1 - alpha_t) for ddim; alpha_s, sigma_s of multistep and
 *              of unipc's row; history / state receive alpha_s x - sigma_s v_g).  With eta = 1, norm_threshold = 0, momentum = 0 at prepare this
 *              is u + guidance (c - u) up to rounding.  halves must be 2, s > 0 (alpha_t in [0, 1)); momentum_buf 16-byte, coef 4-byte aligned.
 *   _pag       perturbed_sum, pag_scale: perturbed-attention guidance (Ahn et al., arXiv 2403.17377; diffusers PAGMixin), v + pag_scale inv
 *              (sum_c - sum_p), inv as above (1 without CFG: c + s (c - p) on the sums), sum_c the conditional plane of noise_sum (plane
 *              halves - 1) and sum_p = perturbed_sum, fp32 [Ftot][HW][4], the prediction of the conditional evaluation whose selected self-attention
 *              maps are the identity, accumulated over the windows like the other planes.  pag_scale == 0 gives the bits of the plain entry where
 *              the planes are finite (0 * Inf is NaN).  halves 1 or 2; pag_scale finite and >= 0; perturbed_sum aligned like noise_sum
 *              (ddim: 4-byte, and latents / variance_noise 2-byte, counter 4-byte). */
int md_cfg_ddim_step(void* latents, const void* noise_sum, const void* counter, int Ftot, int HW, int halves,
                     float guidance, float alpha_t, float alpha_prev, void* stream);
int md_cfg_ddim_step_eta(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, int Ftot, int HW,
                         int halves, float guidance, float alpha_t, float alpha_prev, float eta, void* stream);
int md_cfg_ddim_step_scaled(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, const float* vscale, int Ftot,
                            int HW, int halves, float guidance, float alpha_t, float alpha_prev, float eta, void* stream);
int md_cfg_ddim_step_apg(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, const void* momentum_buf,
                         const float* coef, int Ftot, int HW, int halves, float guidance, float alpha_t, float alpha_prev, float eta, void* stream);
int md_cfg_ddim_step_pag(void* latents, const void* noise_sum, const void* counter, const void* variance_noise, const void* perturbed_sum, int Ftot,
                         int HW, int halves, float guidance, float pag_scale, float alpha_t, float alpha_prev, float eta, void* stream);
int md_cfg_multistep_step(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise, int Ftot,
                          int HW, int halves, float guidance, float alpha_s, float sigma_s, float c_x, float c_m0, float c_m1, float c_z,
                          void* stream);
int md_cfg_multistep_step_scaled(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise,
                                 const float* vscale, int Ftot, int HW, int halves, float guidance, float alpha_s, float sigma_s, float c_x,
                                 float c_m0, float c_m1, float c_z, void* stream);
int md_cfg_multistep_step_apg(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise,
                              const void* momentum_buf, const float* coef, int Ftot, int HW, int halves, float guidance, float alpha_s,
                              float sigma_s, float c_x, float c_m0, float c_m1, float c_z, void* stream);
int md_cfg_multistep_step_pag(void* latents, const void* noise_sum, const void* counter, void* history, const void* variance_noise,
                              const void* perturbed_sum, int Ftot, int HW, int halves, float guidance, float pag_scale, float alpha_s,
                              float sigma_s, float c_x, float c_m0, float c_m1, float c_z, void* stream);
int md_cfg_unipc_step(void* latents, const void* noise_sum, const void* counter, void* state, int Ftot, int HW, int halves, float guidance,
                      const float* row, void* stream);
int md_cfg_unipc_step_scaled(void* latents, const void* noise_sum, const void* counter, void* state, const float* vscale, int Ftot, int HW,
                             int halves, float guidance, const float* row, void* stream);
int md_cfg_unipc_step_apg(void* latents, const void* noise_sum, const void* counter, void* state, const void* momentum_buf, const float* coef,
                          int Ftot, int HW, int halves, float guidance, const float* row, void* stream);
int md_cfg_unipc_step_pag(void* latents, const void* noise_sum, const void* counter, void* state, const void* perturbed_sum, int Ftot, int HW,
                          int halves, float guidance, float pag_scale, const float* row, void* stream);

/* Guidance rescale (rescaled classifier-free guidance, Lin et al. "Common Diffusion Noise Schedules and Sample Steps are Flawed",
 * arXiv 2305.08891 section 3.4; diffusers rescale_noise_cfg), applied to the window-averaged guided output between
 * src/pipelines/pipeline_mikudance.py:670-674 (CFG) and :678 (scheduler.step):
 *   c = noise_sum[1] / counter, v = u + guidance (c - u) formed by the step kernels' own device function, std over ALL Ftot HW 4 elements,
 *   out_scale[0] = 1 - phi + phi std(c) / std(v), one fp32 in device memory (never read back by the library).
 * One deviation from diffusers: std(v) == 0 gives out_scale = 1 (v left unscaled) where diffusers divides by zero; NaN / Inf inputs
 * propagate as they would in the formula.  Deterministic (fixed grid, fixed per-workgroup slices, fixed combine order, no atomics): two
 * calls on the same inputs give the same bits.  halves must be 2, 0 <= phi <= 1, guidance finite; noise_sum 16-byte, workspace 8-byte,
 * counter / out_scale 4-byte aligned; workspace_bytes >= md_cfg_rescale_workspace_bytes(Ftot, HW) (at most 16 KiB).  MD_ERR_ARG otherwise. */
size_t md_cfg_rescale_workspace_bytes(int Ftot, int HW);
int md_cfg_guidance_rescale(const void* noise_sum, const void* counter, int Ftot, int HW, int halves, float guidance, float phi, void* workspace,
                            size_t workspace_bytes, void* out_scale, void* stream);

/* Adaptive projected guidance (APG; Sadat, Hilliges, Weber, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion
 * Models", arXiv 2410.02416, Algorithm 1; diffusers AdaptiveProjectedGuidance), applied to the window-averaged halves between
 * src/pipelines/pipeline_mikudance.py:670-674 (CFG) and :678 (scheduler.step).  It acts on the data prediction, and the statistics are
 * taken PER FRAME over that frame's HW 4 elements (diffusers reduces over every non-batch dimension, i.e. the whole clip).  With
 * a = alpha_s = sqrt(abar_t), s = sigma_s = sqrt(1 - abar_t), x the latents, u = noise_sum[0] / counter, c = noise_sum[1] / counter:
 *   D_c = a x - s c;   m = s (u - c) + momentum m_prev          momentum_buf [Ftot][HW][4] fp32, updated in place; momentum == 0 never
 *                                                               reads it (it may hold NaN then)
 *   N2 = sum m^2, P = sum m D_c, Q = sum D_c^2                  per frame, accumulated in fp64 in a fixed order
 *   S = norm_threshold == 0 || N2 == 0 ? 1 : min(1, norm_threshold / sqrt(N2));   proj = Q == 0 ? 0 : P / Q
 *   coef[fr] = (S, (1 - eta) S proj)                            [Ftot][2] fp32 in device memory (never read back by the library)
 * Deterministic (a fixed number of workgroups per frame over fixed slices, fixed combine order, no atomics): two calls on the same inputs
 * give the same bits.  halves must be 2; momentum finite in (-1, 1), eta in [0, 1], norm_threshold >= 0, alpha_s / sigma_s finite; no
 * pointer may be NULL; latents 8-byte, noise_sum / momentum_buf 16-byte, workspace 8-byte, counter / coef 4-byte aligned;
 * workspace_bytes >= md_cfg_apg_workspace_bytes(Ftot, HW) (384 bytes per frame at most).  MD_ERR_ARG otherwise, with nothing launched. */
size_t md_cfg_apg_workspace_bytes(int Ftot, int HW);
int md_cfg_apg_prepare(const void* latents, const void* noise_sum, const void* counter, void* momentum_buf, int Ftot, int HW, int halves,
                       float alpha_s, float sigma_s, float momentum, float eta, float norm_threshold, void* workspace, size_t workspace_bytes,
                       void* coef, void* stream);

/* The unconditional plane of a sampling step that evaluated the conditional half only (guidance_interval= after Kynkaanniemi et al.,
 * "Applying Guidance in a Limited Interval", arXiv 2404.07724; uncond_cache_interval= after the CFG cache of FasterCache, arXiv 2410.19355,
 * the idea only): an opt-in approximation, between src/pipelines/pipeline_mikudance.py:662-668 (the windows) and :670-678 (CFG + step).
 * noise_sum: the fp32 accumulator [2][Ftot][HW][4] with planes [u, c] as the halves == 2 step entries read it; counter: fp32 [Ftot];
 * delta: fp32 [Ftot][HW][4], kept by the caller between steps.
 *   mode 0 (store):    delta = c_sum / cnt - u_sum / cnt per frame with that frame's counter; noise_sum is not written
 *   mode 1 (restore):  u_sum = c_sum - scale delta cnt; writes the u plane only.  scale 1: the step kernels then see c - u = delta, so their
 *                      u + g (c - u) is c + (g - 1) delta.  scale 0 (no guidance at this step): the product is not formed, delta is not
 *                      read and may be NULL, u_sum = c_sum bit for bit, so the guided v is exactly the conditional mean
 * fp32, each operation rounded on its own (no fma), in this order -- store: inv = 1 / cnt, u = u_sum inv, c = c_sum inv (the step kernels'
 * own u and c), delta = c - u; restore: t = delta cnt, t = scale t, u_sum = c_sum - t.  Every rank of a window-parallel run, holding the
 * same planes after the all-reduce, gets the same bits.  Deterministic, no atomics.  A frame whose counter is 0 is NaN to the step kernels
 * (0 * (1 / 0)) and gets no special case here either: store writes NaN, restore with scale != 0 hands it on.
 * NULL noise_sum / counter, NULL delta unless mode 1 with scale == 0, Ftot <= 0, HW <= 0, mode not 0 or 1, a non-finite scale, noise_sum or
 * delta not 16-byte or counter not 4-byte aligned: MD_ERR_ARG, with nothing launched and every buffer untouched. */
int md_cfg_uncond_cache(void* noise_sum, const void* counter, void* delta, int Ftot, int HW, int mode, float scale, void* stream);

/* Forward noising of a clean latent, the start of video-to-video sampling (`strength` < 1): latents = fp16(a x0 + b latents), computed in
 * fp32, in place, over n fp16 elements.  latents holds the N(0, 1) noise on entry; x0 is the clean VAE latent (already scaled by 0.18215),
 * both packed to the (F, h*w, 4) layout of md_pack_nhwc_f16.  a = sqrt(abar_t), b = sqrt(1 - abar_t) of the first kept timestep, computed by
 * the caller in float64.  Restates diffusers DDIMScheduler.add_noise as the img2img pipelines' prepare_latents call it.  a == 0 never reads
 * x0: the output is then exactly b * noise even where x0 holds Inf or NaN (t = 999 of the zero-terminal-SNR table has abar = 0, so strength
 * 1.0 starts from the noise itself).  n > 0, a and b finite and >= 0, both pointers 2-byte aligned; MD_ERR_ARG otherwise. */
int md_add_noise_f16(void* latents, const void* x0, long n, float a, float b, void* stream);

/* FreeInit noise re-initialisation (Wu et al., arXiv 2312.07537; diffusers FreeInitMixin._apply_free_init): between two sampling passes
 * the result x0 is re-noised to the last training timestep and only its low spatio-temporal frequencies are kept; the high ones come from
 * the fresh draw z.  Per channel, with 3-D transforms over (F, H, W):
 *   out = fp16( z + IDFT3( lpf * DFT3( a x0 + b noise0 - z ) ) )
 * which equals diffusers' real(ifftn(ifftshift(fftshift(fftn(a x0 + b noise0)) LPF + fftshift(fftn(z)) (1 - LPF)))) when lpf is the
 * unshifted table made symmetric under k -> -k (mikudance_amd/free_init.py: freq_filter); the kernel itself takes ANY real table.
 * out, x0, noise0, z: contiguous (F, H, W, 4) fp16 in the layout of md_pack_nhwc_f16, 8-byte aligned; out may alias x0.  lpf: (F, H, W)
 * fp32 in unshifted (fftn) order, 4-byte aligned.  a = sqrt(abar_T), b = sqrt(1 - abar_T) of the last training timestep, from the caller
 * in float64.  a == 0 never reads x0 (the rule of md_add_noise_f16).  All arithmetic is fp32 (dense separable DFT, twiddles from a
 * table of n entries per axis indexed by (j k) mod n), ONE rounding to fp16 on the way out; deterministic: two calls give the same bits.
 * md_free_init_plan: 1 when there is a kernel for the clip (1 <= F, H, W <= 256, every length, not only powers of two), else 0.
 * workspace: 16-byte aligned, workspace_bytes >= md_free_init_workspace_bytes(F, H, W) (6 KiB + 32 bytes per pixel; 0 without a kernel).
 * A shape without a kernel, a NULL pointer, a misaligned pointer, a or b negative or not finite, a short workspace: MD_ERR_ARG, nothing
 * launched. */
int md_free_init_plan(int F, int H, int W);
size_t md_free_init_workspace_bytes(int F, int H, int W);
int md_free_init_mix_f16(void* out, const void* x0, const void* noise0, const void* z, const float* lpf, int F, int H, int W, float a, float b,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Token downsampling of the K / V source of spatial self-attention (ToDo: Token Downsampling, Smith et al., arXiv 2402.13573; the
 * pipeline's kv_downsample=): Q keeps every token, to_k / to_v read the token grid reduced by s per axis.
 * x: [B*Hh*Ww][C] fp16 row-major and contiguous, the tokens of B frames; y: [B*out_stride][C].  With Ho = Hh / s, Wo = Ww / s (integer
 * division: a last row / column that does not fill a block is dropped) and Lk = Ho*Wo, frame b writes rows b*out_stride + oy*Wo + ox:
 *   mode 0 (nearest, the paper's): y = x[b, oy*s, ox*s], a copy: torch F.interpolate(scale_factor=1/s, mode="nearest") on the grid
 *   mode 1 (mean): the s x s block at (oy*s, ox*s), added in fp32 in the order (dy, dx) ascending, times fp32(1 / s^2), rounded ONCE to
 *                  fp16: torch F.avg_pool2d(kernel_size=s, stride=s)
 * Rows [Lk, out_stride) of every frame are written as exact +0: the pad md_attention_fwd_f16 documents, so y goes through the bias-free
 * to_k / to_v and into that entry with kv_stride = out_stride.  Nothing outside the B*out_stride rows of y is written.  16-byte loads and
 * stores, no atomics: two calls give the same bits.
 * s in 2..8, mode 0 or 1, C % 8 == 0, Ho >= 1 and Wo >= 1, out_stride >= Lk and out_stride % 8 == 0, x and y not NULL, 16-byte aligned
 * and not overlapping; MD_ERR_ARG otherwise, with nothing launched. */
int md_token_pool_f16(const void* x, void* y, int B, int Hh, int Ww, int C, int s, int mode, int out_stride, void* stream);

/* Query blur of smoothed-energy guidance (SEG, Hong, arXiv 2408.00760; the pipeline's seg_scale=): the queries of the selected
 * self-attention blocks are filtered over the token grid (TransformerBlock.forward(seg=), through ops.token_blur).
 * x: [B*Hh*Ww][C] fp16 row-major and contiguous, the tokens of B frames, row = (b*Hh + y)*Ww + x (the layout of md_token_pool_f16); y: the
 * same shape.  Every channel is filtered on its own.
 * md_token_blur_f16: separable filter with reflect padding (the official gaussian_blur_2d, taken per axis).  wx: kx fp32 taps along the
 *   grid's x axis, wy: ky taps along y, device tables made by the caller (ops.token_blur: w_j ~ exp(-(j/sigma)^2/2), j = -r..r, float64,
 *   normalised, rounded once).  Output position p adds tap j = 0..k-1 in ascending order, tap j reading position reflect(p + j - k/2) with
 *   reflect(i) = -i for i < 0 and 2(n-1) - i for i >= n (torch "reflect": the edge is not repeated).  First x -> workspace along x, then
 *   workspace -> y along y: fp32 accumulation and an fp32 intermediate, ONE rounding to fp16.  A one-tap filter of weight 1 returns x bit
 *   for bit.  kx, ky odd, 1 <= kx <= Ww + 1, 1 <= ky <= Hh + 1; Hh, Ww <= 224 (a line is staged in 64 KiB of LDS).
 * md_token_mean_f16: sigma = infinity, the reference's inf_blur: every token of frame b becomes that frame's per-channel mean over its L
 *   tokens (fp32 sums in a fixed order, times fp32(1/L), one rounding).  It is not the limit of the reflect-padded filter.
 * workspace: md_token_blur_workspace_bytes(B, Hh, Ww, C) bytes (B*Hh*Ww*C*4; the mean, with Hh*Ww = L, needs no more), 16-byte aligned, not
 * overlapping x or y.  No atomics: two calls give the same bits.  Nothing outside the B*Hh*Ww rows of y is written.
 * C % 8 == 0, all sizes positive, x / y / workspace / tables not NULL, 16-byte aligned, x and y not overlapping; MD_ERR_ARG otherwise, with
 * nothing launched and y untouched. */
size_t md_token_blur_workspace_bytes(int B, int Hh, int Ww, int C);
int md_token_blur_f16(const void* x, void* y, int B, int Hh, int Ww, int C, const float* wy, int ky, const float* wx, int kx, void* workspace,
                      void* stream);
int md_token_mean_f16(const void* x, void* y, int B, int L, int C, void* workspace, void* stream);

/* Shifted-tile reorder for tiled spatial self-attention (MSW-MSA of HiDiffusion, Zhang et al., arXiv 2311.17528; the pipeline's
 * tile_attention=): every frame's Hh x Ww token grid is cut into t x t tiles of th x tw tokens, th = Hh / t, tw = Ww / t, Lt = th*tw, after
 * a cyclic shift by (sy, sx); every tile is then one batch item of md_attention_fwd_f16 (B*t*t items of Lt tokens).
 * Frame-major: [B*Hh*Ww][C] fp16 row-major and contiguous, row = (b*Hh + yy)*Ww + xx (the layout of md_token_pool_f16).
 * Tile-major:  [B*t*t*tile_stride][C]; tile (b, j, i) with j, i < t is batch item (b*t + j)*t + i and its row r*tw + c holds the token
 *              x[b, (j*th + r + sy) mod Hh, (i*tw + c + sx) mod Ww]: torch.roll(grid, (-sy, -sx), (1, 2)) followed by a plain partition.
 * inverse = 0: x frame-major -> y tile-major.  Rows [Lt, tile_stride) of every tile are written as exact +0: the pad md_attention_fwd_f16
 *              documents (the contract of md_token_pool_f16).  tile_stride = Lt for a Q operand; the caller rounds up to a multiple of 8 for
 *              K / V where Lt is none.
 * inverse = 1: x tile-major -> y frame-major, the exact inverse permutation.  The pad rows of x are never read.
 * The wrap-around of a shifted tile is not masked (the paper's code does not mask it either): tokens of opposite frame edges may share a
 * tile.  A copy: every bit pattern (-0, subnormals, NaN payloads) survives; 16-byte loads and stores, no atomics: two calls give the same
 * bits.  Nothing outside the rows of y named above is written.
 * t in 2..8, Hh % t == 0 and Ww % t == 0, 0 <= sy < Hh, 0 <= sx < Ww, tile_stride >= Lt, inverse 0 or 1, C % 8 == 0, x and y not NULL,
 * 16-byte aligned and not overlapping; MD_ERR_ARG otherwise, with nothing launched and y untouched. */
int md_token_tile_f16(const void* x, void* y, int B, int Hh, int Ww, int C, int t, int sy, int sx, int tile_stride, int inverse, void* stream);

/* Resampling of the packed latents for two-pass high-resolution sampling (the pipeline's hires_scale=): the clip sampled at the low size is
 * enlarged to the target size, re-noised by md_add_noise_f16, and the tail of the schedule runs on it.
 * x: (F, Hi, Wi, 4) fp16, the loop's packed latent layout (md_pack_nhwc_f16 with cpad = 4: 8 bytes per pixel); y: (F, Ho, Wo, 4) fp16; both
 * contiguous.  mode 0 nearest-exact, 1 bilinear, 2 bicubic (A = -0.75), each as torch.nn.functional.interpolate(x, size=(Ho, Wo), mode=...,
 * align_corners=False, antialias=False) per frame and channel: output o of an axis with ni inputs and no outputs sits at the source coordinate
 * (o + 0.5) ni / no - 0.5; nearest-exact reads index floor((o + 0.5) ni / no), clamped to ni - 1; bilinear clamps the coordinate at 0 and
 * blends floor and floor + 1 (clamped) by the fraction; bicubic blends the four taps floor - 1 .. floor + 2, their indices clamped to the border.
 * Any ratio, up or down, the two axes independent.  NO antialiasing on the way down: a ratio below 1 skips input pixels (aliasing), exactly
 * like antialias=False.
 * fp32 operations, ONE rounding to fp16 at the store.  Floor and fraction come from the integer division ((2 o + 1) ni - no) / (2 no), and the
 * fraction, the weights and the sums are carried as pairs of floats, so a value that cancels to little is still within an fp16 ulp of the
 * float64 result.  nearest-exact is a copy; a size-preserving call returns x (weights exactly 0 and 1; the sign of a zero may change).
 * Non-finite inputs give non-finite outputs (0 * Inf, as in torch).  One thread per output pixel, 8-byte loads and stores, no atomics: two
 * calls give the same bits.  Nothing outside the F*Ho*Wo pixels of y is written.
 * All sizes positive, F*Hi*Wi and F*Ho*Wo within int, mode 0..2, x and y not NULL, 8-byte aligned and not overlapping; MD_ERR_ARG otherwise,
 * with nothing launched and y untouched. */
int md_latent_resize_f16(const void* x, void* y, int F, int Hi, int Wi, int Ho, int Wo, int mode, void* stream);

/* Seam blending of tiled VAE encode / decode (AutoencoderKL.enable_tiling(); the rules of diffusers 0.24's tiled_encode / tiled_decode): one
 * launch per tile in the place of blend_v -> blend_h -> crop -> torch.cat -> layout change.
 * cur: (B, Th, Tw, ldc) fp16 NHWC with C <= ldc valid channels, the tile as the encoder + quant_conv or the decoder left it, updated IN PLACE;
 * above: (B, Ah, Tw, ldc), the tile above as it stands after its own call, or NULL (Ah is then ignored); left: (B, Th, Lw, ldc), the tile to
 * the left, likewise, or NULL; dst: fp16 or fp32 (dst_is_f32), element (b, c, y, x) at b sB + c sC + y sY + x sX in elements, as in
 * md_unpack_nhwc_f16: the caller's final tensor, already offset to the tile's corner.  For every b < B, y < Th, x < Tw, c < C:
 *   v = cur[y][x]
 *   if above and y < ev':  v = above[Ah - ev' + y][x] (1 - y / ev') + v (y / ev')      ev' = min(Ah, Th, ev)
 *   if left  and x < eh':  v = left[y][Lw - eh' + x]  (1 - x / eh') + v (x / eh')      eh' = min(Lw, Tw, eh)
 *   cur[y][x] = fp16(v)                                 the whole tile: the tiles below and to the right read it
 *   if y < keep_h and x < keep_w:  dst[b, c, y, x] = v  the cropped part (rounded once to fp16 for an fp16 dst)
 * Vertical first, then horizontal, both reading the neighbour after ITS blends, the weights from the clamped extents: diffusers' order and
 * in-place dependence.  An extent of 0 blends nothing.  In place is safe: element (y, x) of cur depends on itself and on other buffers only.
 * fp32 operations, ONE rounding to fp16 (diffusers rounds after every operation); the weights and sums are carried as pairs of floats, so
 * a blend that cancels to little is still within an fp16 ulp of the float64 result.  Weight 0 (y = 0 / x = 0) returns the neighbour exactly.
 * Non-finite inputs give non-finite outputs (0 * Inf, as in torch).  One thread per 8 bytes of channels (ldc % 4 == 0 and cur / above / left
 * 8-byte aligned) or per pixel (anything else, e.g. the decoder's 3-channel image); no atomics: two calls give the same bits.  Nothing
 * outside the C valid channels of cur and the keep_h x keep_w window of dst is written; the strides of dst are the caller's word.
 * cur and dst not NULL; B, Th, Tw, C, ldc positive, C <= ldc; ev, eh >= 0; 1 <= keep_h <= Th, 1 <= keep_w <= Tw; Ah > 0 with above, Lw > 0
 * with left; every tile below 2^31 elements; cur / above / left 2-byte aligned and dst to its element; cur not overlapping above or left;
 * MD_ERR_ARG otherwise, with nothing launched and every buffer untouched. */
int md_tile_blend_f16(void* cur, int ldc, const void* above, int Ah, const void* left, int Lw, void* dst, int dst_is_f32, int B, int Th,
                      int Tw, int C, int ev, int eh, int keep_h, int keep_w, long sB, long sC, long sY, long sX, void* stream);

/* The pipeline's output boundary: decoded frames -> the uint8 H x W x C bytes every writer takes, one launch in the place of the reference's
 * (video / 2 + 0.5).clamp(0, 1) (three elementwise passes), the permuted copy, the fp32 host array and the writer's (x * 255).astype(uint8).
 * src: fp16, or fp32 with src_is_f32, element (b, c, y, x) at b sB + c sC + y sY + x sX in elements: the decoders' own NHWC result (sC = 1,
 * sX = ldc >= C), a finished NCHW tensor (sX = 1), or any other strided view.  dst: bytes, (b, y, x, c) at b dB + y dY + x C + c: packed
 * H x W x C frames whose row pitch dY and frame pitch dB are the caller's, so a frame can be written straight into a larger canvas.
 * The arithmetic is the reference's chain operation by operation, not the single expression trunc(clamp(127.5 v + 127.5)):
 *   f32_math = 0 (fp16 tensors):  a = fp16(v / 2);  s = fp16(a + 0.5), one round-to-nearest-even;  s clamped to [0, 1];  q = fp32(s) * 255
 *                                 rounded to fp32;  the byte is q truncated toward zero
 *   f32_math = 1 (an fp32 VAE boundary):  the same steps with every intermediate in fp32; an fp16 source converts exactly
 * src_is_f32 = 1 requires f32_math = 1.  +Inf gives 255 and -Inf gives 0.  NaN gives 0: the float path's cast of a NaN to uint8 is undefined
 * (C and numpy), so this value is a choice of this entry point.
 * One thread per 4 pixels of a row; the loads and the byte writer are csrc/frame_io.h's, stated there (vector loads where a whole unit is
 * contiguous and aligned in src, nothing outside the view's span read; 4-byte stores where the 4 C bytes are aligned).  256 threads, at most 2048
 * blocks, a grid-stride loop past that; no atomics: two calls give the same bits.  Nothing outside the B H rows of W C bytes of dst is
 * written; the strides of src are the caller's word.
 * src and dst not NULL; C in 1..4; B, H, W positive and B*H*W within int; src_is_f32 and f32_math 0 or 1; dY >= W C; dB >= (H - 1) dY + W C;
 * src aligned to its element (dst needs no alignment); MD_ERR_ARG otherwise, with nothing launched and dst untouched. */
int md_frames_u8(const void* src, int src_is_f32, int f32_math, void* dst, int B, int H, int W, int C, long sB, long sC, long sY, long sX,
                 long dB, long dY, void* stream);

/* Persistent launchers (gemm_sp_kernel behind md_gemm_f16 / md_conv*_f16) start one workgroup per CU of the device.  A caller that launches
 * on a stream created with a CU mask (hipExtStreamCreateWithCUMask: a partition of the chip shared with another stream) tells the
 * library how many CUs that stream owns: grids and the tile-choice model then use `ncu` (a multiple of 8: the same number of CUs on each
 * of the 8 XCDs, which also keeps workgroup b on XCD b % 8) until md_set_cu_limit(0) restores the device's own count.  Process-wide, not
 * per stream; the streaming kernels (K = 320 / 640 projections) keep their 256-workgroup grids.  tools/cu_partition.py is the user
 * (profiles/r06_ab_cu_partition.log).  Returns MD_OK, or MD_ERR_ARG for a negative count or one that is not a multiple of 8. */
int md_set_cu_limit(int ncu);

/* Dispatch queries (no device access, nothing launched): which kernel the automatic dispatch of md_gemm_f16 / md_conv3x3_nhwc_f16
 * selects for a problem on a chip with `ncu` compute units, for dense 16-byte aligned operands.  epi: bit 0 residual, bit 1
 * row-broadcast operand, bit 2 bias.  Returns 1MN gemm_sp_kernel with wave tile (MT, NT) = (M, N) (135 = 192x320, 134 = 192x256,
 * 124 = 128x256, 132 = 192x128, 142 = 256x128, 144 = 256x256 GEGLU; +1000 on swapped operands for a transposed output, +2000 when the
 * residual enters the accumulators through the matrix core inside the K loop instead of in the epilogue: K tiles > 32 x 32 sub-tiles of the wave tile), 210 / 220 / 230 the W-stationary
 * streaming kernel (K = 320 / K = 640 / GEGLU), 301 / 302 / 303 the multi-workgroup kernel (64-column / 256x128 / 128x128 tiles),
 * or a negative MD_ERR code.  They pin the measured dispatch table in CPU tests. */
int md_gemm_plan(int M, int N, int K, int act, int transpose_out, int epi, int ncu);
int md_conv3x3_plan(int B, int Hin, int Win, int Cin, int Cout, int stride, int upsample, int epi, int ncu);

/* The same question for a call AS IT IS MADE: the arguments of md_gemm_f16 / md_conv_nhwc_f16 without the stream.  They run what the launch
 * runs up to, but not including, the launch itself: the same argument checks (the negative code the launch would return comes back), the
 * same MD_GEMM_SP / MD_GEMM_SP_NT values (read once per process), the CU count of the current device or of md_set_cu_limit (256 without
 * a device).  So a misaligned or sliced operand, an activation, a pinned tile or a CU limit shows in the answer.  Pointer values and pitches
 * are read, memory is not; nothing is launched.  Returns the plan code (as md_gemm_plan); when the token matrix runs in row blocks the code
 * is that of each full-size block, *blocks (> 1) their number and *tail_code the code of the shorter last block (both may be NULL). */
int md_gemm_plan_call(const void* A, int lda, const void* W, void* C, int ldc, int M, int N, int K, const void* bias,
                      const void* residual, int ldr, const void* rowadd, int ldra, int rows_per_group, int act,
                      int transpose_out, int* blocks, int* tail_code);
int md_conv_plan_call(const void* X, int ldx, const void* W, void* Y, int ldy, int B, int Hin, int Win, int Cin, int Cout, int kw,
                      int stride, int upsample, int pad_lo, const void* bias, const void* residual, int ldr, const void* rowadd,
                      int ldra, int rows_per_group, int act);

#ifdef __cplusplus
}
#endif
#endif
