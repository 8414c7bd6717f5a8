/*
 * mmx_relevancy.h -- C-ABI of libmmx_hip.so, the MI355X (gfx950) relevancy-propagation engine.
 *
 * The reference (hila-chefer/Transformer-MM-Explainability) has NO FFI boundary: its hot path is
 * Python calling stock ATen kernels.  The entry points below are what a ctypes binding of that path
 * binds instead of those ATen call sequences; each cites the reference site it replaces
 * (paths relative to the reference checkout).  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every pointer named *_dev / documented "device" is a HIP device pointer owned by the caller;
 *     pointer TABLES (const void* const*) are HOST arrays of device pointers
 *   - plain C types only: no torch / hip types in the signatures; `stream` is a hipStream_t passed
 *     as void* (NULL = default stream)
 *   - all launches are stream-ordered, never synchronise, never allocate (scratch is caller-provided;
 *     sizes from the *_workspace_bytes queries)
 *   - return value: 0 = ok, MMX_E* < 0 on error (no exceptions cross the boundary);
 *     mmx_last_error() gives a thread-local message
 *   - relevancy matrices R are always fp32 row-major; captured attention / gradient buffers are
 *     `dtype` (MMX_F32 / MMX_F16 / MMX_BF16), row-major [B, H, Nq, Nk] with index b*H + h
 *     (== CLIP's [B*H, N, N], CLIP/clip/auxilary.py:194)
 */
#ifndef MMX_RELEVANCY_H
#define MMX_RELEVANCY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Within a version entry points are only ever ADDED (the *_ex forms); a binding checks ==.
 * 2 (round 5 / 6): mmx_lxmert_schedule_ex and mmx_lxmert_schedule_v2 removed, mmx_lxmert_schedule gained `text_len_dev`,
 *    `workspace_dev`, `workspace_bytes` (a caller built against version 1 would pass `stream` where a pointer is expected), and
 *    several mmx_set_option keys now return MMX_EINVAL -- an incompatible change, hence the bump.  A version-1 binding fails its
 *    mmx_abi_version() check instead of misreading arguments. */
#define MMX_ABI_VERSION 2
#define MMX_MAX_LAYERS 48

enum mmx_dtype { MMX_F32 = 0, MMX_F16 = 1, MMX_BF16 = 2 };
/* OR-ed into the `slab_dtype` argument of mmx_attn_capture_fwd_ex / _bwd_ex: run the attention products on the bf16 matrix
 * cores (v_mfma_f32_16x16x32_bf16: operands rounded to bf16 as they are read, fp32 accumulation, softmax / dS arithmetic in
 * fp32) instead of the exact-fp32 MFMA.  BASELINE config 5 (a bf16 CLIP body, CLIP/clip/model.py:381-402). */
#define MMX_ATTN_MMA_BF16 0x100
/* Backward only: `do_dev` holds bf16 and dq / dk / dv are written as bf16 (the gradient stream between the bf16 GEMMs of a
 * bf16 body needs no conversion passes); strides stay in elements, 16-byte aligned.  With MMX_ATTN_MMA_BF16: any shape the
 * streaming kernels serve.  WITHOUT it (round 4): the exact-fp32 arithmetic of the whole-head kernels around bf16 gradient
 * I/O -- fp32 slabs, Nk <= 128, Nq <= 256, head_dim % 4 == 0 and <= 64, 8-byte aligned gradient rows; MMX_ENOTSUP otherwise.
 * No entry point reads or writes outside the buffers it is handed (16-bit slabs: the vector loads of the streaming kernels
 * fall back to element loads for the last few elements of a slab). */
#define MMX_ATTN_IO_BF16 0x200

enum mmx_status {
    MMX_OK = 0,
    MMX_EINVAL = -22,       /* bad argument (null pointer, non-positive size, unsupported dtype) */
    MMX_ENOTSUP = -95,      /* shape outside what the kernels support (message says which limit) */
    MMX_EWORKSPACE = -105,  /* workspace too small */
    MMX_EHIP = -1000        /* -1000 - hipError_t */
};

/* flags for mmx_mm_attention_rules / chain schedules */
#define MMX_MM_NORMALIZE 1u        /* apply handle_residual to R_ss / R_qq (apply_normalization=True) */
#define MMX_MM_SELF_IN_RULE10 2u   /* apply_self_in_rule_10=True; if clear the addition is cam_sq itself */
#define MMX_MM_NAN_TO_ZERO 4u      /* DETR: R_sq_addition[isnan] = 0 (DETR/modules/ExplanationGenerator.py:42) */

/* scale placement of the attention-capture op */
#define MMX_SCALE_Q_FIRST 0   /* q*scale, then q.k^T  (CLIP/clip/auxilary.py:153, DETR/modules/layers.py:745) */
#define MMX_SCALE_SCORES 1    /* (q.k^T)/sqrt(d)      (lxmert_lrp.py:399, BERT_ours.py:325) */

int mmx_abi_version(void);
const char* mmx_last_error(void);
/* tuning knobs (process-wide; results stay within the parity tolerance for every setting):
 *   "self_chain_algo"    0 auto: one workgroup per (sample, layer group); with more than one group the last arriver of a sample
 *                        multiplies the group products (re-associated at the group boundaries).  fp32 slabs run the kernels with
 *                        barrier-free stream waves -- csrc/relevancy_chain_groups.hip (several groups: every A_bar of the group
 *                        resident in LDS) / csrc/relevancy_chain_cols.hip (one group, N >= 40: ring of A_bar images) --, everything
 *                        else the fused kernel of relevancy_chain_fused.hip | 1: the fused kernel everywhere (same bits) |
 *                        4: same as 0 | 5: relevancy_chain_cols.hip for every
 *                        fp32 shape (strict layer order, bit-identical to "self_chain_groups" = 1)
 *   "self_chain_cols_c" / "self_chain_cols_nb"   0 auto (1 / as many as fit, <= 6) | workgroups per sample that split the COLUMNS of R
 *                        (each reduces the full A_bar; measured slower than layer groups, profiles/r05_chain_cols_probe.txt) / LDS
 *                        images of A_bar in the ring, of relevancy_chain_cols.hip
 *   "self_chain_pipe"    4 (default) fused chain kernel (algo 1 / one group / 16-bit slabs), fp32 slabs, N >= 40: the stream waves run a software pipeline of raw buffer loads (the
 *                        next batch of 8 16-byte loads in flight across the head reduction, the LDS write and the per-layer barrier)
 *                        with up to 4 KB contiguous per (head, array) and wave | 2 / 1: at most 2 / 1 KB contiguous |
 *                        0 the plain chunk loop of rounds 1-2.  Same arithmetic, bit-identical results
 *   "self_chain_nt"      1 (default) the pipelined stream waves load the read-once slabs with the nt (streaming) cache policy (a
 *                        probability slab shared by the batch keeps the default policy) | 0: default policy everywhere.  Same results
 *   "self_chain_groups"  0 auto (the fewest groups that put a workgroup on ~70 % of the CUs, at most 4, never more workgroups than
 *                        CUs; 1 below 1 MB per sample) | 1..8 layer groups per sample (1 = strict sequential order)
 *   "self_chain_rows"    0 (default) N > 128: avg_heads_kernel + the tiled product, two launches per layer with A_bar through memory |
 *                        1: no second right-hand side: a layer of the chain is ONE launch -- the head reduction of a 16-row block into
 *                        LDS, then that block row of A_bar . R on the exact-fp32 MFMA (csrc/relevancy_chain_rows.hip; same results to
 *                        summation order, measured 0.87x the speed of the default at 577 tokens: profiles/r06_chain_rows_probe.txt)
 *   "attn_head"          1 (default) register-resident whole-head attention kernels (Nk <= 128, Nq <= 256) | 0 never
 *   "attn_head_tile_skip" 1 (default) the whole-head kernels skip the products of 16-key tiles whose probabilities are exact zeros for a
 *                        whole 16-row strip (causal / padding masks; same bits, dP stays dense) | 0 never (A / B runs)
 *   "attn_stream"        1 (default) long-sequence streaming attention kernels | 0 only the general tiled kernels (any head_dim, any
 *                        alignment: what every shape the other families turn down runs on)
 *   "attn_bf16_v3"       non-zero (default): third-generation bf16 backward of the shared-forward row-relevancy mode | 0: second generation
 *   "attn_bf16_v2"       1 (default) second-generation bf16 backward | 0: the streaming kernels' bf16 path
 *   "attn_fwd_split"     1 (default) streaming forward on a small grid (< 160 workgroups of 64 rows, fp32 slabs):
 *                        16-row workgroups whose waves split the keys | 0 always the 64-row kernel
 *   "text_live_rows"     1 (default) mmx_live_rows builds the live-row list (the row-list backward of a causal tower: mmx_gemm_rows_f32
 *                        and the *_rows kernels) | 0: it declines with MMX_ENOTSUP and the caller runs the dense backward (A / B runs)
 *   "text_live_rows_fwd" 1 (default) the forward of that tower runs on the live rows too (mmx_gemm_rows_bias_f32, mmx_add_layernorm_fwd_rows)
 *                        | 0: dense forward, row-list backward (A / B runs); without "text_live_rows" it has no effect
 *   "text_live_attn"     1 (default) inside that forward route the attention takes the caption lengths too (mmx_attn_capture_fwd_live /
 *                        _bwd_live: no dead row of q / k / v is read, no zero fill of qkv) | 0: dense attention over a zero-filled qkv (A / B runs)
 *   "text_live_rows_half" 0 (default) an fp16 body (the reference's convert_weights mode) keeps the dense text tower | 1: it takes the row-list
 *                        route too, its GEMMs on mmx_gemm_rows_f16 / mmx_gemm_rows_bias_f16 (needs "text_live_rows" and "text_live_rows_fwd")
 *   "clip_head_fused"    1 (default) CLIP interpret / interpret_grouped take the similarity head's gradients from mmx_clip_head_f32 (one
 *                        launch) | 0: the autograd head over CLIP.logits (A / B runs; another rounding of the same formula)
 *   "gemm_rows_tm"       32 (default) | 64: rows per workgroup tile of mmx_gemm_rows_f32 (same products, another order of the k sum)
 *   "gemm_rows_tn"       0 (default: 32 for N <= 512, else 64) | 32 | 64: columns per workgroup tile of mmx_gemm_rows_f32 at 32 rows (same
 *                        products, another order of the k sum; 64-row tiles are always 64 wide)
 *   "gemm_rows_pf"       0 (default: 4) | 3 | 4: slabs of K that mmx_gemm_rows_f32 / mmx_gemm_rows_bias_f32 request ahead
 *                        into registers (A / B runs; the same bits at every depth: the order of the k sum does not depend on it)
 *   "debug_flags"        profiling only (phase skipping), 0 in production; one meaning per bit for every chain kernel the dispatcher
 *                        may pick: 1 return before the hand-off / combine | 4 matrix waves skip the MFMAs | 8 layer-group kernel:
 *                        ticket without combine | 16 column kernel: no block rotation
 * These are A / B switches for tests and probes (every remaining value is the default for some shape or the reference arm of an
 * equivalence test); round 5 removed the kernel families that were nobody's default (self_chain_algo 2, self_chain_big, attn_small,
 * linear_stream, bmm_tile, the 4-wave / fourth-generation bf16 variants, the one-workgroup bi-modal schedule).
 * Unknown keys / out-of-range values return MMX_EINVAL. */
int mmx_set_option(const char* key, int value);

/* ---------------------------------------------------------------------------------------------
 * Rule 5: A_bar[b] = mean_h( clamp(grad[b,h] * attn[b,h], min=0) )              out: [B, Nq, Nk] fp32
 * replaces avg_heads (DETR/modules/ExplanationGenerator.py:19-24, lxmert/.../ExplanationGenerator.py:18-23,
 * ViT notebook cell 7:2-7) and the inline reshape/mul/clamp/mean of CLIP_explainability.ipynb cell 6:26-31.
 * Unbatched callers pass B=1 and H = (product of all leading dims).
 */
int mmx_avg_heads(const void* attn_dev, const void* grad_dev, void* out_dev,
                  int B, int H, int Nq, int Nk, int dtype, void* stream);
/* Same with an explicit batch stride (in elements) for the attention slab: H*Nq*Nk (or -1) = per-sample slabs, 0 = ONE
 * forward pass shared by all B samples of `grad` (shared-forward mode, see mmx_relevancy_self_chain_ex). */
int mmx_avg_heads_ex(const void* attn_dev, const void* grad_dev, void* out_dev,
                     int B, int H, int Nq, int Nk, int dtype, int64_t attn_batch_stride, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The fused self-attention chain (rules 5+6 [+7]) -- ONE launch for all layers:
 *     R <- R_init (identity if NULL);  for l in 0..n_layers-1:  R <- R + A_bar_l . R
 *     optional second right-hand side (rule 7): R_sq <- R_sq + A_bar_l . R_sq      (R_sq: [B, N, M])
 * replaces the per-layer loops of CLIP_explainability.ipynb cell 6:22-32 / 6:45-55, CLIP/example.py:22-30,
 * ViT notebook cell 7:28-33, VisualBERT/.../ExplanationGenerator.py:86-93,
 * DETR/modules/ExplanationGenerator.py:110-118 (encoder) -- `start_layer` is applied by the caller by
 * passing the pointer sub-range.
 *   attn_layers/grad_layers: HOST arrays of n_layers device pointers, each [B, H, N, N] `dtype`
 *   R_init_dev: NULL or [B, N, N] fp32;  R_out_dev: [B, N, N] fp32
 *   Rsq_init_dev/Rsq_out_dev: NULL or [B, N, M] fp32 (M = 0 when unused)
 *   workspace_dev: NULL allowed when mmx_self_chain_workspace_bytes() == 0 for the shape (fused path)
 */
size_t mmx_self_chain_workspace_bytes(int n_layers, int B, int H, int N, int M, int dtype);
int mmx_relevancy_self_chain(const void* const* attn_layers, const void* const* grad_layers, int n_layers,
                             int B, int H, int N, int dtype,
                             const void* R_init_dev, void* R_out_dev,
                             const void* Rsq_init_dev, void* Rsq_out_dev, int M,
                             void* workspace_dev, size_t workspace_bytes, void* stream);

/* Same, with an explicit batch stride (in elements) of the ATTENTION slabs: H*N*N (or -1) for per-sample slabs, 0 when
 * one forward pass is shared by the whole batch (the reference's CLIP `interpret` repeats ONE image B times,
 * CLIP_explainability.ipynb cell 6:3, so the image tower's probabilities are identical for every sample while the
 * gradients differ).  Gradient slabs are always per sample. */
int mmx_relevancy_self_chain_ex(const void* const* attn_layers, const void* const* grad_layers, int n_layers,
                                int B, int H, int N, int dtype, int64_t attn_batch_stride,
                                const void* R_init_dev, void* R_out_dev,
                                const void* Rsq_init_dev, void* Rsq_out_dev, int M,
                                void* workspace_dev, size_t workspace_bytes, void* stream);

/* Same, with flags (ABI 2, added in round 6).
 *   MMX_CHAIN_CAUSAL  the probability slabs come out of CAUSALLY MASKED attention (CLIP's text tower: CLIP/clip/model.py:334-340
 *                     `build_attention_mask`, applied in CLIP/clip/auxilary.py:232-236): every entry above the diagonal is an exact 0,
 *                     hence clamp(grad * attn, 0) is 0 there for any finite gradient, and the fp32 chain kernels do not READ the
 *                     4-element chunks that lie entirely above the diagonal (of either slab) -- about half the bytes of the launch.
 *                     Results are bit-identical to flags = 0 on such slabs.  The caller vouches for the mask: the kernels do not
 *                     look at the skipped entries (a non-finite gradient above the diagonal, which the reference would turn into a
 *                     NaN, goes unseen).  Ignored by the paths that have no use for it (16-bit slabs, N > 128, a second right-hand side). */
#define MMX_CHAIN_CAUSAL 1u
int mmx_relevancy_self_chain_flags(const void* const* attn_layers, const void* const* grad_layers, int n_layers,
                                   int B, int H, int N, int dtype, int64_t attn_batch_stride,
                                   const void* R_init_dev, void* R_out_dev,
                                   const void* Rsq_init_dev, void* Rsq_out_dev, int M, unsigned flags,
                                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same chain in the reference's HALF-PRECISION mode.  On a GPU the reference runs the CLIP model after
 * `convert_weights` (CLIP/clip/model.py:381-402, 440) and creates R in the dtype of the fp16 attention probabilities
 * (CLIP_explainability.ipynb cell 6:20,43), so `grad * cam`, `.clamp(min=0).mean(dim=1)`, `torch.bmm(cam, R)` and
 * `R + ...` each produce an fp16 tensor (fp32 arithmetic inside the op, ONE rounding of its result).  This entry point
 * applies exactly those roundings (round to nearest even, overflow to inf like torch) around the fp32 sums of the kernels.
 *   slabs: fp32 or fp16 (`dtype`), R_out_dev: [B, N, N] fp32 storage holding fp16-representable values (R starts as I)
 *   workspace: mmx_self_chain_workspace_bytes(n_layers, B, H, N, 0, dtype) bytes (0 for N <= 128: one fused launch) */
int mmx_relevancy_self_chain_half(const void* const* attn_layers, const void* const* grad_layers, int n_layers,
                                  int B, int H, int N, int dtype, int64_t attn_batch_stride, void* R_out_dev,
                                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched fp32 matmul on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32):
 *     C[b] = (accumulate ? Cin[b] : 0) + op(A[b]) . B[b],   op = transpose if trans_a
 * A: [batch, M, K] (or [batch, K, M] if trans_a), B: [batch, K, N], C/Cin: [batch, M, N]; a batch
 * stride of 0 broadcasts an operand.  Cin may alias C only if it does not alias A or B.
 * replaces torch.matmul / torch.bmm in rules 6, 7, 10, 11 (DETR/.../ExplanationGenerator.py:27-43,
 * lxmert/.../ExplanationGenerator.py:26-42) and in compute_rollout_attention.
 */
int mmx_bmm_f32(const void* A_dev, const void* B_dev, const void* Cin_dev, void* C_dev,
                int batch, int M, int N, int K, int trans_a,
                int64_t stride_a, int64_t stride_b, int64_t stride_c,
                int nan_to_zero, void* stream);

/* y = x . Wt + bias on the same kernel (32 x 32 tiles at these sizes):  x [M, K], Wt [K, N] (the TRANSPOSED nn.Linear weight,
 * row-major), bias [N] or NULL, y [M, N], fp32 contiguous.  For the handful of one-sample projections of a shared forward where
 * the library's heuristic picks a 256-row tile for ~100 rows (DETR decoder, 100 queries, 256 -> 256: 30 us in the library, 9 us
 * here -- profiles/r03_detr_probe.txt); everything else stays on the library GEMMs, which are faster from 256 x 512 outputs up. */
int mmx_linear_f32(const void* x_dev, const void* wt_dev, const void* bias_dev, void* out_dev, int M, int N, int K, void* stream);

/* One row per sample <-> a dense [B, N, E] fp32 tensor (the top block of a CLIP tower carries a gradient on ONE token per sample,
 * the class / EOT token: CLIP/clip/model.py:235, 360):  mmx_rows_to_dense: out[b, n, :] = (n == rows[b]) ? vals[b, :] : 0;
 * mmx_rows_add: dense[b, rows[b], :] += vals[b, :].  rows: int64 [B], vals [B, E], E % 4 == 0.  A rows[b] outside [0, N) names no row:
 * sample b of out is all zero / sample b of dense is left as it is (nothing is read or written out of bounds).  vals and out / dense
 * 16-byte aligned, rows 8-byte (MMX_EINVAL otherwise: there is no misaligned route). */
int mmx_rows_to_dense(const void* vals_dev, const void* rows_dev, void* out_dev, int B, int N, int E, void* stream);
int mmx_rows_add(void* dense_dev, const void* rows_dev, const void* vals_dev, int B, int N, int E, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Row-list backward of a CAUSALLY MASKED tower whose feature is read at ONE token per sample (CLIP's text tower: the mask of
 * CLIP/clip/model.py:334-340, the EOT token of model.py:360).  The upstream gradient enters at row eot[b] only and causal attention
 * hands gradient to keys j <= i only, so in every layer every gradient row past eot[b] is an exact zero.  These entry points run the
 * row-wise steps of the hand-written backward on the live rows alone, chosen ON THE DEVICE (nothing is read back; a captured
 * hipGraph replays them for any input):
 *   mmx_live_rows               rows[0 .. *count) = b * N + p for p <= clamp(eot[b], 0, N - 1), packed in (b, p) order; eot: int64 [B],
 *                               rows: int32 [B * N] (capacity: every input fits), count: int32 [1].  MMX_ENOTSUP when option
 *                               "text_live_rows" is 0 (mmx_set_option): the caller then runs the dense path.
 *   mmx_gemm_rows_f32           C[r] = A[r] . W for the listed rows r, exact fp32 on the MFMA.  A: [cap_rows, K], C: [cap_rows, N], W: [K, N]
 *                               (an nn.Linear weight as stored, [out, in], used as x @ weight), fp32 contiguous.  Eligible: N % 4 == 0,
 *                               K % 4 == 0, 16-byte aligned operands; MMX_ENOTSUP otherwise.  Unlisted rows of C are not written, ids outside
 *                               [0, cap_rows) are skipped.  Option "gemm_rows_tm": 32 (default) or 64 rows per workgroup tile.
 *   mmx_quick_gelu_bwd_rows     mmx_quick_gelu_bwd on the listed rows of [cap_rows, row_elems] tensors (row_elems % 4 == 0).
 *   mmx_layernorm_bwd_add_rows  mmx_layernorm_bwd_add on the listed rows (x / mean / rstd per row: x_rows == cap_rows).
 * Non-finite values: the dense path multiplies the zero gradient of a dead row with that row's activations, so a non-finite
 * activation at a padded position turns into a NaN there, as in the reference; these entry points never visit the row, and the
 * caller's dead rows stay what they were (the attention backward is handed zeros for them).  Same class of deviation as
 * MMX_CHAIN_CAUSAL above; it needs a forward that already produced non-finite activations. */
int mmx_live_rows(const void* eot_dev, int B, int N, void* rows_dev, void* count_dev, void* stream);
int mmx_gemm_rows_f32(const void* a_dev, const void* w_dev, void* c_dev, const void* rows_dev, const void* count_dev,
                      int cap_rows, int N, int K, void* stream);
int mmx_quick_gelu_bwd_rows(const void* x_dev, const void* dy_dev, void* dx_dev, const void* rows_dev, const void* count_dev,
                            int cap_rows, int row_elems, void* stream);
int mmx_layernorm_bwd_add_rows(const void* dy_dev, const void* x_dev, const void* mean_dev, const void* rstd_dev,
                               const void* gamma_dev, const void* d_res_dev, void* dx_dev, const void* rows_dev,
                               const void* count_dev, int cap_rows, int E, void* stream);
/* The FORWARD of such a tower on the same list: row p of a caption depends on rows <= p of that caption only, and the feature, every
 * gradient and both maps depend on rows p <= eot[b] only, so the row-wise steps of the forward run on the listed rows too.
 *   mmx_gemm_rows_bias_f32      C[r] = A[r] . Wt + bias for the listed rows r: a forward nn.Linear.  Wt: [K, N] = the weight TRANSPOSED
 *                               ([in, out]; the caller caches that copy, weights do not change between calls), bias: [N].  The product
 *                               is mmx_gemm_rows_f32's (same tiles, same eligibility, option "gemm_rows_tm"); the bias is added to the
 *                               finished sum.  act_dev != NULL ([cap_rows, N], not C): QuickGELU of C's listed rows is stored there as
 *                               well, with the bits mmx_quick_gelu_fwd gives on C (c_fc: C is the pre-activation the backward keeps).
 *                               Unlisted rows of C and act are neither read nor written.
 *   mmx_add_layernorm_fwd_rows  mmx_add_layernorm_fwd (fp32 h) on the listed rows: sum, h, mean and rstd of unlisted rows are left alone;
 *                               listed rows get the bits the dense kernel gives.
 *   mmx_text_live_rows_fwd_enabled  1 iff options "text_live_rows" and "text_live_rows_fwd" (default 1 | 0: dense forward, row-list
 *                               backward, for A / B runs) are both on. */
int mmx_gemm_rows_bias_f32(const void* a_dev, const void* wt_dev, const void* bias_dev, void* c_dev, void* act_dev,
                           const void* rows_dev, const void* count_dev, int cap_rows, int N, int K, void* stream);
int mmx_add_layernorm_fwd_rows(const void* x_dev, const void* y_dev, const void* gamma_dev, const void* beta_dev,
                               void* sum_dev, void* h_dev, void* mean_dev, void* rstd_dev, const void* rows_dev,
                               const void* count_dev, int cap_rows, int E, float eps, void* stream);
int mmx_text_live_rows_fwd_enabled(void);
/* The same two GEMMs for the reference's HALF-PRECISION mode (convert_weights, CLIP/clip/model.py:381-402: every nn.Linear weight in
 * fp16; the causal mask of model.py:334-340 and the EOT read of model.py:360 as above) on v_mfma_f32_32x32x16_f16:
 *   mmx_gemm_rows_f16           C[r] = half(A[r]) . W_h^T for the listed rows r.  A: [cap_rows, K] fp32 (rounded to fp16 in registers, round to
 *                               nearest even: the bits of x.to(torch.float16)), W_h: [N, K] fp16 row-major (k fastest: an nn.Linear weight
 *                               as stored for a forward, the fp16 copy of weight.t() for the backward's x @ weight), C: [cap_rows, N] fp32
 *                               from fp32 accumulators.  Eligible: N % 8 == 0, K % 8 == 0, 16-byte aligned operands; MMX_ENOTSUP otherwise,
 *                               nothing launched.  Unlisted rows of C are not written, ids outside [0, cap_rows) are skipped.
 *   mmx_gemm_rows_bias_f16      the same + bias[n] (fp32) on the finished sum; act_dev != NULL ([cap_rows, N], not C): QuickGELU of C's listed
 *                               rows is stored there as well, with the bits mmx_quick_gelu_fwd gives on C.
 *   mmx_text_live_rows_half_enabled  1 iff options "text_live_rows_half" (default 0), "text_live_rows" and "text_live_rows_fwd" are all on.
 * Tiles: 32 rows x 64 columns, 32 x 32 for N <= 512; option "gemm_rows_tn" (32 | 64) overrides the choice. */
int mmx_gemm_rows_f16(const void* a_dev, const void* wh_dev, void* c_dev, const void* rows_dev, const void* count_dev,
                      int cap_rows, int N, int K, void* stream);
int mmx_gemm_rows_bias_f16(const void* a_dev, const void* wh_dev, const void* bias_dev, void* c_dev, void* act_dev,
                           const void* rows_dev, const void* count_dev, int cap_rows, int N, int K, void* stream);
int mmx_text_live_rows_half_enabled(void);

/* CLIP's cosine-similarity head (CLIP/clip/model.py:369-378: normalise both features, logits_per_image = exp(logit_scale) * i^ . t^T)
 * and the gradient of the caption notebook's scalar  sum_b logits_per_image[b, b]  (CLIP_explainability.ipynb cell 6:6-10) with
 * respect to both un-normalised features, in closed form and ONE launch -- what the autograd head takes ~33 launches on B rows for.
 * With i^ = i / |i|, t^ = t / |t|, c = i^ . t^, s = exp(logit_scale):
 *     d_img[b] = s (t^_b - c_b i^) / |i|      d_txt[b] = s (i^ - c_b t^_b) / |t_b|      logit_diag[b] = s c_b
 *   img_feat [Bi, D], txt_feat [B, D] fp32 contiguous; pair b reads image row 0 when Bi == 1 (one image for every caption), else row
 *   b / img_group (Bi * img_group == B: img_group captions per image, caption-major as cell 6:3 repeats the images).
 *   logit_scale: DEVICE address of the fp32 parameter (expf is applied in the kernel: no host read).
 *   d_img [B, D], d_txt [B, D], logit_diag [B]: each may be NULL (not all three); none may alias a feature tensor.
 *   1 <= D <= 4096, B >= 1.  One wave per pair, fixed summation order (two runs give the same bits), correctly rounded sqrt and
 *   division, no atomics, no workspace.  MMX_EINVAL before any launch otherwise.
 * mmx_clip_head_fused_enabled: option "clip_head_fused" (default 1). */
int mmx_clip_head_f32(const void* img_feat_dev, const void* txt_feat_dev, const void* logit_scale_dev, void* d_img_dev,
                      void* d_txt_dev, void* logit_diag_dev, int B, int D, int Bi, int img_group, void* stream);
int mmx_clip_head_fused_enabled(void);

/* The chain on VECTORS (rows-only DETR rules): when a caller returns single rows of R_q_i (`aggregated[:, target_index, :]`,
 * DETR/modules/ExplanationGenerator.py:180-182) the encoder product R_ii = (I + A_6) ... (I + A_1) (`:110-118`) is needed only
 * as  R_ii . 1  (the row sums `handle_residual` divides by, `:26-31`) and as  v . R_ii : mat-vecs with the head-averaged maps.
 *   mmx_chain_matvec:  out[b] = base[b] + A[b] . y[b]      mmx_chain_vecmat:  out[b] = base[b] + x[b] . A[b]
 * A [B, N, N], vectors [B, N], fp32; `base` separate from the multiplied vector so the caller can carry the deviation from
 * the start vector (no cancellation at the end); out may not alias y / x; vecmat needs mmx_chain_vecmat_workspace_bytes. */
int mmx_chain_matvec(const void* A_dev, const void* y_dev, const void* base_dev, void* out_dev, int B, int N, void* stream);
size_t mmx_chain_vecmat_workspace_bytes(int B, int N);
int mmx_chain_vecmat(const void* A_dev, const void* x_dev, const void* base_dev, void* out_dev, int B, int N,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* One layer of the row-vector chain without materialising A_bar (ViT nb cell 7:27-33 carried as ONE row, top layer down):
 *   out[b] = base[b] + x[b] . mean_h clamp(grad[b, h] * attn[b, h], 0),   x / base / out [B, N] fp32, slabs [B, H, N, N] of `dtype`
 * (attn_batch_stride: 0 = one forward shared by the batch, < 0 or H*N*N = per sample).  Two launches (partials per 4 slab rows, then
 * their sum in workgroup order: deterministic) instead of mmx_avg_heads + mmx_chain_vecmat's three; out may not alias x;
 * workspace 16-byte aligned, mmx_avg_heads_vecmat_workspace_bytes. */
size_t mmx_avg_heads_vecmat_workspace_bytes(int B, int N);
int mmx_avg_heads_vecmat(const void* attn_dev, const void* grad_dev, const void* x_dev, const void* base_dev, void* out_dev,
                         int B, int H, int N, int dtype, int64_t attn_batch_stride, void* workspace_dev,
                         size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * eq. 8-9: out = (R - I) / rowsum(R - I) + I  (0/0 rows -> NaN like the reference).
 * replaces handle_residual (DETR/.../ExplanationGenerator.py:46-53, lxmert/.../ExplanationGenerator.py:45-54).
 * The reference's `assert diag(R-I) >= 0` is reported through *diag_min_dev (device float, may be NULL):
 * it receives min_i (R[i,i]-1) so the host wrapper can raise AssertionError like the reference.
 */
int mmx_handle_residual(const void* R_dev, void* out_dev, int batch, int N, void* diag_min_dev, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Rules 10 (+11):  R_sq_add = Rn_ss^T . (cam_sq . Rn_qq)   [, R_ss_add = cam_sq . R_qs]
 * replaces apply_mm_attention_rules -- DETR 5-arg form (DETR/.../ExplanationGenerator.py:33-43, flags
 * MMX_MM_NAN_TO_ZERO) and LXMERT 6-arg form (lxmert/.../ExplanationGenerator.py:32-42, R_qs/R_ss_add given).
 *   R_ss [Ns,Ns], R_qq [Nq,Nq], cam_sq [Ns,Nq], R_qs [Nq,Ns] or NULL, outputs R_sq_add [Ns,Nq], R_ss_add [Ns,Ns] or NULL
 *   workspace: mmx_mm_rules_workspace_bytes(Ns, Nq) bytes
 */
size_t mmx_mm_rules_workspace_bytes(int Ns, int Nq);
int mmx_mm_attention_rules(const void* R_ss_dev, const void* R_qq_dev, const void* R_qs_dev,
                           const void* cam_sq_dev, void* R_sq_add_dev, void* R_ss_add_dev,
                           int Ns, int Nq, unsigned flags, void* diag_min_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The whole bi-modal (two-stream, LXMERT-style) schedule in ONE launch -- rules 5, 6, 7, 10, 11 and eq. 8-9:
 *   n_lang language + n_vis vision self-attention layers, then n_x cross layers (language cross, image cross, language
 *   self, image self; the last cross layer runs its language half only), finally R_tt[0,0] = 0.
 * replaces the rule schedule of GeneratorOurs.generate_ours (lxmert/lxmert/src/ExplanationGenerator.py:131-211 with the
 * helpers :18-54, 61-129).  Two phases in one launch: the rule-5 head averages of every (sample, block) are spread over the whole
 * chip (16-byte loads, write-through A_bar blocks into `workspace`), the last-arriving workgroup of a sample runs the 38 rule
 * applications from the L2-resident A_bar blocks on the exact-fp32 MFMA with every relevancy matrix in LDS; needs T, I <= 48.
 *   all tables: HOST arrays of device pointers to fp32 [B, H, Nq, Nk] slabs: lang/x_lang_self [.,.,T,T],
 *   vis/x_img_self [.,.,I,I], x_lang_cross [.,.,T,I], x_img_cross [.,.,I,T]; the image tables need n_x-1 entries.
 *   flags: MMX_MM_NORMALIZE | MMX_MM_SELF_IN_RULE10 (NaNs propagate like the reference's LXMERT variant).
 *   outputs fp32: R_tt [B,T,T], R_ti [B,T,I], optional R_ii [B,I,I], R_it [B,I,T]; diag_min_dev as in
 *   mmx_handle_residual (min over all normalisations), may be NULL.
 */
/* text_len_dev: for a batch that is PADDED to T question tokens, a device array of B ints, the real number of question tokens of
 * every sample (1..T; NULL = all T).  The slabs keep their padded [.., T, ..] shape (padded keys carry zero probability under the
 * attention mask); sample b's rules run on its leading text_len[b] tokens only, and rows / columns of R_tt / R_ti / R_it beyond
 * them are written as zero.  One padded batch replaces the grouping of samples by question length
 * (lxmert/lxmert/perturbation.py:45-83 tokenises one question per call, so the reference never pads).
 * workspace: mmx_lxmert_schedule_workspace_bytes(...) bytes, caller-owned, stream-ordered.  One kernel launch (+ one reset launch
 * for the tickets / diag word).  (Rounds 1-3 had a one-workgroup-per-sample form under this name and an `_ex` / `_v2` pair; round 5
 * keeps the one kernel that serves every shape.) */
size_t mmx_lxmert_schedule_workspace_bytes(int n_lang, int n_vis, int n_x, int B, int T, int I);
int mmx_lxmert_schedule(const void* const* lang_attn, const void* const* lang_grad, int n_lang,
                           const void* const* vis_attn, const void* const* vis_grad, int n_vis,
                           const void* const* x_lang_cross_attn, const void* const* x_lang_cross_grad,
                           const void* const* x_img_cross_attn, const void* const* x_img_cross_grad,
                           const void* const* x_lang_self_attn, const void* const* x_lang_self_grad,
                           const void* const* x_img_self_attn, const void* const* x_img_self_grad, int n_x,
                           int B, int H, int T, int I, unsigned flags, const void* text_len_dev,
                           void* R_tt_dev, void* R_ti_dev, void* R_ii_dev, void* R_it_dev,
                           void* diag_min_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention rollout: prod_{i >= start}( (A_i + I) [/ rowsum] ), left-multiplied.
 * replaces compute_rollout_attention (DETR/.../ExplanationGenerator.py:5-16, lxmert/...:5-15 with
 * normalize=1; VisualBERT/.../ExplanationGenerator.py:5-17 batched with normalize=0).
 *   layers: HOST array of n_layers device pointers, each [B, N, N] fp32 (caller applies start_layer)
 *   out: [B, N, N] fp32; workspace: mmx_rollout_workspace_bytes(B, N)
 */
size_t mmx_rollout_workspace_bytes(int B, int N);
int mmx_rollout_chain(const void* const* layers, int n_layers, int B, int N, int normalize,
                      void* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The attention-only baselines of the bi-modal model for a PADDED batch of ragged questions (csrc/bimodal_baselines.hip).  The
 * reference explains one question per call (lxmert/lxmert/perturbation.py:216-245), so it never pads; here every slab is the fp32
 * [B, H, Nq, Nk] capture slab of a padded batch and every length a DEVICE array of B int32 (NULL = the full extent).  A length
 * outside 1..N is CLAMPED to that range inside the kernel before it is used: it never bounds a loop or forms an address unclamped.
 * Sample b is computed from its LIVE block only -- the leading q_len[b] x k_len[b] entries -- and everything outside that block is
 * written as exact zero.  Fixed summation orders, no atomics: two calls give the same bits, and sample b's output depends neither on
 * B nor on its position in the batch.  Sizes per modality: 1..48 (as mmx_lxmert_schedule).  Every argument is checked before any
 * HIP call: null required pointers, B / H <= 0, sizes outside 1..48, n_text < 2, n_img < 1, tables longer than
 * MMX_BASELINES_MAX_TABLE, a workspace smaller than the query says and outputs that overlap an input (or each other) return
 * MMX_EINVAL with a message in mmx_last_error().
 *
 * mmx_head_mean_live: out [B, Nq, Nk].
 *   grad_dev == NULL: the plain head mean mean_h attn[b, h] (lxmert/lxmert/src/ExplanationGenerator.py:528-529, :534-535).
 *   grad_dev given:   GradCAM (lxmert/lxmert/src/ExplanationGenerator.py:542-547): clamp(mean_h(attn[b, h] * w[b, h]), 0) with
 *                     w[b, h] = the mean of grad[b, h] over the LIVE block: the sum and the divisor are both those of the live block
 *                     (the gradient of a padded batch is not zero at padded key columns, although the probability is).
 *   flags: MMX_HEAD_MEAN_ZERO_CLS writes out[b, 0, 0] = 0 ("disregard the [CLS] token", :539, :592).  One launch, one workgroup per sample.
 *
 * mmx_lxmert_rollout: generate_rollout (lxmert/lxmert/src/ExplanationGenerator.py:595-665 with compute_rollout_attention :5-15).
 *   text_attn: HOST table of n_text >= 2 device slabs [B, H, T, T]: the language layers, then every x-layer's lang_self_att, the
 *              LAST x-layer's being the last entry;  img_attn: HOST table of n_img >= 1 slabs [B, H, I, I]: r_layers, then
 *              visn_self_att of every x-layer but the last;  cross_attn_dev: the last x-layer's visual_attention slab [B, H, T, I].
 *   Per sample, t = clamp(text_len[b], 1, T):  A^_l = (mean_h A_l[:t, :t] + I) / its row sums;  R' = A^_{n_text-2} ... A^_0;
 *   R_ii = the same product over the image table;  R_ti = R'^T . (C . R_ii), C the head mean of the cross slab's rows < t (:656);
 *   R_tt = A^_{n_text-1} . R' (:662), R_tt[0, 0] = 0 (:665).
 *   outputs fp32: R_tt [B, T, T], R_ti [B, T, I] (zero beyond t), optional R_ii [B, I, I].
 *   workspace: mmx_lxmert_rollout_workspace_bytes(...) bytes (0 for arguments the entry would refuse), 16-byte aligned, caller-owned,
 *   stream-ordered.
 *   Two plain launches ordered by the stream (no ticket, no spin-wait): B x (n_text + n_img + 1) workgroups take the head means
 *   (+ I, normalised) of every slab, read exactly once, into the workspace; one workgroup per sample then runs the products from
 *   LDS on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32; no reduced-precision product anywhere). */
#define MMX_BASELINES_MAX_TABLE 32
#define MMX_HEAD_MEAN_ZERO_CLS 1u
int mmx_head_mean_live(const void* attn_dev, const void* grad_dev, void* out_dev, int B, int H, int Nq, int Nk,
                       const void* q_len_dev, const void* k_len_dev, unsigned flags, void* stream);
size_t mmx_lxmert_rollout_workspace_bytes(int n_text, int n_img, int B, int T, int I);
int mmx_lxmert_rollout(const void* const* text_attn, int n_text, const void* const* img_attn, int n_img,
                       const void* cross_attn_dev, int B, int H, int T, int I, const void* text_len_dev, void* R_tt_dev,
                       void* R_ti_dev, void* R_ii_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The LRP baselines of the bi-modal model for a PADDED batch of ragged questions (csrc/bimodal_baselines.hip), on the LRP cams that
 * the body's relprop leaves in the capture slabs.  The contract of the block above holds word for word: fp32 [B, H, Nq, Nk] slabs,
 * DEVICE int32 lengths (NULL = the full extent) clamped to 1..N inside the kernel, sample b computed from its LIVE block only, exact
 * zeros outside it.  An entry outside the live block is never summed, multiplied into a live entry or divided by: its value -- a NaN
 * included -- does not matter.  Fixed summation orders, no atomics.  Every argument is checked before any HIP call: null required
 * pointers and null table entries, B / H <= 0, sizes outside 1..48, n_text < 1, n_img < 1, tables longer than
 * MMX_BASELINES_MAX_TABLE, a workspace that is too small or not 16-byte aligned, and outputs that overlap an input or each other
 * return MMX_EINVAL with a message in mmx_last_error().
 *
 * mmx_lxmert_attr: generate_transformer_attr (lxmert/lxmert/src/ExplanationGenerator.py:373-460 with avg_heads :18-23).
 *   text_cam / text_grad: HOST tables of n_text >= 1 device slabs [B, H, T, T], the LRP cams and the gradients of the language layers,
 *              then every x-layer's lang_self_att (:405-411, :431-435, :453-457);  img_cam / img_grad: n_img >= 1 slabs [B, H, I, I]:
 *              r_layers, then visn_self_att of every x-layer but the last (:414-420, :437-441);  cross_cam_dev / cross_grad_dev: the
 *              last x-layer's visual_attention [B, H, T, I] (:447-449).
 *   Per sample, t = clamp(text_len[b], 1, T):  A_bar(C, G) = (sum_h max(0, G_h . C_h)) / H, the clamp per head before the sum (a NaN
 *   stays a NaN, as torch.clamp keeps it), heads in ascending order;  R_tt = I_t, R_tt <- R_tt + A_bar_l R_tt for l = 0 .. n_text - 1
 *   (:411);  R_ii the same over the image table (:420);  R_ti[:t, :] = A_bar(cross)[:t, :] (:451);  R_tt[0, 0] = 0 (:459).
 *   outputs fp32: R_tt [B, T, T], R_ti [B, T, I] (zero beyond t), R_ii [B, I, I].
 *   workspace: mmx_lxmert_attr_workspace_bytes(...) bytes (0 for arguments the entry would refuse), 16-byte aligned, caller-owned,
 *   stream-ordered.
 *   Two plain launches ordered by the stream: B x (n_text + n_img + 1) workgroups form every A_bar once (16-byte loads, every slab
 *   read exactly once; the cross block is written straight to R_ti); one workgroup per sample then runs both chains from LDS on the
 *   exact-fp32 MFMA (v_mfma_f32_16x16x4_f32).
 *
 * mmx_head_minmax_live: the per-map step of generate_partial_lrp (lxmert/lxmert/src/ExplanationGenerator.py:489-505): out [B, Nq, Nk],
 *   out[b] = (m - min m) / (max m - min m) with m = mean_h cam[b, h] (:493, :498, :502-503), the extremes over the live
 *   q_len[b] x k_len[b] block.  max == min gives 0 / 0 = NaN over the live block (a one-entry block included), as the reference's
 *   expression does, and a NaN anywhere in the live block of m makes the whole live block NaN, as torch.min / torch.max do.
 *   flags: MMX_HEAD_MEAN_ZERO_CLS writes out[b, 0, 0] = 0 AFTER the normalisation (:505).  One launch, one workgroup per sample. */
size_t mmx_lxmert_attr_workspace_bytes(int n_text, int n_img, int B, int T, int I);
int mmx_lxmert_attr(const void* const* text_cam, const void* const* text_grad, int n_text, const void* const* img_cam,
                    const void* const* img_grad, int n_img, const void* cross_cam_dev, const void* cross_grad_dev, int B, int H, int T,
                    int I, const void* text_len_dev, void* R_tt_dev, void* R_ti_dev, void* R_ii_dev, void* workspace_dev,
                    size_t workspace_bytes, void* stream);
int mmx_head_minmax_live(const void* cam_dev, void* out_dev, int B, int H, int Nq, int Nk, const void* q_len_dev,
                         const void* k_len_dev, unsigned flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The attention-only baselines of the single-stream (VisualBERT-style) model for a PADDED batch of ragged questions
 * (csrc/selfattn_baselines.hip).  The reference explains one question per call and trims its text padding
 * (VisualBERT/mmf/models/visual_bert.py:578-588), so it never pads; here every slab is the fp32 [B, H, N, N] capture slab of a padded
 * batch whose sequence is [T text positions | V regions], N = T + V, and text_len / vis_len are DEVICE arrays of B int32 (NULL = the
 * full extent), CLAMPED inside the kernel to 2..T and 1..V before any use.  Sample b's live index set is
 * L_b = [0, t_b) u [T, T + v_b), n_b = t_b + v_b -- the text padding sits in the MIDDLE of the sequence -- and all three methods return
 * ONE row of their N x N map: the row of the token the 'vqa' pooler reads, c_b = t_b - 2 (cls_index = input_mask.sum(1) - 2,
 * VisualBERT/mmf/models/transformers/backends/ExplanationGenerator.py:160, :178, :209).  Every output is [B, N] fp32 in the padded
 * layout, exact zero outside L_b and at column c_b (cls_per_token_score[:, cls_index] = 0, :162, :180, :211).  Fixed summation
 * orders, no atomics: two calls give the same bits, and sample b's output depends neither on B nor on its position in the batch.
 * Limits: T >= 2, V >= 1, N <= 256, tables of at most MMX_BASELINES_MAX_TABLE slabs.  Every argument is checked before any HIP
 * call: null required pointers, B / H <= 0, sizes outside the limits, a table that is too long or has a null entry, a workspace that
 * is too small or not 16-byte aligned, an output or workspace that overlaps an input or the other one return MMX_EINVAL with a
 * message in mmx_last_error().  The workspace queries return 0 for arguments the entries refuse.
 *
 * mmx_selfattn_row_live:
 *   grad_dev == NULL: raw attention (ExplanationGenerator.py:155-166): out[b, j] = (sum_h attn[b, h, c_b, j]) / H for j in L_b; one
 *                     launch that reads one row per head; no workspace (workspace_dev may be NULL).
 *   grad_dev given:   attention GradCAM (ExplanationGenerator.py:200-211) on the live block only:
 *                     w[b, h] = (sum of grad[b, h] over L_b x L_b) / float(n_b^2) (the sum first, then one division),
 *                     cam = max(0, (sum_h attn[b, h] w[b, h]) / H) on L_b x L_b (a NaN stays a NaN), mn / mx its minimum / maximum there,
 *                     out[b, j] = (cam[c_b, j] - mn) / (mx - mn): a plain division, NaN when mx == mn as in the reference.  The
 *                     gradient of a padded batch is not zero at padded keys and padded query rows hold garbage: sums, divisor, minimum
 *                     and maximum use L_b only.  Three plain launches ordered by the stream: B x H workgroups for w, B x ceil(N / 8)
 *                     for cam / min / max of a strip of rows, B for the row; attn and grad are each read at most once.
 *                     workspace: mmx_selfattn_row_live_workspace_bytes(B, H, T, V) bytes, 16-byte aligned, caller-owned.
 *
 * mmx_selfattn_rollout_row: generate_rollout (ExplanationGenerator.py:168-180) with compute_rollout_attention (:5-17), which adds I,
 *   does NOT normalise the rows and multiplies from the left.  Only row c_b of (I + A_{L-1}) ... (I + A_0) is returned, A_l the head
 *   mean (sum_h attn_l[b, h]) / H, so a row vector is carried from the top table entry down: x = e_{c_b}; x <- x + x . A_l for
 *   l = n_layers - 1 ... 0.  attn_table: HOST table of n_layers >= 1 device slabs, already sliced to start_layer:.
 *   Two plain launches: B x n_layers x ceil(N^2 / 2048) workgroups take the head means into the workspace (every slab read once, 16-byte
 *   loads, chunks of padded query rows skipped; rows of the workspace are ceil(N / 4) * 4 floats apart); one workgroup per sample then
 *   runs the n_layers vector-matrix steps in plain fp32 FMA with x in LDS.  Its row loads are unconditional, aligned and from clamped
 *   addresses, so eight rows per lane -- the next layer's included -- stay in flight behind counted waits (vmcnt(7)).
 *   workspace: mmx_selfattn_rollout_row_workspace_bytes(n_layers, B, T, V) bytes, 16-byte aligned, caller-owned, stream-ordered. */
size_t mmx_selfattn_row_live_workspace_bytes(int B, int H, int T, int V);
int mmx_selfattn_row_live(const void* attn_dev, const void* grad_dev, void* out_dev, int B, int H, int T, int V,
                          const void* text_len_dev, const void* vis_len_dev, void* workspace_dev, size_t workspace_bytes,
                          void* stream);
size_t mmx_selfattn_rollout_row_workspace_bytes(int n_layers, int B, int T, int V);
int mmx_selfattn_rollout_row(const void* const* attn_table, int n_layers, int B, int H, int T, int V, const void* text_len_dev,
                             const void* vis_len_dev, void* out_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* mmx_selfattn_ours_row: generate_ours (VisualBERT/mmf/models/transformers/backends/ExplanationGenerator.py:68-107) for a PADDED
 *   batch of ragged questions, in the layout and under the rules of the baselines above.  Per layer l (:86-93)
 *   A_l = (sum_h max(0, grad_l[b, h] * attn_l[b, h])) / H -- the clamp per head, BEFORE the sum; a NaN stays a NaN -- and
 *   R <- R + A_l R from layer 0 up, so R = (I + A_{L-1}) ... (I + A_0).  Only row c_b = t_b - 2 is returned (:94-97): x = e_{c_b};
 *   x <- x + x . A_l for l = n_layers - 1 ... 0 on sample b's live set, exact zero outside it and at column c_b.
 *   attn_table / grad_table: HOST tables of n_layers device slabs [B, H, N, N] fp32, entry l of both belonging to one layer.  Any cam
 *   slab may stand in for attn: generate_transformer_att's rows (:42-56) are the same arithmetic on LRP cams.
 *   The gradient of a padded batch is not zero at padded key columns and padded query rows hold garbage; neither reaches the output.
 *   Two plain launches ordered by the stream: B x n_layers x ceil(N^2 / 2048) workgroups form A_l on the live rows (16-byte loads
 *   inside a head's own block, heads in ascending order, chunks of padded query rows neither read nor written) into the workspace
 *   in mmx_selfattn_rollout_row's layout; that entry's row kernel then carries x.  Fixed summation orders, no atomics: two calls give
 *   the same bits, and sample b's output depends neither on B nor on its position in the batch.
 *   Refused with MMX_EINVAL before any HIP call: what mmx_selfattn_rollout_row refuses, for both tables, and
 *   B x n_layers x ceil(N^2 / 2048) > 2^31 - 1 (a one-dimensional grid).
 *   workspace: mmx_selfattn_ours_row_workspace_bytes(n_layers, B, T, V) bytes (0 for arguments the entry refuses), 16-byte aligned,
 *   caller-owned, stream-ordered. */
size_t mmx_selfattn_ours_row_workspace_bytes(int n_layers, int B, int T, int V);
int mmx_selfattn_ours_row(const void* const* attn_table, const void* const* grad_table, int n_layers, int B, int H, int T, int V,
                          const void* text_len_dev, const void* vis_len_dev, void* out_dev, void* workspace_dev,
                          size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * On-device post-processing of relevancy maps (one workgroup per map, no host round trip):
 *  mmx_heatmap_bilinear_minmax: [B, g, g] patch maps -> bilinear upsample to [B, S, S] (torch interpolate semantics,
 *    align_corners=False) + min-max normalisation; replaces CLIP_explainability.ipynb cell 7:14-18 and
 *    Transformer_MM_explainability_ViT.ipynb cell 8:25-28.  MMX_ENOTSUP, nothing launched: g > 64 (the patch map is staged in LDS),
 *    S > 46340 (the S * S pixels of a map are counted in int).  B * S * S is not limited: offsets across maps are 64-bit.
 *  mmx_otsu_masks: [K, n] maps -> min-max to [0,255], truncate to 8 bit, Otsu threshold (OpenCV getThreshVal_Otsu_8u),
 *    masks [K, n] fp32 in {0, 255}; thresholds_dev: optional int32 [K] (NULL: not written); replaces
 *    DETR/mask_generator.py:116-121 (D2H copy + cv2.threshold per kept query).  MMX_ENOTSUP, nothing launched: n > 2^31 - 1 - 256 (the
 *    pixel index is an int stepped by 256).  K * n is not limited.
 *  Both: MMX_EINVAL for a null in / out pointer or a non-positive size.
 *  Special values.  The extremes are taken with fminf / fmaxf, so a NaN pixel does not move them: a heat-map pixel with a NaN among its
 *    four taps (a tap of weight 0 included) is NaN and no other pixel changes; an Otsu NaN pixel is level 0, mask 0.  (The reference's
 *    numpy min / max would make the whole map NaN: a deliberate deviation.)  A map whose upsampled range is 0 gives an all-NaN heat
 *    map (0 / 0, as in the reference); a constant map gives Otsu levels 0, threshold 0 and an all-zero mask.  A +-inf pixel: heat map
 *    NaN where it is tapped with weight 0, and where the blend itself is infinite the range is, so every finite pixel is 0 (+inf) or
 *    NaN (-inf); Otsu all levels 0, threshold 0, mask 0.  tests/postprocess_bounds.py restates all of it.
 */
int mmx_heatmap_bilinear_minmax(const void* in_dev, void* out_dev, int B, int g, int S, void* stream);
int mmx_otsu_masks(const void* cam_dev, void* masks_dev, void* thresholds_dev, int K, int n, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Attention-capture op (replaces the save_attn / save_attn_gradients Python hooks):
 * forward : P = softmax(scale.Q.K^T + mask) written straight into the caller's capture slab, O = P.V
 * backward: dP = dO.V^T written straight into the caller's gradient slab (this IS the hooked
 *           attn gradient), dS = P*(dP - rowsum(dP*P)), dQ, dK, dV
 * replaces CLIP/clip/auxilary.py:225-252, DETR/modules/layers.py:753-762, lxmert_lrp.py:398-414,
 * BERT_ours.py:323-343 (+ the autograd of those ops).
 * Layouts (element strides, last dim contiguous): q(b,h,n,:) = q_dev + b*q_sb + h*q_sh + n*q_sn, same for
 * k, v, o and their gradients.  probs/dprobs: [B, H, Nq, Nk] contiguous, `dtype`-typed capture slabs are
 * fp32 in this ABI version.  mask_dev: NULL or additive fp32 mask, element (b,i,j) at
 * mask_dev + b*mask_sb + i*mask_sq + j (mask_sb = 0 / mask_sq = 0 broadcast).
 * `scale` is the multiplier d^-0.5 in MMX_SCALE_Q_FIRST mode and the divisor sqrt(d) in MMX_SCALE_SCORES mode
 * (the reference multiplies resp. divides; keeping the operation keeps the rounding).
 * Backward takes `probs_sb`, the batch stride of P in elements: H*Nq*Nk for a per-sample slab, 0 when ONE forward's
 * P is shared by every sample of the batch (shared-forward / batched-backward, see clip_explainability.py); q/k/v
 * batch strides may be 0 likewise.  dprobs is always per sample.
 * need_dqkv = 0 skips dS/dQ/dK/dV (lowest layer: only the captured gradient is wanted).
 */
int mmx_attn_capture_fwd(const void* q_dev, const void* k_dev, const void* v_dev,
                         int64_t q_sb, int64_t q_sh, int64_t q_sn,
                         int64_t k_sb, int64_t k_sh, int64_t k_sn,
                         int64_t v_sb, int64_t v_sh, int64_t v_sn,
                         const void* mask_dev, int64_t mask_sb, int64_t mask_sq,
                         void* probs_dev, void* o_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                         int B, int H, int Nq, int Nk, int D, float scale, int scale_mode, void* stream);

size_t mmx_attn_capture_bwd_workspace_bytes(int B, int H, int Nq);   /* rowsum(dP*P): [B, H, Nq] fp32 */
int mmx_attn_capture_bwd(const void* q_dev, const void* k_dev, const void* v_dev,
                         int64_t q_sb, int64_t q_sh, int64_t q_sn,
                         int64_t k_sb, int64_t k_sh, int64_t k_sn,
                         int64_t v_sb, int64_t v_sh, int64_t v_sn,
                         const void* probs_dev, int64_t probs_sb,
                         const void* do_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                         void* dprobs_dev,
                         void* dq_dev, void* dk_dev, void* dv_dev,
                         int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                         int64_t dk_sb, int64_t dk_sh, int64_t dk_sn,
                         int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                         int B, int H, int Nq, int Nk, int D, float scale, int scale_mode,
                         int need_dqkv, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same two entry points with an element type for the capture slabs (`probs`, `dprobs`): MMX_F32, MMX_F16 or
 * MMX_BF16 (the GPU notebooks of the reference run the models in fp16; BASELINE config 5 asks for bf16 capture).
 * P and dL/dP are rounded to nearest even when they are stored; the forward's O is computed from the unrounded P,
 * the backward reads the stored (rounded) P.  q/k/v/O and their gradients stay fp32.  Half-precision slabs are written
 * by the long-sequence streaming kernels only: head_dim % 4 == 0 and 16-byte aligned q/k/v views, else MMX_ENOTSUP.
 * The rule kernels (mmx_avg_heads*, mmx_relevancy_self_chain*) read all three slab types and accumulate in fp32.
 * `fwd_o_dev` (backward, optional, may be NULL): the forward's O with its (batch, head, token) strides; batch stride 0
 * when one forward is shared.  With it the streaming backward gets rowsum(dP * P) = rowsum(dO * O) from one row-wise
 * dot product instead of a first sweep over all keys (a third of its MFMA work). */
int mmx_attn_capture_fwd_ex(const void* q_dev, const void* k_dev, const void* v_dev,
                            int64_t q_sb, int64_t q_sh, int64_t q_sn,
                            int64_t k_sb, int64_t k_sh, int64_t k_sn,
                            int64_t v_sb, int64_t v_sh, int64_t v_sn,
                            const void* mask_dev, int64_t mask_sb, int64_t mask_sq,
                            void* probs_dev, int slab_dtype,
                            void* o_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                            int B, int H, int Nq, int Nk, int D, float scale, int scale_mode, void* stream);
int mmx_attn_capture_bwd_ex(const void* q_dev, const void* k_dev, const void* v_dev,
                            int64_t q_sb, int64_t q_sh, int64_t q_sn,
                            int64_t k_sb, int64_t k_sh, int64_t k_sn,
                            int64_t v_sb, int64_t v_sh, int64_t v_sn,
                            const void* probs_dev, int64_t probs_sb, int slab_dtype,
                            const void* do_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                            const void* fwd_o_dev, int64_t fo_sb, int64_t fo_sh, int64_t fo_sn,
                            void* dprobs_dev,
                            void* dq_dev, void* dk_dev, void* dv_dev,
                            int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                            int64_t dk_sb, int64_t dk_sh, int64_t dk_sn,
                            int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                            int B, int H, int Nq, int Nk, int D, float scale, int scale_mode,
                            int need_dqkv, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The capture pair with a LIVE LENGTH per sample, for the row-list route of a causally masked text tower (mmx_live_rows): sample b
 * has L = clamp(eot_dev[b], 0, Nq - 1) + 1 live rows, eot_dev: int64 [B] on the device, read by the kernels (nothing comes back to the
 * host, so a captured hipGraph follows the captions it is replayed with).  `mask_dev` must be a causal mask and Nq == Nk.
 *   forward:  no row >= L of q / k / v is read.  Rows < L of P and O get the bits mmx_attn_capture_fwd_ex gives them on a q / k / v
 *             whose rows >= L are zeros; rows >= L of P get that call's bits too (the softmax of zero scores under the mask), rows
 *             >= L of O are NOT written.
 *   backward: no row >= L of q / k / v / dO is read (rows >= L of P are not read either).  dP is written whole: rows < L with the bits
 *             of mmx_attn_capture_bwd_ex on operands whose rows >= L are zeros, rows >= L exact zeros.  dq / dk / dv: rows < L only,
 *             same bits; rows >= L are NOT written.
 * Served by live-length instantiations of the whole-head fp32 kernels only: mmx_attn_live_shape(Nq, Nk, D) returns MMX_OK where one
 * exists, MMX_ENOTSUP where not, and launches nothing
 * (today: Nq == Nk in 65 ... 80, head_dim <= 64 and % 4 == 0 -- CLIP's text towers have 77 tokens) and option "text_live_attn" (default 1 | 0
 * for A / B runs) is on; otherwise these calls return MMX_ENOTSUP and the caller keeps mmx_attn_capture_*_ex on a zero-filled q / k / v. */
int mmx_attn_live_shape(int Nq, int Nk, int D);
int mmx_attn_capture_fwd_live(const void* q_dev, const void* k_dev, const void* v_dev,
                              int64_t q_sb, int64_t q_sh, int64_t q_sn,
                              int64_t k_sb, int64_t k_sh, int64_t k_sn,
                              int64_t v_sb, int64_t v_sh, int64_t v_sn,
                              const void* mask_dev, int64_t mask_sb, int64_t mask_sq,
                              void* probs_dev, int slab_dtype,
                              void* o_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                              int B, int H, int Nq, int Nk, int D, float scale, int scale_mode,
                              const void* eot_dev, void* stream);
int mmx_attn_capture_bwd_live(const void* q_dev, const void* k_dev, const void* v_dev,
                              int64_t q_sb, int64_t q_sh, int64_t q_sn,
                              int64_t k_sb, int64_t k_sh, int64_t k_sn,
                              int64_t v_sb, int64_t v_sh, int64_t v_sn,
                              const void* probs_dev, int64_t probs_sb, int slab_dtype,
                              const void* do_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                              void* dprobs_dev,
                              void* dq_dev, void* dk_dev, void* dv_dev,
                              int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                              int64_t dk_sb, int64_t dk_sh, int64_t dk_sn,
                              int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                              int B, int H, int Nq, int Nk, int D, float scale, int scale_mode,
                              int need_dqkv, const void* eot_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Attention forward WITHOUT a capture slab: O = softmax(scale.Q.K^T + mask).V and nothing else.  The inference forward of the
 * perturbation test (vit_perturbation.py), whose S x B re-runs of the model never look at P.  Arguments, layouts, mask
 * broadcast strides and both scale modes as mmx_attn_capture_fwd, minus `probs_dev`; exact fp32; the same shape space as the
 * fp32 capture forward (head_dim <= 64, else MMX_ENOTSUP), served by the same three kernel families under the same rules:
 *   - where the capture forward runs its whole-head kernel (Nk <= 128, Nq <= 256, head_dim % 4 == 0, aligned views): that
 *     kernel with the P store compiled out -- O is bit-identical to the capture forward's;
 *   - longer sequences: ONE sweep over the keys with a running row maximum (the accumulators are rescaled when the maximum
 *     moves, one division at the end): two products per key tile instead of the capture forward's three.  Same result up
 *     to fp32 rounding; a fully masked row is NaN as there;
 *   - any other head_dim / unaligned views: the general tiled kernel with the store compiled out.
 * Every argument is checked before any HIP call (MMX_EINVAL). */
int mmx_attn_fwd(const void* q_dev, const void* k_dev, const void* v_dev,
                 int64_t q_sb, int64_t q_sh, int64_t q_sn,
                 int64_t k_sb, int64_t k_sh, int64_t k_sn,
                 int64_t v_sb, int64_t v_sh, int64_t v_sn,
                 const void* mask_dev, int64_t mask_sb, int64_t mask_sq,
                 void* o_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                 int B, int H, int Nq, int Nk, int D, float scale, int scale_mode, void* stream);

/* mmx_attn_fwd with a LIVE LENGTH per sample: the no-slab forward of the row-list inference route of a causally masked text tower
 * (Transformer.forward_nocapture(live=...), the re-runs of the caption perturbation test, clip_text_perturbation.py).  Arguments of
 * mmx_attn_fwd plus eot_dev (int64 [B] on the device), placed as in mmx_attn_capture_fwd_live; `mask_dev` must be a causal mask and
 * Nq == Nk (else MMX_EINVAL).  With L = clamp(eot_dev[b], 0, Nq - 1) + 1: no row >= L of q / k / v is read; rows < L of O carry the
 * bits mmx_attn_capture_fwd_live writes to O (which are the bits of mmx_attn_fwd on operands whose rows >= L are zeros); rows >= L of
 * O are NOT written.  Same shape space and option as the capture pair above (mmx_attn_live_shape), else MMX_ENOTSUP and nothing is
 * launched.  Every argument is checked before any HIP call. */
int mmx_attn_fwd_live(const void* q_dev, const void* k_dev, const void* v_dev,
                      int64_t q_sb, int64_t q_sh, int64_t q_sn,
                      int64_t k_sb, int64_t k_sh, int64_t k_sn,
                      int64_t v_sb, int64_t v_sh, int64_t v_sn,
                      const void* mask_dev, int64_t mask_sb, int64_t mask_sq,
                      void* o_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                      int B, int H, int Nq, int Nk, int D, float scale, int scale_mode,
                      const void* eot_dev, void* stream);

/* Patch perturbation test for image models (the positive / negative perturbation test of the paper at patch granularity;
 * evaluator: vit_perturbation.py; same removal order and step counts as the bi-modal evaluators, lxmert/lxmert/perturbation.py:112).
 * mmx_patch_ranks: scores [B, P] fp32 -> ranks [B, P] int32, ranks[b][i] = position of patch i in ONE stable descending order
 *   of row b -- torch.sort(descending=True, stable=True): among equal scores the lower index first, +0.0 == -0.0, NaN before
 *   +inf.  1 <= P <= 4096 (a 64 x 64 grid), else MMX_EINVAL.  The positive test ranks the negated map (the caller negates).
 * mmx_perturb_patches: images [B, C, R, R] fp32, ranks [B, (R / patch)^2] int32, counts [S] int32 ON THE DEVICE, fill [C] fp32
 *   -> out [S, B, C, R, R]:  out[s][b][c][y][x] = ranks[b][(y / patch) * (R / patch) + x / patch] < counts[s]
 *   ? images[b][c][y][x] : fill[c].  One launch writes all S copies.  R % patch != 0 or S / B / C < 1: MMX_EINVAL.
 * Both check every argument before any HIP call. */
int mmx_patch_ranks(const void* scores_dev, void* ranks_dev, int B, int P, void* stream);
int mmx_perturb_patches(const void* images_dev, const void* ranks_dev, const void* counts_dev, const void* fill_dev,
                        void* out_dev, int B, int C, int R, int patch, int S, void* stream);

/* Token perturbation test for CLIP captions (evaluator: clip_text_perturbation.py): the text half of the reference's bi-modal test,
 * lxmert/lxmert/perturbation.py:158-176 -- the first and the last token always stay, the int((1 - step) * W) top-scoring words stay in
 * their original order, the rest is dropped -- on CLIP's EOT convention (CLIP/clip/model.py:360).  One launch builds the S perturbed
 * copies of B captions:
 *   ids [B, N] int64, scores [B, N] fp32 (one per POSITION), counts [S, N - 1] int32 ON THE DEVICE
 *   -> out_ids [S, B, N] int64, out_eot [S, B] int64, ranks [B, N] int32 (or NULL).
 * Per caption b: e = index of the FIRST maximum of ids[b] (text.argmax(dim=-1); an all-zero row gives 0); the words are the positions
 * 1 <= p < e, W = max(e - 1, 0); scores outside the words are never read.  rank[p] = position of word p in ONE stable descending
 * order of the words' scores, the total order of mmx_patch_ranks (lower index first among equals, +0.0 == -0.0, NaN before +inf);
 * ranks[b][p] receives it at the words and -1 elsewhere.  Step s keeps word p iff rank[p] < counts[s][W]; the host fills
 * counts[s][w] = int((1 - step_s) * w), w = 0 ... N - 2, in host float arithmetic (lxmert/lxmert/perturbation.py:112) -- the kernel
 * does no float arithmetic on steps.  out_ids[s][b] = [ids[b][0], kept words in ascending position, ids[b][e], 0, ...] and
 * out_eot[s][b] = 1 + kept (e = 0: [ids[b][0], 0, ...] and 0), so argmax(out_ids[s][b]) == out_eot[s][b].  The positive test ranks
 * the negated scores (the caller negates).  2 <= N <= 256, 1 <= S <= 64, B >= 1, else MMX_EINVAL; every argument is checked before
 * any HIP call. */
int mmx_perturb_tokens(const void* ids_dev, const void* scores_dev, const void* counts_dev, void* out_ids_dev, void* out_eot_dev,
                       void* ranks_dev, int B, int N, int S, void* stream);

/* Perturbation test of the single-stream (VisualBERT-style) model for a PADDED batch of ragged questions (evaluator:
 * visualbert_perturbation.py; VisualBERT/mmf/trainers/core/evaluation_loop.py:100-159).  Layout as for the mmx_selfattn_* baselines:
 * the sequence is [T text positions | V regions], cam is the [B, T + V] fp32 relevancy row in the padded layout, text_len a DEVICE
 * array of B int32, CLAMPED inside the kernels to 3 .. T before any use (so a length outside it never indexes out of bounds).  Both
 * rank with the ONE stable descending order of mmx_patch_ranks (lower index first among equals, +0.0 == -0.0, NaN before +inf);
 * positive != 0 ranks the negated scores.  Nothing is read back; no atomics, no workspace, workgroups independent of each other.
 * Limits: T >= 3, V >= 1, T + V <= 256, at most 64 steps / groups, B >= 1, else MMX_EINVAL; null pointers and an output that overlaps
 * an input or another output are refused the same way.  Every argument is checked before any HIP call.
 *
 * mmx_selfattn_perturb_regions: the image test (evaluation_loop.py:100-127; the physical gather of the kept regions, :113-120).
 *   emb [B, T + V, E] fp32: the embedded and LayerNorm-ed rows of every item (row-wise, so computed once and shared by all steps;
 *   a visual token has no index-dependent term, VisualBERT/mmf/modules/embeddings.py:399-417, so a gather in any order is the same
 *   model); counts [G] int32 ON THE DEVICE, the DISTINCT keep counts c_0 > c_1 > ... (each clamped to 0 .. V), built once by the
 *   host from int((1 - step) * V) (evaluation_loop.py:111).
 *   -> x [R, E] fp32, R = B * sum_g (T + c_g): the sequence (g, b) starts at row off_g + b * (T + c_g), off_g = B * sum_{h < g} (T + c_h),
 *      and holds the T text rows of item b as they are, then emb[b, T + order_b[j]] for j < c_g (order_b: the regions by rank);
 *      mask [R] fp32: the additive key mask, -10000.0 at text positions >= text_len[b], 0 elsewhere;
 *      pooled [G, B] int64: the packed row of token text_len[b] - 2 (the token the 'vqa' pooler reads);
 *      ranks [B, V] int32 (or NULL): == mmx_patch_ranks of the (negated) region scores.
 *   R is what the host sized x / mask for; a sequence that would end past it (counts that do not match R) is not written.
 *   One workgroup per (b, g); each ranks its own V scores in LDS (V^2 compares) and streams its rows with 16-byte loads / stores when
 *   E % 4 == 0 and emb / x are 16-byte aligned, one float at a time otherwise.  Besides the shared limits: 1 <= E <= 2^20 and
 *   B * G <= 2^31 - 1 (the grid is one-dimensional), else MMX_EINVAL.  mmx_selfattn_perturb_text has no upper limit on B.
 *
 * mmx_selfattn_perturb_text: the text test (evaluation_loop.py:129-159).  ids / segments [B, T] int64, counts [S, T] int32 ON THE
 *   DEVICE with counts[s][w] = int((1 - step_s) * w) in host arithmetic (:140).  Per question, n = the clamped length, c = n - 2: the
 *   words are the positions 1 .. c - 1 (W = n - 3 of them, scores cam[b, 1 .. c - 1], :135), positions 0, c, c + 1 always stay
 *   (:147); step s keeps word p iff rank[p] < counts[s][W].
 *   -> out_ids / out_segments / out_mask [S, B, T] int64: the kept positions in their original order, left-aligned, zeros behind them
 *      (mask 1 at the kept); new_len [S, B] int64 = 3 + kept.
 *   One wave per question, the structure (and the key / counting / compaction code) of mmx_perturb_tokens. */
int mmx_selfattn_perturb_regions(const void* emb_dev, const void* cam_dev, const void* text_len_dev, const void* counts_dev,
                                 void* x_dev, void* mask_dev, void* pooled_dev, void* ranks_dev, int B, int T, int V, int E, int G,
                                 int64_t R, int positive, void* stream);
int mmx_selfattn_perturb_text(const void* ids_dev, const void* segments_dev, const void* cam_dev, const void* text_len_dev,
                              const void* counts_dev, void* out_ids_dev, void* out_segments_dev, void* out_mask_dev, void* new_len_dev,
                              int B, int T, int V, int S, int positive, void* stream);

/* Text perturbation test of the two-stream (LXMERT) model for a PADDED batch of ragged questions (evaluator: lxmert_perturbation.py;
 * lxmert/lxmert/perturbation.py:160-178): [CLS] and [SEP] always stay, the int((1 - step) * W) top-scoring words stay in their original
 * order, left-aligned so that the position embeddings see 0, 1, 2, ..., the rest is dropped.  One launch builds the S perturbed copies
 * of B questions and writes each step's sequences where the caller wants them, at the caller's width:
 *   ids / types [B, T] int64, cam [B, T] fp32 (one score per POSITION), text_len [B] int32 ON THE DEVICE, CLAMPED inside the kernel to
 *   2 .. T before any use, counts [S, T - 1] int32 ON THE DEVICE with counts[s][w] = int((1 - step_s) * w) in host arithmetic (:168),
 *   place [S][3] int64 IN HOST MEMORY: base_s, stride_s, width_s (copied into the kernel's arguments: S <= 64).
 * Per question, n = the clamped length: the words are the positions 1 .. n - 2 (W = n - 2 of them), positions 0 and n - 1 always stay;
 * rank[p] = position of word p in ONE stable descending order of the words' scores, the total order of mmx_patch_ranks (lower index
 * first among equals, +0.0 == -0.0, NaN before +inf); positive != 0 ranks the negated scores; scores outside the words are never
 * read.  Step s keeps word p iff rank[p] < counts[s][W].
 *   -> out_ids / out_types int64 and out_mask fp32 (LXMERT's attention_mask is float), out_elems elements each: sequence (s, b)
 *      occupies the elements base_s + b * stride_s + [0, width_s) of each and holds the kept positions in ascending order, then zeros
 *      (mask 1.0 at the kept).  The kernel writes all width_s elements and nothing outside them; a sequence longer than width_s is
 *      TRUNCATED there, never overrun.  2 + int((1 - step_s) * (T - 2)) bounds the new length of every question of the batch;
 *      new_len [S, B] int64 = 2 + kept, untruncated (new_len > width_s: the caller's width was too small);
 *      ranks [B, T] int32 (or NULL): the rank at the words, -1 elsewhere.
 * One wave per question on the key / counting / compaction code of mmx_perturb_tokens; no atomics, no workspace, nothing read back,
 * workgroups independent.  MMX_EINVAL with a message, before any HIP call, for: a null pointer (ranks may be NULL); T outside
 * 2 .. 256, S outside 1 .. 64, B < 1, out_elems outside 1 .. 2^40; width_s outside 1 .. T, stride_s < width_s, base_s < 0; a last
 * sequence that ends past out_elems; two steps whose sequences may overlap -- two steps are accepted only if (a) they have the same
 * stride and their windows [base mod stride, + width) are disjoint within a period without wrapping, or (b) their overall ranges
 * [base_s, base_s + (B - 1) * stride_s + width_s) are disjoint; an output that overlaps an input or another output. */
int mmx_lxmert_perturb_text(const void* ids_dev, const void* types_dev, const void* cam_dev, const void* text_len_dev,
                            const void* counts_dev, const int64_t* place_host, void* out_ids_dev, void* out_types_dev,
                            void* out_mask_dev, void* new_len_dev, void* ranks_dev, int64_t out_elems, int B, int T, int S, int positive,
                            void* stream);

/* Row-relevancy mode of the backward (BASELINE config 5; CLIP `interpret`, CLIP/clip/... notebook cell 7:27-37, returns
 * only `R[:, 0, 1:]` of the image tower): row 0 of  R_final = (I + A_L) ... (I + A_start)  is  e_0^T (I + A_L) ... , i.e.
 * a ROW vector carried from the top layer down -- the order the backward visits the layers anyway:
 *     rel_out[b] = rel_in[b] + rel_in[b] . A_bar_l[b],   A_bar_l = mean_h clamp(dP * P, 0).
 * The query-side kernel reduces that product from the dP / P values it already holds (deterministic: per-workgroup
 * partial rows summed in a fixed order), so for this layer dP is neither written nor re-read and no N x N A_bar or R
 * exists.  Same arguments as mmx_attn_capture_bwd_ex plus the two rows (`rel_in_dev`, `rel_out_dev`: fp32 [B, Nq],
 * may not alias); `dprobs_dev` may be NULL; `slab_dtype` must carry MMX_ATTN_MMA_BF16; Nq == Nk. */
size_t mmx_attn_capture_bwd_rowrel_workspace_bytes(int B, int H, int Nq, int Nk);
int mmx_attn_capture_bwd_rowrel(const void* q_dev, const void* k_dev, const void* v_dev,
                                int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                int64_t v_sb, int64_t v_sh, int64_t v_sn,
                                const void* probs_dev, int64_t probs_sb, int slab_dtype,
                                const void* do_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                                const void* fwd_o_dev, int64_t fo_sb, int64_t fo_sh, int64_t fo_sn,
                                void* dprobs_dev,
                                void* dq_dev, void* dk_dev, void* dv_dev,
                                int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                                int64_t dk_sb, int64_t dk_sh, int64_t dk_sn,
                                int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                                int B, int H, int Nq, int Nk, int D, float scale, int scale_mode,
                                int need_dqkv, const void* rel_in_dev, void* rel_out_dev,
                                void* workspace_dev, size_t workspace_bytes, void* stream);

/* Row-relevancy mode on the EXACT-fp32 kernels (ViT `generate_relevance` / CLIP `interpret` over a batch of distinct images:
 * both need only row 0 of R): the same row update as mmx_attn_capture_bwd_rowrel with the products on
 * v_mfma_f32_16x16x4_f32, as in mmx_attn_capture_bwd_ex.  N <= 128: the whole-head kernel reduces one partial row per head;
 * longer sequences: the streaming query-side kernel, one partial row per (head, 64-row tile); both summed in a fixed order
 * (deterministic).  dq / dk / dv are bit-identical to mmx_attn_capture_bwd_ex on the same arguments; clamp(NaN, 0) = NaN as in
 * mmx_avg_heads_vecmat.  Same arguments as mmx_attn_capture_bwd_rowrel; `slab_dtype` must be MMX_F32 (no flags); Nq == Nk;
 * `dprobs_dev` may be NULL, except with need_dqkv on the streaming path (its key side reads dP back): MMX_EINVAL there. */
size_t mmx_attn_capture_bwd_rowrel_f32_workspace_bytes(int B, int H, int Nq, int Nk);
int mmx_attn_capture_bwd_rowrel_f32(const void* q_dev, const void* k_dev, const void* v_dev,
                                    int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                    int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                    int64_t v_sb, int64_t v_sh, int64_t v_sn,
                                    const void* probs_dev, int64_t probs_sb, int slab_dtype,
                                    const void* do_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                                    const void* fwd_o_dev, int64_t fo_sb, int64_t fo_sh, int64_t fo_sn,
                                    void* dprobs_dev,
                                    void* dq_dev, void* dk_dev, void* dv_dev,
                                    int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                                    int64_t dk_sb, int64_t dk_sh, int64_t dk_sn,
                                    int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                                    int B, int H, int Nq, int Nk, int D, float scale, int scale_mode,
                                    int need_dqkv, const void* rel_in_dev, void* rel_out_dev,
                                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* Grouped row mode: K targets per image over a batch of M = n_images distinct images in one call (CLIP/example.py:8-32 with the
 * top-K prompts of every image; CLIP_explainability.ipynb cell 6, caption i against image i, with K captions per image; the ViT
 * notebook's two classes per image).  `B` is the TARGET count T = M * K, in K-major order: target t explains image t % M.
 * Per IMAGE (batch index t % M, with their given batch strides): q, k, v, probs (probs_sb) and the forward's O (fwd_o_dev).
 * Per TARGET (batch t): do, dq / dk / dv, dprobs (where written) and rel_in / rel_out.  Every target computes exactly what
 * mmx_attn_capture_bwd_rowrel_f32 computes on per-target copies of its image's operands (bit-identical, NaN policy included);
 * an image's K targets run next to each other on one XCD (its P / K / V come from L2).  Same arguments as that entry plus
 * `n_images`; MMX_EINVAL when n_images < 1 or B % n_images != 0 (checked before any HIP call), otherwise the same refusals
 * (MMX_EINVAL / MMX_ENOTSUP / MMX_EWORKSPACE) for the same reasons.  The workspace is per target: query it with B = T. */
size_t mmx_attn_capture_bwd_rowrel_f32_grouped_workspace_bytes(int B, int H, int Nq, int Nk);
int mmx_attn_capture_bwd_rowrel_f32_grouped(const void* q_dev, const void* k_dev, const void* v_dev,
                                            int64_t q_sb, int64_t q_sh, int64_t q_sn,
                                            int64_t k_sb, int64_t k_sh, int64_t k_sn,
                                            int64_t v_sb, int64_t v_sh, int64_t v_sn,
                                            const void* probs_dev, int64_t probs_sb, int slab_dtype,
                                            const void* do_dev, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                                            const void* fwd_o_dev, int64_t fo_sb, int64_t fo_sh, int64_t fo_sn,
                                            void* dprobs_dev,
                                            void* dq_dev, void* dk_dev, void* dv_dev,
                                            int64_t dq_sb, int64_t dq_sh, int64_t dq_sn,
                                            int64_t dk_sb, int64_t dk_sh, int64_t dk_sn,
                                            int64_t dv_sb, int64_t dv_sh, int64_t dv_sn,
                                            int B, int H, int Nq, int Nk, int D, float scale, int scale_mode,
                                            int need_dqkv, const void* rel_in_dev, void* rel_out_dev, int n_images,
                                            void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * K2-DETR: the decoder half of DETR's rule schedule for ROWS of R_q_i -- rules 5, 6, 7 and 10 with
 * eq. 8-9 and the NaN policy of DETR/modules/ExplanationGenerator.py:19-53 (rule functions), :120-140 (handle_co_attn_*) --
 * in four launches for all decoder layers.  For sample k and explained query t_k = targets[k]:
 *     s[k][:] = sum_l clean_l ? u_l . N(R_qq^(l))^T . C_l : 0,     u_l = e_t^T (I + B_L) ... (I + B_(l+1)),
 * B_l / C_l = mean_h clamp(grad * attn, 0) of decoder layer l's self- / cross-attention, R_qq^(l) = (I + B_l) ... (I + B_1),
 * N = handle_residual; clean_l = no NaN in N(R_qq^(l)) nor in C_l (the reference zeroes the NaNs of the rule-10 addition,
 * :42).  The caller finishes row t_k of R_q_i as s . N(R_ii) (mmx_chain_vecmat over the encoder maps).
 * Layer tables are HOST arrays of device pointers: self_* [K | 1, H, Q, Q], cross_* [K | 1, H, Q, Ni] fp32 contiguous;
 * *_attn_bstride = batch stride of the probability slabs in elements, 0 when ONE forward is shared by the K samples; the
 * gradient slabs are always per sample.  targets_dev: int64 [K].  s_out_dev: fp32 [K, Ni].  diag_min_dev (may be NULL):
 * min over samples and layers of diag(R_qq^(l) - I), the value handle_residual asserts to be >= 0.  Q <= 128.
 */
size_t mmx_detr_decoder_rows_workspace_bytes(int n_layers, int K, int Q, int Ni);
int mmx_detr_decoder_rows(const void* const* self_attn, const void* const* self_grad, const void* const* cross_attn,
                          const void* const* cross_grad, int n_layers, int K, int H, int Q, int Ni,
                          int64_t self_attn_bstride, int64_t cross_attn_bstride, const void* targets_dev,
                          void* s_out_dev, void* diag_min_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The attention-only baselines of DETR for ALL K kept queries of one image in one pass (csrc/detr_baselines.hip): raw attention
 * (DETR/modules/ExplanationGenerator.py:226-238), rollout (:240-273 with compute_rollout_attention, :5-16) and attention GradCAM
 * (:275-305).  Every method returns row t_k = targets[k] of a [Q, Ni] map, out [K, Ni] fp32, and works on row vectors only.
 * Notation: P_x [H, Q, Ni] the LAST decoder layer's cross-attention slab, A_l [H, Ni, Ni] the encoder self-attention slabs,
 * B_l [H, Q, Q] the decoder self-attention slabs, a bar = (sum_h .) / H, M^ = (Mbar + I) / rowsum(Mbar + I).
 *
 * mmx_detr_cross_rows:
 *   cross_grad_dev == NULL: raw attention, out[k, :] = Pbar_x[t_k, :]; one launch, no workspace (workspace_dev may be NULL).
 *   cross_grad_dev given:   GradCAM.  w[k, h] = (sum_{q, j} grad[k, h, q, j]) / float(Q Ni), the sum over the WHOLE [Q, Ni] block as
 *                           grad.mean([1, 2]) states it (rows q != t_k are not assumed to be zero), the sum first, then one division;
 *                           out[k, :] = max(0, (sum_h P_x[h, t_k, :] w[k, h]) / H) (a NaN stays a NaN).  grad_bstride (elements) is
 *                           H Q Ni for per-sample gradient slabs [K, H, Q, Ni] or 0 when ONE slab [H, Q, Ni] serves every k.  Two
 *                           launches: (k, h, strip of 8192 floats) sums into the workspace, then (k, 256 columns) adds the strips'
 *                           sums in order.  workspace: mmx_detr_cross_rows_workspace_bytes(K, H, Q, Ni), 16-byte aligned.
 * mmx_detr_rollout_rows: with R_qq = B^_Ld ... B^_1 and R_ii = A^_Le ... A^_1, row t_k of R_qq^T (Pbar_x R_ii) is
 *   ((R_qq e_t)^T Pbar_x) R_ii:   1. u_k = B^_Ld( ... (B^_1 e_t)),  y <- (Bbar_l y + y) / r_l, r_l[i] = 1 + sum_j Bbar_l[i, j];
 *   2. s_k = u_k^T Pbar_x;   3. x <- s_k, for l = Le ... 1: x <- w Abar_l + w, w[i] = x[i] / r_l[i], r_l[i] = 1 + sum_j Abar_l[i, j].
 *   No Ni x Ni product exists.  enc_table / dec_self_table: HOST tables of n_enc / n_dec device slabs, entry 0 the FIRST layer.
 *   Every slab is read once: Le x ceil(Ni / 4) workgroups take the head mean of strips of four rows (one contiguous, 16-byte aligned
 *   run per head, 16-byte loads) into the workspace with r_l; the K vectors then go through each layer's head mean together, a strip of
 *   eight rows and eight vectors per workgroup, partials per strip summed in strip order by the next launch.  Le H Ni^2 4 bytes of
 *   slabs (173 MB at 950 tokens) plus Le Ni^2 4 of head means written and read back.
 *   workspace: mmx_detr_rollout_rows_workspace_bytes(n_enc, n_dec, K, Q, Ni) bytes, 16-byte aligned, caller-owned, stream-ordered.
 * targets_dev: int64 [K] on the device, clamped to 0 .. Q - 1 inside the kernels before they form an address.
 * Limits: 1 <= Q <= 128, 1 <= Ni <= 2048, 1 <= H <= 32, 1 <= K <= 2^20, tables of 1 .. MMX_BASELINES_MAX_TABLE entries, fp32
 * contiguous slabs.  Plain launches ordered by the stream, fixed summation orders, no atomics: two calls give the same bits, and row
 * k's bits depend neither on K nor on k's position.  Every argument is checked before any HIP call: a null required pointer or table
 * entry, a size outside the limits, a grad_bstride that is neither 0 nor H Q Ni, a workspace that is too small or not 16-byte
 * aligned, an output or workspace that overlaps an input or the other one return MMX_EINVAL with a message in mmx_last_error().
 * The workspace queries return 0 for arguments the entries refuse. */
size_t mmx_detr_cross_rows_workspace_bytes(int K, int H, int Q, int Ni);
int mmx_detr_cross_rows(const void* cross_attn_dev, const void* cross_grad_dev, int64_t grad_bstride, const void* targets_dev,
                        void* out_dev, int K, int H, int Q, int Ni, void* workspace_dev, size_t workspace_bytes, void* stream);
size_t mmx_detr_rollout_rows_workspace_bytes(int n_enc, int n_dec, int K, int Q, int Ni);
int mmx_detr_rollout_rows(const void* const* enc_table, int n_enc, const void* const* dec_self_table, int n_dec,
                          const void* cross_attn_dev, const void* targets_dev, void* out_dev, int K, int H, int Q, int Ni,
                          void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * LRP relevance through the attention core: the two `einsum` relprops inside the reference's
 * MultiheadAttention.relprop (DETR/modules/layers.py:770-781; einsum = RelPropSimple, layers.py:54-66, each result halved;
 * softmax / dropout relprops are the identity, layers.py:170-186), which the reference evaluates by re-running the einsums
 * and calling torch.autograd.grad.  With S = safe_divide(cam_O, O) (layers.py:11-14) and Z = (scale q).k^T:
 *   cam_P = P * (S.V^T) / 2   (-> cam_probs_dev, what the reference stores with save_attn_cam, layers.py:776)
 *   cam_V = V * (P^T.S) / 2,   S1 = safe_divide(cam_P, Z),   cam_Q = (scale q) * (S1.k) / 2,   cam_K = k * (S1^T.(scale q)) / 2
 * q / k / v / o / cam_o and the three outputs use the (batch, head, token) element strides of the capture op; probs and
 * cam_probs are [B, H, Nq, Nk] fp32 contiguous.  MMX_SCALE_Q_FIRST: q is multiplied by `scale` first (DETR, layers.py:741);
 * MMX_SCALE_SCORES: Z is the raw q.k^T product (BERT-style modules divide afterwards).  head_dim <= 64.  Two launches
 * (query side, then key side) on `stream`; no workspace.
 */
int mmx_attn_relprop(const void* q_dev, const void* k_dev, const void* v_dev, const void* o_dev, const void* cam_o_dev,
                     int64_t q_sb, int64_t q_sh, int64_t q_sn, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                     int64_t v_sb, int64_t v_sh, int64_t v_sn, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                     int64_t co_sb, int64_t co_sh, int64_t co_sn,
                     const void* probs_dev, void* cam_probs_dev, void* cam_q_dev, void* cam_k_dev, void* cam_v_dev,
                     int64_t cq_sb, int64_t cq_sh, int64_t cq_sn, int64_t ck_sb, int64_t ck_sh, int64_t ck_sn,
                     int64_t cv_sb, int64_t cv_sh, int64_t cv_sn,
                     int B, int H, int Nq, int Nk, int D, float scale, int scale_mode, void* stream);

/* The same core in halves (BertSelfAttention.relprop, VisualBERT/mmf/models/transformers/backends/BERT_ours.py:345-395, applies
 * Add.relprop of [scores / sqrt(d), attention_mask] -- a rule with whole-tensor sums -- between the two matmul relprops):
 *   MMX_LRP_VALUES: cam_P (-> cam_probs_dev) and cam_V from cam_O;  q / k are still read (tiling), cam_q / cam_k may be NULL.
 *   MMX_LRP_SCORES: cam_Q and cam_K from S1 = safe_divide(cam_scores, Z);  cam_scores_dev [B, H, Nq, Nk] fp32 = the relevance of
 *                   the pre-softmax scores the caller derived from cam_P;  v / o / cam_o / probs / cam_probs / cam_v may be NULL.
 * MMX_LRP_VALUES | MMX_LRP_SCORES with cam_scores_dev == NULL is mmx_attn_relprop (LxmertAttention.relprop,
 * lxmert/lxmert/src/lxmert_lrp.py:422-461: its attention_mask slot is never assigned, the Add rule is skipped). */
#define MMX_LRP_VALUES 1
#define MMX_LRP_SCORES 2
int mmx_attn_relprop_phase(const void* q_dev, const void* k_dev, const void* v_dev, const void* o_dev, const void* cam_o_dev,
                           int64_t q_sb, int64_t q_sh, int64_t q_sn, int64_t k_sb, int64_t k_sh, int64_t k_sn,
                           int64_t v_sb, int64_t v_sh, int64_t v_sn, int64_t o_sb, int64_t o_sh, int64_t o_sn,
                           int64_t co_sb, int64_t co_sh, int64_t co_sn,
                           const void* probs_dev, void* cam_probs_dev, void* cam_q_dev, void* cam_k_dev, void* cam_v_dev,
                           int64_t cq_sb, int64_t cq_sh, int64_t cq_sn, int64_t ck_sb, int64_t ck_sh, int64_t ck_sn,
                           int64_t cv_sb, int64_t cv_sh, int64_t cv_sn,
                           int B, int H, int Nq, int Nk, int D, float scale, int scale_mode,
                           const void* cam_scores_dev, int phase, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused elementwise halves of the alpha-beta LRP layer rules (csrc/lrp_kernels.hip).  All tensors
 * fp32, contiguous, device pointers; stream-ordered; deterministic two-stage sums.  workspace: mmx_lrp_workspace_bytes().
 *   mmx_lrp_split_signs    out [rows, 2n] = [clamp(x, min=0) | clamp(x, max=0)]                (Linear.relprop's px / nx,
 *                          DETR/modules/layers.py:411-414; the same split of W is cached by the caller)
 *   mmx_lrp_safe_divide    out = safe_divide(a, b)                                              (layers.py:11-14)
 *   mmx_lrp_linear_combine out [rows, n] = xx[:, :n] * y[:, :n] + xx[:, n:] * y[:, n:]           (layers.py:424-430, alpha = 1);
 *                          r_dev != NULL: then out *= safe_divide(sum(r), sum(out))             (layers.py:432, DETR flavour)
 *   mmx_lrp_add_relprop    Add.relprop (layers.py:197-222) on [batch, per] views: the three sums per batch item (batch = 1:
 *                          whole-tensor sums, the reference's one-sample pass)
 *   mmx_lrp_clone_relprop  Clone.relprop (layers.py:257-267): out = x * sum_i safe_divide(r_i, x), r_list = HOST array of
 *                          n_r <= 8 device pointers
 */
size_t mmx_lrp_workspace_bytes(void);
int mmx_lrp_split_signs(const void* x_dev, void* out_dev, int64_t rows, int n, void* stream);
int mmx_lrp_safe_divide(const void* a_dev, const void* b_dev, void* out_dev, int64_t n, void* stream);
int mmx_lrp_linear_combine(const void* xx_dev, const void* y_dev, void* out_dev, int64_t rows, int n,
                           const void* r_dev, int64_t r_numel, void* workspace_dev, void* stream);
int mmx_lrp_add_relprop(const void* r_dev, const void* a_dev, const void* b_dev, void* ra_dev, void* rb_dev,
                        int batch, int64_t per, void* workspace_dev, void* stream);
int mmx_lrp_clone_relprop(const void* const* r_list, int n_r, const void* x_dev, void* out_dev, int64_t n, void* stream);
/* MultiheadAttention.relprop's closing q / k rescale (DETR/modules/layers.py:791-799), two launches, in place on cam_k / cam_q:
 * if all_zero(cam_v after its projection rule) and not all_zero(cam_v before it), cam_k *= safe_divide(|ks| / (|ks| + |qs|) *
 * sum(cam_o), ks) and cam_q likewise (ks, qs = their sums).  n_*: element counts. */
int mmx_lrp_mha_rescale(const void* v_pre_dev, int64_t n_vpre, const void* v_post_dev, int64_t n_vpost, void* cam_k_dev,
                        int64_t n_k, void* cam_q_dev, int64_t n_q, const void* cam_o_dev, int64_t n_o,
                        void* workspace_dev, void* stream);


/* ---------------------------------------------------------------------------------------------
 * Fused QuickGELU of the CLIP body's MLP, y = x * sigmoid(1.702 x) (CLIP/clip/model.py:162-164): one HBM pass forward,
 * one backward (dx from x and dy; nothing saved but x) instead of PyTorch's 3 + 5 elementwise kernels.
 * fp32, contiguous, 16-byte aligned, n elements.
 */
int mmx_quick_gelu_fwd(const void* x_dev, void* y_dev, int64_t n, void* stream);
/* x * sigmoid(1.702 x) with a bf16 result (n % 4 == 0): the activation of a bf16 body only feeds the next GEMM */
int mmx_quick_gelu_fwd_bf16(const void* x_dev, void* y_dev, int64_t n, void* stream);
int mmx_quick_gelu_bwd(const void* x_dev, const void* dy_dev, void* dx_dev, int64_t n, void* stream);
/* Same with x ([x_n] elements) broadcast over the leading dimension of dy / dx ([n] elements, n % x_n == 0, x_n % 4 == 0):
 * the shared-forward backward has ONE activation tensor for B upstream gradients. */
/* bf16 gradient stream (BASELINE config 5's bf16 body): dy / dx bf16, x fp32 (broadcast over the batch as above; x_n % 8 == 0);
 * LayerNorm backward + residual with a bf16 upstream gradient, written as fp32 (`dx_dev`, the next residual) and / or bf16
 * (`dx_bf16_dev`, the next GEMM's operand) -- either may be NULL.  Shapes as mmx_layernorm_bwd_add below; x, gamma, d_res and dx
 * 16-byte aligned, the bf16 dy and dx_bf16 8-byte (MMX_EINVAL otherwise: there is no misaligned route, every kernel behind this entry
 * takes 8- and 16-byte groups). */
int mmx_quick_gelu_bwd_bcast_bf16(const void* x_dev, const void* dy_dev, void* dx_dev, int64_t n, int64_t x_n, void* stream);
int mmx_layernorm_bwd_add_bf16(const void* dy_dev, const void* x_dev, const void* mean_dev, const void* rstd_dev,
                               const void* gamma_dev, const void* d_res_dev, void* dx_dev, void* dx_bf16_dev,
                               int64_t rows, int x_rows, int E, void* stream);
int mmx_quick_gelu_bwd_bcast(const void* x_dev, const void* dy_dev, void* dx_dev, int64_t n, int64_t x_n, void* stream);

/* LayerNorm input gradient + residual add with forward statistics shared by the batch (shared-forward backward of the
 * CLIP image tower / ViT): dx[r] = d_res[r] + LN'(dy[r]; x[r % x_rows], mean, rstd, gamma).  dy, d_res (may be NULL),
 * dx: [rows, E]; x: [x_rows, E]; mean, rstd: [x_rows]; gamma: [E]; fp32 contiguous, E % 4 == 0; dy, x, gamma, d_res and dx
 * 16-byte aligned (MMX_EINVAL otherwise; the row-list form mmx_layernorm_bwd_add_rows asks the same). */
int mmx_layernorm_bwd_add(const void* dy_dev, const void* x_dev, const void* mean_dev, const void* rstd_dev,
                          const void* gamma_dev, const void* d_res_dev, void* dx_dev, int64_t rows, int x_rows, int E,
                          void* stream);

/* Residual add fused with the LayerNorm that follows it in a pre-LN block (CLIP/clip/model.py:195-197: x = x + attn(...);
 * ... ln_2(x)): sum = x + y (written to sum_dev: the next residual), h = LayerNorm(sum) * gamma + beta, and the row
 * statistics mean / rstd that mmx_layernorm_bwd_add consumes.  y_dev == NULL: plain LayerNorm of x (sum_dev unused).
 * x, y, sum, h: [rows, E]; mean, rstd: [rows]; gamma, beta: [E]; fp32 contiguous, E % 4 == 0, E <= 4096; x, y, gamma, beta, sum
 * and h 16-byte aligned (a bf16 h: 8-byte; MMX_EINVAL otherwise; mmx_add_layernorm_fwd_rows asks the same). */
int mmx_add_layernorm_fwd(const void* x_dev, const void* y_dev, const void* gamma_dev, const void* beta_dev,
                          void* sum_dev, void* h_dev, void* mean_dev, void* rstd_dev, int64_t rows, int E, float eps,
                          void* stream);
/* The same with h_dtype = MMX_F32 | MMX_BF16: a bf16 body (CLIP/clip/model.py:381-402 converts the weights to half precision) feeds
 * h to a half-precision GEMM only, so the kernel writes it as bf16 (round to nearest even) instead of a conversion pass. */
int mmx_add_layernorm_fwd_ex(const void* x_dev, const void* y_dev, const void* gamma_dev, const void* beta_dev,
                             void* sum_dev, void* h_dev, void* mean_dev, void* rstd_dev, int64_t rows, int E,
                             float eps, int h_dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kernel timing helper for bench.py: runs `fn`-independent HIP-event timing on `stream` is done in
 * Python via these thin wrappers so that events live on the SAME stream the kernels are launched on.
 */
int mmx_event_create(void** event_out);
int mmx_event_destroy(void* event);
int mmx_event_record(void* event, void* stream);
int mmx_event_elapsed_ms(void* start, void* stop, float* ms_out); /* synchronises on `stop` */

#ifdef __cplusplus
}
#endif
#endif /* MMX_RELEVANCY_H */
