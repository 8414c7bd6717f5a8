// Argument blocks shared by the tiled (attention_kernels.hip), whole-head (attention_head.hip), streaming (attention_stream.hip)
// and bf16-MFMA (attention_bf16.hip, attention_bf16_v3.hip) kernels.  The entries of attention_kernels.hip value-initialise one
// (`AttnBwdArgs a{};`) and fill it once; kernels take it by value, so a new member goes behind the last one.
// What those files share besides: attention_align.h (Strides, the one row-alignment test of the eligibility rules),
// attention_launch.h (the launch helper and the head-dim / slab-type / key-tile dispatches), attention_bf16_words.h (device side:
// packed-bf16 words, exp_fast, the LDS tile layouts of the bf16-MFMA generations).
#pragma once
#include "mmx_common.h"
#include "attention_align.h"

namespace mmx {

struct AttnFwdArgs {
    const float *q, *k, *v;
    Strides qs, ks, vs;
    const float* mask; int64_t mask_sb, mask_sq;
    float* probs; float* o; Strides os;
    int B, H, Nq, Nk, D;
    float scale; int scale_mode;
    int debug;  // profiling only (attention_head.hip); 0 from every entry
    int slab_dt;  // MMX_F32 | MMX_F16 | MMX_BF16: element type behind `probs` (non-fp32: streaming kernels only)
    int mma_bf16; // 1: products on v_mfma_f32_16x16x32_bf16 (operands rounded to bf16, fp32 accumulate, fp32 softmax)
    int tile_skip = 0;  // whole-head kernels: skip the products of key tiles that are masked out for a whole wave (attention_head.hip)
    int no_probs = 0;   // mmx_attn_fwd: inference forward, `probs` is NULL (read by the host dispatchers only: they pick the NOP instantiations)
    // Whole-head kernels, causally masked self-attention only (mmx_attn_capture_fwd_live): eot [B] int64 on the device -- sample b has
    // L = clamp(eot[b], 0, Nq - 1) + 1 live rows (live_rows_kernel's formula, read by the kernel: nothing comes back to the host); no row
    // >= L of q / k / v is read and none of o is written.  nullptr: off.  (Last member: the offsets of the others stay what they were.)
    const long long* eot = nullptr;
};

struct AttnBwdArgs {
    const float *q, *k, *v;
    Strides qs, ks, vs;
    const float* probs; int64_t probs_sb;  // batch stride of P in elements (0: one P shared by the whole batch)
    const float* dout; Strides os;
    const float* o; Strides oos;   // optional forward output O (same logical shape as dout): delta = rowsum(dO * O) without a sweep
    float* dprobs;
    float *dq, *dk, *dv;
    Strides dqs, dks, dvs;
    float* delta;  // [B, H, Nq] workspace: rowsum(dP * P)
    int B, H, Nq, Nk, D;
    float scale; int scale_mode; int need_dqkv;
    int slab_dt;  // element type behind `probs` and `dprobs` (see AttnFwdArgs)
    int debug;    // tuning knob of attention_head.hip (stagger)
    int mma_bf16; // see AttnFwdArgs (streaming kernels only)
    // Row-relevancy mode (mmx_attn_capture_bwd_rowrel, streaming bf16-MFMA kernels only): instead of (or besides) storing
    // dP, every query-side workgroup reduces  part[k] = sum_{q in its 64 rows} rel_v[b][q] * clamp(dP * P, 0)[q][k]  of
    // its head into rel_part[b][h * nrt + row_tile][k]; rel_v == nullptr: off.
    const float* rel_v;
    float* rel_part;
    float* rel_out;   // rel_v + (1 / H) sum of the partial rows: written by the path that ran (it knows how many rows it made)
    // MMX_ATTN_IO_BF16 (bf16-MFMA streaming kernels only): `dout` is bf16 and dq / dk / dv are written as bf16 (the
    // gradient stream between the bf16 GEMMs of a bf16 body); strides stay in elements.  q / k / v / o / delta: fp32.
    int io_bf16;
    int tile_skip = 0;  // whole-head kernels: skip the products of all-zero probability tiles (attention_head.hip, with_tile_count)
    // Grouped row mode (mmx_attn_capture_bwd_rowrel_f32_grouped; exact-fp32 row-relevancy mode only): the B targets are K = grp_k
    // per image over M = B / K images, K-major -- target t explains image t % M.  q / k / v / probs / o are per IMAGE (batch index
    // t % M with their own batch strides); dout, dq / dk / dv, dprobs, delta and the relevancy rows are per TARGET.  0: off.
    int grp_k = 0;
    // see AttnFwdArgs::eot (mmx_attn_capture_bwd_live): no row >= L of q / k / v / dout / o is read, dq / dk / dv are written for the rows
    // < L only, the dP slab is written whole (exact zeros in the rows >= L).  nullptr: off.
    const long long* eot = nullptr;
};

int attn_fwd_head_try(const AttnFwdArgs& a, hipStream_t s, int* rc_out);    // attention_head.hip (register-resident)
int attn_bwd_head_try(const AttnBwdArgs& a, hipStream_t s, int* rc_out);
// is there a live-length (eot) instantiation of the whole-head kernels for this shape, and are they switched on?
bool attn_head_live_shape(int Nq, int Nk, int D);
int attn_fwd_stream_try(const AttnFwdArgs& a, hipStream_t s, int* rc_out);   // attention_stream.hip
int attn_bwd_stream_try(const AttnBwdArgs& a, hipStream_t s, int* rc_out);
// out[b][k] = v_in[b][k] + inv_h * sum_{j < J} part[b][j][k]   (row-relevancy mode, second pass; attention_kernels.hip)
int rel_row_update(const float* v_in, const float* part, float* out, int B, int J, int N, float inv_h, hipStream_t s);
int attn_bwd_bf16_try(const AttnBwdArgs& a, hipStream_t s, int* rc_out);     // attention_bf16.hip (2nd-generation bf16 MFMA backward)
void attn_bf16_v2_enable(int on);
// attention_bf16_v3.hip: third generation, shared-forward + bf16 gradient stream + row-relevancy mode only (BASELINE config 5)
int attn_bwd_bf16_v3_try(const AttnBwdArgs& a, void* prep, size_t prep_bytes, hipStream_t s, int* rc_out);
size_t attn_bwd_bf16_v3_prep_bytes(int H, int N);
void attn_bf16_v3_enable(int mode);

}  // namespace mmx
