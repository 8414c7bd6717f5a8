// K_clip_head: the gradients of CLIP's cosine-similarity head in closed form, forward and backward in ONE launch.
//
// The explained scalar of the caption notebook is  sum_b logits_per_image[b, b]  (CLIP_explainability.ipynb cell 6:6-10) with
// logits_per_image = exp(logit_scale) * i^ . t^T over the normalised features (CLIP/clip/model.py:369-378).  Every pair b owns its
// two feature rows (the notebook repeats the image per caption, cell 6:3), so with i^ = i / |i|, t^ = t / |t|, c = i^ . t^ and
// s = exp(logit_scale):
//     d_img[b] = s (t^ - c i^) / |i|        d_txt[b] = s (i^ - c t^) / |t|        logit_diag[b] = s c
// Autograd spends ~13 forward and ~20 backward launches on 64 rows for this (expand + contiguous, two norms, two divisions, exp, the
// scale, two B x B products of which one is never read, torch.eye, and the backward of all that), each one a dependent kernel
// boundary in front of both towers' backwards.
//
// One wave per pair (a 64-thread workgroup), plain vector stores, no atomics, no hand-off between workgroups, no LDS, no scratch.
// Lane l sums the elements l, l + 64, ... in that order, the 64 partial sums meet in an xor butterfly: the same order in every run,
// so two runs give the same bits.  sqrtf and / are the correctly rounded ones hipcc emits by default; no reciprocal / rsqrt
// approximation anywhere.  logit_scale is read on the device and expf applied here: no host read, no launch of its own.
#include "mmx_common.h"

namespace mmx {

// option "clip_head_fused": 1 (default) interpret / interpret_grouped take the head from this kernel | 0: autograd (A / B runs)
static int g_clip_head_fused = 1;
bool clip_head_option(const char* key, int value) {
    if (strcmp(key, "clip_head_fused") == 0 && value >= 0 && value <= 1) { g_clip_head_fused = value; return true; }
    return false;
}

__global__ __launch_bounds__(64) void clip_head_kernel(const float* img, const float* txt, const float* logit_scale, float* d_img,
                                                       float* d_txt, float* logit_diag, int B, int D, int Bi, int img_group) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const int lane = threadIdx.x;
    const int ib = Bi == 1 ? 0 : b / img_group;                  // < Bi: the host checked Bi * img_group == B
    const float* iv = img + static_cast<int64_t>(ib) * D;
    const float* tv = txt + static_cast<int64_t>(b) * D;
    float ii = 0.f, tt = 0.f, it = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float x = iv[k], y = tv[k];
        ii += x * x;
        tt += y * y;
        it += x * y;
    }
    ii = wave_sum(ii);
    tt = wave_sum(tt);
    it = wave_sum(it);
    const float ni = sqrtf(ii), nt = sqrtf(tt);
    const float c = it / (ni * nt);
    const float s = expf(*logit_scale);
    if (logit_diag && lane == 0) logit_diag[b] = s * c;
    float* di = d_img ? d_img + static_cast<int64_t>(b) * D : nullptr;
    float* dt = d_txt ? d_txt + static_cast<int64_t>(b) * D : nullptr;
    for (int k = lane; k < D; k += 64) {
        const float xh = iv[k] / ni, yh = tv[k] / nt;
        if (di) di[k] = s * (yh - c * xh) / ni;
        if (dt) dt[k] = s * (xh - c * yh) / nt;
    }
}

}  // namespace mmx

using namespace mmx;

extern "C" int mmx_clip_head_fused_enabled(void) { return g_clip_head_fused; }

extern "C" int mmx_clip_head_f32(const void* img_feat_dev, const void* txt_feat_dev, const void* logit_scale_dev, void* d_img_dev,
                                 void* d_txt_dev, void* logit_diag_dev, int B, int D, int Bi, int img_group, void* stream) {
    MMX_CHECK_ARG(img_feat_dev && txt_feat_dev && logit_scale_dev, "mmx_clip_head_f32: null pointer");
    MMX_CHECK_ARG(d_img_dev || d_txt_dev || logit_diag_dev, "mmx_clip_head_f32: null pointer for every output");
    MMX_CHECK_ARG(B > 0 && D > 0 && D <= 4096, "mmx_clip_head_f32: B=%d D=%d (1 <= B, 1 <= D <= 4096)", B, D);
    MMX_CHECK_ARG(Bi > 0 && img_group > 0 && (Bi == 1 || static_cast<int64_t>(Bi) * img_group == B),
                  "mmx_clip_head_f32: Bi=%d image rows x img_group=%d is not B=%d pairs (Bi == 1: one image for every pair)", Bi,
                  img_group, B);
    MMX_CHECK_ARG(d_img_dev != img_feat_dev && d_img_dev != txt_feat_dev && d_txt_dev != img_feat_dev && d_txt_dev != txt_feat_dev,
                  "mmx_clip_head_f32: an output may not alias a feature tensor");
    clip_head_kernel<<<static_cast<unsigned>(B), 64, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float*>(img_feat_dev), static_cast<const float*>(txt_feat_dev), static_cast<const float*>(logit_scale_dev),
        static_cast<float*>(d_img_dev), static_cast<float*>(d_txt_dev), static_cast<float*>(logit_diag_dev), B, D, Bi, img_group);
    MMX_LAUNCH_CHECK("clip_head_kernel");
    return MMX_OK;
}
