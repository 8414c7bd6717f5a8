// The baselines of the bi-modal (LXMERT-style) model for a PADDED batch of ragged questions: raw attention, attention GradCAM and
// rollout (lxmert/lxmert/src/ExplanationGenerator.py:508-540, :542-593, :595-665 with :5-15), and on the LRP cams transformer
// attribution and partial LRP (:373-460, :462-506).
//
// The reference explains one question per call, so nothing of it is ever padded.  In a padded batch the probability slabs are zero
// at padded key columns, but the GRADIENT slabs are not (dP = dO . V^T has a value wherever V has a row), and padded query rows hold
// whatever the body computed for a pad token.  Every kernel here therefore works on sample b's LIVE block only -- the leading
// q_len[b] x k_len[b] entries -- for the sums AND for the divisors, and writes exact zeros everywhere else.  Lengths are device
// int32 arrays; a value outside 1..N is clamped to that range before it bounds a loop or forms an address.
//
//   head_mean_live_kernel   one workgroup per sample: mean_h P[b, h] on the live block, or GradCAM clamp(mean_h(P[b, h] w[b, h]), 0)
//                           with w[b, h] = the mean of G[b, h] over the live block (a wave per head, lanes striding the live block,
//                           xor butterfly).
//   rollout_means_kernel    workgroup (b, k) of B x (n_text + n_img + 1): the head mean of block k of sample b (16-byte loads at
//                           4-byte alignment, heads in order), + I and row normalisation on the live block for the self-attention
//                           blocks, written ONCE to the workspace, zero outside the live block.  Every slab is read exactly once.
//   rollout_chain_kernel    one workgroup per sample: the two left-multiplied products and R_ti = R'^T (C R_ii) with every matrix
//                           in LDS, on the exact-fp32 MFMA tiles of bimodal_tile.h; the next block is in flight (registers) while
//                           the current product runs.
//   attr_means_kernel       workgroup (b, k): A_bar = (sum_h max(0, G_h . C_h)) / H of an LRP cam / gradient pair (avg_heads), the
//                           self-attention blocks to the workspace, the last cross block straight to R_ti (:451).
//   attr_chain_kernel       one workgroup per sample: R <- R + A_bar_l . R from R = I over the text and the image table (transformer
//                           attribution, :373-460), laid out like rollout_chain_kernel.
//   head_minmax_live_kernel one workgroup per sample: the head mean of an LRP cam, min-max normalised over the live block (partial
//                           LRP, :489-505).
// The rollout and attribution pairs are two plain launches each: stream order is the only synchronisation (no tickets, no spinning).
// Fixed summation orders, no atomics: two runs give the same bits, and sample b's result depends neither on B nor on b.
#include "mmx_common.h"
#include "bimodal_tile.h"

namespace mmx {

constexpr int kBlMax = 48;          // tokens per modality (== kBmMax of bimodal_kernels.hip, ops.LXMERT_FUSED_MAX_TOKENS)
constexpr int kBlMaxTable = MMX_BASELINES_MAX_TABLE;
constexpr int kHmThreads = 256;
constexpr int kHmPer = (kBlMax * kBlMax + kHmThreads - 1) / kHmThreads;   // live entries one thread owns (9)
constexpr int kRcThreads = 512;
constexpr int kRcWaves = kRcThreads / 64;

// the clamped length of sample b: NEVER used unclamped
__device__ __forceinline__ int live_len(const int* len, int b, int N) { return len ? min(max(len[b], 1), N) : N; }

__global__ __launch_bounds__(kHmThreads) void head_mean_live_kernel(const float* __restrict__ attn, const float* __restrict__ grad,
                                                                    float* __restrict__ out, int H, int Nq, int Nk,
                                                                    const int* q_len, const int* k_len, unsigned flags) {
    __shared__ float w_lds[64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = live_len(q_len, b, Nq), k = live_len(k_len, b, Nk);
    const int hs = Nq * Nk, live = q * k;
    const float* P = attn + static_cast<int64_t>(b) * H * hs;
    const float* G = grad ? grad + static_cast<int64_t>(b) * H * hs : nullptr;
    float* O = out + static_cast<int64_t>(b) * hs;

    // thread tid owns the live entries n = tid, tid + 256, ... (n counts the live block row by row)
    float acc[kHmPer];
    int off[kHmPer];
#pragma unroll
    for (int u = 0; u < kHmPer; ++u) {
        const int n = tid + u * kHmThreads;
        const int i = n / k;
        off[u] = n < live ? i * Nk + (n - i * k) : -1;
        acc[u] = 0.f;
    }
    if (!G) {
        for (int h = 0; h < H; ++h)
#pragma unroll
            for (int u = 0; u < kHmPer; ++u)
                if (off[u] >= 0) acc[u] += P[static_cast<int64_t>(h) * hs + off[u]];
    } else {
        const float cnt = static_cast<float>(live);
        for (int h0 = 0; h0 < H; h0 += 64) {
            const int nh = min(64, H - h0);
            for (int hh = wave; hh < nh; hh += kHmThreads / 64) {        // w[b, h]: one wave per head, the live block only
                const float* Gh = G + static_cast<int64_t>(h0 + hh) * hs;
                float s = 0.f;
                int i = lane / k, j = lane - i * k;
                for (int n = lane; n < live; n += 64) {
                    s += Gh[i * Nk + j];
                    j += 64;
                    while (j >= k) { j -= k; ++i; }
                }
                s = wave_sum(s);
                if (lane == 0) w_lds[hh] = s / cnt;
            }
            __syncthreads();
            for (int hh = 0; hh < nh; ++hh) {
                const float w = w_lds[hh];
#pragma unroll
                for (int u = 0; u < kHmPer; ++u)
                    if (off[u] >= 0) acc[u] += P[static_cast<int64_t>(h0 + hh) * hs + off[u]] * w;
            }
            __syncthreads();
        }
    }
    const float fH = static_cast<float>(H);
    for (int e = tid; e < hs; e += kHmThreads) {                          // everything outside the live block: exact zeros
        const int i = e / Nk, j = e - i * Nk;
        if (i >= q || j >= k) O[e] = 0.f;
    }
#pragma unroll
    for (int u = 0; u < kHmPer; ++u) {
        if (off[u] < 0) continue;
        float v = acc[u] / fH;
        if (G) v = relu_nan(v);
        if ((flags & MMX_HEAD_MEAN_ZERO_CLS) && off[u] == 0) v = 0.f;
        O[off[u]] = v;
    }
}

struct RolloutArgs {
    const float* text[kBlMaxTable];    // [B, H, T, T]; the last entry is the last x-layer's language self-attention
    const float* img[kBlMaxTable];     // [B, H, I, I]
    const float* cross;                // [B, H, T, I]
    int n_text, n_img, B, H, T, I;
    const int* text_len;
    float* ws;                         // [B][nblk][bs]: blocks in the order text, img, cross, row stride = the block's padded key count
    int bs;
    float *R_tt, *R_ti, *R_ii;
};

constexpr int kRmLd = kBlMax + 1;

__global__ __launch_bounds__(kHmThreads) void rollout_means_kernel(const RolloutArgs a) {
    __shared__ float m[kBlMax * kRmLd];
    __shared__ float rs[kBlMax];
    const int tid = threadIdx.x;
    const int nblk = a.n_text + a.n_img + 1;
    const int b = blockIdx.x / nblk, k = blockIdx.x - b * nblk;
    const int t = live_len(a.text_len, b, a.T);
    const bool is_text = k < a.n_text, is_cross = k == nblk - 1;
    const float* __restrict__ src = is_text ? a.text[k] : is_cross ? a.cross : a.img[k - a.n_text];
    const int Nq = is_text || is_cross ? a.T : a.I, Nk = is_text ? a.T : a.I;
    const int lq = is_text || is_cross ? t : a.I, lk = is_text ? t : a.I;
    const int H = a.H, hs = Nq * Nk;
    const int64_t sample = static_cast<int64_t>(b) * H * hs, slab_end = static_cast<int64_t>(a.B) * H * hs;
    const float fH = static_cast<float>(H);

    for (int c = tid; c * 4 < hs; c += kHmThreads) {
        const int p = c * 4;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (sample + static_cast<int64_t>(H - 1) * hs + p + 3 < slab_end) {     // the 16-byte loads stay inside the slab
            int h = 0;
            for (; h + 6 <= H; h += 6) {
                f32x4 v[6];
#pragma unroll
                for (int u = 0; u < 6; ++u) v[u] = ldg4_u(src + sample + static_cast<int64_t>(h + u) * hs + p);
#pragma unroll
                for (int u = 0; u < 6; ++u) s += v[u];
            }
            for (; h < H; ++h) s += ldg4_u(src + sample + static_cast<int64_t>(h) * hs + p);
        } else {
            for (int e = 0; e < 4 && p + e < hs; ++e)
                for (int h = 0; h < H; ++h) s[e] += src[sample + static_cast<int64_t>(h) * hs + p + e];
        }
        int row = p / Nk, col = p - row * Nk;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (p + e < hs) m[row * kRmLd + col] = s[e] / fH;
            if (++col == Nk) { col = 0; ++row; }
        }
    }
    __syncthreads();
    if (!is_cross && tid < lq) {                 // row sums of (A_bar + I) over the live block, columns in order
        float s = 0.f;
        for (int j = 0; j < lk; ++j) s += m[tid * kRmLd + j] + (j == tid ? 1.f : 0.f);
        rs[tid] = s;
    }
    __syncthreads();
    float* dst = a.ws + (static_cast<int64_t>(b) * nblk + k) * a.bs;
    for (int e = tid; e < hs; e += kHmThreads) {
        const int i = e / Nk, j = e - i * Nk;
        float v = 0.f;
        if (i < lq && j < lk) v = is_cross ? m[i * kRmLd + j] : (m[i * kRmLd + j] + (i == j ? 1.f : 0.f)) / rs[i];
        dst[e] = v;
    }
}

__global__ __launch_bounds__(kRcThreads) void rollout_chain_kernel(const RolloutArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int PT = a.T, I = a.I;
    const int t = live_len(a.text_len, b, PT);
    const int nblk = a.n_text + a.n_img + 1;
    const int m16 = max(PT, I), D16 = ((m16 + 15) >> 4) << 4, LD = D16 + 4, MS = D16 * LD;
    auto mat = [&](int i) { return M2{smem + i * MS, LD}; };
    // 0 the staged block  1, 2 the text product (ping-pong; then R' and R_tt, then C . R_ii)  3, 4 the image product (then R_ti)
    const M2 S = mat(0);
    M2 curT = mat(1), nxtT = mat(2), curI = mat(3), nxtI = mat(4);
    for (int e = tid; e < 5 * MS; e += kRcThreads) smem[e] = 0.f;
    __syncthreads();

    const float* wsb = a.ws + static_cast<int64_t>(b) * nblk * a.bs;
    auto block_hs = [&](int k) { return k < a.n_text ? PT * PT : k == nblk - 1 ? PT * I : I * I; };
    f32x4 pre[2];
    auto issue = [&](int k) {                   // workspace -> registers: <= 2 chunks per lane (48 x 48 / 4 / 512)
        const int hs = block_hs(k);
        const f32x4* src = reinterpret_cast<const f32x4*>(wsb + static_cast<int64_t>(k) * a.bs);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = tid + u * kRcThreads;
            pre[u] = (c * 4 < hs) ? src[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto commit = [&](int k, M2 dst) {          // registers -> LDS (the block is already zero outside its live part)
        const int hs = block_hs(k), pk = k < a.n_text ? PT : I;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = tid + u * kRcThreads;
            if (c * 4 < hs) {
                int row = c * 4 / pk, col = c * 4 - row * pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (c * 4 + e < hs) dst.at(row, col) = pre[u][e];
                    if (++col == pk) { col = 0; ++row; }
                }
            }
        }
    };
    const int li = lane & 15, lk4 = (lane >> 4) * 4;
    // D[:M, :N] = A . B (A: M x K, or K x M with ta), 16 x 16 tiles dealt to the waves
    auto product = [&](bool ta, M2 A, int M, int K, M2 Bm, int N, M2 D) {
        const int tr = (M + 15) >> 4, tc = (N + 15) >> 4;
        for (int tl = wave; tl < tr * tc; tl += kRcWaves) {
            const int ti = tl / tc, i0 = ti * 16, j0 = (tl - ti * tc) * 16;
            const f32x4 acc = ta ? bm_tile<true>(A, Bm, i0, j0, K, lane) : bm_tile<false>(A, Bm, i0, j0, K, lane);
            const int col = j0 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + lk4 + r;
                if (row < M && col < N) D.at(row, col) = acc[r];
            }
        }
    };

    issue(0);
    for (int k = 0; k < nblk; ++k) {
        const bool first_t = k == 0, first_i = k == a.n_text;
        commit(k, first_t ? curT : first_i ? curI : S);
        if (k + 1 < nblk) issue(k + 1);
        lds_barrier();
        if (first_t || first_i) continue;        // a product starts from its first matrix
        if (k < a.n_text - 1) {                  // R' <- A_k . R'
            product(false, S, t, t, curT, t, nxtT);
            lds_barrier();
            const M2 x = curT; curT = nxtT; nxtT = x;
        } else if (k == a.n_text - 1) {          // R_tt = A_last . R'  (R' stays in curT for R_ti)
            product(false, S, t, t, curT, t, nxtT);
            lds_barrier();
            for (int e = tid; e < PT * PT; e += kRcThreads) {
                const int i = e / PT, j = e - i * PT;
                a.R_tt[static_cast<int64_t>(b) * PT * PT + e] = (i < t && j < t && e != 0) ? nxtT.at(i, j) : 0.f;   // [0, 0]: the [CLS] token (:665)
            }
            lds_barrier();
        } else if (k < nblk - 1) {               // R_ii <- A_k . R_ii
            product(false, S, I, I, curI, I, nxtI);
            lds_barrier();
            const M2 x = curI; curI = nxtI; nxtI = x;
        } else {                                 // R_ti = R'^T . (C . R_ii)  (:656)
            product(false, S, t, I, curI, I, nxtT);
            lds_barrier();
            product(true, curT, t, t, nxtT, I, nxtI);
            lds_barrier();
        }
    }
    for (int e = tid; e < PT * I; e += kRcThreads) {
        const int i = e / I, j = e - i * I;
        a.R_ti[static_cast<int64_t>(b) * PT * I + e] = (i < t) ? nxtI.at(i, j) : 0.f;
    }
    if (a.R_ii)
        for (int e = tid; e < I * I; e += kRcThreads) a.R_ii[static_cast<int64_t>(b) * I * I + e] = curI.at(e / I, e % I);
}

// ---- the LRP baselines of a padded batch: transformer attribution (:373-460) and the min-max step of partial LRP (:489-505)
struct AttrArgs {
    const float* text_c[kBlMaxTable];  // LRP cams [B, H, T, T]: the language layers, then every x-layer's lang_self_att
    const float* text_g[kBlMaxTable];  // their gradients
    const float* img_c[kBlMaxTable];   // [B, H, I, I]: r_layers, then visn_self_att of every x-layer but the last
    const float* img_g[kBlMaxTable];
    const float *cross_c, *cross_g;    // [B, H, T, I]: the last x-layer's visual_attention
    int n_text, n_img, B, H, T, I;
    const int* text_len;
    float* ws;                         // [B][n_text + n_img][bs]: A_bar of the self-attention blocks, row stride = the padded key count
    int bs;
    float *R_tt, *R_ti, *R_ii;
};

// workgroup (b, k) of B x (n_text + n_img + 1): A_bar = (sum_h max(0, G_h . C_h)) / H of block k of sample b, the clamp per head and
// the heads in order (avg_heads, :18-23), zero outside the live block.  The self-attention blocks go to the workspace, the cross
// block IS R_ti (:451).  An entry outside the live block is loaded with its 16-byte chunk and dropped: it meets no live entry.
__global__ __launch_bounds__(kHmThreads) void attr_means_kernel(const AttrArgs a) {
    const int tid = threadIdx.x;
    const int nself = a.n_text + a.n_img, nblk = nself + 1;
    const int b = blockIdx.x / nblk, k = blockIdx.x - b * nblk;
    const int t = live_len(a.text_len, b, a.T);
    const bool is_text = k < a.n_text, is_cross = k == nself;
    const float* __restrict__ C = is_text ? a.text_c[k] : is_cross ? a.cross_c : a.img_c[k - a.n_text];
    const float* __restrict__ G = is_text ? a.text_g[k] : is_cross ? a.cross_g : a.img_g[k - a.n_text];
    const int Nq = is_text || is_cross ? a.T : a.I, Nk = is_text ? a.T : a.I;
    const int lq = is_text || is_cross ? t : a.I, lk = is_text ? t : a.I;
    const int H = a.H, hs = Nq * Nk;
    const int64_t sample = static_cast<int64_t>(b) * H * hs, slab_end = static_cast<int64_t>(a.B) * H * hs;
    const float fH = static_cast<float>(H);
    float* dst = is_cross ? a.R_ti + static_cast<int64_t>(b) * hs : a.ws + (static_cast<int64_t>(b) * nself + k) * a.bs;

    for (int c = tid; c * 4 < hs; c += kHmThreads) {
        const int p = c * 4;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (sample + static_cast<int64_t>(H - 1) * hs + p + 3 < slab_end) {     // the 16-byte loads stay inside the slab
            int h = 0;
            for (; h + 3 <= H; h += 3) {
                f32x4 cv[3], gv[3];
#pragma unroll
                for (int u = 0; u < 3; ++u) {
                    cv[u] = ldg4_u(C + sample + static_cast<int64_t>(h + u) * hs + p);
                    gv[u] = ldg4_u(G + sample + static_cast<int64_t>(h + u) * hs + p);
                }
#pragma unroll
                for (int u = 0; u < 3; ++u)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] += relu_nan(gv[u][e] * cv[u][e]);
            }
            for (; h < H; ++h) {
                const f32x4 cv = ldg4_u(C + sample + static_cast<int64_t>(h) * hs + p);
                const f32x4 gv = ldg4_u(G + sample + static_cast<int64_t>(h) * hs + p);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += relu_nan(gv[e] * cv[e]);
            }
        } else {
            for (int e = 0; e < 4 && p + e < hs; ++e)
                for (int h = 0; h < H; ++h) {
                    const int64_t at = sample + static_cast<int64_t>(h) * hs + p + e;
                    s[e] += relu_nan(G[at] * C[at]);
                }
        }
        int row = p / Nk, col = p - row * Nk;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (p + e < hs) dst[p + e] = (row < lq && col < lk) ? s[e] / fH : 0.f;
            if (++col == Nk) { col = 0; ++row; }
        }
    }
}

// one workgroup per sample: R <- R + A_bar_l . R from R = I for the text table and for the image table (:405-457), every matrix in
// LDS on the exact-fp32 MFMA tiles; block l + 1 is in flight (registers) while the product of block l runs.
__global__ __launch_bounds__(kRcThreads) void attr_chain_kernel(const AttrArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const int PT = a.T, I = a.I;
    const int t = live_len(a.text_len, b, PT);
    const int nself = a.n_text + a.n_img;
    const int m16 = max(PT, I), D16 = ((m16 + 15) >> 4) << 4, LD = D16 + 4, MS = D16 * LD;
    auto mat = [&](int i) { return M2{smem + i * MS, LD}; };
    // 0 the staged block  1, 2 the text relevancy (ping-pong)  3, 4 the image relevancy
    const M2 S = mat(0);
    M2 curT = mat(1), nxtT = mat(2), curI = mat(3), nxtI = mat(4);
    for (int e = tid; e < 5 * MS; e += kRcThreads) smem[e] = 0.f;
    __syncthreads();
    for (int i = tid; i < t; i += kRcThreads) curT.at(i, i) = 1.f;
    for (int i = tid; i < I; i += kRcThreads) curI.at(i, i) = 1.f;

    const float* wsb = a.ws + static_cast<int64_t>(b) * nself * a.bs;
    auto block_hs = [&](int k) { return k < a.n_text ? PT * PT : I * I; };
    f32x4 pre[2];
    auto issue = [&](int k) {                   // workspace -> registers: <= 2 chunks per lane (48 x 48 / 4 / 512)
        const int hs = block_hs(k);
        const f32x4* src = reinterpret_cast<const f32x4*>(wsb + static_cast<int64_t>(k) * a.bs);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = tid + u * kRcThreads;
            pre[u] = (c * 4 < hs) ? src[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto commit = [&](int k) {                  // registers -> LDS (the block is already zero outside its live part)
        const int hs = block_hs(k), pk = k < a.n_text ? PT : I;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = tid + u * kRcThreads;
            if (c * 4 < hs) {
                int row = c * 4 / pk, col = c * 4 - row * pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (c * 4 + e < hs) S.at(row, col) = pre[u][e];
                    if (++col == pk) { col = 0; ++row; }
                }
            }
        }
    };
    const int li = lane & 15, lk4 = (lane >> 4) * 4;
    // D[:n, :n] = R[:n, :n] + S[:n, :n] . R[:n, :n], 16 x 16 tiles dealt to the waves
    auto step = [&](int n, M2 R, M2 D) {
        const int tn = (n + 15) >> 4;
        for (int tl = wave; tl < tn * tn; tl += kRcWaves) {
            const int ti = tl / tn, i0 = ti * 16, j0 = (tl - ti * tn) * 16;
            const f32x4 acc = bm_tile<false>(S, R, i0, j0, n, lane);
            const int col = j0 + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + lk4 + r;
                if (row < n && col < n) D.at(row, col) = R.at(row, col) + acc[r];
            }
        }
    };

    issue(0);
    for (int k = 0; k < nself; ++k) {
        commit(k);
        if (k + 1 < nself) issue(k + 1);
        lds_barrier();
        if (k < a.n_text) {
            step(t, curT, nxtT);
            const M2 x = curT; curT = nxtT; nxtT = x;
        } else {
            step(I, curI, nxtI);
            const M2 x = curI; curI = nxtI; nxtI = x;
        }
        lds_barrier();
    }
    for (int e = tid; e < PT * PT; e += kRcThreads) {
        const int i = e / PT, j = e - i * PT;
        a.R_tt[static_cast<int64_t>(b) * PT * PT + e] = (i < t && j < t && e != 0) ? curT.at(i, j) : 0.f;   // [0, 0]: the [CLS] token (:459)
    }
    for (int e = tid; e < I * I; e += kRcThreads) a.R_ii[static_cast<int64_t>(b) * I * I + e] = curI.at(e / I, e % I);
}

// one workgroup per sample: m = mean_h cam[b, h] on the live block, out = (m - min m) / (max m - min m) (:502-503), the extremes over
// the live block with torch's rule that a NaN wins; max == min leaves 0 / 0 = NaN, as the reference's expression does.
__global__ __launch_bounds__(kHmThreads) void head_minmax_live_kernel(const float* __restrict__ cam, float* __restrict__ out, int H,
                                                                      int Nq, int Nk, const int* q_len, const int* k_len,
                                                                      unsigned flags) {
    __shared__ float lo_lds[kHmThreads / 64], hi_lds[kHmThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = live_len(q_len, b, Nq), k = live_len(k_len, b, Nk);
    const int hs = Nq * Nk, live = q * k;
    const float* P = cam + static_cast<int64_t>(b) * H * hs;
    float* O = out + static_cast<int64_t>(b) * hs;

    float acc[kHmPer];
    int off[kHmPer];
#pragma unroll
    for (int u = 0; u < kHmPer; ++u) {
        const int n = tid + u * kHmThreads;
        const int i = n / k;
        off[u] = n < live ? i * Nk + (n - i * k) : -1;
        acc[u] = 0.f;
    }
    for (int h = 0; h < H; ++h)
#pragma unroll
        for (int u = 0; u < kHmPer; ++u)
            if (off[u] >= 0) acc[u] += P[static_cast<int64_t>(h) * hs + off[u]];
    const float fH = static_cast<float>(H);
    float lo = 0.f, hi = 0.f;
    bool any = false;
#pragma unroll
    for (int u = 0; u < kHmPer; ++u) {
        if (off[u] < 0) continue;
        acc[u] /= fH;
        lo = any ? min_nan(lo, acc[u]) : acc[u];
        hi = any ? max_nan(hi, acc[u]) : acc[u];
        any = true;
    }
    // the threads with a live entry are tid < live, a prefix: a wave's lane 0 has one if any of its lanes has
    const float lo0 = __shfl(lo, 0), hi0 = __shfl(hi, 0);
    if (!any) { lo = lo0; hi = hi0; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min_nan(lo, __shfl_xor(lo, o));
        hi = max_nan(hi, __shfl_xor(hi, o));
    }
    if (lane == 0) { lo_lds[wave] = lo; hi_lds[wave] = hi; }
    __syncthreads();
    // wave w holds a live entry iff 64 w < live: an empty wave's words are skipped
    lo = lo_lds[0]; hi = hi_lds[0];
    for (int w = 1; w < kHmThreads / 64; ++w)
        if (w * 64 < live) { lo = min_nan(lo, lo_lds[w]); hi = max_nan(hi, hi_lds[w]); }
    const float span = hi - lo;
    for (int e = tid; e < hs; e += kHmThreads) {                          // everything outside the live block: exact zeros
        const int i = e / Nk, j = e - i * Nk;
        if (i >= q || j >= k) O[e] = 0.f;
    }
#pragma unroll
    for (int u = 0; u < kHmPer; ++u) {
        if (off[u] < 0) continue;
        float v = (acc[u] - lo) / span;
        if ((flags & MMX_HEAD_MEAN_ZERO_CLS) && off[u] == 0) v = 0.f;
        O[off[u]] = v;
    }
}

}  // namespace mmx

using namespace mmx;

static inline int bl_block_floats(int T, int I) {
    const int m = T > I ? T : I;
    return ((m * m + 3) / 4) * 4;
}

extern "C" int mmx_head_mean_live(const void* attn_dev, const void* grad_dev, void* out_dev, int B, int H, int Nq, int Nk,
                                  const void* q_len_dev, const void* k_len_dev, unsigned flags, void* stream) {
    MMX_CHECK_ARG(attn_dev && out_dev, "mmx_head_mean_live: null pointer");
    MMX_CHECK_ARG(B > 0 && H > 0, "mmx_head_mean_live: B=%d H=%d (both >= 1)", B, H);
    MMX_CHECK_ARG(Nq >= 1 && Nq <= kBlMax && Nk >= 1 && Nk <= kBlMax, "mmx_head_mean_live: Nq=%d Nk=%d outside 1..%d", Nq, Nk, kBlMax);
    MMX_CHECK_ARG((flags & ~static_cast<unsigned>(MMX_HEAD_MEAN_ZERO_CLS)) == 0, "mmx_head_mean_live: unknown flags 0x%x", flags);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(B) * Nq * Nk, in_bytes = out_bytes * static_cast<size_t>(H);
    const size_t len_bytes = sizeof(int) * static_cast<size_t>(B);
    const Span out = {out_dev, out_bytes};
    const Span ins[4] = {{attn_dev, in_bytes}, {grad_dev, in_bytes}, {q_len_dev, len_bytes}, {k_len_dev, len_bytes}};
    MMX_CHECK_ARG(!spans_alias(&out, 1, ins, 4), "mmx_head_mean_live: the output may not alias an input");
    head_mean_live_kernel<<<static_cast<unsigned>(B), kHmThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float*>(attn_dev), static_cast<const float*>(grad_dev), static_cast<float*>(out_dev), H, Nq, Nk,
        static_cast<const int*>(q_len_dev), static_cast<const int*>(k_len_dev), flags);
    MMX_LAUNCH_CHECK("head_mean_live_kernel");
    return MMX_OK;
}

extern "C" size_t mmx_lxmert_rollout_workspace_bytes(int n_text, int n_img, int B, int T, int I) {
    if (n_text < 2 || n_img < 1 || n_text > kBlMaxTable || n_img > kBlMaxTable || B < 1 || T < 1 || I < 1 || T > kBlMax || I > kBlMax)
        return 0;
    return align256(sizeof(float) * static_cast<size_t>(B) * (n_text + n_img + 1) * bl_block_floats(T, I));
}

extern "C" int mmx_lxmert_rollout(const void* const* text_attn, int n_text, const void* const* img_attn, int n_img,
                                  const void* cross_attn_dev, int B, int H, int T, int I, const void* text_len_dev, void* R_tt_dev,
                                  void* R_ti_dev, void* R_ii_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    MMX_CHECK_ARG(text_attn && img_attn && cross_attn_dev && R_tt_dev && R_ti_dev && workspace_dev, "mmx_lxmert_rollout: null pointer");
    MMX_CHECK_ARG(B > 0 && H > 0, "mmx_lxmert_rollout: B=%d H=%d (both >= 1)", B, H);
    MMX_CHECK_ARG(T >= 1 && T <= kBlMax && I >= 1 && I <= kBlMax, "mmx_lxmert_rollout: T=%d I=%d outside 1..%d", T, I, kBlMax);
    MMX_CHECK_ARG(n_text >= 2 && n_img >= 1, "mmx_lxmert_rollout: n_text=%d (>= 2: the last entry is the last language block) n_img=%d (>= 1)",
                  n_text, n_img);
    MMX_CHECK_ARG(n_text <= kBlMaxTable && n_img <= kBlMaxTable, "mmx_lxmert_rollout: at most %d slabs per table (n_text=%d n_img=%d)",
                  kBlMaxTable, n_text, n_img);
    const char* me = "mmx_lxmert_rollout";
    const int nblk = n_text + n_img + 1;
    if (int rc = check_grid(me, static_cast<int64_t>(B) * nblk, "B=%d x %d blocks", B, nblk)) return rc;
    const size_t need = mmx_lxmert_rollout_workspace_bytes(n_text, n_img, B, T, I);
    if (int rc = check_workspace(me, "mmx_lxmert_rollout_workspace_bytes", workspace_dev, workspace_bytes, need)) return rc;
    RolloutArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = copy_table(me, "the text table", text_attn, n_text, a.text)) return rc;
    if (int rc = copy_table(me, "the image table", img_attn, n_img, a.img)) return rc;
    const size_t f = sizeof(float), nb = static_cast<size_t>(B);
    const Span outs[4] = {{R_tt_dev, f * nb * T * T}, {R_ti_dev, f * nb * T * I}, {R_ii_dev, f * nb * I * I}, {workspace_dev, need}};
    Span ins[2 * kBlMaxTable + 2];
    int n_in = 0;
    for (int l = 0; l < n_text; ++l) ins[n_in++] = {text_attn[l], f * nb * H * T * T};
    for (int l = 0; l < n_img; ++l) ins[n_in++] = {img_attn[l], f * nb * H * I * I};
    ins[n_in++] = {cross_attn_dev, f * nb * H * T * I};
    ins[n_in++] = {text_len_dev, sizeof(int) * nb};
    MMX_CHECK_ARG(!spans_alias(outs, 4, ins, n_in), "mmx_lxmert_rollout: an output or the workspace may not alias an input or another output");
    a.cross = static_cast<const float*>(cross_attn_dev);
    a.n_text = n_text; a.n_img = n_img; a.B = B; a.H = H; a.T = T; a.I = I;
    a.text_len = static_cast<const int*>(text_len_dev);
    a.ws = static_cast<float*>(workspace_dev);
    a.bs = bl_block_floats(T, I);
    a.R_tt = static_cast<float*>(R_tt_dev); a.R_ti = static_cast<float*>(R_ti_dev); a.R_ii = static_cast<float*>(R_ii_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rollout_means_kernel<<<static_cast<unsigned>(B) * nblk, kHmThreads, 0, s>>>(a);
    MMX_LAUNCH_CHECK("rollout_means_kernel");
    const int m = T > I ? T : I, D16 = ((m + 15) / 16) * 16;
    const size_t lds = sizeof(float) * 5 * static_cast<size_t>(D16) * (D16 + 4);     // <= 49 920 bytes
    rollout_chain_kernel<<<static_cast<unsigned>(B), kRcThreads, lds, s>>>(a);
    MMX_LAUNCH_CHECK("rollout_chain_kernel");
    return MMX_OK;
}

extern "C" int mmx_head_minmax_live(const void* cam_dev, void* out_dev, int B, int H, int Nq, int Nk, const void* q_len_dev,
                                    const void* k_len_dev, unsigned flags, void* stream) {
    MMX_CHECK_ARG(cam_dev && out_dev, "mmx_head_minmax_live: null pointer");
    MMX_CHECK_ARG(B > 0 && H > 0, "mmx_head_minmax_live: B=%d H=%d (both >= 1)", B, H);
    MMX_CHECK_ARG(Nq >= 1 && Nq <= kBlMax && Nk >= 1 && Nk <= kBlMax, "mmx_head_minmax_live: Nq=%d Nk=%d outside 1..%d", Nq, Nk, kBlMax);
    MMX_CHECK_ARG((flags & ~static_cast<unsigned>(MMX_HEAD_MEAN_ZERO_CLS)) == 0, "mmx_head_minmax_live: unknown flags 0x%x", flags);
    const size_t out_bytes = sizeof(float) * static_cast<size_t>(B) * Nq * Nk, in_bytes = out_bytes * static_cast<size_t>(H);
    const size_t len_bytes = sizeof(int) * static_cast<size_t>(B);
    const Span out = {out_dev, out_bytes};
    const Span ins[3] = {{cam_dev, in_bytes}, {q_len_dev, len_bytes}, {k_len_dev, len_bytes}};
    MMX_CHECK_ARG(!spans_alias(&out, 1, ins, 3), "mmx_head_minmax_live: the output may not alias an input");
    head_minmax_live_kernel<<<static_cast<unsigned>(B), kHmThreads, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float*>(cam_dev), static_cast<float*>(out_dev), H, Nq, Nk, static_cast<const int*>(q_len_dev),
        static_cast<const int*>(k_len_dev), flags);
    MMX_LAUNCH_CHECK("head_minmax_live_kernel");
    return MMX_OK;
}

extern "C" size_t mmx_lxmert_attr_workspace_bytes(int n_text, int n_img, int B, int T, int I) {
    if (n_text < 1 || n_img < 1 || n_text > kBlMaxTable || n_img > kBlMaxTable || B < 1 || T < 1 || I < 1 || T > kBlMax || I > kBlMax)
        return 0;
    return align256(sizeof(float) * static_cast<size_t>(B) * (n_text + n_img) * bl_block_floats(T, I));
}

extern "C" int mmx_lxmert_attr(const void* const* text_cam, const void* const* text_grad, int n_text, const void* const* img_cam,
                               const void* const* img_grad, int n_img, const void* cross_cam_dev, const void* cross_grad_dev, int B,
                               int H, int T, int I, const void* text_len_dev, void* R_tt_dev, void* R_ti_dev, void* R_ii_dev,
                               void* workspace_dev, size_t workspace_bytes, void* stream) {
    const char* me = "mmx_lxmert_attr";
    MMX_CHECK_ARG(text_cam && text_grad && img_cam && img_grad && cross_cam_dev && cross_grad_dev && R_tt_dev && R_ti_dev && R_ii_dev &&
                      workspace_dev, "mmx_lxmert_attr: null pointer");
    MMX_CHECK_ARG(B > 0 && H > 0, "mmx_lxmert_attr: B=%d H=%d (both >= 1)", B, H);
    MMX_CHECK_ARG(T >= 1 && T <= kBlMax && I >= 1 && I <= kBlMax, "mmx_lxmert_attr: T=%d I=%d outside 1..%d", T, I, kBlMax);
    MMX_CHECK_ARG(n_text >= 1 && n_img >= 1, "mmx_lxmert_attr: n_text=%d n_img=%d (both >= 1)", n_text, n_img);
    MMX_CHECK_ARG(n_text <= kBlMaxTable && n_img <= kBlMaxTable, "mmx_lxmert_attr: at most %d slabs per table (n_text=%d n_img=%d)",
                  kBlMaxTable, n_text, n_img);
    const int nblk = n_text + n_img + 1;
    if (int rc = check_grid(me, static_cast<int64_t>(B) * nblk, "B=%d x %d blocks", B, nblk)) return rc;
    const size_t need = mmx_lxmert_attr_workspace_bytes(n_text, n_img, B, T, I);
    if (int rc = check_workspace(me, "mmx_lxmert_attr_workspace_bytes", workspace_dev, workspace_bytes, need)) return rc;
    AttrArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = copy_table(me, "the text tables", text_cam, n_text, a.text_c, text_grad, a.text_g)) return rc;
    if (int rc = copy_table(me, "the image tables", img_cam, n_img, a.img_c, img_grad, a.img_g)) return rc;
    const size_t f = sizeof(float), nb = static_cast<size_t>(B);
    const Span outs[4] = {{R_tt_dev, f * nb * T * T}, {R_ti_dev, f * nb * T * I}, {R_ii_dev, f * nb * I * I}, {workspace_dev, need}};
    Span ins[4 * kBlMaxTable + 3];
    int n_in = 0;
    for (int l = 0; l < n_text; ++l) {
        ins[n_in++] = {text_cam[l], f * nb * H * T * T};
        ins[n_in++] = {text_grad[l], f * nb * H * T * T};
    }
    for (int l = 0; l < n_img; ++l) {
        ins[n_in++] = {img_cam[l], f * nb * H * I * I};
        ins[n_in++] = {img_grad[l], f * nb * H * I * I};
    }
    ins[n_in++] = {cross_cam_dev, f * nb * H * T * I};
    ins[n_in++] = {cross_grad_dev, f * nb * H * T * I};
    ins[n_in++] = {text_len_dev, sizeof(int) * nb};
    MMX_CHECK_ARG(!spans_alias(outs, 4, ins, n_in), "mmx_lxmert_attr: an output or the workspace may not alias an input or another output");
    a.cross_c = static_cast<const float*>(cross_cam_dev); a.cross_g = static_cast<const float*>(cross_grad_dev);
    a.n_text = n_text; a.n_img = n_img; a.B = B; a.H = H; a.T = T; a.I = I;
    a.text_len = static_cast<const int*>(text_len_dev);
    a.ws = static_cast<float*>(workspace_dev);
    a.bs = bl_block_floats(T, I);
    a.R_tt = static_cast<float*>(R_tt_dev); a.R_ti = static_cast<float*>(R_ti_dev); a.R_ii = static_cast<float*>(R_ii_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    attr_means_kernel<<<static_cast<unsigned>(B) * nblk, kHmThreads, 0, s>>>(a);
    MMX_LAUNCH_CHECK("attr_means_kernel");
    const int m = T > I ? T : I, D16 = ((m + 15) / 16) * 16;
    const size_t lds = sizeof(float) * 5 * static_cast<size_t>(D16) * (D16 + 4);     // <= 49 920 bytes
    attr_chain_kernel<<<static_cast<unsigned>(B), kRcThreads, lds, s>>>(a);
    MMX_LAUNCH_CHECK("attr_chain_kernel");
    return MMX_OK;
}
