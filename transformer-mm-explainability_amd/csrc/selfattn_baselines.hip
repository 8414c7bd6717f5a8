// The attention-only baselines of the single-stream (VisualBERT-style) model for a PADDED batch of ragged questions: raw attention,
// attention GradCAM and rollout (VisualBERT/mmf/models/transformers/backends/ExplanationGenerator.py:155-166, :200-211, :168-180 with
// :5-17).  All three return ONE row of an N x N map -- the row of the token the 'vqa' pooler reads, c_b = t_b - 2 -- so nothing here
// ever forms an N x N product.
//
// The sequence of a padded batch is [text | text padding | regions | region padding]: N = T + V, sample b's live index set is
// L_b = [0, t_b) u [T, T + v_b), n_b = t_b + v_b.  Lengths are device int32 arrays, clamped to 2..T and 1..V before any use.  The
// probability slabs are exact zero at padded key columns, the GRADIENT slabs are not, and padded query rows hold whatever the body
// computed for a pad token: every sum, divisor, minimum and maximum is taken over L_b x L_b only, and every output is exact zero
// outside L_b and at column c_b.
//
//   sa_raw_row_kernel      one workgroup per sample: (sum_h P[b, h, c_b, j]) / H, one row per head.
//   sa_gradcam_w_kernel    workgroup (b, h): w[b, h] = (sum of G[b, h] over L_b x L_b) / float(n_b^2) -> workspace.
//   sa_gradcam_cam_kernel  workgroup (b, strip of 8 rows): cam = relu((sum_h P[b, h] w[b, h]) / H) on the strip's live rows, its
//                          minimum and maximum and -- in the strip that holds it -- row c_b -> workspace.
//   sa_gradcam_out_kernel  one workgroup per sample: the minimum / maximum over the strips, (row - mn) / (mx - mn).
//   sa_rollout_means_kernel  workgroup (b, layer, strip of 2048 floats): the head mean of every chunk that touches a live row, read
//                          with 16-byte loads, heads in order, written once to the workspace.
//   sa_rollout_row_kernel  one workgroup per sample: x = e_c, x <- x + x . A_l from the top table entry down; x sits in LDS, wave w
//                          takes the live rows w, w + 4, ... (a lane owns four columns).  Every lane loads 16 aligned bytes per row
//                          UNCONDITIONALLY from a clamped address (lanes past the row's end repeat its last chunk, items past the
//                          live rows repeat the last live row times zero), so eight loads and eight FMAs form one basic block and
//                          the waits are counted: a ring of eight rows per lane stays in flight, across the layer boundary too.
//   sa_ours_means_kernel   generate_ours (:68-107) on the same layout: workgroups as sa_rollout_means_kernel, but the matrix of a layer is
//                          rule 5, (sum_h max(0, grad_h * attn_h)) / H with the clamp per head; sa_rollout_row_kernel then runs on it.
// Plain launches ordered by the stream (no tickets, no spinning), fixed summation orders, no atomics: two runs give the same bits,
// and sample b's result depends neither on B nor on b.
#include "mmx_common.h"

namespace mmx {

constexpr int kSaMaxN = 256;                    // T + V (128 text positions + 100 regions must fit)
constexpr int kSaMaxTable = MMX_BASELINES_MAX_TABLE;
constexpr int kSaThreads = 256;
constexpr int kSaWaves = kSaThreads / 64;
constexpr int kSaStripRows = 8;                 // rows of one cam / min-max workgroup (two per wave)
constexpr int kSaMeanChunks = 2;                // 16-byte chunks per thread of a head-mean workgroup
constexpr int kSaMeanStrip = kSaThreads * kSaMeanChunks * 4;     // floats per head-mean workgroup
constexpr int kSaRing = 8;                      // row loads in flight per lane of the row kernel

// the clamped lengths of sample b: NEVER used unclamped
__device__ __forceinline__ int sa_text_len(const int* len, int b, int T) { return len ? min(max(len[b], 2), T) : T; }
__device__ __forceinline__ int sa_vis_len(const int* len, int b, int V) { return len ? min(max(len[b], 1), V) : V; }
__device__ __forceinline__ bool sa_live(int j, int t, int T, int v) { return j < t || (j >= T && j < T + v); }
// the k-th live index, k < t + v
__device__ __forceinline__ int sa_live_at(int k, int t, int T) { return k < t ? k : T + (k - t); }

// columns 4 lane .. 4 lane + 3 of one row of N floats (zeros beyond N); p points at the row
__device__ __forceinline__ f32x4 sa_row4(const float* __restrict__ p, int lane, int N) {
    const int j0 = lane * 4;
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (j0 + 3 < N) {
        r = ldg4_u(p + j0);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (j0 + e < N) r[e] = p[j0 + e];
    }
    return r;
}

__global__ __launch_bounds__(kSaThreads) void sa_raw_row_kernel(const float* __restrict__ attn, float* __restrict__ out, int H, int T,
                                                                int V, const int* text_len, const int* vis_len) {
    const int b = blockIdx.x, j = threadIdx.x, N = T + V;
    if (j >= N) return;
    const int t = sa_text_len(text_len, b, T), v = sa_vis_len(vis_len, b, V), c = t - 2;
    float r = 0.f;
    if (sa_live(j, t, T, v) && j != c) {
        const float* P = attn + (static_cast<int64_t>(b) * H * N + c) * N + j;
        float s = 0.f;
        for (int h = 0; h < H; ++h) s += P[static_cast<int64_t>(h) * N * N];
        r = s / static_cast<float>(H);
    }
    out[static_cast<int64_t>(b) * N + j] = r;
}

__global__ __launch_bounds__(kSaThreads) void sa_gradcam_w_kernel(const float* __restrict__ grad, float* __restrict__ w, int T, int V,
                                                                  const int* text_len, const int* vis_len, int H) {
    __shared__ float part[kSaWaves];
    const int bh = blockIdx.x, b = bh / H, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = T + V;
    const int t = sa_text_len(text_len, b, T), v = sa_vis_len(vis_len, b, V), n = t + v;
    const float* G = grad + static_cast<int64_t>(bh) * N * N;
    bool lv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) lv[e] = sa_live(lane * 4 + e, t, T, v);
    float s = 0.f;
    for (int k = wave; k < n; k += kSaWaves) {                       // live rows only; padded columns are loaded and dropped
        const f32x4 g = sa_row4(G + static_cast<int64_t>(sa_live_at(k, t, T)) * N, lane, N);
#pragma unroll
        for (int e = 0; e < 4; ++e) s += lv[e] ? g[e] : 0.f;
    }
    s = wave_sum(s);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) {
        float total = part[0];
#pragma unroll
        for (int u = 1; u < kSaWaves; ++u) total += part[u];
        w[bh] = total / static_cast<float>(n * n);                   // the sum first, then ONE division by the live count
    }
}

__global__ __launch_bounds__(kSaThreads) void sa_gradcam_cam_kernel(const float* __restrict__ attn, const float* __restrict__ w,
                                                                    float* __restrict__ mm, float* __restrict__ row, int H, int T,
                                                                    int V, int strips, const int* text_len, const int* vis_len) {
    __shared__ float p_mn[kSaWaves], p_mx[kSaWaves];
    const int b = blockIdx.x / strips, s = blockIdx.x - b * strips;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, N = T + V;
    const int t = sa_text_len(text_len, b, T), v = sa_vis_len(vis_len, b, V), c = t - 2;
    const float* P = attn + static_cast<int64_t>(b) * H * N * N;
    const float* wb = w + static_cast<int64_t>(b) * H;
    const float fH = static_cast<float>(H);
    const float inf = __builtin_inff();
    bool lv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) lv[e] = sa_live(lane * 4 + e, t, T, v);
    float mn = inf, mx = -inf;
    for (int i = s * kSaStripRows + wave; i < min((s + 1) * kSaStripRows, N); i += kSaWaves) {
        if (!sa_live(i, t, T, v)) continue;                          // (wave-uniform)
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int h = 0; h < H; ++h) acc += sa_row4(P + (static_cast<int64_t>(h) * N + i) * N, lane, N) * wb[h];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float cam = relu_nan(acc[e] / fH);
            if (lv[e]) {
                mn = min_nan(mn, cam);
                mx = max_nan(mx, cam);
            }
            if (i == c && lane * 4 + e < N) row[static_cast<int64_t>(b) * N + lane * 4 + e] = lv[e] ? cam : 0.f;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = min_nan(mn, __shfl_xor(mn, off));
        mx = max_nan(mx, __shfl_xor(mx, off));
    }
    if (lane == 0) { p_mn[wave] = mn; p_mx[wave] = mx; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int u = 1; u < kSaWaves; ++u) { mn = min_nan(mn, p_mn[u]); mx = max_nan(mx, p_mx[u]); }
        mm[2 * static_cast<int64_t>(blockIdx.x)] = mn;               // a strip without a live row: +inf / -inf, the neutral pair
        mm[2 * static_cast<int64_t>(blockIdx.x) + 1] = mx;
    }
}

__global__ __launch_bounds__(kSaThreads) void sa_gradcam_out_kernel(const float* __restrict__ mm, const float* __restrict__ row,
                                                                    float* __restrict__ out, int T, int V, int strips,
                                                                    const int* text_len, const int* vis_len) {
    const int b = blockIdx.x, j = threadIdx.x, N = T + V;
    if (j >= N) return;
    const int t = sa_text_len(text_len, b, T), v = sa_vis_len(vis_len, b, V), c = t - 2;
    float r = 0.f;
    if (sa_live(j, t, T, v) && j != c) {
        const float* m = mm + 2 * static_cast<int64_t>(b) * strips;
        float mn = m[0], mx = m[1];
        for (int s = 1; s < strips; ++s) { mn = min_nan(mn, m[2 * s]); mx = max_nan(mx, m[2 * s + 1]); }
        r = (row[static_cast<int64_t>(b) * N + j] - mn) / (mx - mn);  // no guard: mx == mn gives NaN, as in the reference
    }
    out[static_cast<int64_t>(b) * N + j] = r;
}

struct SaRolloutArgs {
    const float* attn[kSaMaxTable];    // [B, H, N, N], one entry per layer (the rollout's already sliced to start_layer:)
    int n_layers, B, H, T, V, strips;
    const int *text_len, *vis_len;
    float* ws;                         // [B][n_layers][N][NP] head means, NP = row_stride4(N); rows of padded queries and the
                                       // NP - N floats behind a row are never written, and never used
    float* out;
    const float* grad[kSaMaxTable];    // generate_ours only: [B, H, N, N] the gradients of attn, NOT zero at padded key columns
                                       // (behind everything sa_rollout_row_kernel reads)
};

// what head h adds to the matrix of a layer: its probability (rollout), or rule 5, clamp0(grad_h * attn_h) (generate_ours)
template <bool kOurs>
__device__ __forceinline__ float sa_head_term(float x, float g) {
    if constexpr (kOurs) return relu_nan(g * x);
    else return x;
}

// The matrix of a layer on the live rows: (sum_h term_h) / H, the clamp of rule 5 per head BEFORE the sum, heads in ascending order,
// kHeads of them (kHeads 16-byte loads per slab) in flight.  Padded key columns of a live row are computed and written (the
// gradient there is arbitrary) and never read: the row kernel multiplies by x, which is zero there.
template <bool kOurs, int kHeads>
__device__ __forceinline__ void sa_means_body(const SaRolloutArgs& a) {
    const int tid = threadIdx.x, N = a.T + a.V, hs = N * N, H = a.H;
    int w = blockIdx.x;
    const int s = w % a.strips; w /= a.strips;
    const int l = w % a.n_layers, b = w / a.n_layers;
    const int t = sa_text_len(a.text_len, b, a.T), v = sa_vis_len(a.vis_len, b, a.V);
    const float* __restrict__ P = a.attn[l] + static_cast<int64_t>(b) * H * hs;
    const float* __restrict__ G = kOurs ? a.grad[l] + static_cast<int64_t>(b) * H * hs : P;
    const int NP = row_stride4(N);
    float* dst = a.ws + (static_cast<int64_t>(b) * a.n_layers + l) * N * NP;
    const float fH = static_cast<float>(H);
#pragma unroll
    for (int u = 0; u < kSaMeanChunks; ++u) {
        const int p = s * kSaMeanStrip + (u * kSaThreads + tid) * 4;
        if (p >= hs) continue;
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) any |= p + e < hs && sa_live((p + e) / N, t, a.T, v);
        if (!any) continue;                                          // a chunk of padded query rows: neither read nor written
        f32x4 m = {0.f, 0.f, 0.f, 0.f};
        if (p + 3 < hs) {                                            // the 16-byte loads stay inside the head's own N x N block
            int h = 0;
            for (; h + kHeads <= H; h += kHeads) {
                f32x4 x[kHeads], g[kHeads];
#pragma unroll
                for (int q = 0; q < kHeads; ++q) {
                    x[q] = ldg4_u(P + static_cast<int64_t>(h + q) * hs + p);
                    g[q] = kOurs ? ldg4_u(G + static_cast<int64_t>(h + q) * hs + p) : x[q];
                }
#pragma unroll
                for (int q = 0; q < kHeads; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) m[e] += sa_head_term<kOurs>(x[q][e], g[q][e]);
            }
            for (; h < H; ++h) {
                const f32x4 x = ldg4_u(P + static_cast<int64_t>(h) * hs + p);
                const f32x4 g = kOurs ? ldg4_u(G + static_cast<int64_t>(h) * hs + p) : x;
#pragma unroll
                for (int e = 0; e < 4; ++e) m[e] += sa_head_term<kOurs>(x[e], g[e]);
            }
        } else {
            for (int e = 0; p + e < hs; ++e)
                for (int h = 0; h < H; ++h) {
                    const float x = P[static_cast<int64_t>(h) * hs + p + e];
                    m[e] += sa_head_term<kOurs>(x, kOurs ? G[static_cast<int64_t>(h) * hs + p + e] : x);
                }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (p + e < hs) {
                const int row = (p + e) / N;
                dst[row * NP + (p + e - row * N)] = m[e] / fH;       // rows of the workspace start on 16-byte boundaries
            }
    }
}

// thin wrappers: the kernel names are what the profiles and tools/prof_summary.py select by
__global__ __launch_bounds__(kSaThreads) void sa_rollout_means_kernel(const SaRolloutArgs a) { sa_means_body<false, 6>(a); }
__global__ __launch_bounds__(kSaThreads) void sa_ours_means_kernel(const SaRolloutArgs a) { sa_means_body<true, 4>(a); }

__global__ __launch_bounds__(kSaThreads) void sa_rollout_row_kernel(const SaRolloutArgs a) {
    __shared__ float x[kSaMaxN];
    __shared__ float part[kSaWaves][kSaMaxN];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x, N = a.T + a.V, NP = row_stride4(N), L = a.n_layers;
    const int64_t ls = static_cast<int64_t>(N) * NP;
    const int t = sa_text_len(a.text_len, b, a.T), v = sa_vis_len(a.vis_len, b, a.V), n = t + v, c = t - 2;
    // items of a layer and wave: live rows wave, wave + 4, ..., padded to a multiple of the ring so that a layer ends where an
    // unrolled block ends; an item past the live rows loads a valid row (the last live one) and is multiplied by zero
    const int m8 = (((n + kSaWaves - 1) / kSaWaves + kSaRing - 1) / kSaRing) * kSaRing;
    // every lane loads 16 aligned bytes of its row; lanes past the row's end repeat the last chunk and are dropped at the end
    const float* base = a.ws + static_cast<int64_t>(b) * L * ls + min(lane * 4, NP - 4);
    x[tid] = tid == c ? 1.f : 0.f;
    __syncthreads();

    // the loader walks the flat (layer, item) sequence kSaRing items ahead of the FMAs; past the last layer it repeats layer 0
    int pl = L - 1, pk = 0;
    auto fetch = [&](int u) -> f32x4 {
        const int k = min(wave + kSaWaves * (pk + u), n - 1);
        return *reinterpret_cast<const f32x4*>(base + max(pl, 0) * ls + static_cast<int64_t>(sa_live_at(k, t, a.T)) * NP);
    };
    auto advance = [&]() {
        pk += kSaRing;
        if (pk == m8) { pk = 0; --pl; }
    };
    f32x4 ring[kSaRing];
#pragma unroll
    for (int u = 0; u < kSaRing; ++u) ring[u] = fetch(u);
    advance();
    for (int l = L - 1; l >= 0; --l) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int kk0 = 0; kk0 < m8; kk0 += kSaRing) {                // one basic block: eight loads issued, eight rows consumed
#pragma unroll
            for (int u = 0; u < kSaRing; ++u) {
                const int k = wave + kSaWaves * (kk0 + u);
                const float xi = x[sa_live_at(min(k, n - 1), t, a.T)];
                acc += ring[u] * (k < n ? xi : 0.f);
                __builtin_amdgcn_sched_barrier(0);                   // the FMA stays in front of the refill of ITS register: no
                ring[u] = fetch(u);                                  // renamed ring, no copies (and no drain) at the loop's end
            }
            advance();
        }
        // the layer is done: x <- x + the four waves' partial rows (the next layer's first rows are already in flight)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[wave][lane * 4 + e] = lane * 4 + e < N ? acc[e] : 0.f;
        lds_barrier();
        const float y = x[tid] + ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]));
        x[tid] = sa_live(tid, t, a.T, v) ? y : 0.f;                  // (entry tid is read here by its own thread only)
        lds_barrier();
    }
    if (tid < N) a.out[static_cast<int64_t>(b) * N + tid] = (sa_live(tid, t, a.T, v) && tid != c) ? x[tid] : 0.f;
}

}  // namespace mmx

using namespace mmx;

static inline bool sa_sizes_ok(int T, int V) { return T >= 2 && V >= 1 && T <= kSaMaxN && V <= kSaMaxN && T + V <= kSaMaxN; }
static inline int sa_cam_strips(int N) { return (N + kSaStripRows - 1) / kSaStripRows; }

// workspace of the GradCAM form: w [B, H] | (min, max) [B, strips, 2] | row c_b of cam [B, N], each part 256-byte aligned
extern "C" size_t mmx_selfattn_row_live_workspace_bytes(int B, int H, int T, int V) {
    if (B < 1 || H < 1 || !sa_sizes_ok(T, V)) return 0;
    const size_t f = sizeof(float), nb = static_cast<size_t>(B), N = static_cast<size_t>(T + V);
    return align256(f * nb * H) + align256(f * nb * sa_cam_strips(T + V) * 2) + align256(f * nb * N);
}

extern "C" int mmx_selfattn_row_live(const void* attn_dev, const void* grad_dev, void* out_dev, int B, int H, int T, int V,
                                     const void* text_len_dev, const void* vis_len_dev, void* workspace_dev, size_t workspace_bytes,
                                     void* stream) {
    MMX_CHECK_ARG(attn_dev && out_dev, "mmx_selfattn_row_live: null pointer");
    MMX_CHECK_ARG(B > 0 && H > 0, "mmx_selfattn_row_live: B=%d H=%d (both >= 1)", B, H);
    MMX_CHECK_ARG(sa_sizes_ok(T, V), "mmx_selfattn_row_live: T=%d V=%d outside T >= 2, V >= 1, T + V <= %d", T, V, kSaMaxN);
    const size_t need = grad_dev ? mmx_selfattn_row_live_workspace_bytes(B, H, T, V) : 0;
    if (grad_dev) {
        MMX_CHECK_ARG(workspace_dev, "mmx_selfattn_row_live: null pointer (the GradCAM form needs a workspace)");
        if (int rc = check_workspace("mmx_selfattn_row_live", "mmx_selfattn_row_live_workspace_bytes", workspace_dev, workspace_bytes, need))
            return rc;
    }
    const int N = T + V;
    const size_t f = sizeof(float), nb = static_cast<size_t>(B);
    const size_t in_bytes = f * nb * H * N * N, len_bytes = sizeof(int) * nb;
    const Span outs[2] = {{out_dev, f * nb * N}, {grad_dev ? workspace_dev : nullptr, need}};
    const Span ins[4] = {{attn_dev, in_bytes}, {grad_dev, in_bytes}, {text_len_dev, len_bytes}, {vis_len_dev, len_bytes}};
    MMX_CHECK_ARG(!spans_alias(outs, 2, ins, 4), "mmx_selfattn_row_live: the output or the workspace may not alias an input or each other");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* P = static_cast<const float*>(attn_dev);
    const int* tl = static_cast<const int*>(text_len_dev);
    const int* vl = static_cast<const int*>(vis_len_dev);
    float* out = static_cast<float*>(out_dev);
    if (!grad_dev) {
        sa_raw_row_kernel<<<static_cast<unsigned>(B), kSaThreads, 0, s>>>(P, out, H, T, V, tl, vl);
        MMX_LAUNCH_CHECK("sa_raw_row_kernel");
        return MMX_OK;
    }
    const int strips = sa_cam_strips(N);
    char* ws = static_cast<char*>(workspace_dev);
    float* w = reinterpret_cast<float*>(ws);
    float* mm = reinterpret_cast<float*>(ws + align256(f * nb * H));
    float* row = reinterpret_cast<float*>(ws + align256(f * nb * H) + align256(f * nb * strips * 2));
    sa_gradcam_w_kernel<<<static_cast<unsigned>(B) * H, kSaThreads, 0, s>>>(static_cast<const float*>(grad_dev), w, T, V, tl, vl, H);
    MMX_LAUNCH_CHECK("sa_gradcam_w_kernel");
    sa_gradcam_cam_kernel<<<static_cast<unsigned>(B) * strips, kSaThreads, 0, s>>>(P, w, mm, row, H, T, V, strips, tl, vl);
    MMX_LAUNCH_CHECK("sa_gradcam_cam_kernel");
    sa_gradcam_out_kernel<<<static_cast<unsigned>(B), kSaThreads, 0, s>>>(mm, row, out, T, V, strips, tl, vl);
    MMX_LAUNCH_CHECK("sa_gradcam_out_kernel");
    return MMX_OK;
}

extern "C" size_t mmx_selfattn_rollout_row_workspace_bytes(int n_layers, int B, int T, int V) {
    if (n_layers < 1 || n_layers > kSaMaxTable || B < 1 || !sa_sizes_ok(T, V)) return 0;
    const size_t N = static_cast<size_t>(T + V);
    return align256(sizeof(float) * static_cast<size_t>(B) * n_layers * N * row_stride4(T + V));
}

// the rollout (grad_table null) and generate_ours: the matrices of the layers into the workspace, then the row chain on them
static int sa_chain_row(const void* const* attn_table, const void* const* grad_table, int n_layers, int B, int H, int T, int V,
                        const void* text_len_dev, const void* vis_len_dev, void* out_dev, void* workspace_dev, size_t workspace_bytes,
                        void* stream) {
    const bool ours = grad_table != nullptr;
    const char* me = ours ? "mmx_selfattn_ours_row" : "mmx_selfattn_rollout_row";
    MMX_CHECK_ARG(attn_table && out_dev && workspace_dev, "%s: null pointer", me);
    MMX_CHECK_ARG(B > 0 && H > 0, "%s: B=%d H=%d (both >= 1)", me, B, H);
    MMX_CHECK_ARG(sa_sizes_ok(T, V), "%s: T=%d V=%d outside T >= 2, V >= 1, T + V <= %d", me, T, V, kSaMaxN);
    MMX_CHECK_ARG(n_layers >= 1 && n_layers <= kSaMaxTable, "%s: n_layers=%d outside 1..%d", me, n_layers, kSaMaxTable);
    const int N = T + V;
    const int strips = (N * N + kSaMeanStrip - 1) / kSaMeanStrip;
    const int64_t groups = static_cast<int64_t>(B) * n_layers * strips;
    if (int rc = check_grid(me, groups, "B=%d x n_layers=%d x %d strips", B, n_layers, strips)) return rc;
    const size_t need = mmx_selfattn_rollout_row_workspace_bytes(n_layers, B, T, V);
    const char* query = ours ? "mmx_selfattn_ours_row_workspace_bytes" : "mmx_selfattn_rollout_row_workspace_bytes";
    if (int rc = check_workspace(me, query, workspace_dev, workspace_bytes, need)) return rc;
    SaRolloutArgs a;
    memset(&a, 0, sizeof(a));
    if (int rc = copy_table(me, ours ? "a table" : "the table", attn_table, n_layers, a.attn, grad_table, a.grad)) return rc;
    const size_t f = sizeof(float), nb = static_cast<size_t>(B);
    const Span outs[2] = {{out_dev, f * nb * N}, {workspace_dev, need}};
    Span ins[2 * kSaMaxTable + 2];
    int n_in = 0;
    for (int l = 0; l < n_layers; ++l) {
        ins[n_in++] = {attn_table[l], f * nb * H * N * N};
        if (ours) ins[n_in++] = {grad_table[l], f * nb * H * N * N};
    }
    ins[n_in++] = {text_len_dev, sizeof(int) * nb};
    ins[n_in++] = {vis_len_dev, sizeof(int) * nb};
    MMX_CHECK_ARG(!spans_alias(outs, 2, ins, n_in), "%s: the output or the workspace may not alias an input or each other", me);
    a.n_layers = n_layers; a.B = B; a.H = H; a.T = T; a.V = V; a.strips = strips;
    a.text_len = static_cast<const int*>(text_len_dev);
    a.vis_len = static_cast<const int*>(vis_len_dev);
    a.ws = static_cast<float*>(workspace_dev);
    a.out = static_cast<float*>(out_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (ours) {
        sa_ours_means_kernel<<<static_cast<unsigned>(groups), kSaThreads, 0, s>>>(a);
        MMX_LAUNCH_CHECK("sa_ours_means_kernel");
    } else {
        sa_rollout_means_kernel<<<static_cast<unsigned>(groups), kSaThreads, 0, s>>>(a);
        MMX_LAUNCH_CHECK("sa_rollout_means_kernel");
    }
    sa_rollout_row_kernel<<<static_cast<unsigned>(B), kSaThreads, 0, s>>>(a);
    MMX_LAUNCH_CHECK("sa_rollout_row_kernel");
    return MMX_OK;
}

extern "C" int mmx_selfattn_rollout_row(const void* const* attn_table, int n_layers, int B, int H, int T, int V,
                                        const void* text_len_dev, const void* vis_len_dev, void* out_dev, void* workspace_dev,
                                        size_t workspace_bytes, void* stream) {
    return sa_chain_row(attn_table, nullptr, n_layers, B, H, T, V, text_len_dev, vis_len_dev, out_dev, workspace_dev, workspace_bytes,
                        stream);
}

// the workspace is the rollout's: one head-mean matrix per (sample, layer)
extern "C" size_t mmx_selfattn_ours_row_workspace_bytes(int n_layers, int B, int T, int V) {
    return mmx_selfattn_rollout_row_workspace_bytes(n_layers, B, T, V);
}

extern "C" int mmx_selfattn_ours_row(const void* const* attn_table, const void* const* grad_table, int n_layers, int B, int H, int T,
                                     int V, const void* text_len_dev, const void* vis_len_dev, void* out_dev, void* workspace_dev,
                                     size_t workspace_bytes, void* stream) {
    MMX_CHECK_ARG(grad_table, "mmx_selfattn_ours_row: null pointer");
    return sa_chain_row(attn_table, grad_table, n_layers, B, H, T, V, text_len_dev, vis_len_dev, out_dev, workspace_dev, workspace_bytes,
                        stream);
}
