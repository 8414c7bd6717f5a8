// The attention-only baselines of DETR for ALL K kept queries of one image in one pass: raw attention
// (DETR/modules/ExplanationGenerator.py:226-238), rollout (:240-273 with compute_rollout_attention, :5-16) and attention GradCAM
// (:275-305).  All three return ROW t_k = targets[k] of a [Q, Ni] map, so everything here is done on row vectors.
//
// Notation: P_x [H, Q, Ni] the last decoder layer's cross-attention slab, A_l [H, Ni, Ni] the encoder self-attention slabs,
// B_l [H, Q, Q] the decoder self-attention slabs, a bar = (sum_h .) / H, M^ = (M~ + I) / rowsum(M~ + I) with M~ the barred matrix.
//
//   raw attention   out[k, :] = P~_x[t_k, :].
//   GradCAM         w[k, h] = (sum_{q, j} grad[k, h, q, j]) / (Q Ni)  -- over the WHOLE [Q, Ni] block, as grad.mean([1, 2]) states it;
//                   out[k, :] = max(0, (sum_h P_x[h, t_k, :] w[k, h]) / H).
//   rollout         R_qq = B^_Ld ... B^_1, R_ii = A^_Le ... A^_1; row t_k of R_qq^T (P~_x R_ii) is ((R_qq e_t)^T P~_x) R_ii:
//                   1. u_k = B^_Ld( ... (B^_1 e_t)):   y <- (B~_l y + y) / r_l,  r_l[i] = 1 + sum_j B~_l[i, j]   (bottom-up, Q-vectors)
//                   2. s_k = u_k^T P~_x                                                                     (an Ni-vector)
//                   3. x <- s_k; for l = Le ... 1:  x <- w A~_l + w,  w[i] = x[i] / r_l[i],  r_l[i] = 1 + sum_j A~_l[i, j].
//                   No Ni x Ni product ever exists; R_ii, R_qq and P~_x R_ii are never formed.
//
// Launches (plain, ordered by the stream; no tickets, no spinning, no atomics; every sum in a fixed order):
//   dc_raw_kernel        (k, 256 columns): the H values of row t_k, heads in order, one division.
//   dc_w_part_kernel     (k, h, strip of 8192 floats of the [Q, Ni] gradient block): 16-byte loads, the strip's sum -> workspace.
//   dc_cam_kernel        (k, 256 columns): w[k, h] = (the strips' sums, in order) / float(Q Ni), then the FMA over the heads.
//   db_enc_means_kernel  (layer, strip of 4 rows): every encoder slab is read ONCE, here.  Four consecutive rows of a head are one
//                        contiguous run of 4 Ni floats that starts 16-byte aligned whatever Ni is; it is read with UNCONDITIONAL 16-byte loads
//                        (the one chunk past a head's end from a clamped address), a batch of heads in flight, summed heads in order.  The strip's head mean goes to LDS, from there to the
//                        workspace (rows ceil(Ni / 4) * 4 floats apart, zeros behind a row) together with r_l of its four rows (a wave per
//                        row).  Le x ceil(Ni / 4) workgroups: 1428 at 950 tokens.
//   db_flat_means_kernel B~_l and P~_x, an element per thread, written once: no decoder slab is read again per k.
//   db_dec_chain_kernel  one workgroup per k: step 1 with y in LDS, a wave per row (B~_l comes from the workspace: 40 KB a layer).
//   db_s_kernel          (k, 256 columns): step 2, an FMA per query in order.
//   db_enc_step_kernel   (8 vectors, strip of 8 rows) of layer l: partial[strip][k][:] = sum_{i in strip} w[k, i] A~_l[i, :], FMAs in row
//                        order, every row loaded once for the eight vectors with aligned 16-byte loads from clamped addresses.
//   db_enc_reduce_kernel (k, 256 columns): x[k, j] <- (the strips' partials, in order) + w[k, j]; the last layer writes the output.
// A vector's arithmetic never looks at K or at k: row k's bits depend neither on K nor on k's position, and two calls give the same
// bits.  targets are clamped to 0 .. Q - 1 before they form an address.
#include "mmx_common.h"

namespace mmx {

constexpr int kDbMaxQ = 128;
constexpr int kDbMaxNi = 2048;
constexpr int kDbMaxH = 32;
constexpr int kDbMaxK = 1 << 20;                // grid.x carries K (x H for the GradCAM sums)
constexpr int kDbMaxTable = MMX_BASELINES_MAX_TABLE;
constexpr int kDbThreads = 256;
constexpr int kDbWaves = kDbThreads / 64;
constexpr int kDbMeanRows = 4;                  // rows of a head-mean strip: 4 Ni floats start 16-byte aligned for every Ni
constexpr int kDbHeadBatch = 8;                 // heads in flight per chunk of the head-mean stream
constexpr int kDbStepRows = 8;                  // rows of a vector-matrix strip
constexpr int kDbStepVecs = 8;                  // vectors carried through a strip by one workgroup
constexpr int kDcStripChunks = 8;               // 16-byte chunks per thread of a gradient strip
constexpr int kDcStrip = kDbThreads * kDcStripChunks * 4;     // floats per gradient strip

__device__ __forceinline__ int db_target(const int64_t* targets, int k, int Q) {
    const int64_t t = targets[k];
    return t < 0 ? 0 : (t > Q - 1 ? Q - 1 : static_cast<int>(t));
}
__device__ __forceinline__ f32x4 fma4(float w, f32x4 a, f32x4 acc) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = __builtin_fmaf(w, a[e], acc[e]);
    return r;
}

// ------------------------------------------------------------------------------------------------ raw attention / GradCAM
__global__ __launch_bounds__(kDbThreads) void dc_raw_kernel(const float* __restrict__ attn, const int64_t* __restrict__ targets,
                                                            float* __restrict__ out, int H, int Q, int Ni) {
    const int k = blockIdx.x, j = blockIdx.y * kDbThreads + threadIdx.x;
    if (j >= Ni) return;
    const int t = db_target(targets, k, Q);
    const int64_t hs = static_cast<int64_t>(Q) * Ni;
    const float* P = attn + static_cast<int64_t>(t) * Ni + j;
    float s = P[0];
    for (int h = 1; h < H; ++h) s += P[h * hs];
    out[static_cast<int64_t>(k) * Ni + j] = s / static_cast<float>(H);
}

// the sum of one strip of the flat [Q Ni] gradient block of (k, h): per thread kDcStripChunks chunks in order, the four components as
// (0 + 1) + (2 + 3), the xor tree of the wave, the four waves as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(kDbThreads) void dc_w_part_kernel(const float* __restrict__ grad, float* __restrict__ wpart, int n,
                                                               int strips) {
    __shared__ float part[kDbWaves];
    const int kh = blockIdx.x, s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (a shared slab is launched for k = 0 only: kh = h; per-sample slabs are contiguous, bstride = H n, so block kh starts at kh n)
    const float* G = grad + static_cast<int64_t>(kh) * n;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < kDcStripChunks; ++c) {
        const int p = s * kDcStrip + (c * kDbThreads + tid) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (p + 3 < n) {
            v = ldg4_u(G + p);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p + e < n) v[e] = G[p + e];
        }
        acc += v;
    }
    float t = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (lane == 0) part[wave] = t;
    __syncthreads();
    if (tid == 0) wpart[static_cast<int64_t>(kh) * strips + s] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(kDbThreads) void dc_cam_kernel(const float* __restrict__ attn, const float* __restrict__ wpart,
                                                            int shared_grad, const int64_t* __restrict__ targets,
                                                            float* __restrict__ out, int H, int Q, int Ni, int strips) {
    __shared__ float w[kDbMaxH];
    const int k = blockIdx.x, tid = threadIdx.x, j = blockIdx.y * kDbThreads + tid;
    if (tid < H) {
        const float* p = wpart + (static_cast<int64_t>(shared_grad ? 0 : k) * H + tid) * strips;
        float s = p[0];
        for (int u = 1; u < strips; ++u) s += p[u];
        w[tid] = s / static_cast<float>(Q * Ni);                     // the sum first, then ONE division by the block's size
    }
    __syncthreads();
    if (j >= Ni) return;
    const int t = db_target(targets, k, Q);
    const int64_t hs = static_cast<int64_t>(Q) * Ni;
    const float* P = attn + static_cast<int64_t>(t) * Ni + j;
    float acc = P[0] * w[0];
    for (int h = 1; h < H; ++h) acc = __builtin_fmaf(P[h * hs], w[h], acc);
    out[static_cast<int64_t>(k) * Ni + j] = relu_nan(acc / static_cast<float>(H));
}

// ------------------------------------------------------------------------------------------------ rollout
struct DbTable {
    const float* p[kDbMaxTable];
};

struct DbRolloutArgs {
    int n_enc, n_dec, K, H, Q, Ni, NP, strips;     // strips = ceil(Ni / kDbStepRows)
    const int64_t* targets;
    float* abar;      // [n_enc][Ni][NP]
    float* renc;      // [n_enc][Ni]
    float* bbar;      // [n_dec][Q][Q]
    float* pbar;      // [Q][Ni]
    float* u;         // [K][Q]
    float* x;         // [K][Ni]
    float* part;      // [strips][K][NP]
    float* out;       // [K][Ni]
};

__global__ __launch_bounds__(kDbThreads) void db_enc_means_kernel(const DbTable tab, const DbRolloutArgs a) {
    __shared__ float m[kDbMeanRows * kDbMaxNi];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Ni = a.Ni, NP = a.NP, H = a.H;
    const int strips4 = (Ni + kDbMeanRows - 1) / kDbMeanRows;
    const int l = blockIdx.x / strips4, s = blockIdx.x - l * strips4;
    const int i0 = s * kDbMeanRows, rows = min(kDbMeanRows, Ni - i0), n = rows * Ni;
    const int64_t hs = static_cast<int64_t>(Ni) * Ni, p0 = static_cast<int64_t>(i0) * Ni;
    const float* __restrict__ head0 = tab.p[l];
    const float fH = static_cast<float>(H);
    if (hs >= 4) {
        // every chunk is loaded UNCONDITIONALLY: the one chunk of a layer that would run past the head's Ni x Ni block (the last of
        // the last strip, when Ni^2 is no multiple of 4) is loaded from the clamped position hs - 4 and shifted into place
        // afterwards, so a chunk is one basic block of loads and adds and the waits are counted
        for (int c = tid; c * 4 < n; c += kDbThreads) {
            const int p = c * 4;
            const int64_t P = p0 + p, q = P < hs - 4 ? P : hs - 4;
            const int d = static_cast<int>(P - q);                   // 0, or 1 .. 3 for that one chunk
            const float* __restrict__ src = head0 + q;
            f32x4 acc = ldg4_u(src);
            int h = 1;
            for (; h + kDbHeadBatch <= H; h += kDbHeadBatch) {
                f32x4 v[kDbHeadBatch];
#pragma unroll
                for (int u = 0; u < kDbHeadBatch; ++u) v[u] = ldg4_u(src + (h + u) * hs);
#pragma unroll
                for (int u = 0; u < kDbHeadBatch; ++u) acc += v[u];
            }
            for (; h < H; ++h) acc += ldg4_u(src + h * hs);
            const f32x4 r = d == 0 ? acc
                          : d == 1 ? f32x4{acc[1], acc[2], acc[3], 0.f}
                          : d == 2 ? f32x4{acc[2], acc[3], 0.f, 0.f} : f32x4{acc[3], 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p + e < n) m[p + e] = r[e] / fH;
        }
    } else if (tid == 0) {                                           // Ni = 1: one float per head
        float t = head0[0];
        for (int h = 1; h < H; ++h) t += head0[h * hs];
        m[0] = t / fH;
    }
    __syncthreads();
    if (wave < rows) {                                               // r_l of row i0 + wave: lane partials, then the xor tree
        float t = 0.f;
        for (int j = lane; j < Ni; j += 64) t += m[wave * Ni + j];
        t = wave_sum(t);
        if (lane == 0) a.renc[static_cast<int64_t>(l) * Ni + i0 + wave] = 1.0f + t;
    }
    float* dst = a.abar + (static_cast<int64_t>(l) * Ni + i0) * NP;
    for (int e = tid; e < rows * NP; e += kDbThreads) {
        const int row = e / NP, col = e - row * NP;
        dst[e] = col < Ni ? m[row * Ni + col] : 0.f;
    }
}

// dst[y][p] = (sum_h tab[y][h n + p]) / H, heads in order
__global__ __launch_bounds__(kDbThreads) void db_flat_means_kernel(const DbTable tab, float* __restrict__ dst, int H, int n) {
    const int p = blockIdx.x * kDbThreads + threadIdx.x, y = blockIdx.y;
    if (p >= n) return;
    const float* src = tab.p[y] + p;
    float s = src[0];
    for (int h = 1; h < H; ++h) s += src[static_cast<int64_t>(h) * n];
    dst[static_cast<int64_t>(y) * n + p] = s / static_cast<float>(H);
}

__global__ __launch_bounds__(kDbThreads) void db_dec_chain_kernel(const DbRolloutArgs a) {
    __shared__ float y[kDbMaxQ], yn[kDbMaxQ];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Q = a.Q;
    const int t = db_target(a.targets, k, Q);
    if (tid < kDbMaxQ) y[tid] = tid == t ? 1.f : 0.f;
    __syncthreads();
    const bool has0 = lane < Q, has1 = lane + 64 < Q;
    for (int l = 0; l < a.n_dec; ++l) {
        const float* B = a.bbar + static_cast<int64_t>(l) * Q * Q;
        const float y0 = y[lane], y1 = y[lane + 64];
        for (int i = wave; i < Q; i += kDbWaves) {
            const float b0 = has0 ? B[i * Q + lane] : 0.f, b1 = has1 ? B[i * Q + lane + 64] : 0.f;
            const float d = wave_sum(__builtin_fmaf(b1, y1, b0 * y0));
            const float rs = wave_sum(b0 + b1);
            if (lane == 0) yn[i] = (d + y[i]) / (1.0f + rs);
        }
        __syncthreads();
        if (tid < Q) y[tid] = yn[tid];
        __syncthreads();
    }
    if (tid < Q) a.u[static_cast<int64_t>(k) * Q + tid] = y[tid];
}

__global__ __launch_bounds__(kDbThreads) void db_s_kernel(const DbRolloutArgs a) {
    __shared__ float u[kDbMaxQ];
    const int k = blockIdx.x, tid = threadIdx.x, j = blockIdx.y * kDbThreads + tid, Q = a.Q, Ni = a.Ni;
    if (tid < Q) u[tid] = a.u[static_cast<int64_t>(k) * Q + tid];
    __syncthreads();
    if (j >= Ni) return;
    float acc = 0.f;
    for (int q = 0; q < Q; ++q) acc = __builtin_fmaf(u[q], a.pbar[static_cast<int64_t>(q) * Ni + j], acc);
    a.x[static_cast<int64_t>(k) * Ni + j] = acc;
}

__global__ __launch_bounds__(kDbThreads) void db_enc_step_kernel(const DbRolloutArgs a, int l) {
    __shared__ float wv[kDbStepVecs][kDbStepRows];
    const int tid = threadIdx.x, Ni = a.Ni, NP = a.NP, K = a.K;
    const int k0 = blockIdx.x * kDbStepVecs, s = blockIdx.y, i0 = s * kDbStepRows;
    if (tid < kDbStepVecs * kDbStepRows) {
        const int kk = tid / kDbStepRows, ii = tid - kk * kDbStepRows, k = k0 + kk, i = i0 + ii;
        wv[kk][ii] = (k < K && i < Ni) ? a.x[static_cast<int64_t>(k) * Ni + i] / a.renc[static_cast<int64_t>(l) * Ni + i] : 0.f;
    }
    __syncthreads();
    const int nch = NP / 4;
    // a thread owns the 16-byte chunks tid and tid + 256 of a row; past the row's end it repeats the last chunk and drops the result
    const int c0 = tid, c1 = tid + kDbThreads, cc0 = min(c0, nch - 1), cc1 = min(c1, nch - 1);
    f32x4 acc0[kDbStepVecs], acc1[kDbStepVecs];
#pragma unroll
    for (int kk = 0; kk < kDbStepVecs; ++kk) {
        acc0[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc1[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float* A = a.abar + static_cast<int64_t>(l) * Ni * NP;
    f32x4 r0[kDbStepRows], r1[kDbStepRows];
#pragma unroll
    for (int ii = 0; ii < kDbStepRows; ++ii) {                       // rows past Ni repeat the last row, times w = 0
        const float* row = A + static_cast<int64_t>(min(i0 + ii, Ni - 1)) * NP;
        r0[ii] = *reinterpret_cast<const f32x4*>(row + 4 * cc0);
        r1[ii] = *reinterpret_cast<const f32x4*>(row + 4 * cc1);
    }
#pragma unroll
    for (int ii = 0; ii < kDbStepRows; ++ii) {
#pragma unroll
        for (int kk = 0; kk < kDbStepVecs; ++kk) {
            const float w = wv[kk][ii];
            acc0[kk] = fma4(w, r0[ii], acc0[kk]);
            acc1[kk] = fma4(w, r1[ii], acc1[kk]);
        }
    }
#pragma unroll
    for (int kk = 0; kk < kDbStepVecs; ++kk) {
        const int k = k0 + kk;
        if (k >= K) break;
        float* dst = a.part + (static_cast<int64_t>(s) * K + k) * NP;
        if (c0 < nch) *reinterpret_cast<f32x4*>(dst + 4 * c0) = acc0[kk];
        if (c1 < nch) *reinterpret_cast<f32x4*>(dst + 4 * c1) = acc1[kk];
    }
}

__global__ __launch_bounds__(kDbThreads) void db_enc_reduce_kernel(const DbRolloutArgs a, int l, float* __restrict__ dst) {
    const int k = blockIdx.x, j = blockIdx.y * kDbThreads + threadIdx.x, Ni = a.Ni, NP = a.NP, K = a.K;
    if (j >= Ni) return;
    const float* p = a.part + static_cast<int64_t>(k) * NP + j;
    const int64_t ss = static_cast<int64_t>(K) * NP;
    float acc = p[0];
    for (int s = 1; s < a.strips; ++s) acc += p[s * ss];
    const int64_t at = static_cast<int64_t>(k) * Ni + j;
    const float w = a.x[at] / a.renc[static_cast<int64_t>(l) * Ni + j];
    dst[at] = acc + w;
}

}  // namespace mmx

using namespace mmx;

static inline bool db_sizes_ok(int K, int H, int Q, int Ni) {
    return K >= 1 && K <= kDbMaxK && H >= 1 && H <= kDbMaxH && Q >= 1 && Q <= kDbMaxQ && Ni >= 1 && Ni <= kDbMaxNi;
}
static inline int dc_strips(int Q, int Ni) { return (Q * Ni + kDcStrip - 1) / kDcStrip; }

// workspace of the GradCAM form: the strips' sums [K, H, strips]
extern "C" size_t mmx_detr_cross_rows_workspace_bytes(int K, int H, int Q, int Ni) {
    if (!db_sizes_ok(K, H, Q, Ni)) return 0;
    return align256(sizeof(float) * static_cast<size_t>(K) * H * dc_strips(Q, Ni));
}

extern "C" int mmx_detr_cross_rows(const void* cross_attn_dev, const void* cross_grad_dev, int64_t grad_bstride, const void* targets_dev,
                                   void* out_dev, int K, int H, int Q, int Ni, void* workspace_dev, size_t workspace_bytes,
                                   void* stream) {
    MMX_CHECK_ARG(cross_attn_dev && targets_dev && out_dev, "mmx_detr_cross_rows: null pointer");
    MMX_CHECK_ARG(db_sizes_ok(K, H, Q, Ni), "mmx_detr_cross_rows: K=%d H=%d Q=%d Ni=%d outside 1 <= K <= %d, 1 <= H <= %d, 1 <= Q <= %d, "
                  "1 <= Ni <= %d", K, H, Q, Ni, kDbMaxK, kDbMaxH, kDbMaxQ, kDbMaxNi);
    const size_t f = sizeof(float), slab = f * H * Q * Ni;
    const size_t need = cross_grad_dev ? mmx_detr_cross_rows_workspace_bytes(K, H, Q, Ni) : 0;
    if (cross_grad_dev) {
        MMX_CHECK_ARG(grad_bstride == 0 || grad_bstride == static_cast<int64_t>(H) * Q * Ni,
                      "mmx_detr_cross_rows: grad_bstride=%lld is neither 0 (one shared slab) nor H Q Ni = %lld",
                      static_cast<long long>(grad_bstride), static_cast<long long>(H) * Q * Ni);
        MMX_CHECK_ARG(workspace_dev, "mmx_detr_cross_rows: null pointer (the GradCAM form needs a workspace)");
        if (int rc = check_workspace("mmx_detr_cross_rows", "mmx_detr_cross_rows_workspace_bytes", workspace_dev, workspace_bytes, need))
            return rc;
    }
    const size_t grad_bytes = slab * (grad_bstride ? static_cast<size_t>(K) : 1);
    const Span outs[2] = {{out_dev, f * static_cast<size_t>(K) * Ni}, {cross_grad_dev ? workspace_dev : nullptr, need}};
    const Span ins[3] = {{cross_attn_dev, slab}, {cross_grad_dev, grad_bytes}, {targets_dev, sizeof(int64_t) * static_cast<size_t>(K)}};
    MMX_CHECK_ARG(!spans_alias(outs, 2, ins, 3), "mmx_detr_cross_rows: the output or the workspace may not alias an input or each other");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* P = static_cast<const float*>(cross_attn_dev);
    const int64_t* tg = static_cast<const int64_t*>(targets_dev);
    float* out = static_cast<float*>(out_dev);
    const dim3 cols(static_cast<unsigned>(K), static_cast<unsigned>((Ni + kDbThreads - 1) / kDbThreads));
    if (!cross_grad_dev) {
        dc_raw_kernel<<<cols, kDbThreads, 0, s>>>(P, tg, out, H, Q, Ni);
        MMX_LAUNCH_CHECK("dc_raw_kernel");
        return MMX_OK;
    }
    const int strips = dc_strips(Q, Ni), shared_grad = grad_bstride == 0;
    float* wpart = static_cast<float*>(workspace_dev);
    const dim3 wgrid(static_cast<unsigned>(shared_grad ? 1 : K) * H, static_cast<unsigned>(strips));
    dc_w_part_kernel<<<wgrid, kDbThreads, 0, s>>>(static_cast<const float*>(cross_grad_dev), wpart, Q * Ni, strips);
    MMX_LAUNCH_CHECK("dc_w_part_kernel");
    dc_cam_kernel<<<cols, kDbThreads, 0, s>>>(P, wpart, shared_grad, tg, out, H, Q, Ni, strips);
    MMX_LAUNCH_CHECK("dc_cam_kernel");
    return MMX_OK;
}

namespace {
struct DbLayout {
    size_t abar, renc, bbar, pbar, u, x, part, total;
};
DbLayout db_layout(int n_enc, int n_dec, int K, int Q, int Ni) {
    const size_t f = sizeof(float), NP = row_stride4(Ni), strips = (Ni + kDbStepRows - 1) / kDbStepRows, nk = static_cast<size_t>(K);
    DbLayout L;
    size_t at = 0;
    L.abar = at; at += align256(f * n_enc * Ni * NP);
    L.renc = at; at += align256(f * n_enc * Ni);
    L.bbar = at; at += align256(f * n_dec * Q * Q);
    L.pbar = at; at += align256(f * Q * Ni);
    L.u = at;    at += align256(f * nk * Q);
    L.x = at;    at += align256(f * nk * Ni);
    L.part = at; at += align256(f * strips * nk * NP);
    L.total = at;
    return L;
}
bool db_tables_ok(int n_enc, int n_dec) { return n_enc >= 1 && n_enc <= kDbMaxTable && n_dec >= 1 && n_dec <= kDbMaxTable; }
}  // namespace

// head means of the encoder slabs [n_enc, Ni, NP] | r [n_enc, Ni] | B~ [n_dec, Q, Q] | P~_x [Q, Ni] | u [K, Q] | x [K, Ni] |
// partials [ceil(Ni / 8), K, NP], each part 256-byte aligned
extern "C" size_t mmx_detr_rollout_rows_workspace_bytes(int n_enc, int n_dec, int K, int Q, int Ni) {
    if (!db_tables_ok(n_enc, n_dec) || !db_sizes_ok(K, 1, Q, Ni)) return 0;
    return db_layout(n_enc, n_dec, K, Q, Ni).total;
}

extern "C" int mmx_detr_rollout_rows(const void* const* enc_table, int n_enc, const void* const* dec_self_table, int n_dec,
                                     const void* cross_attn_dev, const void* targets_dev, void* out_dev, int K, int H, int Q, int Ni,
                                     void* workspace_dev, size_t workspace_bytes, void* stream) {
    MMX_CHECK_ARG(enc_table && dec_self_table && cross_attn_dev && targets_dev && out_dev && workspace_dev,
                  "mmx_detr_rollout_rows: null pointer");
    MMX_CHECK_ARG(db_sizes_ok(K, H, Q, Ni), "mmx_detr_rollout_rows: K=%d H=%d Q=%d Ni=%d outside 1 <= K <= %d, 1 <= H <= %d, 1 <= Q <= %d, "
                  "1 <= Ni <= %d", K, H, Q, Ni, kDbMaxK, kDbMaxH, kDbMaxQ, kDbMaxNi);
    MMX_CHECK_ARG(db_tables_ok(n_enc, n_dec), "mmx_detr_rollout_rows: tables of %d and %d entries outside 1..%d", n_enc, n_dec, kDbMaxTable);
    const DbLayout L = db_layout(n_enc, n_dec, K, Q, Ni);
    const char* me = "mmx_detr_rollout_rows";
    if (int rc = check_workspace(me, "mmx_detr_rollout_rows_workspace_bytes", workspace_dev, workspace_bytes, L.total)) return rc;
    DbTable enc, dec, cross;
    memset(&enc, 0, sizeof(enc));
    memset(&dec, 0, sizeof(dec));
    memset(&cross, 0, sizeof(cross));
    if (int rc = copy_table(me, "the encoder table", enc_table, n_enc, enc.p)) return rc;
    if (int rc = copy_table(me, "the decoder table", dec_self_table, n_dec, dec.p)) return rc;
    cross.p[0] = static_cast<const float*>(cross_attn_dev);
    const size_t f = sizeof(float), nk = static_cast<size_t>(K);
    const Span outs[2] = {{out_dev, f * nk * Ni}, {workspace_dev, L.total}};
    Span ins[2 * kDbMaxTable + 2];
    int n_in = 0;
    for (int l = 0; l < n_enc; ++l) ins[n_in++] = {enc_table[l], f * H * Ni * Ni};
    for (int l = 0; l < n_dec; ++l) ins[n_in++] = {dec_self_table[l], f * H * Q * Q};
    ins[n_in++] = {cross_attn_dev, f * H * Q * Ni};
    ins[n_in++] = {targets_dev, sizeof(int64_t) * nk};
    MMX_CHECK_ARG(!spans_alias(outs, 2, ins, n_in), "mmx_detr_rollout_rows: the output or the workspace may not alias an input or each other");
    char* ws = static_cast<char*>(workspace_dev);
    DbRolloutArgs a;
    memset(&a, 0, sizeof(a));
    a.n_enc = n_enc; a.n_dec = n_dec; a.K = K; a.H = H; a.Q = Q; a.Ni = Ni;
    a.NP = row_stride4(Ni);
    a.strips = (Ni + kDbStepRows - 1) / kDbStepRows;
    a.targets = static_cast<const int64_t*>(targets_dev);
    a.abar = reinterpret_cast<float*>(ws + L.abar);
    a.renc = reinterpret_cast<float*>(ws + L.renc);
    a.bbar = reinterpret_cast<float*>(ws + L.bbar);
    a.pbar = reinterpret_cast<float*>(ws + L.pbar);
    a.u = reinterpret_cast<float*>(ws + L.u);
    a.x = reinterpret_cast<float*>(ws + L.x);
    a.part = reinterpret_cast<float*>(ws + L.part);
    a.out = static_cast<float*>(out_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned uK = static_cast<unsigned>(K);
    const dim3 cols(uK, static_cast<unsigned>((Ni + kDbThreads - 1) / kDbThreads));
    db_flat_means_kernel<<<dim3((Q * Q + kDbThreads - 1) / kDbThreads, n_dec), kDbThreads, 0, s>>>(dec, a.bbar, H, Q * Q);
    MMX_LAUNCH_CHECK("db_flat_means_kernel (decoder)");
    db_flat_means_kernel<<<dim3((Q * Ni + kDbThreads - 1) / kDbThreads, 1), kDbThreads, 0, s>>>(cross, a.pbar, H, Q * Ni);
    MMX_LAUNCH_CHECK("db_flat_means_kernel (cross)");
    db_dec_chain_kernel<<<uK, kDbThreads, 0, s>>>(a);
    MMX_LAUNCH_CHECK("db_dec_chain_kernel");
    db_s_kernel<<<cols, kDbThreads, 0, s>>>(a);
    MMX_LAUNCH_CHECK("db_s_kernel");
    db_enc_means_kernel<<<static_cast<unsigned>(n_enc) * ((Ni + kDbMeanRows - 1) / kDbMeanRows), kDbThreads, 0, s>>>(enc, a);
    MMX_LAUNCH_CHECK("db_enc_means_kernel");
    const dim3 step((uK + kDbStepVecs - 1) / kDbStepVecs, static_cast<unsigned>(a.strips));
    for (int l = n_enc - 1; l >= 0; --l) {
        db_enc_step_kernel<<<step, kDbThreads, 0, s>>>(a, l);
        MMX_LAUNCH_CHECK("db_enc_step_kernel");
        db_enc_reduce_kernel<<<cols, kDbThreads, 0, s>>>(a, l, l == 0 ? a.out : a.x);
        MMX_LAUNCH_CHECK("db_enc_reduce_kernel");
    }
    return MMX_OK;
}
