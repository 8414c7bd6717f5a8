// The self-attention relevancy chain  R <- R + A_bar_l . R,  A_bar_l = mean_h clamp(G_l * A_l, 0)  (rules 5 + 6) behind its C entries
// (include/mmx_relevancy.h): the chain's options, the ONE function that decides which kernel runs with how many layer groups, the
// entries built on it, the two-launch split path for long sequences, and the fp16-mode chain's long path.  The kernels themselves:
// relevancy_chain_fused.hip (K1), relevancy_chain_groups.hip (K1g), relevancy_chain_cols.hip (K1c), relevancy_chain_rows.hip.
#include "mmx_common.h"

namespace mmx {

// ----------------------------------------------------------------------------------------- options
// option "debug_flags" (profiling only), ONE meaning per bit whatever kernel the dispatcher picks:
//   1  return before the hand-off / combine (fused + groups kernels; the cols kernel has neither and ignores it)
//   4  matrix waves skip the MFMAs (all three kernels)          8  groups kernel: take the ticket, skip the combine
//   16 cols kernel: no block rotation
//   32 / 64  long-sequence layer kernel (relevancy_chain_rows.hip): no head reduction / return after the head reduction
static int g_debug_flags = 0;
static int g_chain_pipe = 4;     // option "self_chain_pipe": software-pipelined stream waves of the fused chain (fp32 slabs):
                                 // 0 off | 1 one chunk per lane and head | 2 / 4: up to that many contiguous chunks
static int g_chain_nt = 1;       // option "self_chain_nt": nt cache policy on the read-once slab loads of the pipelined stream waves
                                 // (default since round 4: text tower 85.8 -> 82.0 us, image 65.5 -> 63.8 us inside the replayed step)
static int g_chain_groups = 0;  // layer groups per sample of the per-sample kernel: 0 auto, 1 = strict sequential order
static int g_chain_rows = 0;    // option "self_chain_rows": 0 (default) avg_heads_kernel + the tiled product, two launches per layer | 1: N > 128, one
                                // right-hand side: a layer is ONE launch (relevancy_chain_rows.hip: head reduction of a 16-row block into LDS +
                                // that block row of the product).  Built in round 6, parity-green, and NOT faster: 27.6 vs 24.0 ms for the 24
                                // layers of cfg 5's slab variant (profiles/r06_chain_rows_probe.txt has the phase split and why)
static int g_chain_algo = 0;  // 0 auto = 4: layer groups with barrier-free stream waves where they apply (fp32 slabs, G > 1), else the fused
                              // per-sample kernel | 1: the fused kernel everywhere | 5: relevancy_chain_cols.hip wherever it applies

bool chain_option(const char* key, int value) {
    if (strcmp(key, "self_chain_cols_c") == 0 && value >= 0 && value <= 8) { chain_cols_options(value, -1); return true; }
    if (strcmp(key, "self_chain_cols_nb") == 0 && value >= 0 && value <= 8) { chain_cols_options(-1, value); return true; }
    if (strcmp(key, "self_chain_algo") == 0 && (value == 0 || value == 1 || value == 4 || value == 5)) { g_chain_algo = value; return true; }
    if (strcmp(key, "self_chain_pipe") == 0 && value >= 0 && value <= 4) { g_chain_pipe = value; return true; }
    if (strcmp(key, "self_chain_rows") == 0 && value >= 0 && value <= 1) { g_chain_rows = value; return true; }
    if (strcmp(key, "self_chain_nt") == 0 && value >= 0 && value <= 1) { g_chain_nt = value; return true; }
    if (strcmp(key, "self_chain_groups") == 0 && value >= 0 && value <= 8) { g_chain_groups = value; return true; }
    if (strcmp(key, "debug_flags") == 0) { g_debug_flags = value; return true; }
    return false;
}

// ----------------------------------------------------------------------------------------- the route
enum ChainKernel { kChainFused, kChainGroups, kChainCols, kChainSplit, kChainRows };
struct ChainRoute {
    ChainKernel kernel;
    int G;              // layer groups per sample (1 outside the fused and groups kernels)
};

static int chain_groups(int n_layers, int B, int H, int N) {
    if (n_layers < 2) return 1;
    int G = g_chain_groups;
    if (G == 0) {
        // auto: split only when a sample streams enough bytes to pay for the hand-off (>= 1 MB).  Then the FEWEST groups that put a
        // workgroup on ~70 % of the CUs: every further group adds an exact-fp32 product to the serial combine on ONE CU (~2.9 us each
        // at 77 tokens) while the stream rate is flat from ~190 workgroups on; never more workgroups than CUs (a second round of
        // workgroups costs far more than idle CUs: B = 96 / 128 at CLIP's text shape: G = 4 141 / 155 us, G = 2 96 / 120 us); at
        // most 4.  profiles/r05_chain_groups_probe.txt (B = 16 ... 128); rounds 1-4 used 4 groups up to B = 128.
        const double sample_bytes = 8.0 * n_layers * H * N * N;
        if (sample_bytes < 1e6) {
            G = 1;
        } else {
            const int cus = device_cu_count();
            G = (7 * cus + 10 * B - 1) / (10 * B);
            while (G > 1 && B * G > cus) --G;
            if (G > 4) G = 4;
        }
    }
    return G < n_layers ? G : n_layers;
}

// Which kernel runs, with how many layer groups: the only place that knows the rule (tests/chain_bounds.py::chain_route restates it
// for the tests).
//   N > 128, or an R_sq right-hand side (M > 0): per layer avg_heads + the tiled product; option self_chain_rows: one launch per layer.
//   fp32 slabs (not under self_chain_algo = 1) take the kernels with barrier-free stream waves: one group and N >= 40 (algo 5: wherever
//   it applies) the cols kernel with one workgroup per sample -- the fused kernel's single-group form, same bits; several groups the
//   groups kernel where its LDS images fit.  Everything else, 16-bit slabs included, the fused kernel.
static ChainRoute chain_route(int n_layers, int B, int H, int N, int M, int dtype) {
    if ((N + 15) / 16 > 8 || M != 0) return {g_chain_rows && M == 0 && chain_rows_layer_applies(N) ? kChainRows : kChainSplit, 1};
    const int G = chain_groups(n_layers, B, H, N);
    const bool barrier_free = g_chain_algo != 1 && dtype == MMX_F32;
    if (barrier_free && self_chain_cols_applies(n_layers, B, H, N) && (g_chain_algo == 5 || (N >= 40 && G == 1))) return {kChainCols, 1};
    if (barrier_free && G > 1 && self_chain_groups_applies(n_layers, G, H, N)) return {kChainGroups, G};
    return {kChainFused, G};
}

static size_t group_counter_bytes(int B) { return align256(sizeof(unsigned) * static_cast<size_t>(B)); }

static size_t chain_workspace_bytes(const ChainRoute& r, int B, int N, int M) {
    if (r.kernel == kChainSplit || r.kernel == kChainRows) {
        const size_t mat = align256(sizeof(float) * static_cast<size_t>(B) * N * N);
        const size_t sq = M > 0 ? align256(sizeof(float) * static_cast<size_t>(B) * N * M) : 0;
        return 2 * mat + sq;  // A_bar + R ping-pong [+ R_sq ping-pong]
    }
    if (r.G == 1) return 0;   // strict layer order, one workgroup per sample: no scratch
    return group_counter_bytes(B) + align256(sizeof(float) * static_cast<size_t>(B) * r.G * N * N);
}

// ----------------------------------------------------------------------------------------- entry checks
// The argument checks of mmx_relevancy_self_chain_flags and mmx_relevancy_self_chain_half (the latter: no R_sq, fp32 / fp16 slabs only,
// its own name in every text).  *attn_batch_stride < 0 becomes the full stride.
static int check_chain_args(const char* name, bool half, const void* const* attn_layers, const void* const* grad_layers, int n_layers,
                            int B, int H, int N, int M, int dtype, int64_t* attn_batch_stride, const void* R_out, const void* Rsq_out) {
    const int64_t full_stride = static_cast<int64_t>(H) * N * N;
    if (*attn_batch_stride < 0) *attn_batch_stride = full_stride;
    MMX_CHECK_ARG(*attn_batch_stride == 0 || *attn_batch_stride == full_stride,
                  "%s: attn_batch_stride must be 0 (shared forward) or H*N*N", half ? name : "mmx_relevancy_self_chain_ex");
    MMX_CHECK_ARG(attn_layers && grad_layers && R_out, "%s: null pointer", name);
    MMX_CHECK_ARG(n_layers >= 0 && n_layers <= MMX_MAX_LAYERS, "%s: n_layers %d not in [0, %d]", name, n_layers, MMX_MAX_LAYERS);
    MMX_CHECK_ARG(B > 0 && H > 0 && N > 0 && M >= 0, "%s: non-positive size", name);
    MMX_CHECK_ARG((M > 0) == (Rsq_out != nullptr), "%s: R_sq output and M must agree", name);
    if (half) MMX_CHECK_ARG(dtype == MMX_F32 || dtype == MMX_F16, "%s: slabs must be fp32 or fp16, got %d", name, dtype);
    else MMX_CHECK_ARG(dtype == MMX_F32 || dtype == MMX_F16 || dtype == MMX_BF16, "%s: dtype %d", name, dtype);
    for (int l = 0; l < n_layers; ++l) MMX_CHECK_ARG(attn_layers[l] && grad_layers[l], "%s: null layer pointer %d", name, l);
    return MMX_OK;
}

// ----------------------------------------------------------------------------------------- long sequences
// split path: per layer  A_bar = avg_heads(A_l, G_l);  R' = R + A_bar . R  [; R_sq' = R_sq + A_bar . R_sq];  rows_path: one launch per
// layer (relevancy_chain_rows.hip).  ws: what chain_workspace_bytes asked for.
static int chain_split(const ChainCall& c, bool rows_path, int dtype, const void* Rsq_init_dev, void* Rsq_out_dev, int M, void* ws_dev,
                       void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n_layers = c.n_layers, B = c.B, N = c.N;
    const int64_t nn = static_cast<int64_t>(N) * N, nm = static_cast<int64_t>(N) * M;
    const size_t mat = align256(sizeof(float) * static_cast<size_t>(B) * N * N);
    char* ws = static_cast<char*>(ws_dev);
    float* abar = reinterpret_cast<float*>(ws);
    float* Rpong = reinterpret_cast<float*>(ws + mat);
    float* SQpong = reinterpret_cast<float*>(ws + 2 * mat);
    float* Rout = c.R_out;
    float* SQout = static_cast<float*>(Rsq_out_dev);

    // state starts in the buffer that makes the LAST product land in the caller's output
    float* Rcur = (n_layers % 2 == 0) ? Rout : Rpong;
    float* SQcur = (n_layers % 2 == 0) ? SQout : SQpong;
    hipError_t e;
    if (c.R_init) {
        e = hipMemcpyAsync(Rcur, c.R_init, sizeof(float) * B * nn, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(R_init)");
    } else if (!rows_path || n_layers == 0) {
        int rc = identity_async(Rcur, B, N, s);
        if (rc) return rc;
    }
    if (rows_path) {
        // one launch per layer: the head reduction lands in LDS and is multiplied from there (relevancy_chain_rows.hip); the first
        // layer of a chain that starts at the identity is R = I + A_bar (no product, the identity is never materialised)
        for (int l = 0; l < n_layers; ++l) {
            float* Rnxt = (Rcur == Rout) ? Rpong : Rout;
            const float* Rin = (l == 0 && !c.R_init) ? nullptr : Rcur;
            int rc = chain_rows_layer_launch(c, l, Rin, Rnxt, dtype, s);
            if (rc) return rc;
            Rcur = Rnxt;
        }
        return MMX_OK;
    }
    if (M > 0) {
        if (Rsq_init_dev) {
            e = hipMemcpyAsync(SQcur, Rsq_init_dev, sizeof(float) * B * nm, hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(R_sq_init)");
        } else {
            int rc = zero_async(SQcur, sizeof(float) * B * nm, s);
            if (rc) return rc;
        }
    }
    // (Round 5 measured the head reductions on a side stream one layer ahead of the products -- A_bar_{l+1} does not depend on R_l,
    // one kernel is an HBM stream, the other an MFMA loop -- and found NO gain at 197 / 577 / 950 tokens, with or without capping
    // the product's workgroups per CU: profiles/r05_chain_split_roofline.txt.  One stream, two launches per layer.)
    for (int l = 0; l < n_layers; ++l) {
        int rc = avg_heads_launch(c.attn[l], c.grad[l], abar, B, c.H, N, N, dtype, c.attn_bstride, stream);
        if (rc) return rc;
        float* Rnxt = (Rcur == Rout) ? Rpong : Rout;
        rc = mmx_bmm_f32(abar, Rcur, Rcur, Rnxt, B, N, N, N, 0, nn, nn, nn, 0, stream);
        if (rc) return rc;
        Rcur = Rnxt;
        if (M > 0) {
            float* SQnxt = (SQcur == SQout) ? SQpong : SQout;
            rc = mmx_bmm_f32(abar, SQcur, SQcur, SQnxt, B, N, M, N, 0, nn, nm, nm, 0, stream);
            if (rc) return rc;
            SQcur = SQnxt;
        }
    }
    return MMX_OK;
}

}  // namespace mmx

// =====================================================================================================
// C-ABI entry points (see include/mmx_relevancy.h)
// =====================================================================================================
using namespace mmx;

// R' = round_f16(R + round_f16(P)): the two roundings of `R = R + torch.bmm(cam, R)` on fp16 tensors
__global__ __launch_bounds__(256) void half_chain_add_kernel(const float* __restrict__ R, const float* __restrict__ P,
                                                             float* __restrict__ out, int64_t n) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) out[i] = round_f16(R[i] + round_f16(P[i]));
}

extern "C" size_t mmx_self_chain_workspace_bytes(int n_layers, int B, int H, int N, int M, int dtype) {
    return chain_workspace_bytes(chain_route(n_layers, B, H, N, M, dtype), B, N, M);
}

extern "C" int mmx_relevancy_self_chain(const void* const* attn_layers, const void* const* grad_layers, int n_layers,
                                        int B, int H, int N, int dtype, const void* R_init_dev, void* R_out_dev,
                                        const void* Rsq_init_dev, void* Rsq_out_dev, int M, void* workspace_dev,
                                        size_t workspace_bytes, void* stream) {
    return mmx_relevancy_self_chain_ex(attn_layers, grad_layers, n_layers, B, H, N, dtype, -1, R_init_dev, R_out_dev,
                                       Rsq_init_dev, Rsq_out_dev, M, workspace_dev, workspace_bytes, stream);
}

extern "C" int mmx_relevancy_self_chain_ex(const void* const* attn_layers, const void* const* grad_layers, int n_layers,
                                           int B, int H, int N, int dtype, int64_t attn_batch_stride,
                                           const void* R_init_dev, void* R_out_dev, const void* Rsq_init_dev,
                                           void* Rsq_out_dev, int M, void* workspace_dev, size_t workspace_bytes,
                                           void* stream) {
    return mmx_relevancy_self_chain_flags(attn_layers, grad_layers, n_layers, B, H, N, dtype, attn_batch_stride, R_init_dev, R_out_dev,
                                          Rsq_init_dev, Rsq_out_dev, M, 0u, workspace_dev, workspace_bytes, stream);
}

extern "C" int mmx_relevancy_self_chain_flags(const void* const* attn_layers, const void* const* grad_layers, int n_layers,
                                              int B, int H, int N, int dtype, int64_t attn_batch_stride,
                                              const void* R_init_dev, void* R_out_dev, const void* Rsq_init_dev,
                                              void* Rsq_out_dev, int M, unsigned flags, void* workspace_dev, size_t workspace_bytes,
                                              void* stream) {
    MMX_CHECK_ARG((flags & ~MMX_CHAIN_CAUSAL) == 0u, "mmx_relevancy_self_chain_flags: unknown flag bits %#x", flags);
    if (int rc = check_chain_args("mmx_relevancy_self_chain", false, attn_layers, grad_layers, n_layers, B, H, N, M, dtype,
                                  &attn_batch_stride, R_out_dev, Rsq_out_dev))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const ChainCall c{attn_layers, grad_layers, n_layers, B, H, N, attn_batch_stride, static_cast<const float*>(R_init_dev),
                      static_cast<float*>(R_out_dev), g_chain_nt, (flags & MMX_CHAIN_CAUSAL) ? 1 : 0, g_debug_flags};
    const ChainRoute route = chain_route(n_layers, B, H, N, M, dtype);
    const size_t need = chain_workspace_bytes(route, B, N, M);
    if (need && (workspace_bytes < need || !workspace_dev)) {
        set_error("mmx_relevancy_self_chain: workspace %zu < %zu", workspace_bytes, need);
        return MMX_EWORKSPACE;
    }
    ChainGroups grp{route.G, nullptr, nullptr};
    if (route.G > 1) {
        grp.counters = static_cast<unsigned*>(workspace_dev);
        grp.parts = reinterpret_cast<float*>(static_cast<char*>(workspace_dev) + group_counter_bytes(B));
    }
    switch (route.kernel) {
        case kChainCols: return self_chain_cols_launch(c, s);
        case kChainGroups: return self_chain_groups_launch(c, grp, s);
        case kChainFused:   // (below ~40 tokens the pipeline's bookkeeping costs more than it hides)
            return self_chain_fused_launch(c, dtype, grp, N * N >= 1600 ? g_chain_pipe : 0, false, s);
        default: return chain_split(c, route.kernel == kChainRows, dtype, Rsq_init_dev, Rsq_out_dev, M, workspace_dev, stream);
    }
}

// The reference's HALF-PRECISION chain (CLIP_explainability.ipynb cell 6:20-32, 43-55 on a model after `convert_weights`,
// CLIP/clip/model.py:381-402: R is created in the dtype of the fp16 attention probabilities): same rule, every tensor-level result
// rounded to fp16.  R_out: fp32 storage of fp16-representable values.  N <= 128: the fused kernel, one workgroup per sample;
// larger N: avg_heads + bmm + a rounding add per layer (workspace: mmx_self_chain_workspace_bytes(..., M = 0)).
extern "C" int mmx_relevancy_self_chain_half(const void* const* attn_layers, const void* const* grad_layers, int n_layers,
                                             int B, int H, int N, int dtype, int64_t attn_batch_stride, void* R_out_dev,
                                             void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (int rc = check_chain_args("mmx_relevancy_self_chain_half", true, attn_layers, grad_layers, n_layers, B, H, N, 0, dtype,
                                  &attn_batch_stride, R_out_dev, nullptr))
        return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* R = static_cast<float*>(R_out_dev);
    if ((N + 15) / 16 <= 8) {
        const ChainCall c{attn_layers, grad_layers, n_layers, B, H, N, attn_batch_stride, nullptr, R, 0, 0, 0};
        return self_chain_fused_launch(c, dtype, ChainGroups{1, nullptr, nullptr}, 0, true, s);
    }
    const size_t need = mmx_self_chain_workspace_bytes(n_layers, B, H, N, 0, dtype);
    if (workspace_bytes < need || !workspace_dev) {
        set_error("mmx_relevancy_self_chain_half: workspace %zu < %zu", workspace_bytes, need);
        return MMX_EWORKSPACE;
    }
    const int64_t nn = static_cast<int64_t>(N) * N;
    const size_t mat = align256(sizeof(float) * static_cast<size_t>(B) * N * N);
    char* ws = static_cast<char*>(workspace_dev);
    float* abar = reinterpret_cast<float*>(ws);
    float* prod = reinterpret_cast<float*>(ws + mat);
    int rc = identity_async(R, B, N, s);
    if (rc) return rc;
    for (int l = 0; l < n_layers; ++l) {
        rc = avg_heads_launch(attn_layers[l], grad_layers[l], abar, B, H, N, N, dtype, attn_batch_stride, stream, true);
        if (rc) return rc;
        rc = mmx_bmm_f32(abar, R, nullptr, prod, B, N, N, N, 0, nn, nn, nn, 0, stream);
        if (rc) return rc;
        const int64_t n = static_cast<int64_t>(B) * nn;
        half_chain_add_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, s>>>(R, prod, R, n);
        MMX_LAUNCH_CHECK("half_chain_add_kernel");
    }
    return MMX_OK;
}
