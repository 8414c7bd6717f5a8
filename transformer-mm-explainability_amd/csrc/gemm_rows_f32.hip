// K_gemm_rows_f32: C[r] = A[r] . W for the rows r of a device-side list, exact fp32 on v_mfma_f32_32x32x2_f32 -- the input-gradient
// GEMMs of a causally masked tower's backward (CLIP's text tower, CLIP/clip/model.py:334-340, 360: the feature is read at the EOT
// token, so every gradient row past it is an exact zero; 89 % of the rows at caption lengths), plus the kernel that builds the list.
//
// The product uses the tiles of bmm_f32_tiles.hip (k-fastest A tile read with one ds_read_b128 per four MFMA steps, n-fastest B tile, 16-byte
// global loads, two LDS stages with one barrier per K slab and PF slabs requested ahead into registers); its K loop, the row list and
// the epilogue are those of gemm_rows_core.h, shared with gemm_rows_f16.hip.  What differs from bmm_f32_tiles.hip besides them:
//   * few rows must still spread over the chip: TM = 32 rows x 64 columns per workgroup, the four waves as 2 column halves x 2 shares of
//     every K slab (their accumulators meet in LDS at the end, added in a fixed order); 32 x 32: four shares of one MFMA tile, twice the
//     workgroups; TM = 64 is the 2 x 2 layout of bmm_f32_tiles.hip.
// W is the nn.Linear parameter as stored ([out, in] = [K, N] row-major here), used as x @ weight like ops.backward_gemm.
#include "gemm_rows_core.h"

namespace mmx {

static int g_text_live_rows = 1;   // option "text_live_rows": 1 (default) the row-list backward route is offered | 0: mmx_live_rows declines
static int g_gemm_rows_tm = 32;    // option "gemm_rows_tm": rows per workgroup tile, 32 (default) or 64 (A / B runs)
static int g_gemm_rows_tn = 0;     // option "gemm_rows_tn": columns per workgroup tile at 32 rows, 0 (default: from the shape) | 32 | 64 (A / B runs)
static int g_text_live_rows_fwd = 1;   // option "text_live_rows_fwd": 1 (default) the forward of that tower takes the route too | 0: dense forward
static int g_gemm_rows_pf = 0;     // option "gemm_rows_pf": slabs of K requested ahead (the register ring), 0 (default: rows_depth) | 3 | 4 (A / B runs)
bool text_live_rows_option(const char* key, int value) {
    if (strcmp(key, "text_live_rows") == 0 && value >= 0 && value <= 1) { g_text_live_rows = value; return true; }
    if (strcmp(key, "text_live_rows_fwd") == 0 && value >= 0 && value <= 1) { g_text_live_rows_fwd = value; return true; }
    if (strcmp(key, "gemm_rows_tm") == 0 && (value == 32 || value == 64)) { g_gemm_rows_tm = value; return true; }
    if (strcmp(key, "gemm_rows_tn") == 0 && (value == 0 || value == 32 || value == 64)) { g_gemm_rows_tn = value; return true; }
    if (strcmp(key, "gemm_rows_pf") == 0 && (value == 0 || value == 3 || value == 4)) { g_gemm_rows_pf = value; return true; }
    return false;
}
int gemm_rows_tn_option() { return g_gemm_rows_tn; }

// rows[0 .. count) = b * N + p for p <= clamp(eot[b], 0, N - 1), samples in order, positions in order; one workgroup.
__global__ __launch_bounds__(256) void live_rows_kernel(const long long* __restrict__ eot, int B, int N, int* __restrict__ rows,
                                                        int* __restrict__ count) {
    __shared__ int len[256], off[256];
    __shared__ int base;
    if (threadIdx.x == 0) base = 0;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + threadIdx.x;
        if (b < B) {
            const long long e = eot[b];
            len[threadIdx.x] = static_cast<int>(e < 0 ? 0 : (e > N - 1 ? N - 1 : e)) + 1;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int run = base;
            const int n = min(256, B - b0);
            for (int i = 0; i < n; ++i) { off[i] = run; run += len[i]; }
            base = run;
        }
        __syncthreads();
        const int n = min(256, B - b0);
        for (int i = 0; i < n; ++i)
            for (int p = threadIdx.x; p < len[i]; p += 256) rows[off[i] + p] = (b0 + i) * N + p;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

// The fp32 operands on the skeleton of gemm_rows_core.h.  EPI 1 / 2 (+ bias): W is the cached [in, out] copy of the nn.Linear weight.
template <int TM, int TN, int BK, int PF, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_rows_f32_kernel(const float* __restrict__ A, const float* __restrict__ W,
                                                               float* __restrict__ C, const int* __restrict__ rows,
                                                               const int* __restrict__ count, int cap, int N, int K,
                                                               const float* __restrict__ bias, float* __restrict__ C2) {
    constexpr int WR = TM / 32, WC = TN / 32;        // wave rows x wave columns (one 32 x 32 MFMA tile per wave)
    constexpr int WK = 4 / (WR * WC);                // waves sharing an output tile, each on its own 8-wide k groups of a slab
    constexpr int NG = BK / 8 / WK;                  // k groups of a slab per wave: 4 MFMAs each, half of them on either side of the barrier
    constexpr int LA = BK + 4;                       // A stage: [TM][BK + 4] floats, k fastest
    constexpr int LB = TN + 4;                       // B stage: [BK][TN + 4] floats, n fastest
    constexpr int CA = TM * BK / 1024, CB = BK * TN / 1024;   // 16-byte chunks of a slab per thread
    constexpr int RA = 1024 / BK, RB = 1024 / TN;    // tile rows / k rows between two chunks of a thread
    static_assert(WR * WC * WK == 4 && NG >= 2 && NG % 2 == 0 && CA >= 1 && CB >= 1 && PF >= 2, "tile shape");
    __shared__ __attribute__((aligned(16))) float As[2][TM * LA];
    __shared__ __attribute__((aligned(16))) float Bs[2][BK * LB];
    __shared__ __attribute__((aligned(16))) float red[WK > 1 ? (WK - 1) * WR * WC * 16 * 64 : 4];
    __shared__ int rid[TM];                          // dense row of every tile row, -1: none

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wc = wave % WC, wr = (wave / WC) % WR, wk = wave / (WC * WR);
    const RowsTilePos p = rows_tile_pos<TM, TN>(rows, count, cap, N);
    if (p.empty()) return;
    p.publish<TM>(rid);
    const int m0 = p.m0, n0 = p.n0;

    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;

    // per-thread chunk addresses, fixed for the whole K loop: CA 16-byte chunks of the A slab (tile rows ar + i RA), CB of the B slab
    // (k rows kb + i RB of one column chunk)
    const int ar = tid / (BK / 4), ka = (tid % (BK / 4)) * 4;
    bool oka[CA];
    const float* pa[CA];
#pragma unroll
    for (int i = 0; i < CA; ++i) {
        const int arow = p.dense_row(m0 + ar + i * RA);
        oka[i] = arow >= 0;
        pa[i] = A + static_cast<int64_t>(oka[i] ? arow : 0) * K;
    }
    const int kb = tid / (TN / 4), nbl = (tid % (TN / 4)) * 4;
    const bool okb = n0 + nbl < N;                   // N % 4 == 0: a chunk is inside or outside as a whole
    const float* pb = W + (okb ? n0 + nbl : 0);
    struct Slab { f32x4 a[CA], b[CB]; };
    Slab ring[PF];                                   // slab t waits in register set t % PF
    auto fetch = [&](int t, Slab& x) {               // any t: an address past K is clamped to the last chunk (K % 4 == 0) / last row
        const int k0 = t * BK;
#pragma unroll
        for (int i = 0; i < CA; ++i) x.a[i] = ldg4_u(pa[i] + min(k0 + ka, K - 4));
#pragma unroll
        for (int i = 0; i < CB; ++i) x.b[i] = ldg4_u(pb + static_cast<int64_t>(min(k0 + kb + i * RB, K - 1)) * N);
    };
    auto stash = [&](int stage, int t, const Slab& x) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const int k0 = t * BK;
#pragma unroll
        for (int i = 0; i < CA; ++i)
            *reinterpret_cast<f32x4*>(&As[stage][(ar + i * RA) * LA + ka]) = (oka[i] && k0 + ka < K) ? x.a[i] : z;
#pragma unroll
        for (int i = 0; i < CB; ++i)
            *reinterpret_cast<f32x4*>(&Bs[stage][(kb + i * RB) * LB + nbl]) = (okb && k0 + kb + i * RB < K) ? x.b[i] : z;
    };

    // MFMA operands of one slab: step t of the wave's g-th k group (group jj = wk + g WK of the slab) takes k = 8 jj + 4 (lane >> 5) + t
    const int li = lane & 31, lg = lane >> 5;
    struct Frag { f32x4 a[NG]; float b[NG][4]; };
    auto read_frag = [&](Frag& f, int stage) {
        const float* Asl = &As[stage][(wr * 32 + li) * LA + 4 * lg];
        const float* Bsl = &Bs[stage][(4 * lg) * LB + wc * 32 + li];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int jj = wk + g * WK;
            f.a[g] = *reinterpret_cast<const f32x4*>(Asl + 8 * jj);
#pragma unroll
            for (int t = 0; t < 4; ++t) f.b[g][t] = Bsl[(8 * jj + t) * LB];
        }
    };
    auto mfma_half = [&](const Frag& f, int h) {
#pragma unroll
        for (int g = h * (NG / 2); g < (h + 1) * (NG / 2); ++g)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[g][t], f.b[g][t], acc, 0, 0, 0);
    };

    rows_k_pipeline<PF, false, Frag>(ring, (K + BK - 1) / BK, fetch, stash, read_frag, mfma_half);
    rows_finish<EPI, WK, WR * WC>(acc, red, p, rid, wr, wc, wk, wr * WC + wc, lane, N, C, bias, C2);
}

// The tile of a launch: rows x columns per workgroup, chosen from the options and the shape only (the live count stays on the device).
// pf: the depth of the register ring, option "gemm_rows_pf" or rows_depth() of the tile.  What profiles/gemm_rows_depth_probe.txt measured
// at the step's shapes (531 live rows): four slabs ahead beat three on every tile at every shape, six and eight were no better than four;
// at four, 32 columns beat 64 at N = 512 for K = 512, 1536 and 2048 (twice the workgroups where 64 columns leave half the chip idle) and
// lost or tied at N = 1536 and 2048 -- the rule of gemm_rows_f16.hip.
struct RowsTile { int tm, tn, pf; };
static int rows_depth(int tm, int tn) { return 4; }
static RowsTile rows_tile(int N, int K) {
    const int tm = g_gemm_rows_tm == 64 ? 64 : 32;
    const int tn = tm == 64 ? 64 : (g_gemm_rows_tn ? g_gemm_rows_tn : (N <= 512 ? 32 : 64));
    return {tm, tn, g_gemm_rows_pf ? g_gemm_rows_pf : rows_depth(tm, tn)};
}

}  // namespace mmx

#ifndef MMX_GEMM_ROWS_EMU   // (the host emulation takes the kernel, not the launches)
namespace mmx {
// One tile at the depth pf of its register ring (the depths option "gemm_rows_pf" accepts; rows_tile() hands out no other).
template <int TM, int TN, int BK, int EPI, class... Args>
static void launch_gemm_rows_depth(int pf, unsigned g, hipStream_t s, Args... args) {
    if (pf == 3)
        gemm_rows_f32_kernel<TM, TN, BK, 3, EPI><<<g, 256, 0, s>>>(args...);
    else
        gemm_rows_f32_kernel<TM, TN, BK, 4, EPI><<<g, 256, 0, s>>>(args...);
}
template <int EPI>
static void launch_gemm_rows(RowsTile t, unsigned g, hipStream_t s, const float* A, const float* W, float* C, const int* rows,
                             const int* count, int cap_rows, int N, int K, const float* bias, float* C2) {
    if (t.tm == 64)
        launch_gemm_rows_depth<64, 64, 32, EPI>(t.pf, g, s, A, W, C, rows, count, cap_rows, N, K, bias, C2);
    else if (t.tn == 32)
        launch_gemm_rows_depth<32, 32, 64, EPI>(t.pf, g, s, A, W, C, rows, count, cap_rows, N, K, bias, C2);
    else
        launch_gemm_rows_depth<32, 64, 32, EPI>(t.pf, g, s, A, W, C, rows, count, cap_rows, N, K, bias, C2);
}

}  // namespace mmx

using namespace mmx;

extern "C" int mmx_live_rows(const void* eot_dev, int B, int N, void* rows_dev, void* count_dev, void* stream) {
    MMX_CHECK_ARG(eot_dev && rows_dev && count_dev, "mmx_live_rows: null pointer");
    MMX_CHECK_ARG(B > 0 && N > 0 && static_cast<int64_t>(B) * N < (1ll << 31), "mmx_live_rows: B=%d N=%d (B * N must fit an int)", B, N);
    if (!g_text_live_rows) {
        set_error("mmx_live_rows: the row-list route is switched off (option text_live_rows = 0)");
        return MMX_ENOTSUP;
    }
    live_rows_kernel<<<1, 256, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const long long*>(eot_dev), B, N,
                                                                      static_cast<int*>(rows_dev), static_cast<int*>(count_dev));
    MMX_LAUNCH_CHECK("live_rows_kernel");
    return MMX_OK;
}

extern "C" int mmx_gemm_rows_f32(const void* a_dev, const void* w_dev, void* c_dev, const void* rows_dev, const void* count_dev,
                                 int cap_rows, int N, int K, void* stream) {
    MMX_CHECK_ARG(a_dev && w_dev && c_dev && rows_dev && count_dev, "mmx_gemm_rows_f32: null pointer");
    MMX_CHECK_ARG(cap_rows > 0 && N > 0 && K > 0, "mmx_gemm_rows_f32: cap_rows=%d N=%d K=%d", cap_rows, N, K);
    if (!rows_operands_ok("mmx_gemm_rows_f32", a_dev, w_dev, c_dev, N, K, 4)) return MMX_ENOTSUP;
    const RowsTile tm = rows_tile(N, K);
    const unsigned wgs = rows_grid("mmx_gemm_rows_f32", tm.tm, tm.tn, cap_rows, N);
    if (!wgs) return MMX_EINVAL;
    launch_gemm_rows<0>(tm, wgs, static_cast<hipStream_t>(stream), static_cast<const float*>(a_dev), static_cast<const float*>(w_dev),
                        static_cast<float*>(c_dev), static_cast<const int*>(rows_dev), static_cast<const int*>(count_dev), cap_rows, N, K,
                        nullptr, nullptr);
    MMX_LAUNCH_CHECK("gemm_rows_f32_kernel");
    return MMX_OK;
}

extern "C" int mmx_text_live_rows_fwd_enabled(void) { return g_text_live_rows && g_text_live_rows_fwd; }

extern "C" int mmx_gemm_rows_bias_f32(const void* a_dev, const void* wt_dev, const void* bias_dev, void* c_dev, void* act_dev,
                                      const void* rows_dev, const void* count_dev, int cap_rows, int N, int K, void* stream) {
    MMX_CHECK_ARG(a_dev && wt_dev && bias_dev && c_dev && rows_dev && count_dev, "mmx_gemm_rows_bias_f32: null pointer");
    MMX_CHECK_ARG(cap_rows > 0 && N > 0 && K > 0, "mmx_gemm_rows_bias_f32: cap_rows=%d N=%d K=%d", cap_rows, N, K);
    MMX_CHECK_ARG(act_dev != c_dev, "mmx_gemm_rows_bias_f32: the activation needs a buffer of its own");
    if (!rows_operands_ok("mmx_gemm_rows_bias_f32", a_dev, wt_dev, c_dev, N, K, 4)) return MMX_ENOTSUP;
    const RowsTile tm = rows_tile(N, K);
    const unsigned wgs = rows_grid("mmx_gemm_rows_bias_f32", tm.tm, tm.tn, cap_rows, N);
    if (!wgs) return MMX_EINVAL;
    const float *A = static_cast<const float*>(a_dev), *W = static_cast<const float*>(wt_dev), *bias = static_cast<const float*>(bias_dev);
    const int *rows = static_cast<const int*>(rows_dev), *count = static_cast<const int*>(count_dev);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (act_dev)
        launch_gemm_rows<2>(tm, wgs, s, A, W, static_cast<float*>(c_dev), rows, count, cap_rows, N, K, bias, static_cast<float*>(act_dev));
    else
        launch_gemm_rows<1>(tm, wgs, s, A, W, static_cast<float*>(c_dev), rows, count, cap_rows, N, K, bias, nullptr);
    MMX_LAUNCH_CHECK("gemm_rows_f32_kernel<bias>");
    return MMX_OK;
}
#endif
