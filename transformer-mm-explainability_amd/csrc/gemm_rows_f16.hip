// K_gemm_rows_f16: C[r] = half(A[r]) . W for the rows r of a device-side list on v_mfma_f32_32x32x16_f16, fp32 accumulators and fp32
// output -- the GEMMs of a causally masked tower in the reference's own half-precision mode (convert_weights, CLIP/clip/model.py:381-402;
// the mask of model.py:334-340 and the EOT read of model.py:360 make every row past a caption's EOT token dead, 89 % of the rows at
// caption lengths).  Same contract as gemm_rows_f32.hip, on the same skeleton (gemm_rows_core.h): the grid is sized for the capacity, the count is read on the device, a
// workgroup past it returns before any barrier, a row id goes through the list once, ids outside [0, cap) name no row, unlisted rows
// are neither read nor written, EPI 0 / 1 / 2 = plain | + bias | + bias and QuickGELU of it to a second tensor, one launch for every
// input (a hipGraph replays it).  No scratch, no atomics, no workspace.
//
// Operands.  A is fp32 in memory (the tape's activations and gradients: no conversion pass in front of the kernel), fetched with
// 16-byte loads from clamped addresses and rounded to fp16 in registers on its way to LDS: static_cast<_Float16>, round to nearest
// even (v_cvt_f16_f32 / v_cvt_pk_f16_f32; NOT the pkrtz builtin, which rounds toward zero) -- the bits of x.to(torch.float16).  The
// weight is fp16 and k-fastest, W_h [N][K] row-major: for a forward nn.Linear the cached fp16 copy of the parameter as stored
// ([out, in]), for the backward's x @ weight a cached fp16 copy of weight.t().contiguous().  16-byte loads of 8 halves.
//
// MFMA.  v_mfma_f32_32x32x16_f16: with r = lane & 31, h = lane >> 5 a lane holds A[row r][k = 8 h + j] and B[k = 8 h + j][col r],
// j = 0..7.  Both LDS images are k-fastest ([tile row][BK + 8] and [tile column][BK + 8] halves), so each fragment is ONE ds_read_b128
// and no transposed read is needed.  C / D: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) -- the fp32 kernel's map, and
// its epilogue.
//
// Choices (the matrix-core work of a slab is 8x shorter than in the fp32 kernel: the loop is load- and LDS-bound):
//   * 32-row tiles (few live rows must spread over the chip); 32 x 64 columns: the four waves are 2 column halves x 2 k shares,
//     32 x 32: four k shares of one MFMA tile.  The shares meet in LDS at the end, added in a fixed order.
//   * BK = 64 halves at 64 columns, 128 at 32: a slab is then 8 KiB of A (fp32) + 8 KiB (4 KiB at 32 columns) of W_h in flight per
//     stage -- four 16-byte loads per thread (six at 32 columns) -- and two MFMAs per wave, one on either side of the barrier.
//     K = 512 is 8 / 4 slabs.
//   * PF = 3 slabs of 64 (2 slabs of 128) requested ahead into registers, the same 192 / 256 k in flight per thread row either way; two
//     LDS stages, one barrier per slab, the last slab peeled; the steady state is one basic block whose waits in front of the
//     ds_write_b128 are counted vmcnt (ISA: s_waitcnt vmcnt(8) in each of the three steps at 64 columns, vmcnt(6) in each of the two at
//     32; a scheduling barrier at the head of a step keeps the compiler from hoisting the selects of the later slabs' registers,
//     which turned every wait into vmcnt(0)).
//   * ISA (gfx950, -O3): 64 columns 119 VGPRs, 35,968 B LDS; 32 columns 126 VGPRs, 47,232 B LDS; no scratch, no spills, v_cvt_pk_f16_f32 for every
//     conversion, ds_read_b128 / ds_write_b128 only on the two stages.
//   * row pitch BK + 8 halves (144 / 272 bytes = 9 / 17 sixteen-byte slots, odd): the 16 lanes that ds_read_b128 serves together
//     hold 16 rows that are distinct mod 16, so their slots cover the 64 banks once (MI355X LDS: bank = (a / 4) mod 64 for b128
//     reads) -- conflict-free without a swizzle.  The ds_write_b128 of 8 consecutive lanes are 128 contiguous bytes of one tile row.
//   * a thread converts the 8 floats of two adjacent 16-byte loads and stores them as one 16-byte LDS chunk.
#include "gemm_rows_core.h"

namespace mmx {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// option "text_live_rows_half": 0 (default) an fp16 body keeps its dense text tower | 1: it takes the row-list route on this kernel
static int g_text_live_rows_half = 0;
bool gemm_rows_half_option(const char* key, int value) {
    if (strcmp(key, "text_live_rows_half") == 0 && value >= 0 && value <= 1) { g_text_live_rows_half = value; return true; }
    return false;
}

template <int TM, int TN, int BK, int PF, int EPI>
__global__ __launch_bounds__(256, 2) void gemm_rows_f16_kernel(const float* __restrict__ A, const _Float16* __restrict__ Wh,
                                                               float* __restrict__ C, const int* __restrict__ rows,
                                                               const int* __restrict__ count, int cap, int N, int K,
                                                               const float* __restrict__ bias, float* __restrict__ C2) {
    constexpr int WC = TN / 32;                      // wave columns (one 32 x 32 MFMA tile per wave)
    constexpr int WK = 4 / WC;                       // waves sharing an output tile, each on its own 16-wide k groups of a slab
    constexpr int NG = BK / 16 / WK;                 // MFMAs of a slab per wave, half of them on either side of the barrier
    constexpr int LK = BK + 8;                       // row pitch of both stages in halves, k fastest
    constexpr int CPR = BK / 8;                      // 16-byte LDS chunks (8 halves) of a tile row
    constexpr int RS = 256 / CPR;                    // tile rows between two chunks of a thread
    constexpr int CA = TM / RS, CB = TN / RS;        // chunks of a slab per thread
    static_assert(TM == 32 && WC * WK == 4 && NG >= 2 && NG % 2 == 0 && CA >= 1 && CB >= 1 && PF >= 2, "tile shape");
    __shared__ __attribute__((aligned(16))) _Float16 As[2][TM * LK];
    __shared__ __attribute__((aligned(16))) _Float16 Bs[2][TN * LK];
    __shared__ __attribute__((aligned(16))) float red[(WK - 1) * WC * 16 * 64];
    __shared__ int rid[TM];                          // dense row of every tile row, -1: none

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wc = wave % WC, wk = wave / WC;
    const RowsTilePos p = rows_tile_pos<TM, TN>(rows, count, cap, N);
    if (p.empty()) return;
    p.publish<TM>(rid);
    const int m0 = p.m0, n0 = p.n0;

    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;

    // per-thread chunk addresses, fixed for the whole K loop: 8 consecutive k of tile rows cr + i RS of A (two 16-byte loads of fp32)
    // and of tile columns cr + i RS of W_h (one 16-byte load of fp16)
    const int cr = tid / CPR, kc = (tid % CPR) * 8;
    bool oka[CA], okb[CB];
    const float* pa[CA];
    const _Float16* pb[CB];
#pragma unroll
    for (int i = 0; i < CA; ++i) {
        const int arow = p.dense_row(m0 + cr + i * RS);
        oka[i] = arow >= 0;
        pa[i] = A + static_cast<int64_t>(oka[i] ? arow : 0) * K;
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) {
        const int n = n0 + cr + i * RS;
        okb[i] = n < N;
        pb[i] = Wh + static_cast<int64_t>(okb[i] ? n : 0) * K;
    }
    struct Slab { f32x4 a[CA][2]; f32x4 b[CB]; };    // (b: 8 halves, carried as 16 raw bytes)
    Slab ring[PF];                                   // slab t waits in register set t % PF
    auto fetch = [&](int t, Slab& x) {               // any t: an address past K is clamped to the last chunk (K % 8 == 0)
        const int kk = min(t * BK + kc, K - 8);
#pragma unroll
        for (int i = 0; i < CA; ++i) {
            x.a[i][0] = ldg4_u(pa[i] + kk);
            x.a[i][1] = ldg4_u(pa[i] + kk + 4);
        }
#pragma unroll
        for (int i = 0; i < CB; ++i) x.b[i] = ldg4_u(reinterpret_cast<const float*>(pb[i] + kk));
    };
    auto stash = [&](int stage, int t, const Slab& x) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        const bool inside = t * BK + kc < K;
#pragma unroll
        for (int i = 0; i < CA; ++i) {
            const bool ok = oka[i] && inside;
            const f32x4 lo = ok ? x.a[i][0] : z, hi = ok ? x.a[i][1] : z;
            f16x8 h;                                 // round to nearest even, the bits of .to(torch.float16)
#pragma unroll
            for (int j = 0; j < 4; ++j) { h[j] = static_cast<_Float16>(lo[j]); h[4 + j] = static_cast<_Float16>(hi[j]); }
            *reinterpret_cast<f16x8*>(&As[stage][(cr + i * RS) * LK + kc]) = h;
        }
#pragma unroll
        for (int i = 0; i < CB; ++i)
            *reinterpret_cast<f32x4*>(&Bs[stage][(cr + i * RS) * LK + kc]) = (okb[i] && inside) ? x.b[i] : z;
    };

    // MFMA operands of one slab: the wave's g-th k group (group jj = wk + g WK of the slab) takes k = 16 jj + 8 (lane >> 5) + j
    const int li = lane & 31, lg = lane >> 5;
    struct Frag { f16x8 a[NG], b[NG]; };
    auto read_frag = [&](Frag& f, int stage) {
        const _Float16* Asl = &As[stage][li * LK + 8 * lg];
        const _Float16* Bsl = &Bs[stage][(wc * 32 + li) * LK + 8 * lg];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const int jj = wk + g * WK;
            f.a[g] = *reinterpret_cast<const f16x8*>(Asl + 16 * jj);
            f.b[g] = *reinterpret_cast<const f16x8*>(Bsl + 16 * jj);
        }
    };
    auto mfma_half = [&](const Frag& f, int h) {
#pragma unroll
        for (int g = h * (NG / 2); g < (h + 1) * (NG / 2); ++g)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a[g], f.b[g], acc, 0, 0, 0);
    };

    rows_k_pipeline<PF, true, Frag>(ring, (K + BK - 1) / BK, fetch, stash, read_frag, mfma_half);   // (true: the fence of "Choices")
    rows_finish<EPI, WK, WC>(acc, red, p, rid, 0, wc, wk, wc, lane, N, C, bias, C2);
}

// The tile of a launch, from option "gemm_rows_tn" and the shape only (the live count stays on the device): 32 rows x 64 columns,
// 32 x 32 for N <= 512 (twice the workgroups where the column tiles are few).
static int half_tile_tn(int N) {
    const int tn = gemm_rows_tn_option();
    return tn ? tn : (N <= 512 ? 32 : 64);
}

}  // namespace mmx

#ifndef MMX_GEMM_ROWS_EMU   // (the host emulation takes the kernel, not the launches)
namespace mmx {
template <int EPI>
static int launch_gemm_rows_half(const char* what, hipStream_t s, const void* a_dev, const void* wh_dev, void* c_dev, const void* rows_dev,
                                 const void* count_dev, int cap_rows, int N, int K, const void* bias_dev, void* act_dev) {
    const int tn = half_tile_tn(N);
    const unsigned g = rows_grid(what, 32, tn, cap_rows, N);
    if (!g) return MMX_EINVAL;
    const float* A = static_cast<const float*>(a_dev);
    const _Float16* Wh = static_cast<const _Float16*>(wh_dev);
    float *C = static_cast<float*>(c_dev), *C2 = static_cast<float*>(act_dev);
    const int *rows = static_cast<const int*>(rows_dev), *count = static_cast<const int*>(count_dev);
    const float* bias = static_cast<const float*>(bias_dev);
    if (tn == 32)
        gemm_rows_f16_kernel<32, 32, 128, 2, EPI><<<g, 256, 0, s>>>(A, Wh, C, rows, count, cap_rows, N, K, bias, C2);
    else
        gemm_rows_f16_kernel<32, 64, 64, 3, EPI><<<g, 256, 0, s>>>(A, Wh, C, rows, count, cap_rows, N, K, bias, C2);
    MMX_LAUNCH_CHECK(what);
    return MMX_OK;
}

}  // namespace mmx

using namespace mmx;

extern "C" int mmx_gemm_rows_f16(const void* a_dev, const void* wh_dev, void* c_dev, const void* rows_dev, const void* count_dev,
                                 int cap_rows, int N, int K, void* stream) {
    MMX_CHECK_ARG(a_dev && wh_dev && c_dev && rows_dev && count_dev, "mmx_gemm_rows_f16: null pointer");
    MMX_CHECK_ARG(cap_rows > 0 && N > 0 && K > 0, "mmx_gemm_rows_f16: cap_rows=%d N=%d K=%d", cap_rows, N, K);
    if (!rows_operands_ok("mmx_gemm_rows_f16", a_dev, wh_dev, c_dev, N, K, 8)) return MMX_ENOTSUP;
    return launch_gemm_rows_half<0>("mmx_gemm_rows_f16", static_cast<hipStream_t>(stream), a_dev, wh_dev, c_dev, rows_dev, count_dev,
                                    cap_rows, N, K, nullptr, nullptr);
}

extern "C" int mmx_gemm_rows_bias_f16(const void* a_dev, const void* wh_dev, const void* bias_dev, void* c_dev, void* act_dev,
                                      const void* rows_dev, const void* count_dev, int cap_rows, int N, int K, void* stream) {
    MMX_CHECK_ARG(a_dev && wh_dev && bias_dev && c_dev && rows_dev && count_dev, "mmx_gemm_rows_bias_f16: null pointer");
    MMX_CHECK_ARG(cap_rows > 0 && N > 0 && K > 0, "mmx_gemm_rows_bias_f16: cap_rows=%d N=%d K=%d", cap_rows, N, K);
    MMX_CHECK_ARG(act_dev != c_dev, "mmx_gemm_rows_bias_f16: the activation needs a buffer of its own");
    if (!rows_operands_ok("mmx_gemm_rows_bias_f16", a_dev, wh_dev, c_dev, N, K, 8)) return MMX_ENOTSUP;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (act_dev)
        return launch_gemm_rows_half<2>("mmx_gemm_rows_bias_f16", s, a_dev, wh_dev, c_dev, rows_dev, count_dev, cap_rows, N, K, bias_dev,
                                        act_dev);
    return launch_gemm_rows_half<1>("mmx_gemm_rows_bias_f16", s, a_dev, wh_dev, c_dev, rows_dev, count_dev, cap_rows, N, K, bias_dev,
                                    nullptr);
}

extern "C" int mmx_text_live_rows_half_enabled(void) { return g_text_live_rows_half && mmx_text_live_rows_fwd_enabled(); }
#endif
