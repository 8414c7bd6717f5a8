// The skeleton of the row-list GEMM kernels (gemm_rows_f32.hip: exact fp32, gemm_rows_f16.hip: fp16 operands), everything that does
// not depend on the operand format: the tile prologue over the device-side row list, the K pipeline, the meeting of the k shares, the
// epilogue, the host-side argument checks.  A kernel supplies its LDS arrays and its operand handling (Slab / Frag, fetch, stash,
// read_frag, mfma_half) as lambdas; everything here is forced inline into it.  The contract both kernels share:
//   * M is a DEVICE-side count: the grid is sized for the capacity (every row of the dense tensor), a workgroup whose row tile starts
//     at or beyond the count returns at once.  Nothing is read back, the launch is the same for every input (hipGraph replays it).
//   * a thread's A row address goes through the list once, before the K loop; output rows are scattered back to the same dense
//     layout, unlisted rows are neither read nor written.
//   * workgroups are NOT made XCD-contiguous: the live tiles are the first few of the capacity grid, and the plain round-robin spreads
//     exactly those over the eight XCDs.
// (The host emulation, tools/host/gemm_rows_emu.cpp, compiles this file and both kernels for the CPU: MMX_GEMM_ROWS_EMU.)
#pragma once
#ifndef MMX_GEMM_ROWS_EMU
#include "mmx_common.h"
#endif

namespace mmx {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// The row tile of a workgroup: rows [m0, m0 + TM) of the list's first M entries, columns [n0, n0 + TN) of the product.  A kernel
// begins `const RowsTilePos p = rows_tile_pos<TM, TN>(...); if (p.empty()) return; p.publish<TM>(rid);`.
struct RowsTilePos {
    const int* rows;
    int M, cap, m0, n0;
    // the tile starts at or beyond the count: the workgroup returns (workgroup-uniform: no barrier has been reached)
    __device__ __forceinline__ bool empty() const { return m0 >= M; }
    __device__ __forceinline__ int dense_row(int gm) const {
        const int r = gm < M ? rows[gm] : -1;
        return static_cast<unsigned>(r) < static_cast<unsigned>(cap) ? r : -1;   // an id outside the tensor is no row at all
    }
    // rid[i] = dense row of tile row i, -1: none (published by the barrier in front of the first slab)
    template <int TM>
    __device__ __forceinline__ void publish(int* rid) const {
        const int tid = threadIdx.x;
        if (tid < TM) rid[tid] = dense_row(m0 + tid);
    }
};
template <int TM, int TN>
__device__ __forceinline__ RowsTilePos rows_tile_pos(const int* __restrict__ rows, const int* __restrict__ count, int cap, int N) {
    const int M = min(*count, cap);
    const int tiles_n = (N + TN - 1) / TN;
    const int bx = blockIdx.x % tiles_n, by = blockIdx.x / tiles_n;
    return {rows, M, cap, by * TM, bx * TN};
}

// The K loop is a software pipeline without a predicate in its steady state:
//   * global loads are issued unconditionally, PF slabs ahead, from an address clamped into the tensor (row 0 for a tile row
//     that names no dense row, the last chunk / last row of K past the end); what must not count is replaced by zeros when the
//     registers go to LDS.  No branch surrounds a load, so the wait in front of the ds_write is a counted vmcnt.
//   * a wave holds the MFMA operands of the current slab in registers.  It issues the first half of the slab's MFMAs, passes the
//     one barrier of the slab (the next slab is then complete in the other LDS stage), requests the next slab's operands and
//     issues the second half of the MFMAs while those reads are under way.
//   * the last slab is peeled out of the loop (nothing left to stash or to read ahead).
// fetch(t, slab): request slab t of K into registers, any t | stash(stage, t, slab): those registers to LDS stage `stage`, zeros for
// what is outside | read_frag(frag, stage): a wave's MFMA operands of a stage | mfma_half(frag, h): half h = 0 | 1 of the slab's MFMAs.
// ring: PF register sets, slab t waits in set t % PF.  FENCE: a step starts with a scheduling barrier (the fp16 kernel: it keeps the
// selects of the later slabs' registers, and with them their waits, out of this step).
template <int PF, bool FENCE, class Frag, class Slab, class Fetch, class Stash, class ReadFrag, class MfmaHalf>
__device__ __forceinline__ void rows_k_pipeline(Slab (&ring)[PF], int nslab, const Fetch& fetch, const Stash& stash,
                                                const ReadFrag& read_frag, const MfmaHalf& mfma_half) {
    fetch(0, ring[0]);
    stash(0, 0, ring[0]);
#pragma unroll
    for (int j = 1; j <= PF; ++j) fetch(j, ring[j % PF]);   // slabs 1 .. PF in flight (set 0 is free again)
    lds_barrier();
    Frag cur;
    read_frag(cur, 0);
    // slab s: stash slab s + 1 (every wave left stage (s + 1) & 1, slab s - 1, before the barrier of slab s - 1: lds_barrier() waits
    // for the wave's reads), half of the MFMAs, the barrier, the reads of slab s + 1, the other half
    auto step = [&](int s, Slab& x, bool refill) {
        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
        stash((s + 1) & 1, s + 1, x);
        if (refill) fetch(s + 1 + PF, x);
        mfma_half(cur, 0);
        lds_barrier();
        Frag nxt;
        read_frag(nxt, (s + 1) & 1);
        mfma_half(cur, 1);
        cur = nxt;
    };
    int s = 0;
    for (; s + PF < nslab; s += PF)                  // steady state: one basic block, no test between the PF steps
#pragma unroll
        for (int j = 0; j < PF; ++j) step(s + j, ring[(j + 1) % PF], true);
#pragma unroll
    for (int j = 0; j < PF - 1; ++j) {               // at most PF - 1 steps are left, and nothing they would request is inside K
        if (s + j + 1 >= nslab) break;
        step(s + j, ring[(j + 1) % PF], false);
    }
    mfma_half(cur, 0);
    mfma_half(cur, 1);
}

// The end of a tile.  (1) The k shares meet: the WK waves that worked on output tile `tile` of the workgroup's NT, each on its own k groups
// of every slab -- wk > 0 hand their accumulators to wk = 0 through red[(WK - 1) * NT * 16 * 64] and are done, wk = 0 adds them in order.
// (2) EPI, what happens to a finished row of the product on its way out.  0: stored as it is (the backward's input-gradient GEMMs) |
// 1: + bias[n] (a forward nn.Linear) | 2: + bias[n], stored to C, and QuickGELU of it stored to C2 (c_fc: the backward's tape wants the
// pre-activation, c_proj the activation; quick_gelu_f is the device function of quick_gelu_fwd_kernel, so C2 has the bits
// ops.quick_gelu_fwd(C) would have).  acc is one 32 x 32 MFMA tile: column lane & 31 of the wave's columns (wc), row
// (v & 3) + 8 (v >> 2) + 4 (lane >> 5) of the wave's rows (wr); scattered through rid[].
// One function, so that the compiler may sink a share's additions to the rows that are stored and fetch the bias under the LDS reads.
template <int EPI, int WK, int NT>
__device__ __forceinline__ void rows_finish(f32x16& acc, float* red, const RowsTilePos& p, const int* rid, int wr, int wc, int wk, int tile,
                                            int lane, int N, float* __restrict__ C, const float* __restrict__ bias, float* __restrict__ C2) {
    if constexpr (WK > 1) {                          // (else one wave owns a tile's whole K: nothing to add)
        if (wk > 0)
#pragma unroll
            for (int v = 0; v < 16; ++v) red[(((wk - 1) * NT + tile) * 16 + v) * 64 + lane] = acc[v];
        lds_barrier();
        if (wk > 0) return;
#pragma unroll
        for (int q = 0; q < WK - 1; ++q)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[v] += red[((q * NT + tile) * 16 + v) * 64 + lane];
    }
    const int li = lane & 31, lg = lane >> 5;
    const int gn = p.n0 + wc * 32 + li;
    if (p.m0 + wr * 32 >= p.M || gn >= N) return;
    float bv = 0.f;
    if constexpr (EPI != 0) bv = bias[gn];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r = rid[wr * 32 + (v >> 2) * 8 + lg * 4 + (v & 3)];
        if (r < 0) continue;
        if constexpr (EPI == 0) {
            C[static_cast<int64_t>(r) * N + gn] = acc[v];
        } else {
            const float m = acc[v] + bv;
            C[static_cast<int64_t>(r) * N + gn] = m;
            if constexpr (EPI == 2) C2[static_cast<int64_t>(r) * N + gn] = quick_gelu_f(m);
        }
    }
}

// Host side.  The operands a kernel can take: N and K multiples of `mult` (a 16-byte chunk of its narrowest operand), 16-byte aligned.
inline bool rows_operands_ok(const char* what, const void* a, const void* w, const void* c, int N, int K, int mult) {
    if (N % mult || K % mult || ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(c)) & 15u)) {
        set_error("%s: N=%d and K=%d must be multiples of %d and the operands 16-byte aligned", what, N, K, mult);
        return false;
    }
    return true;
}
// The grid of a launch with tm x tn tiles, sized for the capacity: one workgroup per tile, column tiles fastest.  0: too large.
inline unsigned rows_grid(const char* what, int tm, int tn, int cap_rows, int N) {
    const int64_t wgs = static_cast<int64_t>((N + tn - 1) / tn) * ((cap_rows + tm - 1) / tm);
    if (wgs < (1ll << 31)) return static_cast<unsigned>(wgs);
    set_error("%s: cap_rows=%d x N=%d is too large a grid", what, cap_rows, N);
    return 0;
}

}  // namespace mmx
