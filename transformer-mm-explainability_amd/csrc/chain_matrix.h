// The matrix-wave and hand-off pieces of the N <= 128 relevancy chain kernels (relevancy_chain_fused.hip, relevancy_chain_groups.hip,
// relevancy_chain_cols.hip), next to the stream wave of chain_stream.h.  Device code only (their launchers' helpers: chain_launch.h).
//
// A matrix wave owns one 16-column slab of R in REGISTERS, in the MFMA C/D layout: R[t][r] of lane l is element
// (row 16 t + 4 (l >> 4) + r, column 16 slab + (l & 15)).  Because the k-order of a dot product is free, k is visited as (t, r, l >> 4):
// the B operand of v_mfma_f32_16x16x4_f32 is then exactly the register R[t][r] the lane already holds -- R never moves; the A operand
// (A_bar, an LDS image of NP = 16 NT rows with row stride NP + 4 floats, pads zero) is one ds_read_b128 per 4 MFMAs.  Only the functions
// here know that layout; a kernel asks chain_lane() for its lane's place once and hands it on.
#pragma once
#include "mmx_common.h"

#include <type_traits>

namespace mmx {

template <int NT> constexpr int kChainNP = NT * 16;        // rows / columns of an A_bar image
template <int NT> constexpr int kChainS = NT * 16 + 4;     // its row stride in floats

// a lane's place in the layout above: its column of R and the first of its four rows inside a 16-row tile
struct ChainLane { int col, rq; };
__device__ __forceinline__ ChainLane chain_lane(int slab, int lane) { return {slab * 16 + (lane & 15), (lane >> 4) * 4}; }

// `n4` 16-byte words of LDS <- 0 by the whole workgroup (the pads of the images must read as 0, the counters start at 0)
__device__ __forceinline__ void chain_lds_zero(float* smem, int n4, int tid, int threads) {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < n4; i += threads) reinterpret_cast<f32x4*>(smem)[i] = z;
}

// Workgroup w of a grid of B * P -> (sample b, part): the P workgroups of a sample on ONE XCD (workgroup w runs on XCD w % 8), so that
// what they share meets in that XCD's L2.  A placement hint only -- nothing depends on it.
__device__ __forceinline__ void chain_xcd_placement(int w, int B, int P, int& b, int& part) {
    const int full = (B >> 3) * 8 * P;
    if (w < full) { b = (w & 7) + 8 * ((w >> 3) / P); part = (w >> 3) % P; }
    else { b = (B >> 3) * 8 + (w - full) / P; part = (w - full) % P; }
}

// R <- this lane's share of the N x N matrix at src + base (zeros past N); from_src false: of the identity.  I: the type the row offset
// is formed in (the fused kernel keeps its 64-bit arithmetic, the others their 32-bit one: N <= 128 either way).
template <typename I, int NT>
__device__ __forceinline__ void chain_slab_load(f32x4 (&R)[NT], bool from_src, const float* src, int64_t base, int N, ChainLane q) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = t * 16 + q.rq + r;
            float v = 0.f;
            if (row < N && q.col < N) v = from_src ? src[base + static_cast<I>(row) * N + q.col] : (row == q.col ? 1.f : 0.f);
            R[t][r] = v;
        }
}

// this lane's share of R -> the N x N matrix at dst + base.  wt: write-through stores (a hand-off that follows needs no L2 write-back
// fence).  poisoned: a wait of this wave gave up -- the result says so (NaN), it does not lie.
template <typename I, int NT>
__device__ __forceinline__ void chain_slab_store(float* dst, int64_t base, const f32x4 (&R)[NT], int N, ChainLane q, bool wt,
                                                 bool poisoned) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = t * 16 + q.rq + r;
            if (row < N && q.col < N) {
                float* p = dst + (base + static_cast<I>(row) * N + q.col);
                const float v = poisoned ? __builtin_nanf("") : R[t][r];
                if (wt) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else *p = v;
            }
        }
}

// Accumulator of output tile ti (rows 16 ti .. 16 ti + 15 of this wave's slab) of  img . R:  4 NT MFMAs.  tri (MMX_CHAIN_CAUSAL, R
// started as the identity: img, R and the product are lower triangular): only the k tiles tj <= t <= ti, tj = the wave's slab, are
// visited -- the skipped ones multiply exact zeros.  A kernel without a causal form passes std::false_type.
template <int NT, typename Tri>
__device__ __forceinline__ f32x4 chain_tile_product(const float* img, int ti, const f32x4 (&R)[NT], int lane, ChainLane q, Tri tri, int tj) {
    const float* Ab = img + (lane & 15) * kChainS<NT> + q.rq;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (tri && (t > ti || t < tj)) continue;      // (tj is wave-uniform)
        const f32x4 av = *reinterpret_cast<const f32x4*>(Ab + ti * 16 * kChainS<NT> + t * 16);
        acc = mfma16x16x4(av[0], R[t][0], acc);
        acc = mfma16x16x4(av[1], R[t][1], acc);
        acc = mfma16x16x4(av[2], R[t][2], acc);
        acc = mfma16x16x4(av[3], R[t][3], acc);
    }
    return acc;
}

// Wait until the LDS arrival counter `cnt` holds the elements of tile ti (rows 16 ti .. of an N x N image), `uses` times over; true:
// gave up.  Bounded like every wait here: the stream waves of the workgroup deliver in microseconds or something is broken.
__device__ __forceinline__ bool chain_tile_wait(const unsigned* cnt, int N, int ti, unsigned uses) {
    const unsigned expect = uses * static_cast<unsigned>(max(0, min(N, ti * 16 + 16) - ti * 16) * N);
    int turns = 0;
    while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < expect && ++turns < (1 << 24))
        __builtin_amdgcn_s_sleep(1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    return turns >= (1 << 24);      // never seen
}

// Hand-off of a workgroup's partial product: every storing wave drains its write-through stores, then thread 0 takes the sample's
// ticket and the workgroup learns it through an LDS word.  -> the ticket (G - 1: this workgroup arrived last)
__device__ __forceinline__ unsigned chain_handoff_ticket(unsigned* counter, unsigned* ticket_lds, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) *ticket_lds = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    return *ticket_lds;
}

}  // namespace mmx
