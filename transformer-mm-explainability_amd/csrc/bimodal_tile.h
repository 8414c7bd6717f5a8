// The LDS matrix view and the exact-fp32 16 x 16 MFMA tile product of the bi-modal kernels (bimodal_kernels.hip: the rule schedule;
// bimodal_baselines.hip: the rollout chain).  One copy, so that both families sum a product in the same order.
#pragma once
#include "mmx_common.h"

namespace mmx {

struct M2 {               // an LDS matrix [D16][ld]
    float* p;
    int ld;
    __device__ __forceinline__ float& at(int i, int j) const { return p[i * ld + j]; }
};

// one 16 x 16 tile of A[i0.., :K] . B[:K, j0..]; TA: A is stored K x M.  The A operand is masked beyond K, so only B's rows
// beyond K have to be finite (they are zero: no matrix is ever written outside its valid block).  The contraction runs in
// groups of 16 (four MFMA k-steps): the eight operand reads of a group are issued before its first MFMA, so the LDS latency is
// paid once per group instead of once per k-step (K <= 48: at most three groups; rows up to round16(K) <= D16 exist).
template <bool TA>
__device__ __forceinline__ f32x4 bm_tile(M2 A, M2 B, int i0, int j0, int K, int lane) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int li = lane & 15, lk = lane >> 4;
    const float* ap = TA ? A.p + lk * A.ld + i0 + li : A.p + (i0 + li) * A.ld + lk;
    const float* bp = B.p + lk * B.ld + j0 + li;
    const int astep = TA ? 4 * A.ld : 4, bstep = 4 * B.ld;
    for (int k0 = 0; k0 < K; k0 += 16) {
        float av[4], bv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            av[s] = ap[s * astep];
            bv[s] = bp[s * bstep];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma16x16x4((k0 + 4 * s + lk < K) ? av[s] : 0.f, bv[s], acc);
        ap += 4 * astep; bp += 4 * bstep;
    }
    return acc;
}

}  // namespace mmx
