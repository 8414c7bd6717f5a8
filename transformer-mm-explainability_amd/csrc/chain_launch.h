// Host helpers the launchers of the N <= 128 relevancy chain kernels share (relevancy_chain_fused.hip, relevancy_chain_groups.hip,
// relevancy_chain_cols.hip): the argument-record fill from a ChainCall (mmx_common.h), the NT dispatch, the dynamic-LDS attribute.
#pragma once
#include "mmx_common.h"

#include <type_traits>

namespace mmx {

// the members every chain kernel's argument record shares (ChainArgs, GroupsArgs, ColsArgs), from what the entry validated
template <typename Args>
inline void chain_fill_args(Args& r, const ChainCall& c) {
    memset(&r, 0, sizeof(r));
    for (int l = 0; l < c.n_layers; ++l) { r.attn[l] = c.attn[l]; r.grad[l] = c.grad[l]; }
    r.n_layers = c.n_layers; r.B = c.B; r.H = c.H; r.N = c.N;
    r.R_init = c.R_init;
    r.R_out = c.R_out;
    r.attn_bstride = c.attn_bstride;
    r.nt = c.nt;
    r.debug = c.debug;
}
// ... and those of the kernels on chain_stream.h
template <typename Args>
inline void chain_fill_stream_args(Args& r, const ChainCall& c) {
    chain_fill_args(r, c);
    r.nchunks = (c.N * c.N + 3) / 4;
    r.row_magic = static_cast<unsigned>((0x100000000ull + c.N - 1) / c.N);
    r.causal = c.causal;
}

// f(std::integral_constant<int, NT>) for NT = ceil(N / 16) in 1 .. 8
template <typename F>
inline int dispatch_nt(int nt, F&& f) {
    switch (nt) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        default: return f(std::integral_constant<int, 8>{});
    }
}

// a kernel that asks for more than 48 KiB of dynamic LDS has to be told so
template <typename K>
inline int set_dynamic_lds(K kernel, size_t bytes) {
    if (bytes <= 48 * 1024) return MMX_OK;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(bytes));
    return e == hipSuccess ? MMX_OK : hip_fail(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
}

}  // namespace mmx
