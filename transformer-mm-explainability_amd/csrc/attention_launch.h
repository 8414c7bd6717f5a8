// Host helpers the launchers of the attention kernels share (attention_kernels.hip, attention_head.hip, attention_stream.hip,
// attention_bf16.hip, attention_bf16_v3.hip): the launch itself and the three run-time -> template-argument dispatches.
#pragma once
#include "mmx_common.h"
#include "chain_launch.h"   // set_dynamic_lds

#include <type_traits>

namespace mmx {

// kern<<<grid, threads, lds, s>>>(args...) with the dynamic-LDS attribute where it is needed; `name` goes into the launch error
template <typename K, typename... Args>
inline int launch_attn(K kern, dim3 grid, int threads, size_t lds, hipStream_t s, const char* name, const Args&... args) {
    const int rc = set_dynamic_lds(kern, lds);
    if (rc) return rc;
    kern<<<grid, threads, lds, s>>>(args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MMX_OK : hip_fail(e, name);
}

// f(std::integral_constant<int, DP>): the padded head dim of the instantiation that serves head_dim D (<= 64, checked by the caller)
template <typename F>
inline int by_head_dim(int D, F&& f) {
    return D <= 32 ? f(std::integral_constant<int, 32>{}) : f(std::integral_constant<int, 64>{});
}

// f(std::integral_constant<int, DT>) for the three element types of a capture slab and 1 ("launched": f leaves the rc where its
// caller wants it); 0 ("not eligible") for anything else
template <typename F>
inline int by_slab_dtype(int dt, F&& f) {
    switch (dt) {
        case MMX_F32: f(std::integral_constant<int, MMX_F32>{}); return 1;
        case MMX_F16: f(std::integral_constant<int, MMX_F16>{}); return 1;
        case MMX_BF16: f(std::integral_constant<int, MMX_BF16>{}); return 1;
        default: return 0;
    }
}

// f(std::integral_constant<int, NTK>) for NTK = ceil(Nk / 16) in 1 .. 8 (the whole-head kernels); MMX_ENOTSUP outside
template <typename F>
inline int by_key_tiles(int ntk, F&& f) {
    switch (ntk) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        case 5: return f(std::integral_constant<int, 5>{});
        case 6: return f(std::integral_constant<int, 6>{});
        case 7: return f(std::integral_constant<int, 7>{});
        case 8: return f(std::integral_constant<int, 8>{});
        default: return MMX_ENOTSUP;
    }
}

}  // namespace mmx
