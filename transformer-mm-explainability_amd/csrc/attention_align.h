// The strides of a [B, H, N, D] attention operand view and the one alignment test the eligibility rules of the attention kernels
// (attention_kernels.hip, attention_head.hip, attention_stream.hip, attention_bf16.hip, attention_bf16_v3.hip) are written in.
// No HIP include: tools/host/attention_align_main.cpp compiles this header alone with a plain host compiler.
#pragma once
#include <stdint.h>

namespace mmx {

struct Strides { int64_t sb, sh, sn; };   // batch, head, row: in ELEMENTS

// Does every row of the view start on a multiple of `align_bytes` (a power of two)?  That is: the base pointer, the row stride, the
// head stride and -- `batch_stride`: the kernel adds b * sb (false: it reads batch 0 only, a shared operand, or the caller tests sb
// against another bound) -- the batch stride, in bytes of `elem_bytes` each.  The kernels' vector accesses decide the rest:
//   fp32 operands read as float4 (16 bytes), bf16 gradient rows read as 8 elements:   elem 4 or 2, align 16
//   bf16 gradient rows of the whole-head kernels, 4-element chunks:                      elem 2, align 8
//   dK / dV of the bf16-MFMA kernels, stored as (d, d + 1) pairs or single floats:       elem 2 or 4, align 4
inline bool rows_aligned(const void* p, const Strides& s, int elem_bytes, int align_bytes, bool batch_stride) {
    uintptr_t bits = reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(s.sh * elem_bytes) | static_cast<uintptr_t>(s.sn * elem_bytes);
    if (batch_stride) bits |= static_cast<uintptr_t>(s.sb * elem_bytes);
    return (bits & static_cast<uintptr_t>(align_bytes - 1)) == 0;
}

}  // namespace mmx
