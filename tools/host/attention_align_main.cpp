// Stand-alone host check of csrc/attention_align.h (tools/check_attention_align.py compiles and runs it; no GPU, no HIP header).
// The attention kernel files had five spellings of "are these rows aligned" (and two open-coded ones beside them); they are written
// out below as they stood, and each is compared with mmx::rows_aligned in the argument form its call site uses now, over every
//   pointer offset (from a 16-byte boundary) in {0, 2, 4, 8, 12, 16}  x  each of sb, sh, sn in {0, 1, 2, 3, 4, 6, 8, 12}
// = 3072 cases per form.  Exit status 0 and "attention_align: ok", or 1 after the first mismatches.
#include <stdio.h>

#include "attention_align.h"

using mmx::Strides;
using mmx::rows_aligned;

// ---- the former expressions
// attention_head.hip
static bool head_aligned16(const void* p, int64_t s0, int64_t s1, int64_t s2) {
    return ((reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(s0 * 4) | static_cast<uintptr_t>(s1 * 4) |
             static_cast<uintptr_t>(s2 * 4)) & 15u) == 0;
}
// attention_stream.hip
static bool stream_aligned16(const float* p, const Strides& s) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && s.sb % 4 == 0 && s.sh % 4 == 0 && s.sn % 4 == 0;
}
// attention_bf16.hip
static bool v2_al16(const void* p, const Strides& s, int elem) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (s.sb * elem) % 16 == 0 && (s.sh * elem) % 16 == 0 && (s.sn * elem) % 16 == 0;
}
// attention_bf16_v3.hip
static bool v3_al16(const void* p, const Strides& s, int elem) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (s.sh * elem) % 16 == 0 && (s.sn * elem) % 16 == 0;
}
// attn_bwd_head_try's lambda (a.io_bf16 is the captured flag)
static bool head_io_ok(int io_bf16, const void* p, const Strides& st) {
    return io_bf16 ? ((reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(st.sb * 2) | static_cast<uintptr_t>(st.sh * 2) |
                       static_cast<uintptr_t>(st.sn * 2)) & 7u) == 0
                   : head_aligned16(p, st.sb, st.sh, st.sn);
}
// set_slabs (attention_kernels.hip): true = the forward's O is dropped as a hint
static bool slabs_o_unaligned(const void* o, const Strides& oos) {
    return reinterpret_cast<uintptr_t>(o) % 16 || oos.sb % 4 || oos.sh % 4 || oos.sn % 4;
}
// the dk (and dv) terms of attn_bwd_bf16_try / attn_bwd_bf16_v3_try: true = not eligible
static bool dkv_unaligned4(const void* dk, const Strides& dks, int e) {
    return reinterpret_cast<uintptr_t>(dk) % 4 || (dks.sn * e) % 4 || (dks.sh * e) % 4 || (dks.sb * e) % 4;
}

static int g_fail = 0;
static long g_cases = 0;
#define EXPECT_SAME(form, was, is)                                                                                   \
    do {                                                                                                            \
        if ((was) != (is) && ++g_fail <= 10)                                                                        \
            printf("%s: offset %d sb %lld sh %lld sn %lld: was %d, is %d\n", form, off, (long long)s.sb, (long long)s.sh, \
                   (long long)s.sn, int(was), int(is));                                                             \
    } while (0)

int main() {
    alignas(16) static char buf[64];
    const int offsets[] = {0, 2, 4, 8, 12, 16};
    const int64_t strides[] = {0, 1, 2, 3, 4, 6, 8, 12};
    for (int off : offsets)
        for (int64_t sb : strides)
            for (int64_t sh : strides)
                for (int64_t sn : strides) {
                    const void* p = buf + off;
                    const Strides s{sb, sh, sn};
                    ++g_cases;
                    EXPECT_SAME("head aligned16", head_aligned16(p, s.sb, s.sh, s.sn), rows_aligned(p, s, 4, 16, true));
                    EXPECT_SAME("stream aligned16", stream_aligned16(static_cast<const float*>(p), s), rows_aligned(p, s, 4, 16, true));
                    EXPECT_SAME("bf16 al16, elem 4", v2_al16(p, s, 4), rows_aligned(p, s, 4, 16, true));
                    EXPECT_SAME("bf16 al16, elem 2", v2_al16(p, s, 2), rows_aligned(p, s, 2, 16, true));
                    EXPECT_SAME("bf16_v3 al16, elem 4", v3_al16(p, s, 4), rows_aligned(p, s, 4, 16, false));
                    EXPECT_SAME("bf16_v3 al16, elem 2", v3_al16(p, s, 2), rows_aligned(p, s, 2, 16, false));
                    EXPECT_SAME("bf16_v3 al16 and sb, elem 2", v3_al16(p, s, 2) && !((s.sb * 2) % 16), rows_aligned(p, s, 2, 16, true));
                    EXPECT_SAME("head io_ok, fp32", head_io_ok(0, p, s), rows_aligned(p, s, 4, 16, true));
                    EXPECT_SAME("head io_ok, bf16", head_io_ok(1, p, s), rows_aligned(p, s, 2, 8, true));
                    EXPECT_SAME("set_slabs hint", !slabs_o_unaligned(p, s), rows_aligned(p, s, 4, 16, true));
                    EXPECT_SAME("dk / dv, elem 4", !dkv_unaligned4(p, s, 4), rows_aligned(p, s, 4, 4, true));
                    EXPECT_SAME("dk / dv, elem 2", !dkv_unaligned4(p, s, 2), rows_aligned(p, s, 2, 4, true));
                }
    printf("attention_align: 12 forms x %ld cases, %d mismatches\n", g_cases, g_fail);
    if (g_fail) return 1;
    printf("attention_align: ok\n");
    return 0;
}
