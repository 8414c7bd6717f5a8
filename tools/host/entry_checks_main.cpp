// Stand-alone host check of csrc/entry_checks.h (tools/check_entry_checks.py compiles and runs it; no GPU, no HIP header).
//   ranges_overlap  every pair of ranges with start 0..7 and length 1..4 against the intersection of their byte sets
//   spans_alias     every list of up to 3 outputs and up to 2 inputs drawn from those ranges and the null span, against its definition
//                   on the byte sets: an output meets an input, or an output meets a later output
//   by hand         touching ranges, a one-byte overlap, containment, null on either side, one span as output and input, two equal
//                   outputs; align256 at 0, 1, 255, 256, 257
// Exit status 0 and "entry_checks: ok", or 1 after the first mismatches.
#include <stdio.h>

#include "entry_checks.h"

using mmx::Span;

static int g_fail = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (++g_fail <= 10) printf("line %d: %s\n", __LINE__, #cond);     \
        }                                                                     \
    } while (0)

static char g_buf[16];   // every range lies inside it: start + length <= 11

struct Cand {
    Span span;
    unsigned bytes;      // bit i: the range holds g_buf[i]
};

int main() {
    Cand cand[33];
    int n = 0;
    for (int start = 0; start < 8; ++start)
        for (int len = 1; len <= 4; ++len) cand[n++] = {{g_buf + start, static_cast<size_t>(len)}, ((1u << len) - 1u) << start};
    const int n_ranges = n;
    cand[n++] = {{nullptr, 4}, 0u};   // a null pointer overlaps nothing, whatever its size

    long pairs = 0, lists = 0;
    for (int i = 0; i < n_ranges; ++i)
        for (int j = 0; j < n_ranges; ++j, ++pairs)
            EXPECT(mmx::ranges_overlap(cand[i].span.p, cand[i].span.bytes, cand[j].span.p, cand[j].span.bytes) ==
                   ((cand[i].bytes & cand[j].bytes) != 0));

    for (int n_out = 0; n_out <= 3; ++n_out)
        for (int n_in = 0; n_in <= 2; ++n_in) {
            int idx[5] = {0, 0, 0, 0, 0};   // outputs first, then inputs; an odometer over the candidates
            const int slots = n_out + n_in;
            for (;;) {
                Span outs[3], ins[2];
                bool want = false;
                for (int o = 0; o < n_out; ++o) {
                    outs[o] = cand[idx[o]].span;
                    for (int i = 0; i < n_in; ++i) want |= (cand[idx[o]].bytes & cand[idx[n_out + i]].bytes) != 0;
                    for (int p = o + 1; p < n_out; ++p) want |= (cand[idx[o]].bytes & cand[idx[p]].bytes) != 0;
                }
                for (int i = 0; i < n_in; ++i) ins[i] = cand[idx[n_out + i]].span;
                EXPECT(mmx::spans_alias(outs, n_out, ins, n_in) == want);
                ++lists;
                int s = 0;
                while (s < slots && ++idx[s] == n) idx[s++] = 0;
                if (s == slots) break;
            }
        }

    const Span a = {g_buf, 4}, touch = {g_buf + 4, 4}, one = {g_buf + 3, 4}, inside = {g_buf + 1, 2}, null4 = {nullptr, 4};
    EXPECT(!mmx::ranges_overlap(a.p, a.bytes, touch.p, touch.bytes) && !mmx::ranges_overlap(touch.p, touch.bytes, a.p, a.bytes));
    EXPECT(!mmx::spans_alias(&a, 1, &touch, 1) && !mmx::spans_alias(&touch, 1, &a, 1));
    EXPECT(mmx::spans_alias(&a, 1, &one, 1) && mmx::spans_alias(&one, 1, &a, 1));
    EXPECT(mmx::spans_alias(&a, 1, &inside, 1) && mmx::spans_alias(&inside, 1, &a, 1));
    EXPECT(!mmx::spans_alias(&null4, 1, &a, 1) && !mmx::spans_alias(&a, 1, &null4, 1));
    EXPECT(!mmx::ranges_overlap(nullptr, 4, g_buf, 4) && !mmx::ranges_overlap(g_buf, 4, nullptr, 4) &&
           !mmx::ranges_overlap(nullptr, 4, nullptr, 4));
    EXPECT(mmx::spans_alias(&a, 1, &a, 1));
    const Span twice[2] = {a, a}, apart[2] = {a, touch}, with_null[2] = {null4, null4};
    EXPECT(mmx::spans_alias(twice, 2, nullptr, 0));
    EXPECT(!mmx::spans_alias(apart, 2, nullptr, 0));
    EXPECT(!mmx::spans_alias(with_null, 2, nullptr, 0));
    EXPECT(!mmx::spans_alias(nullptr, 0, &a, 1));
    const Span ins_overlap[2] = {a, one};   // inputs may overlap each other
    EXPECT(!mmx::spans_alias(&touch, 0, ins_overlap, 2));

    EXPECT(mmx::align256(0) == 0 && mmx::align256(1) == 256 && mmx::align256(255) == 256 && mmx::align256(256) == 256 &&
           mmx::align256(257) == 512);

    if (g_fail) {
        printf("entry_checks: %d mismatches\n", g_fail);
        return 1;
    }
    printf("entry_checks: ok (%ld pairs, %ld lists)\n", pairs, lists);
    return 0;
}
