// Stand-alone host check of csrc/text_placement.h (tools/check_text_placement.py compiles and runs it; no GPU, no HIP header).
//   every table of 1 or 2 steps with base -1..7, stride 0..5, width 0..4, for B = 1..3, T = 3 and out_elems 0..14 (and a sample of
//   3-step tables), against the SETS of elements the sequences occupy:
//     the per-step rules in their order (width, stride, base, overrun: the largest element of the step >= out_elems);
//     OVERLAP exactly when a pair of steps passes neither rule, both restated on the sets -- (a) same stride, no window wraps past
//     the period, and the residue sets are disjoint; (b) the hulls [min, max] of the two sets are disjoint;
//     an accepted table never has two steps that share an element and never an element at or past out_elems (soundness);
//     with B == 1 a refused pair does share an element (rule (b) is exact there).
//   by hand: the two-group layout of the evaluator at T = 20, one element too few, an interleave that wraps, values near 2^62.
// Exit status 0 and "text_placement: ok", or 1 after the first mismatches.
#include <stdio.h>

#include <set>

#include "text_placement.h"

static int g_fail = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            if (++g_fail <= 10) printf("line %d: %s\n", __LINE__, #cond);     \
        }                                                                     \
    } while (0)

typedef std::set<int64_t> Set;

static Set elements(const int64_t* p, int B) {
    Set out;
    for (int b = 0; b < B; ++b)
        for (int64_t i = 0; i < p[2]; ++i) out.insert(p[0] + b * p[1] + i);
    return out;
}

static bool meet(const Set& a, const Set& b) {
    for (int64_t x : a)
        if (b.count(x)) return true;
    return false;
}

// the acceptance rule of a pair, restated on the sets (both steps have passed the per-step rules)
static bool pair_accepted(const int64_t* a, const int64_t* b, int B) {
    const Set ea = elements(a, B), eb = elements(b, B);
    if (*ea.rbegin() < *eb.begin() || *eb.rbegin() < *ea.begin()) return true;   // (b)
    if (a[1] != b[1]) return false;
    if (a[0] % a[1] + a[2] > a[1] || b[0] % b[1] + b[2] > b[1]) return false;    // a window wraps past the period
    Set ra, rb;
    for (int64_t x : ea) ra.insert(x % a[1]);
    for (int64_t x : eb) rb.insert(x % b[1]);
    return !meet(ra, rb);
}

static mmx::TextPlaceError step_rule(const int64_t* p, int B, int T, int64_t out_elems) {
    if (p[2] < 1 || p[2] > T) return mmx::TEXT_PLACE_WIDTH;
    if (p[1] < p[2]) return mmx::TEXT_PLACE_STRIDE;
    if (p[0] < 0) return mmx::TEXT_PLACE_BASE;
    if (*elements(p, B).rbegin() >= out_elems) return mmx::TEXT_PLACE_OVERRUN;
    return mmx::TEXT_PLACE_OK;
}

static long g_tables = 0;

static void check_table(const int64_t* place, int S, int B, int T, int64_t out_elems) {
    ++g_tables;
    int s0 = -7, s1 = -7;
    const mmx::TextPlaceError got = mmx::check_text_placement(place, S, B, T, out_elems, &s0, &s1);
    for (int s = 0; s < S; ++s) {
        const mmx::TextPlaceError want = step_rule(place + 3 * s, B, T, out_elems);
        if (want != mmx::TEXT_PLACE_OK) {
            EXPECT(got == want && s0 == s && s1 == -1);
            return;
        }
    }
    bool all = true;
    for (int s = 0; s < S; ++s)
        for (int t = s + 1; t < S; ++t) {
            const bool ok = pair_accepted(place + 3 * s, place + 3 * t, B);
            const bool share = meet(elements(place + 3 * s, B), elements(place + 3 * t, B));
            EXPECT(!(ok && share));                          // soundness of the rule itself
            if (B == 1) EXPECT(ok == !share);
            if (!ok && all) {
                EXPECT(got == mmx::TEXT_PLACE_OVERLAP && s0 == s && s1 == t);
                all = false;
            }
        }
    if (all) EXPECT(got == mmx::TEXT_PLACE_OK);
}

int main() {
    const int T = 3;
    for (int B = 1; B <= 3; ++B)
        for (int64_t out_elems = 0; out_elems <= 14; out_elems += (out_elems < 4 ? 1 : 5)) {
            int64_t place[9];
            for (place[0] = -1; place[0] <= 7; ++place[0])
                for (place[1] = 0; place[1] <= 5; ++place[1])
                    for (place[2] = 0; place[2] <= 4; ++place[2]) {
                        check_table(place, 1, B, T, out_elems);
                        if (step_rule(place, B, T, out_elems) != mmx::TEXT_PLACE_OK) continue;
                        for (place[3] = -1; place[3] <= 7; ++place[3])
                            for (place[4] = 0; place[4] <= 5; ++place[4])
                                for (place[5] = 0; place[5] <= 4; ++place[5]) {
                                    check_table(place, 2, B, T, out_elems);
                                    if (step_rule(place + 3, B, T, out_elems) != mmx::TEXT_PLACE_OK || (place[3] + place[4]) % 3) continue;
                                    for (place[6] = 0; place[6] <= 7; place[6] += 2)
                                        for (place[7] = 1; place[7] <= 5; place[7] += 2)
                                            for (place[8] = 1; place[8] <= 2; ++place[8]) check_table(place, 3, B, T, out_elems);
                                }
                    }
        }

    int s0, s1;
    // the evaluator's two groups at T = 20, B = 2: (20, 15, 11 | 6, 5, 4, 3, 2, 2), sample-major inside a group
    // (the second block starts at a multiple of its stride 36, so that no window of a period wraps)
    const int64_t two[27] = {0, 60, 20, 20, 60, 20, 40, 60, 20, 144, 36, 6, 150, 36, 6, 156, 36, 6, 162, 36, 6, 168, 36, 6, 174, 36, 6};
    EXPECT(mmx::check_text_placement(two, 9, 2, 20, 216, &s0, &s1) == mmx::TEXT_PLACE_OK);
    EXPECT(mmx::check_text_placement(two, 9, 2, 20, 215, &s0, &s1) == mmx::TEXT_PLACE_OVERRUN && s0 == 8);
    int64_t moved[27];
    for (int i = 0; i < 27; ++i) moved[i] = two[i];
    moved[9] = 119;                                           // step 3 one element into the first group's block
    EXPECT(mmx::check_text_placement(moved, 9, 2, 20, 216, &s0, &s1) == mmx::TEXT_PLACE_OVERLAP && s0 == 2 && s1 == 3);
    moved[9] = 145;                                           // ... and one element into step 4's window
    EXPECT(mmx::check_text_placement(moved, 9, 2, 20, 216, &s0, &s1) == mmx::TEXT_PLACE_OVERLAP && s0 == 3 && s1 == 4);
    for (int j = 0; j < 6; ++j) moved[9 + 3 * j] = 121 + 6 * j;   // the second block off its period: element-disjoint, but a window wraps
    EXPECT(mmx::check_text_placement(moved, 9, 2, 20, 216, &s0, &s1) == mmx::TEXT_PLACE_OVERLAP);
    const int64_t wrap[6] = {3, 4, 2, 1, 4, 2};               // same stride, element-disjoint, but the first window wraps: refused
    EXPECT(mmx::check_text_placement(wrap, 2, 3, 20, 64, &s0, &s1) == mmx::TEXT_PLACE_OVERLAP);
    const int64_t big = static_cast<int64_t>(1) << 62;
    const int64_t far[3] = {big, big, 2};                     // no product is formed: an overrun, not an overflow
    EXPECT(mmx::check_text_placement(far, 1, 3, 20, big + 2, &s0, &s1) == mmx::TEXT_PLACE_OVERRUN);
    EXPECT(mmx::check_text_placement(far, 1, 1, 20, big + 2, &s0, &s1) == mmx::TEXT_PLACE_OK);
    EXPECT(mmx::check_text_placement(far, 1, 1, 20, big + 1, &s0, &s1) == mmx::TEXT_PLACE_OVERRUN);
    EXPECT(mmx::check_text_placement(far, 1, 1, 20, -1, &s0, &s1) == mmx::TEXT_PLACE_OVERRUN);

    if (g_fail) {
        printf("text_placement: %d mismatches\n", g_fail);
        return 1;
    }
    printf("text_placement: ok (%ld tables)\n", g_tables);
    return 0;
}
