// Host-only check of the placement table of mmx_lxmert_perturb_text: where the S x B perturbed sequences of a batch land in the flat
// output buffers.  No HIP header, so a plain host compiler builds it (tools/host/text_placement_main.cpp checks it by brute force on
// small tables against the sets of elements the sequences occupy).
//
// place[s] = {base_s, stride_s, width_s}: sequence (s, b) occupies the elements base_s + b * stride_s + [0, width_s), b = 0 .. B - 1.
#pragma once
#include <stdint.h>

namespace mmx {

enum TextPlaceError {
    TEXT_PLACE_OK = 0,
    TEXT_PLACE_WIDTH,      // width_s outside 1 .. T
    TEXT_PLACE_STRIDE,     // stride_s < width_s: the sequences of one step would overlap
    TEXT_PLACE_BASE,       // base_s < 0
    TEXT_PLACE_OVERRUN,    // the last sequence of a step ends past out_elems
    TEXT_PLACE_OVERLAP,    // two steps that are neither interleaved legally nor apart
};

// one past the last element of step s: base + (B - 1) * stride + width (the caller has bounded it by out_elems: no overflow)
inline int64_t text_place_end(const int64_t* p, int B) { return p[0] + static_cast<int64_t>(B - 1) * p[1] + p[2]; }

// Two steps are accepted only if (a) they have the same stride and their windows [base mod stride, + width) are disjoint within a
// period WITHOUT wrapping past it, or (b) their overall ranges [base, end) are disjoint.  Both are sufficient for the element sets to
// be disjoint; with B == 1 rule (b) is also necessary.
inline bool text_steps_apart(const int64_t* a, const int64_t* b, int B) {
    if (text_place_end(a, B) <= b[0] || text_place_end(b, B) <= a[0]) return true;          // (b)
    if (a[1] != b[1]) return false;
    const int64_t ra = a[0] % a[1], rb = b[0] % b[1];                                        // (a): stride >= width >= 1, base >= 0
    if (ra + a[2] > a[1] || rb + b[2] > b[1]) return false;
    return ra + a[2] <= rb || rb + b[2] <= ra;
}

// The whole table (S steps of three int64 each).  TEXT_PLACE_OK, or the first failed rule with the step(s) in *s0 / *s1 (s1 = -1 when
// the rule concerns one step).  B >= 1, T >= 1, S >= 1 and out_elems are the caller's (checked there).
inline TextPlaceError check_text_placement(const int64_t* place, int S, int B, int T, int64_t out_elems, int* s0, int* s1) {
    *s1 = -1;
    for (int s = 0; s < S; ++s) {
        const int64_t* p = place + 3 * s;
        *s0 = s;
        if (p[2] < 1 || p[2] > T) return TEXT_PLACE_WIDTH;
        if (p[1] < p[2]) return TEXT_PLACE_STRIDE;
        if (p[0] < 0) return TEXT_PLACE_BASE;
        // base + (B - 1) * stride + width <= out_elems, without forming a product that could overflow
        if (out_elems < 0 || p[0] > out_elems || p[2] > out_elems - p[0]) return TEXT_PLACE_OVERRUN;
        if (B > 1 && p[1] > (out_elems - p[0] - p[2]) / (B - 1)) return TEXT_PLACE_OVERRUN;
    }
    for (int s = 0; s < S; ++s)
        for (int t = s + 1; t < S; ++t)
            if (!text_steps_apart(place + 3 * s, place + 3 * t, B)) {
                *s0 = s;
                *s1 = t;
                return TEXT_PLACE_OVERLAP;
            }
    return TEXT_PLACE_OK;
}

}  // namespace mmx
