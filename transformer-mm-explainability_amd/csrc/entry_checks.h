// Host-only arithmetic of the entry checks: sizes of workspace parts and the alias test of an entry's buffers.  No HIP header, so a
// plain host compiler builds it (tools/host/entry_checks_main.cpp checks it exhaustively on small ranges).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mmx {

// every part of a carved workspace starts 256-byte aligned
inline size_t align256(size_t n) { return (n + 255) & ~static_cast<size_t>(255); }

// [a, a + na) and [b, b + nb) share a byte (a null pointer overlaps nothing): the alias checks of the entries
inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (!a || !b) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + nb && b0 < a0 + na;
}

struct Span {
    const void* p;
    size_t bytes;
};

// an output overlaps an input, or an output overlaps a LATER output (inputs may overlap each other)
inline bool spans_alias(const Span* outs, int n_out, const Span* ins, int n_in) {
    bool alias = false;
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i) alias |= ranges_overlap(outs[o].p, outs[o].bytes, ins[i].p, ins[i].bytes);
        for (int p = o + 1; p < n_out; ++p) alias |= ranges_overlap(outs[o].p, outs[o].bytes, outs[p].p, outs[p].bytes);
    }
    return alias;
}

}  // namespace mmx
