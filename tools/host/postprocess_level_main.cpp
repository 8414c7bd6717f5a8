// Stand-alone host check of csrc/postprocess_level.h (tools/check_postprocess_level.py compiles and runs it; no GPU, no HIP header).
// otsu_level is compared with
//   * the bare cast it replaced, static_cast<int>((c - lo) / range * 255.f) clamped to [0, 255], on every value where that cast is
//     defined: a grid over [lo, hi] of six maps and the floats next to each level boundary;
//   * the stated answer where it is not: NaN pixel, 0 / 0 of a constant map, inf / inf -> 0; above the range -> 255; below -> 0.
// Exit status 0 and "postprocess_level: ok", or 1 after the first mismatches.
#include <stdio.h>

#include <limits>

#include "postprocess_level.h"

static int failures = 0;

static void expect(float c, float lo, float range, int want, const char* what) {
    const int got = mmx::otsu_level(c, lo, range);
    if (got != want && ++failures <= 10) printf("MISMATCH %s: c=%a lo=%a range=%a -> %d, expected %d\n", what, c, lo, range, got, want);
}

// the expression as it stood in otsu_kernel: defined for a finite value inside the range of int only
static int former(float c, float lo, float range) {
    const float v = (c - lo) / range * 255.f;
    const int q = static_cast<int>(v);
    return q < 0 ? 0 : (q > 255 ? 255 : q);
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const float los[6] = {0.f, 0.3f, -1.7f, 1e3f, 1e-4f, -0.2f}, ranges[6] = {1.f, 1.5f, 3.1f, 7.f, 2.5e-4f, 0.2f};
    long cases = 0;
    for (int m = 0; m < 6; ++m) {
        const float lo = los[m], hi = lo + ranges[m], range = hi - lo;
        for (int i = 0; i <= 100000; ++i) {
            float c = lo + range * (static_cast<float>(i) / 100000.f);
            c = c < lo ? lo : (c > hi ? hi : c);
            expect(c, lo, range, former(c, lo, range), "grid");
            ++cases;
        }
        for (int k = 0; k <= 255; ++k) {
            float c = lo + range * static_cast<float>(k) / 255.f;
            for (int step = -3; step <= 3; ++step) {
                float x = c;
                for (int s = 0; s < (step < 0 ? -step : step); ++s) x = nextafterf(x, step < 0 ? -inf : inf);
                if (x < lo || x > hi) continue;
                expect(x, lo, range, former(x, lo, range), "level boundary");
                ++cases;
            }
        }
        expect(lo, lo, range, 0, "lo");
        expect(hi, lo, range, 255, "hi");
        // outside the defined conversion
        expect(nan, lo, range, 0, "NaN pixel");
        expect(lo, lo, 0.f, 0, "0 / 0");
        expect(hi, lo, 0.f, 255, "x / 0");
        expect(inf, lo, inf, 0, "inf / inf");
        expect(-inf, lo, inf, 0, "-inf / inf");
        expect(hi, lo, inf, 0, "x / inf");
        expect(lo, -inf, inf, 0, "inf / inf (lo = -inf)");
        expect(3e38f, lo, range, 255, "above the range of int");
        expect(-3e38f, lo, range, 0, "below the range of int");
        expect(inf, lo, range, 255, "+inf over a finite range");
        expect(-inf, lo, range, 0, "-inf over a finite range");
        expect(hi + 2.f * range, lo, range, 255, "above 255");
        expect(lo - range, lo, range, 0, "below 0");
        cases += 15;
    }
    static_assert(static_cast<long long>(mmx::kHeatmapMaxSide) * mmx::kHeatmapMaxSide + 1024 <= 2147483647LL, "S * S + stride fits an int");
    static_assert(static_cast<long long>(mmx::kHeatmapMaxSide + 1) * (mmx::kHeatmapMaxSide + 1) > 2147483647LL, "and the next side does not");
    static_assert(static_cast<long long>(mmx::kOtsuMaxPixels) + 256 <= 2147483647LL, "n + stride fits an int");
    printf("%ld cases, %d mismatches\n", cases, failures);
    if (failures) return 1;
    printf("postprocess_level: ok\n");
    return 0;
}
