// The 8-bit level of one pixel in otsu_kernel, and the size limits of the two post-processing entries.  Plain C++ that a host compiler
// takes as well: tools/check_postprocess_level.py compiles it alone and runs it over NaN, infinite and out-of-range values.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define MMX_PP_HD __host__ __device__
#else
#define MMX_PP_HD
#endif

namespace mmx {

// DETR/mask_generator.py:116 + astype(uint8): (c - lo) / range * 255 in fp32, truncated.  A float that is NaN or outside the range of int has
// no defined conversion in C++, so the value is brought into [0, 255] first: fmaxf(NaN, 0) is 0, hence a NaN (a NaN pixel, or 0 / 0 of a
// constant map, or inf / inf) is level 0.  On a finite value in [0, 255] the two clamps are the identity and the bits are those of the
// bare cast.
MMX_PP_HD inline int otsu_level(float c, float lo, float range) {
    const float v = (c - lo) / range * 255.f;
    return static_cast<int>(fminf(fmaxf(v, 0.f), 255.f));
}

// heatmap_kernel counts pixels in int: p < S * S, p / S, p % S.  46340^2 = 2147395600 is the last square below 2^31, and leaves room for the
// stride of 1024.
constexpr int kHeatmapMaxSide = 46340;
// otsu_kernel steps an int by 256 up to n: the last step must not pass 2^31 - 1.
constexpr int kOtsuMaxPixels = 2147483647 - 256;

}  // namespace mmx
