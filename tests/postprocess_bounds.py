"""Definitions, worst-case rounding bounds, case tables and mutants for the two kernels of ``csrc/postprocess_kernels.hip``: the heat map
(``heatmap_kernel``: bilinear upsample of a ``g x g`` patch map to ``S x S`` + min-max) and the Otsu mask (``otsu_kernel``: min-max to 8-bit
levels, Otsu's threshold, binary mask).  CPU only (numpy): ``tests/test_postprocess_bounds_host.py`` proves the bounds and the tables here,
``tests/test_gpu_postprocess_bounds.py`` holds the kernels to them.  ``u = 2**-24`` is the unit roundoff of fp32.

Heat map -- definition.  The source coordinates belong to the definition (they decide which patches a pixel blends), so they are restated
in fp32 as ATen's ``upsample_bilinear2d(align_corners=False)`` and the kernel compute them:

    scale = f32(g) / f32(S);   f = max(0, (d + 0.5) * scale - 0.5);   i0 = int(f), i1 = i0 + (i0 < g - 1);   l = f - i0 (exact), h = 1 - l

(``coords``), where ``(d + 0.5) * scale - 0.5`` is ONE fused multiply-add, rounded once.  That is what ``hipcc`` makes of the line (the kernel
spells it ``fmaf`` so that it does not hang on a compiler default) and what ATen's vectorised CPU kernels, built with FMA, compute as well;
rounding the product first moves ``f`` by up to an ulp of the product -- up to ``32 u`` in ``l`` at ``g = 64``, several bounds -- on a few
coordinates of a non-dyadic ``g / S`` (``coords(..., "rounded_twice")``; the host test tells which of the two the ATen build at hand uses).  From those fp32 weights and the fp32 patches ``a b / c d`` the value ``v = hy (hx a + lx b) + ly (hx c + lx d)`` and the output
``(v - min v) / (max v - min v)`` are evaluated in float64 (``heatmap_ref``).

Heat map -- bound, counted.  The deepest path of ``v`` in fp32 is the term ``hy hx a``: the rounding of ``hx = 1 - lx`` (1), the product ``hx a`` (2),
its sum with ``lx b`` (3), the rounding of ``hy = 1 - ly`` (4), the product with ``hy`` (5), the last sum (6).  The terms with ``lx`` or ``ly`` carry one
rounding fewer each (``l`` is exact).  ``hipcc`` contracts ``x * y + z`` by default and the kernel spells its multiply-adds as ``fmaf``
(``fma(hy, fma(hx, a, lx b), ly fma(hx, c, lx d))``: 4 roundings on that path); every contraction REMOVES a rounding, so ``k = 6`` covers the
separate and every fused evaluation order.  With ``gamma_k = k u / (1 - k u)`` (the rigorous form of ``k u``):

    e_v = gamma_6 (hy (hx |a| + lx |b|) + ly (hx |c| + lx |d|)),    e = max e_v over the map,
    |out - out64| <= ((e_v + e) + |out64| 2 e) / (range - 2 e) + 3 u |out64|

-- the computed minimum and maximum are each within ``e`` of the true ones, the computed range within ``2 e``, and ``hi - lo``, ``v - lo`` and the
division round once each (the form of the min-max steps in DESIGN.md, LXMERT baselines).  Where ``range <= 2 e`` the pixel is unjudged (infinite
bound); outside the ``constant`` family and ``g = 1`` (one patch IS a constant map) no pixel of the tables is.

Heat map -- identities without a tolerance.  Both passes of the kernel compute the same bits of ``v``, so the pixel that gave ``lo`` comes out as
``0 / range = 0.0`` and the one that gave ``hi`` as ``range / range = 1.0``, exactly.  At ``S = g`` the coordinates are integers, ``v`` is the patch
itself and the output has the bits of the fp32 ``(in - lo) / range``.

Otsu -- definition.  The level is ``mask_generator.py:116`` in fp32, every operation rounded: ``int(((c - lo) / range) * 255)``, truncated
(``otsu_levels``); the threshold is OpenCV's ``getThreshVal_Otsu_8u`` recurrence in float64, every operation rounded (``otsu_restatement``); the
mask is ``level > threshold -> 255``.  All three are judged bit for bit.  Independently of the restated recurrence the threshold is judged
against the definition of Otsu's method: the exhaustive float64 maximiser of the between-class variance (``between_class_variance``), lowest
level on ties.  The recurrence's ``FLT_EPSILON`` guard (skip a level while a class holds less than 2**-23 of the pixels) cannot act below
``n = 2**23`` pixels, where one pixel already is a larger share; it is left unpinned.

Special values -- the contract both kernels state.  ``lo`` / ``hi`` are taken with ``fmin`` / ``fmax``: a NaN pixel does not move them.

* ``range = 0``: the heat map is all NaN (``0 / 0``, as in the reference); Otsu (constant map, ``n = 1``) has every level 0, threshold 0 and an
  all-zero mask.  For the heat map it is the range of the UPSAMPLED fp32 map that counts.  A constant patch map (``g = 1`` is one) has it 0
  for certain at ``S = g`` (``v`` is the patch) and when the constant is 0; elsewhere ``h a + l a`` need not round to ``a``, the range may be an
  ulp of ``a``, and the output is that rounding noise stretched to [0, 1] -- in the reference's own ``interpolate`` as well.  Such a map is
  pinned on what holds either way (``degenerate_map_ok``): all NaN, or no NaN at all with minimum 0.0 and maximum 1.0.
* NaN pixel: a heat-map pixel with a NaN among its four taps (a tap of weight 0 included: ``0 * NaN``) is NaN, every other pixel is what it is
  without the NaN patch in the extremes; an Otsu NaN pixel is level 0 and mask 0.  The reference (numpy ``min`` / ``max``) would make the whole
  map NaN: a documented deviation.
* +-inf pixel: pinned on what the rules above give, as the restatement and the float64 reference compute it.  Heat map: a pixel that taps
  the infinite patch with a weight of 0 anywhere in its blend is NaN (``0 * inf``; at ``S = g`` that is every pixel tapping it, and the other
  pixels are judged as ever); where ``v`` itself is infinite the range is, and every finite pixel is ``x / inf = 0`` for ``+inf`` and
  ``inf / inf = NaN`` for ``-inf``.  Otsu: ``range`` is infinite, all levels 0, threshold 0, mask 0.

Mutants are restatements in this module (``HEATMAP_MUTANTS``, ``OTSU_MUTANTS``)."""
import functools
import math

import numpy as np

U = 2.0 ** -24
K_ROUNDINGS = 6
F32 = np.float32
GAMMA = K_ROUNDINGS * U / (1 - K_ROUNDINGS * U)


# ---------------------------------------------------------------------------------------------------------------------
# heat map
# ---------------------------------------------------------------------------------------------------------------------
def coords(g, S, how="half_pixel"):
    """``i0 i1`` (int64) and ``l h`` (fp32) of the ``S`` destination indices along one axis.  ``how`` other than ``half_pixel``: the
    coordinate mutants."""
    d = np.arange(S, dtype=F32)
    half = F32(0.5)
    if how == "half_pixel":              # one fma: the product of two fp32 is exact in float64, and so is the difference up to its rounding
        f = ((d + half).astype(np.float64) * np.float64(F32(g) / F32(S)) - 0.5).astype(F32)
        f = np.maximum(f, F32(0))
    elif how == "rounded_twice":         # no coordinate of the kernel's: an ATen built without FMA
        f = np.maximum((d + half) * (F32(g) / F32(S)) - half, F32(0))
    elif how == "align_corners":
        f = d * (F32(g - 1) / F32(S - 1) if S > 1 else F32(0))
    elif how == "no_clamp":
        f = (d + half) * (F32(g) / F32(S)) - half
    elif how == "no_shift":
        f = d * (F32(g) / F32(S))
    elif how == "inverted_scale":
        f = np.maximum((d + half) * (F32(S) / F32(g)) - half, F32(0))
    else:
        raise KeyError(how)
    f = f.astype(F32)
    i0 = np.minimum(np.trunc(f).astype(np.int64), g - 1)            # the minimum acts in the mutants only
    i1 = i0 + (i0 < g - 1)
    l = (f - i0.astype(F32)).astype(F32)
    h = (F32(1) - l).astype(F32)
    return i0, i1, l, h


def _taps(src, g, S, how="half_pixel", i1_wraps=False):
    """The four taps ``a b c d`` ``[S, S]`` of one ``[g, g]`` map and the weights ``hy ly [S, 1]``, ``hx lx [1, S]``."""
    i0, i1, l, h = coords(g, S, how)
    flat = src.reshape(-1)
    if i1_wraps:                         # mutant: i0 + 1 whatever the edge -> the next row / the first row again
        i1 = i0 + 1
    y0, y1, x0, x1 = i0[:, None], i1[:, None], i0[None, :], i1[None, :]
    n = g * g
    a, b, c, d = (flat[(y * g + x) % n] for y, x in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    return (a, b, c, d), (h[:, None], l[:, None], h[None, :], l[None, :])


def _blend64(taps, w):
    a, b, c, d = (t.astype(np.float64) for t in taps)
    hy, ly, hx, lx = (t.astype(np.float64) for t in w)
    with np.errstate(invalid="ignore"):
        return hy * (hx * a + lx * b) + ly * (hx * c + lx * d)


def _extremes(v):
    """``fmin`` / ``fmax`` over the map: a NaN does not move them; +inf / -inf of an all-NaN map, as in the kernel."""
    flat = v.reshape(-1)
    return np.fmin.reduce(flat, initial=np.inf), np.fmax.reduce(flat, initial=-np.inf)


def _minmax(v, lo, hi):
    with np.errstate(invalid="ignore", divide="ignore"):
        return (v - lo) / (hi - lo)


def heatmap_ref(src, S, how="half_pixel"):
    """``src [B, g, g]`` fp32 -> dict of float64 ``[B, S, S]``: ``v``, ``out``, ``bound`` (inf where unjudged), and ``range``, ``e`` ``[B]``."""
    src = np.ascontiguousarray(src, F32)
    B, g = src.shape[0], src.shape[1]
    out = {k: np.empty((B, S, S)) for k in ("v", "out", "bound")}
    out["range"], out["e"] = np.empty(B), np.empty(B)
    for b in range(B):
        taps, w = _taps(src[b], g, S, how)
        v = _blend64(taps, w)
        with np.errstate(invalid="ignore"):
            e_v = GAMMA * _blend64([np.abs(t) for t in taps], w)
        lo, hi = _extremes(v)
        o = _minmax(v, lo, hi)
        fin = np.isfinite(e_v)
        e = float(e_v[fin].max()) if fin.any() else math.nan
        with np.errstate(invalid="ignore", divide="ignore"):
            rng = hi - lo
            bound = ((e_v + e) + np.abs(o) * 2 * e) / (rng - 2 * e) + 3 * U * np.abs(o)
        if not rng > 2 * e:
            bound = np.full_like(bound, np.inf)
        out["v"][b], out["out"][b], out["bound"][b], out["range"][b], out["e"][b] = v, o, bound, rng, e
    return out


def heatmap_ratio(got, ref):
    """Worst error / bound over the judged pixels; inf if the NaN pattern differs from the reference's or a judged pixel is not finite.
    An unjudged pixel (infinite bound) counts 0."""
    got = np.asarray(got, np.float64)
    want, bound = ref["out"], ref["bound"]
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return math.inf
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    err = np.abs(got[ok] - want[ok])
    if not np.isfinite(err).all():
        return math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound[ok])
    return float(r.max())


def unjudged(ref):
    """Pixels that have a value in the reference and no finite bound."""
    return int((~np.isnan(ref["out"]) & ~np.isfinite(ref["bound"])).sum())


def all_nan_by_definition(ref, b):
    """Map ``b`` has ``range = 0`` in float64 already -- ``onehot`` at ``S < g`` when no pixel taps the hot patch (64 -> 20, image 0): all NaN,
    and nothing for the min / max identity to hold on."""
    return bool(np.isnan(ref["out"][b]).all())


def _fma(a, b, c):
    """``a * b + c`` rounded once to fp32, through float64 (the product of two fp32 is exact there)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def heatmap_restatement(src, S, fused=False, how="half_pixel"):
    """The kernel in numpy fp32: ``v`` with separate multiplies and adds, or with each ``x * y + z`` rounded once; ``fmin`` / ``fmax`` extremes;
    ``(v - lo) / range``.  -> ``out [B, S, S]`` fp32."""
    src = np.ascontiguousarray(src, F32)
    B, g = src.shape[0], src.shape[1]
    out = np.empty((B, S, S), F32)
    for b in range(B):
        (a, bb, c, d), (hy, ly, hx, lx) = _taps(src[b], g, S, how)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if fused:
                v = _fma(hy, _fma(hx, a, lx * bb), ly * _fma(hx, c, lx * d))          # the kernel's own spelling
            else:
                v = hy * (hx * a + lx * bb) + ly * (hx * c + lx * d)
            assert v.dtype == F32
            lo, hi = _extremes(v)
            out[b] = (v - F32(lo)) / (F32(hi) - F32(lo))
    return out


def identity_at_S_equal_g(src):
    """The bits the output must have at ``S = g``: the fp32 ``(in - lo) / range``."""
    src = np.ascontiguousarray(src, F32)
    out = np.empty_like(src)
    for b in range(src.shape[0]):
        lo, hi = _extremes(src[b])
        with np.errstate(invalid="ignore", divide="ignore"):
            out[b] = (src[b] - F32(lo)) / (F32(hi) - F32(lo))
    return out


def same_bits(a, b):
    """Bit for bit; a NaN matches a NaN whatever its payload."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(((a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))).all())


HEATMAP_FAMILIES = ("randn", "ramp", "onehot", "negative", "offset", "relevancy", "constant", "nan_pixel", "inf_pixel")
# (g, S, B).  Every g of {1, 2, 3, 7, 14, 24, 32, 33, 63, 64}; S < g (14 -> 9, 64 -> 20 and more), S = g, S = 2 g, S = 16 g (14 -> 224,
# 24 -> 336), a non-multiple (7 -> 30); S * S = 81 (fewer pixels than threads), 1024 (S = 32), 1089 (S = 33: a tail of 65); g * g > 1024 (the
# staging loop) from g = 33 on; B in {1, 3, 5}.
HEATMAP_SHAPES = ((1, 1, 3), (1, 5, 1), (2, 2, 5), (2, 4, 1), (2, 9, 3), (2, 32, 5), (3, 3, 1), (3, 6, 3), (3, 33, 5), (3, 48, 1),
                  (7, 5, 3), (7, 7, 5), (7, 14, 1), (7, 30, 3), (7, 112, 1), (14, 9, 5), (14, 14, 3), (14, 28, 1), (14, 224, 3),
                  (24, 24, 1), (24, 48, 5), (24, 336, 1), (32, 32, 3), (32, 33, 5), (32, 64, 1), (33, 20, 1), (33, 33, 3), (33, 66, 5),
                  (63, 40, 3), (63, 63, 1), (63, 126, 3), (64, 20, 5), (64, 64, 1), (64, 128, 3))
HEATMAP_GROUPS = {"g1-3": (1, 2, 3), "g7": (7,), "g14-24": (14, 24), "g32-33": (32, 33), "g63-64": (63, 64)}


def heatmap_shapes(group):
    return [s for s in HEATMAP_SHAPES if s[0] in HEATMAP_GROUPS[group]]


@functools.lru_cache(maxsize=None)
def heatmap_case(family, g, S, B):
    """``[B, g, g]`` fp32 patch maps of one family, every image with its own scale and offset; a function of its arguments only."""
    rng = np.random.default_rng([HEATMAP_FAMILIES.index(family), g, S, B])
    yy, xx = np.meshgrid(np.arange(g, dtype=np.float64), np.arange(g, dtype=np.float64), indexing="ij")
    out = np.empty((B, g, g), F32)
    for b in range(B):
        n = rng.standard_normal((g, g))
        amp, off = 1.0 + 0.5 * b, 0.75 * b
        if family == "randn":
            x = amp * n + off
        elif family == "ramp":
            x = amp * (3.0 * xx + yy) + off
        elif family == "onehot":             # a corner, an edge, the interior, then the other corner and edge
            spots = ((0, 0), (0, g // 2), (g // 2, g // 2), (g - 1, g - 1), (g // 2, g - 1))
            x = np.zeros((g, g))
            x[spots[b % 5]] = amp
        elif family == "negative":
            x = -amp * np.abs(n) - off - 0.1
        elif family == "offset":             # cancellation in v - lo.  e = 6 u 1e3 = 3.6e-4: an amplitude of 0.3 keeps range >> 2 e on 4 patches too
            x = 1e3 + 0.3 * amp * n
        elif family == "relevancy":
            x = np.abs(rng.standard_cauchy((g, g))) * 1e-4 * amp
        elif family == "constant":
            x = np.full((g, g), 0.1 * b)             # image 0: all zeros, where v is exactly 0 at every S
        elif family in ("nan_pixel", "inf_pixel"):
            x = amp * n + off
            at = ((0, 0), (g // 2, g // 3), (g - 1, g - 1))[b % 3]
            x[at] = np.nan if family == "nan_pixel" else (np.inf, -np.inf)[(b // 3) % 2]
        else:
            raise KeyError(family)
        out[b] = x
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def heatmap_case_ref(family, g, S, B):
    """The reference of a table row, computed once and shared."""
    ref = heatmap_ref(heatmap_case(family, g, S, B), S)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def degenerate(family, g):
    """Rows whose every patch map is constant: no bound applies (module docstring, special values)."""
    return family == "constant" or g == 1


def degenerate_map_ok(got, src, S):
    """One ``[S, S]`` output of a constant ``[g, g]`` patch map: all NaN where the upsampled range is 0 for certain (``S = g``, a zero map, a
    non-finite constant); else all NaN, or free of NaN with minimum 0.0 and maximum 1.0."""
    got, src = np.asarray(got), np.asarray(src)
    if np.isnan(got).all():
        return True
    certain = S == src.shape[-1] or not np.isfinite(src).all() or not src.any()
    return not certain and not np.isnan(got).any() and got.min() == 0.0 and got.max() == 1.0


# Mutants: wrong float64 heat maps.  name -> f(src [B, g, g], S) -> [B, S, S]
def _mutant(how="half_pixel", transpose=False, i1_wraps=False, nearest=False, extremes="map", divide_by_hi=False):
    def run(src, S):
        src = np.ascontiguousarray(src, F32)
        B, g = src.shape[0], src.shape[1]
        vs = []
        for b in range(B):
            taps, w = _taps(src[b].T.copy() if transpose else src[b], g, S, how, i1_wraps)
            vs.append(taps[0].astype(np.float64) if nearest else _blend64(taps, w))
        out = np.empty((B, S, S))
        for b in range(B):
            over = {"map": vs[b], "patches": src[b].astype(np.float64), "first_1024": vs[b].reshape(-1)[:1024], "batch": np.stack(vs)}
            lo, hi = _extremes(over[extremes])
            with np.errstate(invalid="ignore", divide="ignore"):
                out[b] = (vs[b] - lo) / hi if divide_by_hi else _minmax(vs[b], lo, hi)
        return out
    return run


HEATMAP_MUTANTS = {
    "align_corners_coordinates": _mutant(how="align_corners"),
    "no_clamp_at_0": _mutant(how="no_clamp"),
    "no_half_pixel_shift": _mutant(how="no_shift"),
    "inverted_scale": _mutant(how="inverted_scale"),
    "transposed_taps": _mutant(transpose=True),
    "i1_not_clamped": _mutant(i1_wraps=True),
    "nearest_tap": _mutant(nearest=True),
    "extremes_over_the_patch_grid": _mutant(extremes="patches"),
    "extremes_over_the_first_1024_pixels": _mutant(extremes="first_1024"),
    "division_by_hi": _mutant(divide_by_hi=True),
    "extremes_shared_across_the_batch": _mutant(extremes="batch"),
}


# ---------------------------------------------------------------------------------------------------------------------
# Otsu
# ---------------------------------------------------------------------------------------------------------------------
def between_class_variance(img):
    """sigma_b^2(t) for t = 0..255, classes {<= t} / {> t}, float64; -inf where a class is empty."""
    hist = np.bincount(img.reshape(-1), minlength=256).astype(np.float64)
    p = hist / hist.sum()
    lv = np.arange(256, dtype=np.float64)
    out = np.full(256, -np.inf)
    for t in range(256):
        q1, q2 = p[:t + 1].sum(), p[t + 1:].sum()
        if q1 <= 0 or q2 <= 0:
            continue
        mu1, mu2 = (lv[:t + 1] * p[:t + 1]).sum() / q1, (lv[t + 1:] * p[t + 1:]).sum() / q2
        out[t] = q1 * q2 * (mu1 - mu2) ** 2
    return out


def exhaustive_threshold(levels):
    """The lowest level that maximises the between-class variance (ties: within 1e-12 of the maximum, the rounding of the sums), or None
    for a histogram with one occupied level."""
    sigma = between_class_variance(np.asarray(levels))
    best = sigma.max()
    if not np.isfinite(best):
        return None
    return int(np.nonzero(sigma >= best * (1 - 1e-12))[0][0])


def otsu_extremes(c, nan_counts=False):
    c = np.asarray(c, F32).reshape(-1)
    if nan_counts:
        with np.errstate(invalid="ignore"):
            return c.min(), c.max()
    return F32(np.fmin.reduce(c, initial=np.inf)), F32(np.fmax.reduce(c, initial=-np.inf))


def otsu_levels(c, lo, hi, how="truncate"):
    """fp32 ``(c - lo) / range * 255`` -> int levels 0..255; NaN -> 0, the rest clamped then converted."""
    c = np.asarray(c, F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rng = F32(hi) - F32(lo)
        if how == "reciprocal":
            v = (c - lo) * (F32(255) / rng)
        else:
            v = (c - lo) / rng * F32(255)
    assert v.dtype == F32
    v = np.where(np.isnan(v), F32(0), np.clip(v, F32(0), F32(255)))
    return (np.rint(v) if how == "round" else np.trunc(v)).astype(np.int64)


def otsu_threshold(hist, n, last_wins=False, fp32=False):
    """OpenCV ``getThreshVal_Otsu_8u``: float64, every operation rounded, the first maximum of the between-class variance."""
    T = F32 if fp32 else float           # a Python float is an IEEE double, each operation rounded once
    scale = T(1.0) / T(n)
    mu = T(0)
    for i in range(256):
        mu = T(mu + T(i) * T(hist[i]))
    mu = T(mu * scale)
    mu1, q1, max_sigma, max_val = T(0), T(0), T(0), 0
    eps = T(np.finfo(np.float32).eps)
    for i in range(256):
        p_i = T(T(hist[i]) * scale)
        mu1 = T(mu1 * q1)
        q1 = T(q1 + p_i)
        q2 = T(T(1) - q1)
        if min(q1, q2) < eps or max(q1, q2) > T(1) - eps:
            continue
        mu1 = T(T(mu1 + T(T(i) * p_i)) / q1)
        mu2 = T(T(mu - T(q1 * mu1)) / q2)
        sigma = T(T(T(q1 * q2) * T(mu1 - mu2)) * T(mu1 - mu2))
        if (sigma >= max_sigma) if last_wins else (sigma > max_sigma):
            max_sigma, max_val = sigma, i
    return max_val


def otsu_restatement(cams, levels="truncate", ge_mask=False, last_wins=False, drop_tail=False, fp32=False, shared_extremes=False,
                     nan_counts=False):
    """``cams [K, n]`` fp32 -> ``masks [K, n]`` fp32 in {0, 255}, ``thresholds [K]`` int32, ``levels [K, n]``.  The keyword arguments are
    the mutants."""
    cams = np.ascontiguousarray(cams, F32)
    K, n = cams.shape
    masks, thr, lev = np.empty((K, n), F32), np.empty(K, np.int32), np.empty((K, n), np.int64)
    for k in range(K):
        lo, hi = otsu_extremes(cams[0 if shared_extremes else k], nan_counts)
        q = otsu_levels(cams[k], lo, hi, levels)
        counted = q[:n - n % 256] if drop_tail else q
        t = otsu_threshold(np.bincount(counted, minlength=256), n, last_wins, fp32)
        masks[k] = np.where((q >= t) if ge_mask else (q > t), F32(255), F32(0))
        thr[k], lev[k] = t, q
    return masks, thr, lev


OTSU_FAMILIES = ("bimodal", "skewed", "relevancy", "two_levels", "three_levels", "symmetric_tie", "lattice", "near_tie", "constant",
                 "nan_pixel", "inf_pixel")
OTSU_NS = (1, 2, 3, 255, 256, 257, 950, 1000, 4099)
OTSU_KS = (1, 6)
SYMMETRIC_TIE = (0.0, 0.0, 1.0, 1.0, 0.5, 0.5, 0.25, 0.75)           # the row of tests/test_otsu_property.py


def _lattice(lo, rng):
    """``lo``, ``hi = lo + rng`` and, for every k = 1..255, the LAST float of a level below k and the FIRST float of level k of the fp32 level
    expression itself (bisection: the level is monotone in the pixel), plus the fp32 ``lo + rng k / 255`` -- every pixel on a level
    boundary or next to one.  3 * 255 + 2 pixels."""
    lo = F32(lo)
    hi = F32(lo + F32(rng))
    k = np.arange(1, 256)
    below, above = np.full(255, lo, F32), np.full(255, hi, F32)            # level(below) < k <= level(above)
    while True:
        mid = ((below.astype(np.float64) + above.astype(np.float64)) / 2).astype(F32)
        open_ = (mid > below) & (mid < above)
        if not open_.any():
            break
        up = otsu_levels(mid, lo, hi) >= k
        above = np.where(open_ & up, mid, above)
        below = np.where(open_ & ~up, mid, below)
    assert (np.nextafter(below, F32(np.inf)) == above).all()
    on = (lo + (hi - lo) * k.astype(F32) / F32(255)).astype(F32)
    return np.concatenate([[lo, hi], below, above, np.clip(on, lo, hi)]).astype(F32)


# pixel counts at the levels (0, 128, 255) of n = 4099 whose two candidate splits differ by 3e-9 ... 1e-8 of the between-class variance:
# far above the rounding of the float64 recurrence, below that of an fp32 one (which picks the other split on the first four)
NEAR_TIES = ((1544, 66, 2489), (1217, 34, 2848), (1596, 76, 2427), (661, 13, 3425), (1308, 40, 2751), (1544, 66, 2489))


def otsu_ns(family):
    """The pixel counts a family is tabled at: ``symmetric_tie``, ``lattice`` and ``near_tie`` have their own."""
    if family == "symmetric_tie":
        return (len(SYMMETRIC_TIE),)
    if family == "lattice":
        return (3 * 255 + 2,)
    if family == "near_tie":
        return (sum(NEAR_TIES[0]),)
    return OTSU_NS


@functools.lru_cache(maxsize=None)
def otsu_case(family, n, K):
    """``[K, n]`` fp32 maps of one family, every map with its own extremes; a function of its arguments only."""
    rng = np.random.default_rng([OTSU_FAMILIES.index(family), n, K])
    out = np.empty((K, n), F32)
    for k in range(K):
        amp, off = 1.0 + 0.5 * k, 0.3 * k
        if family == "bimodal":
            low = rng.normal(0.2, 0.05, n)
            x = np.where(rng.random(n) < 0.63, low, rng.normal(0.8, 0.07, n))
        elif family == "skewed":
            x = rng.gamma(2.0, 1.0, n)
        elif family == "relevancy":
            x = np.abs(rng.standard_cauchy(n)) * 1e-4
        elif family == "two_levels":
            x = rng.choice([0.0, 1.0], size=n, p=[0.7, 0.3])
        elif family == "three_levels":
            x = rng.choice([0.0, 0.4, 1.0], size=n, p=[0.5, 0.3, 0.2])
        elif family == "symmetric_tie":
            x = np.array(SYMMETRIC_TIE)
        elif family == "lattice":
            out[k] = rng.permutation(_lattice((0.0, 0.3, -1.7, 1e3, 1e-4, -0.2)[k], (1.0, 1.5, 3.1, 7.0, 2.5e-4, 0.2)[k]))
            continue
        elif family == "near_tie":
            x = rng.permutation(np.repeat([0.0, 128.5 / 255, 1.0], NEAR_TIES[k]))
        elif family == "constant":
            x = np.full(n, 0.25)
        elif family in ("nan_pixel", "inf_pixel"):
            x = rng.gamma(2.0, 1.0, n)
            bad = np.nan if family == "nan_pixel" else (np.inf, -np.inf)[k % 2]
            x[(0, n // 2, n - 1)[k % 3]] = bad
        out[k] = amp * x + off if family != "relevancy" else amp * x
    out.setflags(write=False)
    return out


def otsu_rows():
    return [(f, n, K) for f in OTSU_FAMILIES for n in otsu_ns(f) for K in OTSU_KS]


OTSU_MUTANTS = {
    "round_to_nearest_levels": dict(levels="round"),
    "multiply_by_255_over_range": dict(levels="reciprocal"),
    "mask_greater_or_equal": dict(ge_mask=True),
    "last_maximiser_wins": dict(last_wins=True),
    "histogram_without_the_tail": dict(drop_tail=True),
    "fp32_recurrence": dict(fp32=True),
    "extremes_of_map_0_for_every_map": dict(shared_extremes=True),
    "nan_counted_into_the_extremes": dict(nan_counts=True),
}
