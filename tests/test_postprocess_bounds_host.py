"""CPU: the bounds and the tables of ``tests/postprocess_bounds.py`` are sound before a kernel is held to them.

* fp32 restatements of the heat map (separate multiplies and adds; every ``a * b + c`` rounded once) and torch's CPU ``interpolate`` + fp32
  min-max are inside the bound at every table row, and the two identities hold for the restatements.
* Outside the constant maps no pixel of the tables is unjudged.
* Every heat-map mutant is at >= 2x a bound on some row; every Otsu mutant changes a mask bit or a threshold on some row.
* The restated Otsu threshold is the exhaustive maximiser's on every row with more than one occupied level.

The catching row of every mutant, and by how much, is printed (past pytest's capture)."""
import math

import numpy as np
import pytest
import torch

import postprocess_bounds as pb

JUDGED = [f for f in pb.HEATMAP_FAMILIES if f != "constant"]


def say(capsys, line):
    with capsys.disabled():
        print("\n  " + line, end="")


def minmax32(v):
    out = np.empty_like(v)
    for b in range(v.shape[0]):
        lo, hi = pb._extremes(v[b])
        with np.errstate(invalid="ignore", divide="ignore"):
            out[b] = (v[b] - np.float32(lo)) / (np.float32(hi) - np.float32(lo))
    return out


def torch_cpu_heatmap(src, S):
    B, g = src.shape[0], src.shape[1]
    v = torch.nn.functional.interpolate(torch.from_numpy(np.array(src)).reshape(B, 1, g, g), size=S, mode="bilinear")
    return minmax32(v.reshape(B, S, S).numpy())


@pytest.mark.parametrize("family", pb.HEATMAP_FAMILIES)
def test_fp32_heat_maps_meet_the_bound_and_the_identities(family, capsys):
    top = {"separate": 0.0, "fused": 0.0}
    for g, S, B in pb.HEATMAP_SHAPES:
        src, ref = pb.heatmap_case(family, g, S, B), pb.heatmap_case_ref(family, g, S, B)
        for name, fused in (("separate", False), ("fused", True)):
            got = pb.heatmap_restatement(src, S, fused)
            if pb.degenerate(family, g):
                assert all(pb.degenerate_map_ok(got[b], src[b], S) for b in range(B)), (family, g, S, name)
                continue
            assert pb.unjudged(ref) == 0, (family, g, S, B)
            r = pb.heatmap_ratio(got, ref)
            top[name] = max(top[name], r)
            assert r <= 1.0, (family, g, S, B, name, r)
            for b in range(B):
                if pb.all_nan_by_definition(ref, b):
                    assert np.isnan(got[b]).all()
                elif np.isfinite(ref["range"][b]):
                    assert np.nanmin(got[b]) == 0.0 and np.nanmax(got[b]) == 1.0, (family, g, S, b, name)
            if S == g and np.isfinite(src).all():    # a tap of weight 0 still carries a NaN / inf into its pixel
                assert pb.same_bits(got, pb.identity_at_S_equal_g(src)), (family, g, name)
            if family == "nan_pixel" and g > 2:      # exactly the pixels with a NaN tap are NaN, and some are not
                for b in range(B):
                    taps, _ = pb._taps(src[b], g, S)
                    assert np.array_equal(np.isnan(got[b]), np.isnan(taps[0] + taps[1] + taps[2] + taps[3])) and not np.isnan(got[b]).all()
    say(capsys, "heat map %-10s restatements, worst error / bound: separate %.3f  fused %.3f" % (family, top["separate"], top["fused"]))


def test_torch_cpu_interpolate_meets_the_bound(capsys):
    """ATen's source reads ``scale * (dst + 0.5) - 0.5``; whether its build rounds that once (FMA) or twice is the compiler's licence, so
    torch is held to the reference on ONE of the two coordinate forms -- the same on every row -- and the form is printed."""
    worst = {}
    for how in ("half_pixel", "rounded_twice"):
        top = 0.0
        for family in JUDGED:
            for g, S, B in pb.HEATMAP_SHAPES:
                if pb.degenerate(family, g) or family in ("nan_pixel", "inf_pixel"):     # ATen copies at S = g, and numpy-style
                    continue                                                             # extremes are the documented deviation
                src = pb.heatmap_case(family, g, S, B)
                if how == "half_pixel":
                    ref = pb.heatmap_case_ref(family, g, S, B)
                else:
                    if np.array_equal(pb.coords(g, S)[2], pb.coords(g, S, how)[2]):
                        continue
                    ref = pb.heatmap_ref(src, S, how)
                top = max(top, pb.heatmap_ratio(torch_cpu_heatmap(src, S), ref))
        worst[how] = top
    say(capsys, "heat map torch cpu interpolate + fp32 min-max, worst error / bound: coordinate rounded once %.3f, rounded twice %.3f"
        % (worst["half_pixel"], worst["rounded_twice"]))
    assert min(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mutant", sorted(pb.HEATMAP_MUTANTS))
def test_every_heat_map_mutant_is_at_twice_a_bound(mutant, capsys):
    wrong = pb.HEATMAP_MUTANTS[mutant]
    best, row, caught, pattern = 0.0, None, 0, 0
    for family in JUDGED:
        for g, S, B in pb.HEATMAP_SHAPES:
            if pb.degenerate(family, g):
                continue
            r = pb.heatmap_ratio(wrong(pb.heatmap_case(family, g, S, B), S), pb.heatmap_case_ref(family, g, S, B))
            caught += r >= 2.0
            pattern += r == math.inf                 # another NaN pattern, or a judged pixel that is not finite
            if best < r < math.inf:
                best, row = r, (family, g, S, B)
    say(capsys, "heat map mutant %-36s at >= 2x on %3d rows (%3d of them by its NaN pattern), most on %s: %.3g x the bound"
        % (mutant, caught, pattern, row, best))
    assert best >= 2.0, (mutant, best, row)


def test_otsu_restatement_is_the_oracle_and_the_exhaustive_maximiser(capsys):
    from oracle import relevancy_np as onp
    rows = judged = 0
    for family, n, K in pb.otsu_rows():
        cams = pb.otsu_case(family, n, K)
        masks, thr, lev = pb.otsu_restatement(cams)
        for k in range(K):
            rows += 1
            want = pb.exhaustive_threshold(lev[k])
            if want is None:                         # one occupied level: constant, n = 1, an infinite range
                assert thr[k] == 0 and not masks[k].any() and not lev[k].any(), (family, n, K, k)
                continue
            judged += 1
            assert thr[k] == want, (family, n, K, k, int(thr[k]), want)
            if np.isfinite(cams[k]).all():           # the oracle takes numpy's NaN-propagating extremes
                m, t = onp.otsu_mask(np.array(cams[k]))
                assert t == thr[k] and np.array_equal(m, masks[k]), (family, n, K, k)
    say(capsys, "otsu restatement: %d maps, %d with more than one occupied level, all on the exhaustive maximiser" % (rows, judged))
    assert judged > rows // 2


def test_otsu_special_values_follow_the_contract():
    for n in (3, 257, 1000):
        for K in pb.OTSU_KS:
            cams = pb.otsu_case("nan_pixel", n, K)
            masks, thr, lev = pb.otsu_restatement(cams)
            clean = np.where(np.isnan(cams), cams[:, 1:2], cams)        # the NaN replaced by a pixel inside the range
            m2, t2, l2 = pb.otsu_restatement(clean)
            bad = np.isnan(cams)
            assert (lev[bad] == 0).all() and (masks[bad] == 0).all()
            assert np.array_equal(lev[~bad], l2[~bad])
            masks, thr, lev = pb.otsu_restatement(pb.otsu_case("inf_pixel", n, K))
            assert not lev.any() and not thr.any() and not masks.any()


def test_the_lattice_sits_on_the_level_boundaries():
    """Every pixel of the family is a level boundary ``lo + range k / 255`` or a neighbouring float: at least a third of them change
    their level under round-to-nearest, and some under the reciprocal form."""
    cams = pb.otsu_case("lattice", pb.otsu_ns("lattice")[0], 6)
    for k in range(6):
        lo, hi = pb.otsu_extremes(cams[k])
        q = pb.otsu_levels(cams[k], lo, hi)
        assert len(np.unique(q)) == 256
        assert (pb.otsu_levels(cams[k], lo, hi, "round") != q).mean() > 0.3
        up, down = np.nextafter(cams[k], np.float32(np.inf)), np.nextafter(cams[k], np.float32(-np.inf))
        at_edge = (pb.otsu_levels(np.minimum(up, hi), lo, hi) != q) | (pb.otsu_levels(np.maximum(down, lo), lo, hi) != q)
        assert at_edge.sum() >= 2 * 255
    assert any((pb.otsu_levels(cams[k], *pb.otsu_extremes(cams[k]), "reciprocal") != pb.otsu_levels(cams[k], *pb.otsu_extremes(cams[k]))).any()
               for k in range(6))


@pytest.mark.parametrize("mutant", sorted(pb.OTSU_MUTANTS))
def test_every_otsu_mutant_changes_a_mask_bit_or_a_threshold(mutant, capsys):
    best, row, caught = -1, None, 0
    for family, n, K in pb.otsu_rows():
        cams = pb.otsu_case(family, n, K)
        masks, thr, _ = pb.otsu_restatement(cams)
        m2, t2, _ = pb.otsu_restatement(cams, **pb.OTSU_MUTANTS[mutant])
        bits, ts = int((masks != m2).sum()), int((thr != t2).sum())
        caught += bool(bits or ts)
        if bits + ts > best:
            best, row, what = bits + ts, (family, n, K), "%d mask bits, %d thresholds" % (bits, ts)
    say(capsys, "otsu mutant %-34s caught on %3d rows, most on %s: %s" % (mutant, caught, row, what))
    assert best > 0, mutant


def test_the_ratio_counts_a_one_sided_nan_as_a_failure():
    ref = {"out": np.array([[0.0, np.nan, 1.0]]), "bound": np.array([[1e-6, 1e-6, 1e-6]])}
    assert pb.heatmap_ratio(np.array([[0.0, np.nan, 1.0]]), ref) == 0.0
    assert pb.heatmap_ratio(np.array([[0.0, 0.5, 1.0]]), ref) == math.inf
    assert pb.heatmap_ratio(np.array([[np.nan, np.nan, 1.0]]), ref) == math.inf
    assert pb.heatmap_ratio(np.array([[0.0, np.nan, np.inf]]), ref) == math.inf
    assert pb.heatmap_ratio(np.array([[2e-6, np.nan, 1.0]]), ref) == 2.0
