"""-m gpu: ``heatmap_kernel`` and ``otsu_kernel`` (``csrc/postprocess_kernels.hip``) through ``postprocess.image_heatmaps`` /
``postprocess.otsu_masks``, held to the definitions, counted bounds and case tables of ``tests/postprocess_bounds.py`` (proved on the CPU by
``tests/test_postprocess_bounds_host.py``, where every mutant of these kernels is shown to leave them).

Heat map: every pixel inside its bound with the reference's NaN pattern, the minimum exactly 0.0 and the maximum exactly 1.0, the bits of the
fp32 ``(in - lo) / range`` at ``S = g``, the special-value contract.  Otsu: masks and thresholds bit for bit on the restatement, thresholds on
the exhaustive maximiser.  Both: outputs between NaN guard bands that come back untouched, the same bits on a second call, and every map's
bits independent of the other maps of its batch.  The worst error / bound of every family is printed and recorded (``parity.note``)."""
import ctypes as C

import numpy as np
import pytest
import torch

import postprocess_bounds as pb
from guard_arena import Arena, ptr, to_device
from parity import note

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def post():
    from transformer_mm_explainability_amd import postprocess
    return postprocess


@pytest.fixture(scope="module")
def entry():
    from transformer_mm_explainability_amd import _lib
    return _lib.lib()


def sync_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def heatmap_on_arena(entry, src, S):
    """The C entry on a guarded output region -> ``[B, S, S]`` numpy; the guard bands are checked."""
    B, g = src.shape[0], src.shape[1]
    arena = Arena([B * S * S])
    rc = entry.mmx_heatmap_bilinear_minmax(ptr(to_device(np.array(src))), ptr(arena.region(0)), B, g, S, sync_stream())
    assert rc == 0, entry.mmx_last_error()
    torch.cuda.synchronize()
    out = arena.region(0).cpu().numpy().reshape(B, S, S)
    arena.buf[arena.spans[0][0]:arena.spans[0][0] + B * S * S] = float("nan")       # the region itself aside, nothing was written
    arena.assert_guards_untouched([0])
    return out


@pytest.mark.parametrize("group", sorted(pb.HEATMAP_GROUPS))
@pytest.mark.parametrize("family", pb.HEATMAP_FAMILIES)
def test_heat_maps_meet_the_bound_the_identities_and_the_contract(post, entry, family, group):
    top, unjudged = 0.0, 0
    for g, S, B in pb.heatmap_shapes(group):
        src, ref = pb.heatmap_case(family, g, S, B), pb.heatmap_case_ref(family, g, S, B)
        dev = to_device(np.array(src).reshape(B, g * g))
        out = post.image_heatmaps(dev, S)
        assert out.shape == (B, S, S) and out.dtype == torch.float32
        got = out.cpu().numpy()
        # the same bits again, behind guard bands, and for every map alone
        assert pb.same_bits(got, post.image_heatmaps(dev, S).cpu().numpy()), (family, g, S, "second call")
        assert pb.same_bits(got, heatmap_on_arena(entry, src, S)), (family, g, S, "guarded")
        for b in range(B):
            alone = post.image_heatmaps(dev[b], S)
            assert alone.shape == (S, S)
            assert pb.same_bits(got[b], alone.cpu().numpy()), (family, g, S, b, "alone")
        if pb.degenerate(family, g):
            assert all(pb.degenerate_map_ok(got[b], src[b], S) for b in range(B)), (family, g, S)
            continue
        unjudged += pb.unjudged(ref)
        r = pb.heatmap_ratio(got, ref)
        print("\npostprocess-bounds heatmap %-10s g=%-2d S=%-3d B=%d error / bound %.3f" % (family, g, S, B, r), end="")
        top = max(top, r)
        assert r <= 1.0, (family, g, S, B, r)
        for b in range(B):
            if pb.all_nan_by_definition(ref, b):
                assert np.isnan(got[b]).all(), (family, g, S, b)
            elif np.isfinite(ref["range"][b]):
                assert np.nanmin(got[b]) == 0.0 and np.nanmax(got[b]) == 1.0, (family, g, S, b)
        if S == g and np.isfinite(src).all():
            assert pb.same_bits(got, pb.identity_at_S_equal_g(src)), (family, g)
    print("\npostprocess-bounds heatmap %-10s %-7s worst error / bound %.3f, unjudged pixels %d" % (family, group, top, unjudged))
    note("heatmap %s error/bound" % family, top, bound=1.0)
    assert unjudged == 0


def test_a_nan_patch_reaches_the_pixels_that_tap_it_and_no_other(post):
    """The contract's NaN rule against a clean run (the patch at the map's median instead): the pixels with the NaN patch among their taps
    are NaN, and every other pixel keeps the bits of the clean run."""
    for g, S in ((7, 30), (14, 9), (33, 66)):
        src = np.array(pb.heatmap_case("randn", g, S, 3))
        for b, at in enumerate(((0, 0), (g // 2, g // 3), (g - 1, g - 1))):
            src[b][at] = np.sort(src[b].reshape(-1))[g * g // 2]            # the median: inside the range
        clean = post.image_heatmaps(to_device(src.reshape(3, -1)), S).cpu().numpy()
        dirty_src = src.copy()
        for b, at in enumerate(((0, 0), (g // 2, g // 3), (g - 1, g - 1))):
            dirty_src[b][at] = np.nan
        dirty = post.image_heatmaps(to_device(dirty_src.reshape(3, -1)), S).cpu().numpy()
        checked = 0
        for b in range(3):
            taps, _ = pb._taps(dirty_src[b], g, S)
            hit = np.isnan(taps[0] + taps[1] + taps[2] + taps[3])
            assert hit.any() and not hit.all()
            assert np.array_equal(np.isnan(dirty[b]), hit), (g, S, b)
            if not (hit & ((clean[b] == 0.0) | (clean[b] == 1.0))).any():       # neither extreme of the clean run came from a hit pixel
                assert pb.same_bits(dirty[b][~hit], clean[b][~hit]), (g, S, b)
                checked += 1
        assert checked >= 2, (g, S)


@pytest.mark.parametrize("family", pb.OTSU_FAMILIES)
def test_otsu_masks_and_thresholds_are_the_definition_bit_for_bit(post, entry, family):
    maps = judged = 0
    for n in pb.otsu_ns(family):
        for K in pb.OTSU_KS:
            cams = pb.otsu_case(family, n, K)
            want_m, want_t, lev = pb.otsu_restatement(cams)
            dev = to_device(np.array(cams))
            masks, thr = post.otsu_masks(dev, return_thresholds=True)
            assert masks.shape == (K, n) and masks.dtype == torch.float32 and thr.shape == (K,) and thr.dtype == torch.int32
            got_m, got_t = masks.cpu().numpy(), thr.cpu().numpy()
            assert np.array_equal(got_t, want_t), (family, n, K, got_t, want_t)
            assert np.array_equal(got_m.view(np.int32), want_m.view(np.int32)), (family, n, K, int((got_m != want_m).sum()))
            for k in range(K):
                maps += 1
                best = pb.exhaustive_threshold(lev[k])
                if best is None:
                    assert got_t[k] == 0 and not got_m[k].any(), (family, n, K, k)
                else:
                    judged += 1
                    assert got_t[k] == best, (family, n, K, k, int(got_t[k]), best)
            # the same bits again, and for every map alone
            m2, t2 = post.otsu_masks(dev, return_thresholds=True)
            assert torch.equal(m2, masks) and torch.equal(t2, thr), (family, n, K, "second call")
            for k in range(K):
                m1, t1 = post.otsu_masks(dev[k:k + 1], return_thresholds=True)
                assert torch.equal(m1[0], masks[k]) and int(t1[0]) == int(thr[k]), (family, n, K, k, "alone")
            # masks and thresholds behind guard bands; then the entry without thresholds: the same masks, nothing else written
            for with_thr in (True, False):
                arena = Arena([K * n, K])
                arena.region(1).view(torch.int32).fill_(-1)
                rc = entry.mmx_otsu_masks(ptr(dev), ptr(arena.region(0)), ptr(arena.region(1)) if with_thr else C.c_void_p(0), K, n,
                                          sync_stream())
                assert rc == 0, entry.mmx_last_error()
                torch.cuda.synchronize()
                assert torch.equal(arena.region(0).reshape(K, n), masks), (family, n, K, with_thr)
                t3 = arena.region(1).view(torch.int32).clone()
                assert torch.equal(t3, thr if with_thr else torch.full_like(thr, -1)), (family, n, K, with_thr)
                arena.region(0).fill_(float("nan"))
                arena.region(1).fill_(float("nan"))
                arena.assert_guards_untouched([0, 0])
    print("\npostprocess-bounds otsu %-13s %3d maps bit for bit, %3d of them judged on the exhaustive maximiser" % (family, maps, judged))
    note("otsu %s differing maps" % family, 0.0, bound=0.0)
