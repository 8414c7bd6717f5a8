"""CPU: the two post-processing entries (``mmx_heatmap_bilinear_minmax``, ``mmx_otsu_masks``) are declared, exported and bound, and refuse
bad arguments and sizes beyond their index arithmetic by return code, before any HIP call."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_heatmap_bilinear_minmax", "mmx_otsu_masks")
PTR = 0x7f0000000000            # made-up device addresses: a launch on them would fail differently
EINVAL, ENOTSUP = -22, -95
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib


def _p(i):
    return C.c_void_p(PTR + 4096 * i)


def _heatmap(B=2, g=7, S=224):
    """in, out, B, g, S, stream"""
    return [_p(0), _p(1), B, g, S, None]


def _otsu(K=6, n=950, thresholds=True):
    """cam, masks, thresholds, K, n, stream"""
    return [_p(0), _p(1), _p(2) if thresholds else None, K, n, None]


def test_symbols_are_declared_exported_and_bound(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)


@pytest.mark.parametrize("missing", [0, 1])
def test_each_null_pointer_is_refused(lib, missing):
    """in / out and cam / masks one at a time; a NULL ``thresholds`` alone asks for no thresholds (so it is not in this list)."""
    handle = lib.lib()
    args = _heatmap()
    args[missing] = None
    assert handle.mmx_heatmap_bilinear_minmax(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()
    for thresholds in (True, False):
        args = _otsu(thresholds=thresholds)
        args[missing] = None
        assert handle.mmx_otsu_masks(*args) == EINVAL
        assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(B=0), dict(g=0), dict(S=0), dict(B=-1), dict(g=-7), dict(S=-224), dict(S=-INT_MAX)])
def test_non_positive_heat_map_sizes_are_refused(lib, sizes):
    handle = lib.lib()
    assert handle.mmx_heatmap_bilinear_minmax(*_heatmap(**sizes)) == EINVAL
    assert b"non-positive" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(K=0), dict(n=0), dict(K=-6), dict(n=-950)])
def test_non_positive_otsu_sizes_are_refused(lib, sizes):
    handle = lib.lib()
    assert handle.mmx_otsu_masks(*_otsu(**sizes)) == EINVAL
    assert b"non-positive" in handle.mmx_last_error()


@pytest.mark.parametrize("g", [65, 128, INT_MAX])
def test_a_patch_grid_above_64_is_not_supported(lib, g):
    """MMX_ENOTSUP, nothing launched (this machine may have no GPU at all): the kernel stages at most 64 x 64 patches in LDS."""
    handle = lib.lib()
    assert handle.mmx_heatmap_bilinear_minmax(*_heatmap(g=g)) == ENOTSUP
    assert b"> 64" in handle.mmx_last_error()


@pytest.mark.parametrize("S", [46341, 65536, INT_MAX])
def test_a_side_whose_square_does_not_fit_an_int_is_not_supported(lib, S):
    """``heatmap_kernel`` counts the ``S * S`` pixels of a map in ``int``; 46340 is the last side whose square is below 2**31."""
    assert 46340 ** 2 <= INT_MAX < 46341 ** 2
    handle = lib.lib()
    for B in (1, 3):
        for g in (1, 14, 64):
            assert handle.mmx_heatmap_bilinear_minmax(*_heatmap(B=B, g=g, S=S)) == ENOTSUP
            assert b"does not fit an int" in handle.mmx_last_error()
    # the wider refusal wins over neither of the earlier ones
    assert handle.mmx_heatmap_bilinear_minmax(*_heatmap(g=65, S=S)) == ENOTSUP
    assert handle.mmx_heatmap_bilinear_minmax(*_heatmap(B=0, S=S)) == EINVAL


@pytest.mark.parametrize("n", [INT_MAX - 255, INT_MAX])
def test_a_map_whose_pixel_index_would_pass_int_max_is_not_supported(lib, n):
    """``otsu_kernel`` steps an ``int`` pixel index by 256 up to ``n``: ``n + 256`` must stay below 2**31."""
    handle = lib.lib()
    for thresholds in (True, False):
        assert handle.mmx_otsu_masks(*_otsu(K=1, n=n, thresholds=thresholds)) == ENOTSUP
        assert b"pixels per map" in handle.mmx_last_error()
