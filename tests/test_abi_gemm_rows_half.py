"""CPU: the three entries of the fp16 row-list GEMM (``mmx_gemm_rows_f16``, ``mmx_gemm_rows_bias_f16``,
``mmx_text_live_rows_half_enabled``) are declared, exported and bound, refuse bad arguments before any HIP call, and option
``text_live_rows_half`` ships off."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_gemm_rows_f16", "mmx_gemm_rows_bias_f16", "mmx_text_live_rows_half_enabled")
PTR = 0x7f0000000000            # made-up, 16-byte aligned device addresses: a launch on them would fail differently
EINVAL, ENOTSUP = -22, -95


@pytest.fixture(scope="module")
def lib():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib


def _p(i):
    return C.c_void_p(PTR + 4096 * i)


def _plain(cap=72, N=64, K=64):
    """a, wh, c, rows, count, cap, N, K, stream"""
    return [_p(0), _p(1), _p(2), _p(3), _p(4), cap, N, K, None]


def _bias(cap=72, N=64, K=64, act=True):
    """a, wh, bias, c, act, rows, count, cap, N, K, stream"""
    return [_p(0), _p(1), _p(5), _p(2), _p(6) if act else None, _p(3), _p(4), cap, N, K, None]


def test_symbols_are_declared_exported_and_bound(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2


@pytest.mark.parametrize("missing", range(5))
def test_each_null_pointer_of_the_plain_entry_is_refused(lib, missing):
    handle = lib.lib()
    args = _plain()
    args[missing] = None
    assert handle.mmx_gemm_rows_f16(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("missing", [0, 1, 2, 3, 5, 6])
def test_each_null_pointer_of_the_bias_entry_is_refused(lib, missing):
    """a / wh / bias / c / rows / count one at a time; a NULL ``act`` alone asks for no activation (so it is not in this list)."""
    handle = lib.lib()
    args = _bias()
    args[missing] = None
    assert handle.mmx_gemm_rows_bias_f16(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(cap=0), dict(N=0), dict(K=0), dict(cap=-3), dict(N=-8), dict(K=-8)])
def test_non_positive_sizes_are_refused(lib, sizes):
    handle = lib.lib()
    assert handle.mmx_gemm_rows_f16(*_plain(**sizes)) == EINVAL
    assert handle.mmx_gemm_rows_bias_f16(*_bias(**sizes)) == EINVAL
    assert handle.mmx_last_error()


def test_the_activation_needs_a_buffer_of_its_own(lib):
    handle = lib.lib()
    args = _bias()
    args[4] = args[3]
    assert handle.mmx_gemm_rows_bias_f16(*args) == EINVAL


@pytest.mark.parametrize("sizes", [dict(N=12), dict(K=20), dict(N=12, K=20)])
def test_widths_that_are_no_multiple_of_8_are_not_supported(lib, sizes):
    """MMX_ENOTSUP, nothing launched (this machine may have no GPU at all)."""
    handle = lib.lib()
    assert handle.mmx_gemm_rows_f16(*_plain(**sizes)) == ENOTSUP
    assert b"multiples of 8" in handle.mmx_last_error()
    assert handle.mmx_gemm_rows_bias_f16(*_bias(**sizes)) == ENOTSUP
    assert handle.mmx_gemm_rows_bias_f16(*_bias(act=False, **sizes)) == ENOTSUP


@pytest.mark.parametrize("which", [0, 1, 2])
def test_an_operand_off_a_16_byte_boundary_is_not_supported(lib, which):
    handle = lib.lib()
    args = _plain()
    args[which] = C.c_void_p(args[which].value + 8)
    assert handle.mmx_gemm_rows_f16(*args) == ENOTSUP
    args = _bias()
    where = (0, 1, 3)[which]
    args[where] = C.c_void_p(args[where].value + 8)
    assert handle.mmx_gemm_rows_bias_f16(*args) == ENOTSUP


def test_the_option_is_off_by_default_and_takes_0_and_1_only(lib):
    handle = lib.lib()
    assert handle.mmx_text_live_rows_half_enabled() == 0
    try:
        assert handle.mmx_set_option(b"text_live_rows_half", 1) == 0
        assert handle.mmx_text_live_rows_half_enabled() == 1
        assert handle.mmx_set_option(b"text_live_rows_half", 2) != 0
        assert handle.mmx_text_live_rows_half_enabled() == 1
        # all three switches: the route of an fp16 body needs the list and the row-list forward as well
        for key in (b"text_live_rows", b"text_live_rows_fwd"):
            assert handle.mmx_set_option(key, 0) == 0
            assert handle.mmx_text_live_rows_half_enabled() == 0
            assert handle.mmx_set_option(key, 1) == 0
            assert handle.mmx_text_live_rows_half_enabled() == 1
        assert handle.mmx_set_option(b"text_live_rows_half", 0) == 0
        assert handle.mmx_text_live_rows_half_enabled() == 0
    finally:
        handle.mmx_set_option(b"text_live_rows", 1)
        handle.mmx_set_option(b"text_live_rows_fwd", 1)
        handle.mmx_set_option(b"text_live_rows_half", 0)
