"""CPU: the entries of the fused CLIP similarity head (``mmx_clip_head_f32``, ``mmx_clip_head_fused_enabled``) are declared, exported
and bound, refuse bad arguments before any HIP call, and option ``clip_head_fused`` ships on and takes 0 and 1 only."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_clip_head_f32", "mmx_clip_head_fused_enabled")
PTR = 0x7f0000000000            # made-up device addresses: a launch on them would fail differently
EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib


def _p(i):
    return C.c_void_p(PTR + 4096 * i)


def _args(B=6, D=36, Bi=3, img_group=2):
    """img_feat, txt_feat, logit_scale, d_img, d_txt, logit_diag, B, D, Bi, img_group, stream"""
    return [_p(0), _p(1), _p(2), _p(3), _p(4), _p(5), B, D, Bi, img_group, None]


def test_symbols_are_declared_exported_and_bound(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    from transformer_mm_explainability_amd import ops
    assert callable(ops.clip_head_grads)


@pytest.mark.parametrize("missing", [0, 1, 2])
def test_each_required_null_pointer_is_refused(lib, missing):
    handle = lib.lib()
    args = _args()
    args[missing] = None
    assert handle.mmx_clip_head_f32(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


def test_a_call_without_any_output_is_refused(lib):
    handle = lib.lib()
    args = _args()
    args[3] = args[4] = args[5] = None
    assert handle.mmx_clip_head_f32(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(B=0), dict(B=-6), dict(D=0), dict(D=-4), dict(D=4097), dict(Bi=0), dict(img_group=0),
                                   dict(Bi=3, img_group=1), dict(Bi=2, img_group=2), dict(Bi=6, img_group=2), dict(Bi=4, img_group=2),
                                   dict(B=65536, Bi=65537, img_group=65536)])
def test_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    """``B <= 0``, ``D <= 0``, ``D > 4096`` and ``Bi * img_group != B`` (the product taken in 64 bits)."""
    handle = lib.lib()
    assert handle.mmx_clip_head_f32(*_args(**sizes)) == EINVAL
    assert handle.mmx_last_error()


@pytest.mark.parametrize("out", [3, 4])
@pytest.mark.parametrize("feature", [0, 1])
def test_an_output_aliasing_a_feature_tensor_is_refused(lib, out, feature):
    handle = lib.lib()
    args = _args()
    args[out] = args[feature]
    assert handle.mmx_clip_head_f32(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_the_option_is_on_by_default_and_takes_0_and_1_only(lib):
    handle = lib.lib()
    assert handle.mmx_clip_head_fused_enabled() == 1
    try:
        assert handle.mmx_set_option(b"clip_head_fused", 0) == 0
        assert handle.mmx_clip_head_fused_enabled() == 0
        for bad in (2, -1):
            assert handle.mmx_set_option(b"clip_head_fused", bad) != 0
            assert handle.mmx_clip_head_fused_enabled() == 0
        assert handle.mmx_set_option(b"clip_head_fused", 1) == 0
        assert handle.mmx_clip_head_fused_enabled() == 1
    finally:
        handle.mmx_set_option(b"clip_head_fused", 1)
