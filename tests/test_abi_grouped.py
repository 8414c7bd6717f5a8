"""CPU: the grouped row-mode entry (``mmx_attn_capture_bwd_rowrel_f32_grouped``) is declared, exported and bound, and refuses
bad arguments with MMX_EINVAL before any HIP call."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mmx_attn_capture_bwd_rowrel_f32_grouped"


@pytest.fixture(scope="module")
def lib():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib


def _args(B, n_images, ptr=0x7f0000000000, ws_bytes=1 << 20):
    """A full argument list of the grouped entry: (B targets, H 4, N 50, D 64) on made-up, aligned device addresses."""
    H, N, D = 4, 50, 64
    p = [C.c_void_p(ptr + 4096 * i) if ptr else None for i in range(12)]
    s = (N * H * D, D, H * D)                                             # bnhd strides (batch, head, token)
    return ([p[0], p[1], p[2]] + list(s) * 3 + [p[3], H * N * N, 0, p[4]] + list(s) + [p[5]] + list(s) + [p[6], p[7], p[8], p[9]]
            + list(s) * 3 + [B, H, N, N, D, C.c_float(0.125), 1, 1, p[10], p[11], n_images, p[0], ws_bytes, None])


def test_grouped_symbol_is_declared_exported_and_bound(lib):
    handle = lib.lib()
    for name in (NAME, NAME + "_workspace_bytes"):
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2


def test_grouped_refuses_null_pointers(lib):
    handle = lib.lib()
    assert getattr(handle, NAME)(*_args(6, 3, ptr=0)) == -22
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("B,n_images", [(6, 0), (6, -1), (6, 4), (5, 2), (0, 1)])
def test_grouped_refuses_image_counts_without_gpu(lib, B, n_images):
    """``n_images < 1`` or a target count that is not a whole number per image: MMX_EINVAL, checked before any HIP call
    (the pointers here are made up: a launch would fail differently)."""
    handle = lib.lib()
    assert getattr(handle, NAME)(*_args(B, n_images)) == -22
    assert handle.mmx_last_error()


def test_grouped_workspace_query(lib):
    handle = lib.lib()
    need = getattr(handle, NAME + "_workspace_bytes")(10, 4, 50, 50)
    assert need > 0
    assert need == handle.mmx_attn_capture_bwd_rowrel_f32_workspace_bytes(10, 4, 50, 50)    # per target, as the per-sample mode
