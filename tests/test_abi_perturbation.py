"""CPU: the three entries of the image perturbation test (``mmx_attn_fwd``, ``mmx_patch_ranks``, ``mmx_perturb_patches``) are
declared, exported and bound, and refuse bad arguments with MMX_EINVAL before any HIP call."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_attn_fwd", "mmx_patch_ranks", "mmx_perturb_patches")
PTR = 0x7f0000000000            # made-up, 16-byte aligned device addresses: a launch on them would fail differently


@pytest.fixture(scope="module")
def lib():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib


def _p(i, ptr=PTR):
    return C.c_void_p(ptr + 4096 * i) if ptr else None


def _attn_args(B=2, H=4, N=50, D=64, ptr=PTR, mode=0):
    s = (N * H * D, D, H * D)                                             # bnhd strides (batch, head, token)
    return [_p(0, ptr), _p(1, ptr), _p(2, ptr)] + list(s) * 3 + [None, 0, 0, _p(3, ptr)] + list(s) + \
           [B, H, N, N, D, C.c_float(0.125), mode, None]


def _rank_args(B=2, P=196, ptr=PTR):
    return [_p(0, ptr), _p(1, ptr), B, P, None]


def _pert_args(B=2, Cc=3, R=224, patch=16, S=9, ptr=PTR):
    return [_p(i, ptr) for i in range(5)] + [B, Cc, R, patch, S, None]


def test_symbols_are_declared_exported_and_bound(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2


@pytest.mark.parametrize("name,args", [("mmx_attn_fwd", _attn_args(ptr=0)), ("mmx_patch_ranks", _rank_args(ptr=0)),
                                       ("mmx_perturb_patches", _pert_args(ptr=0))])
def test_null_pointers_are_refused(lib, name, args):
    handle = lib.lib()
    assert getattr(handle, name)(*args) == -22
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("name,args", [
    ("mmx_patch_ranks", _rank_args(P=0)),
    ("mmx_patch_ranks", _rank_args(P=4097)),
    ("mmx_patch_ranks", _rank_args(B=0)),
    ("mmx_perturb_patches", _pert_args(R=224, patch=15)),
    ("mmx_perturb_patches", _pert_args(R=336, patch=32)),
    ("mmx_perturb_patches", _pert_args(patch=0)),
    ("mmx_perturb_patches", _pert_args(S=0)),
    ("mmx_perturb_patches", _pert_args(B=0)),
    ("mmx_perturb_patches", _pert_args(Cc=0)),
    ("mmx_attn_fwd", _attn_args(B=0)),
    ("mmx_attn_fwd", _attn_args(H=0)),
    ("mmx_attn_fwd", _attn_args(D=0)),
    ("mmx_attn_fwd", _attn_args(N=0)),
    ("mmx_attn_fwd", _attn_args(mode=7)),
])
def test_bad_sizes_are_refused_without_gpu(lib, name, args):
    """MMX_EINVAL with a message, checked before any HIP call (this machine may have no GPU at all)."""
    handle = lib.lib()
    assert getattr(handle, name)(*args) == -22
    assert handle.mmx_last_error()


def test_head_dim_beyond_the_capture_forward_is_not_supported(lib):
    """The no-capture forward serves the fp32 capture forward's shape space: head_dim > 64 is MMX_ENOTSUP in both."""
    handle = lib.lib()
    assert handle.mmx_attn_fwd(*_attn_args(D=80)) == -95
    assert b"head_dim" in handle.mmx_last_error()
