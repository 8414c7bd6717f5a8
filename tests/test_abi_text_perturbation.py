"""CPU: the two entries of the caption perturbation test (``mmx_perturb_tokens``, ``mmx_attn_fwd_live``) are declared, exported and
bound, and refuse bad arguments before any HIP call."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_perturb_tokens", "mmx_attn_fwd_live")
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


def _tok_args(B=2, N=77, S=9, ptr=PTR, ranks=True):
    return [_p(i, ptr) for i in range(5)] + [_p(5, ptr) if ranks else None, B, N, S, None]


def _attn_args(B=2, H=4, N=77, Nk=None, D=64, ptr=PTR, mode=0, eot=True, mask=True):
    s = (N * H * D, D, H * D)                                             # bnhd strides (batch, head, token)
    Nk = N if Nk is None else Nk
    return [_p(0, ptr), _p(1, ptr), _p(2, ptr)] + list(s) * 3 + [_p(4, ptr) if mask else None, 0, Nk, _p(3, ptr)] + list(s) + \
           [B, H, N, Nk, D, C.c_float(0.125), mode, _p(5, ptr) if eot else None, None]


def test_symbols_are_declared_exported_and_bound(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2


@pytest.mark.parametrize("name,args", [("mmx_perturb_tokens", _tok_args(ptr=0)), ("mmx_attn_fwd_live", _attn_args(ptr=0))])
def test_null_pointers_are_refused(lib, name, args):
    handle = lib.lib()
    assert getattr(handle, name)(*args) == -22
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("missing", range(5))
def test_each_null_pointer_of_perturb_tokens_is_refused(lib, missing):
    """ids / scores / counts / out_ids / out_eot one at a time; a NULL ``ranks`` alone is allowed (so it is not in this list)."""
    handle = lib.lib()
    args = _tok_args()
    args[missing] = None
    assert handle.mmx_perturb_tokens(*args) == -22
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("args", [_tok_args(N=1), _tok_args(N=257), _tok_args(S=0), _tok_args(S=65), _tok_args(B=0)])
def test_bad_sizes_are_refused_without_gpu(lib, args):
    """MMX_EINVAL with a message, checked before any HIP call (this machine may have no GPU at all)."""
    handle = lib.lib()
    assert handle.mmx_perturb_tokens(*args) == -22
    assert handle.mmx_last_error()


@pytest.mark.parametrize("args,word", [(_attn_args(N=12), b"live"), (_attn_args(D=80), b"head_dim")])
def test_shapes_outside_the_live_kernels_are_not_supported(lib, args, word):
    handle = lib.lib()
    assert handle.mmx_attn_fwd_live(*args) == -95
    assert word in handle.mmx_last_error()


@pytest.mark.parametrize("args", [_attn_args(N=77, Nk=70), _attn_args(eot=False), _attn_args(mask=False)])
def test_attn_fwd_live_needs_a_self_attention_with_lengths_and_mask(lib, args):
    handle = lib.lib()
    assert handle.mmx_attn_fwd_live(*args) == -22
    assert handle.mmx_last_error()
