"""CPU: the entries of the batched LXMERT baselines (``mmx_head_mean_live``, ``mmx_lxmert_rollout``,
``mmx_lxmert_rollout_workspace_bytes``) are declared, exported, bound and reachable through ``ops``, and refuse bad arguments with
``MMX_EINVAL`` and a message before any HIP call (every call here runs on made-up device addresses, on a machine without a GPU)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_head_mean_live", "mmx_lxmert_rollout", "mmx_lxmert_rollout_workspace_bytes")
PTR = 0x7f0000000000            # made-up device addresses: a launch on them would fail differently
STEP = 1 << 26                  # further apart than any operand of the shapes below is long
EINVAL = -22
MAX_TABLE = 32


@pytest.fixture(scope="module")
def lib():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib


def _p(i):
    return C.c_void_p(PTR + STEP * i)


def _table(first, n):
    arr = (C.c_void_p * max(n, 1))(*[PTR + STEP * (first + l) for l in range(max(n, 1))])
    return C.cast(arr, C.POINTER(C.c_void_p)), arr


def _hm_args(B=5, H=4, Nq=12, Nk=20, flags=0):
    """attn, grad, out, B, H, Nq, Nk, q_len, k_len, flags, stream"""
    return [_p(0), _p(1), _p(2), B, H, Nq, Nk, _p(3), _p(4), flags, None]


def _ro_args(lib, n_text=5, n_img=4, B=5, H=4, T=12, I=20, ws_bytes=None):
    """text table, n_text, image table, n_img, cross, B, H, T, I, text_len, R_tt, R_ti, R_ii, workspace, workspace_bytes, stream"""
    tt, keep_t = _table(10, n_text)
    ti, keep_i = _table(50, n_img)
    need = lib.lib().mmx_lxmert_rollout_workspace_bytes(n_text, n_img, B, T, I)
    args = [tt, n_text, ti, n_img, _p(1), B, H, T, I, _p(2), _p(3), _p(4), _p(5), _p(6), need if ws_bytes is None else ws_bytes, None]
    return args, (keep_t, keep_i)


def test_symbols_are_declared_exported_bound_and_callable_through_ops(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2
    from transformer_mm_explainability_amd import lxmert_explainability as le
    from transformer_mm_explainability_amd import ops
    assert callable(ops.head_mean_live) and callable(ops.attn_gradcam_live) and callable(ops.lxmert_rollout)
    for method in ("generate_rollout_batch", "generate_raw_attn_batch", "generate_attn_gradcam_batch"):
        assert callable(getattr(le.GeneratorBaselines, method))
    assert le.GraphedBaselinesBatch.METHODS == ("rollout", "raw_attn", "attn_gradcam")


def test_ops_refuse_host_tensors():
    import torch
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    x = torch.rand(1, 2, 3, 3)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.head_mean_live(x)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.attn_gradcam_live(x, x)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.lxmert_rollout([x, x], [x], x)


@pytest.mark.parametrize("missing", [0, 2])
def test_head_mean_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args = _hm_args()
    args[missing] = None
    assert handle.mmx_head_mean_live(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("missing", [0, 2, 4, 10, 11, 13])
def test_rollout_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args, _keep = _ro_args(lib)
    args[missing] = None
    assert handle.mmx_lxmert_rollout(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("which", ["text", "img"])
def test_rollout_null_table_entries_are_refused(lib, which):
    handle = lib.lib()
    args, keep = _ro_args(lib)
    (keep[0] if which == "text" else keep[1])[2] = None
    assert handle.mmx_lxmert_rollout(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(Nq=0), dict(Nq=-2), dict(Nq=49), dict(Nk=0),
                                   dict(Nk=49), dict(Nk=1 << 20), dict(flags=2), dict(flags=0x80000000)])
def test_head_mean_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    handle = lib.lib()
    assert handle.mmx_head_mean_live(*_hm_args(**sizes)) == EINVAL
    assert handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(T=0), dict(T=49), dict(T=-5), dict(I=0),
                                   dict(I=49), dict(n_text=1), dict(n_text=0), dict(n_text=-1), dict(n_img=0), dict(n_img=-2),
                                   dict(n_text=MAX_TABLE + 1), dict(n_img=MAX_TABLE + 1)])
def test_rollout_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    """``B, H <= 0``, sizes outside 1..48, ``n_text < 2``, ``n_img < 1`` and tables longer than the compiled maximum."""
    handle = lib.lib()
    args, _keep = _ro_args(lib, **sizes)
    if "H" not in sizes:                                # the query takes no H; for everything else it answers 0
        assert handle.mmx_lxmert_rollout_workspace_bytes(args[1], args[3], args[5], args[7], args[8]) == 0
    args[14] = 1 << 30                                  # (the refusal is about the size, not about the workspace)
    assert handle.mmx_lxmert_rollout(*args) == EINVAL
    assert handle.mmx_last_error()


def test_rollout_workspace_smaller_than_the_query_is_refused(lib):
    handle = lib.lib()
    need = handle.mmx_lxmert_rollout_workspace_bytes(5, 4, 5, 12, 20)
    for short in (0, need - 1):
        args, _keep = _ro_args(lib, ws_bytes=short)
        assert handle.mmx_lxmert_rollout(*args) == EINVAL
        assert b"workspace" in handle.mmx_last_error()


def test_rollout_misaligned_workspace_is_refused(lib):
    handle = lib.lib()
    args, _keep = _ro_args(lib)
    args[13] = C.c_void_p(PTR + STEP * 6 + 4)
    args[14] += 16
    assert handle.mmx_lxmert_rollout(*args) == EINVAL
    assert b"aligned" in handle.mmx_last_error()


@pytest.mark.parametrize("inp", [0, 1, 7, 8])
def test_head_mean_output_aliasing_an_input_is_refused(lib, inp):
    handle = lib.lib()
    args = _hm_args()
    args[2] = args[inp]
    assert handle.mmx_head_mean_live(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_head_mean_output_overlapping_the_slab_is_refused(lib):
    handle = lib.lib()
    args = _hm_args()
    args[2] = C.c_void_p(PTR + 4 * (5 * 4 * 12 * 20 - 1))         # the slab's last float
    assert handle.mmx_head_mean_live(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


@pytest.mark.parametrize("out", [10, 11, 12, 13])
@pytest.mark.parametrize("inp", ["text0", "text_last", "img0", "cross", "text_len"])
def test_rollout_output_aliasing_an_input_is_refused(lib, out, inp):
    handle = lib.lib()
    args, _keep = _ro_args(lib)
    where = {"text0": PTR + STEP * 10, "text_last": PTR + STEP * 14, "img0": PTR + STEP * 50, "cross": PTR + STEP * 1,
             "text_len": PTR + STEP * 2}[inp]
    args[out] = C.c_void_p(where)
    assert handle.mmx_lxmert_rollout(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


@pytest.mark.parametrize("pair", [(10, 11), (10, 12), (11, 13), (12, 13)])
def test_rollout_outputs_aliasing_each_other_are_refused(lib, pair):
    handle = lib.lib()
    args, _keep = _ro_args(lib)
    args[pair[1]] = args[pair[0]]
    assert handle.mmx_lxmert_rollout(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_workspace_query_is_positive_and_monotone_in_the_batch(lib):
    handle = lib.lib()
    last = 0
    for B in (1, 2, 5, 32, 33, 256):
        need = handle.mmx_lxmert_rollout_workspace_bytes(14, 9, B, 20, 36)
        assert need > 0 and need >= last and need >= 4 * B * 24 * 36 * 36
        last = need
    assert handle.mmx_lxmert_rollout_workspace_bytes(2, 1, 1, 1, 1) > 0
    assert handle.mmx_lxmert_rollout_workspace_bytes(MAX_TABLE, MAX_TABLE, 1, 48, 48) > 0
