"""CPU: the entries of the batched VisualBERT baselines (``mmx_selfattn_row_live``, ``mmx_selfattn_rollout_row`` and their workspace
queries) are declared, exported, bound and reachable through ``ops`` and the generator, and refuse bad arguments with ``MMX_EINVAL``
and a message before any HIP call.  Every call here runs on made-up device addresses and every one of them is a REFUSAL: nothing in
this file may pass the argument checks (that NULL ``grad`` / lengths are accepted is shown on real buffers by the ``-m gpu`` suite)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_selfattn_row_live", "mmx_selfattn_row_live_workspace_bytes", "mmx_selfattn_rollout_row",
         "mmx_selfattn_rollout_row_workspace_bytes")
PTR = 0x7f0000000000            # made-up device addresses: a launch on them would fail differently
STEP = 1 << 28                  # further apart than any operand of the shapes below is long
EINVAL = -22
MAX_TABLE = 32
MAX_N = 256


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


def _row_args(lib, B=5, H=4, T=12, V=20, grad=True, ws_bytes=None):
    """attn, grad, out, B, H, T, V, text_len, vis_len, workspace, workspace_bytes, stream"""
    need = lib.lib().mmx_selfattn_row_live_workspace_bytes(B, H, T, V)
    return [_p(0), _p(1) if grad else None, _p(2), B, H, T, V, _p(3), _p(4), _p(5), need if ws_bytes is None else ws_bytes, None]


def _ro_args(lib, n_layers=5, B=5, H=4, T=12, V=20, ws_bytes=None):
    """table, n_layers, B, H, T, V, text_len, vis_len, out, workspace, workspace_bytes, stream"""
    tbl, keep = _table(10, n_layers)
    need = lib.lib().mmx_selfattn_rollout_row_workspace_bytes(n_layers, B, T, V)
    return [tbl, n_layers, B, H, T, V, _p(3), _p(4), _p(2), _p(5), need if ws_bytes is None else ws_bytes, None], keep


BAD_SIZES = [dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(T=1), dict(T=0), dict(T=-5), dict(V=0), dict(V=-2),
             dict(T=128, V=129), dict(T=257, V=1), dict(T=2, V=255), dict(T=1 << 20), dict(V=1 << 30)]


def test_symbols_are_declared_exported_bound_and_callable_through_ops(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    assert callable(ops.selfattn_raw_row) and callable(ops.selfattn_gradcam_row) and callable(ops.selfattn_rollout_row)
    for method in ("generate_rollout_batch", "generate_raw_attn_batch", "generate_attn_gradcam_batch"):
        assert callable(getattr(vb.SelfAttentionGenerator, method))
    assert callable(vb.unpad_row)
    assert vb.GraphedBaselinesBatch.METHODS == ("rollout", "raw_attn", "attn_gradcam")
    assert ops.SELFATTN_MAX_TOKENS == MAX_N and lib.BASELINES_MAX_TABLE == MAX_TABLE


def test_ops_refuse_host_tensors():
    import torch
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    x = torch.rand(1, 2, 5, 5)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.selfattn_raw_row(x, n_text=3)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.selfattn_gradcam_row(x, x, n_text=3)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.selfattn_rollout_row([x, x], n_text=3)


def test_unpad_row_is_the_per_item_layout():
    import torch
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    scores = torch.arange(2 * 9, dtype=torch.float32).reshape(2, 9)               # T = 5, V = 4
    row = vb.unpad_row(scores, 1, 3, padded_text=5)
    assert row.shape == (1, 7) and row[0].tolist() == [9.0, 10.0, 11.0, 14.0, 15.0, 16.0, 17.0]
    with pytest.raises(ValueError):
        vb.unpad_row(scores, 0, 6, padded_text=5)
    with pytest.raises(TypeError):
        vb.unpad_row(scores, 0, 3)                      # the padded text width is a required argument


@pytest.mark.parametrize("missing", [0, 2, 9])
def test_row_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args = _row_args(lib)
    args[missing] = None
    assert handle.mmx_selfattn_row_live(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("missing", [0, 8, 9])
def test_rollout_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args, _keep = _ro_args(lib)
    args[missing] = None
    assert handle.mmx_selfattn_rollout_row(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("entry", [0, 2, 4])
def test_rollout_null_table_entries_are_refused(lib, entry):
    handle = lib.lib()
    args, keep = _ro_args(lib)
    keep[entry] = None
    assert handle.mmx_selfattn_rollout_row(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", BAD_SIZES)
def test_row_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    handle = lib.lib()
    args = _row_args(lib, **sizes)
    assert handle.mmx_selfattn_row_live_workspace_bytes(args[3], args[4], args[5], args[6]) == 0
    args[10] = 1 << 30                                  # (the refusal is about the size, not about the workspace)
    assert handle.mmx_selfattn_row_live(*args) == EINVAL
    assert handle.mmx_last_error()
    args[1] = None
    assert handle.mmx_selfattn_row_live(*args) == EINVAL


@pytest.mark.parametrize("sizes", BAD_SIZES + [dict(n_layers=0), dict(n_layers=-1), dict(n_layers=MAX_TABLE + 1)])
def test_rollout_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    """``B, H <= 0``, sizes outside the limits, an empty table and one longer than the compiled maximum."""
    handle = lib.lib()
    args, _keep = _ro_args(lib, **sizes)
    if "H" not in sizes:                                # the query takes no H; for everything else it answers 0
        assert handle.mmx_selfattn_rollout_row_workspace_bytes(args[1], args[2], args[4], args[5]) == 0
    args[10] = 1 << 30
    assert handle.mmx_selfattn_rollout_row(*args) == EINVAL
    assert handle.mmx_last_error()


def test_workspaces_smaller_than_the_query_are_refused(lib):
    handle = lib.lib()
    need = handle.mmx_selfattn_row_live_workspace_bytes(5, 4, 12, 20)
    for short in (0, need - 1):
        assert handle.mmx_selfattn_row_live(*_row_args(lib, ws_bytes=short)) == EINVAL
        assert b"workspace" in handle.mmx_last_error()
    need = handle.mmx_selfattn_rollout_row_workspace_bytes(5, 5, 12, 20)
    for short in (0, need - 1):
        args, _keep = _ro_args(lib, ws_bytes=short)
        assert handle.mmx_selfattn_rollout_row(*args) == EINVAL
        assert b"workspace" in handle.mmx_last_error()


def test_misaligned_workspaces_are_refused(lib):
    handle = lib.lib()
    args = _row_args(lib)
    args[9] = C.c_void_p(PTR + STEP * 5 + 4)
    args[10] += 16
    assert handle.mmx_selfattn_row_live(*args) == EINVAL
    assert b"aligned" in handle.mmx_last_error()
    args, _keep = _ro_args(lib)
    args[9] = C.c_void_p(PTR + STEP * 5 + 8)
    args[10] += 16
    assert handle.mmx_selfattn_rollout_row(*args) == EINVAL
    assert b"aligned" in handle.mmx_last_error()


@pytest.mark.parametrize("out", [2, 9])
@pytest.mark.parametrize("inp", [0, 1, 7, 8])
def test_row_output_or_workspace_aliasing_an_input_is_refused(lib, out, inp):
    handle = lib.lib()
    args = _row_args(lib)
    args[out] = args[inp]
    assert handle.mmx_selfattn_row_live(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_row_output_overlapping_the_slab_or_the_workspace_is_refused(lib):
    handle = lib.lib()
    args = _row_args(lib)
    args[2] = C.c_void_p(PTR + 4 * (5 * 4 * 32 * 32 - 1))         # the slab's last float
    assert handle.mmx_selfattn_row_live(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()
    args = _row_args(lib)
    args[2] = C.c_void_p(PTR + STEP * 5 + args[10] - 4)            # the workspace's last float
    assert handle.mmx_selfattn_row_live(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


@pytest.mark.parametrize("out", [8, 9])
@pytest.mark.parametrize("inp", ["table0", "table_last", "text_len", "vis_len"])
def test_rollout_output_or_workspace_aliasing_an_input_is_refused(lib, out, inp):
    handle = lib.lib()
    args, _keep = _ro_args(lib)
    where = {"table0": PTR + STEP * 10, "table_last": PTR + STEP * 14, "text_len": PTR + STEP * 3, "vis_len": PTR + STEP * 4}[inp]
    args[out] = C.c_void_p(where)
    assert handle.mmx_selfattn_rollout_row(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_rollout_output_aliasing_the_workspace_is_refused(lib):
    handle = lib.lib()
    args, _keep = _ro_args(lib)
    args[8] = args[9]
    assert handle.mmx_selfattn_rollout_row(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_workspace_queries_are_positive_and_monotone_in_the_batch(lib):
    handle = lib.lib()
    last_row = last_ro = 0
    for B in (1, 2, 5, 32, 33, 256):
        row = handle.mmx_selfattn_row_live_workspace_bytes(B, 12, 24, 100)
        ro = handle.mmx_selfattn_rollout_row_workspace_bytes(12, B, 24, 100)
        assert row > 0 and row >= last_row and row >= 4 * B * (12 + 124)
        assert ro > 0 and ro >= last_ro and ro >= 4 * B * 12 * 124 * 124
        last_row, last_ro = row, ro
    assert handle.mmx_selfattn_row_live_workspace_bytes(1, 1, 2, 1) > 0
    assert handle.mmx_selfattn_row_live_workspace_bytes(1, 1, 128, 100) > 0
    assert handle.mmx_selfattn_row_live_workspace_bytes(1, 1, 128, 128) > 0
    assert handle.mmx_selfattn_rollout_row_workspace_bytes(1, 1, 2, 1) > 0
    assert handle.mmx_selfattn_rollout_row_workspace_bytes(MAX_TABLE, 1, 128, 100) > 0
