"""CPU: the entry of the padded-batch ``generate_ours`` of VisualBERT (``mmx_selfattn_ours_row`` and its workspace query) is declared,
exported, bound and reachable through ``ops`` and the generator, and refuses bad arguments with ``MMX_EINVAL`` and a message before
any HIP call.  Every call here runs on made-up device addresses and every one of them is a REFUSAL: nothing in this file may pass the
argument checks (that NULL lengths are accepted is shown on real buffers by the ``-m gpu`` suite)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_selfattn_ours_row", "mmx_selfattn_ours_row_workspace_bytes")
PTR = 0x7f0000000000            # made-up device addresses: a launch on them would fail differently
STEP = 1 << 28                  # further apart than any operand of the shapes below is long
EINVAL = -22
MAX_TABLE = 32
ATTN0, GRAD0 = 10, 50           # the slots of the two tables' first entries
TEXT_LEN, VIS_LEN, OUT, WS = 3, 4, 2, 5


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


def _args(lib, n_layers=5, B=5, H=4, T=12, V=20, ws_bytes=None):
    """attn table, grad table, n_layers, B, H, T, V, text_len, vis_len, out, workspace, workspace_bytes, stream"""
    at, keep_a = _table(ATTN0, n_layers)
    gt, keep_g = _table(GRAD0, n_layers)
    need = lib.lib().mmx_selfattn_ours_row_workspace_bytes(n_layers, B, T, V)
    return [at, gt, n_layers, B, H, T, V, _p(TEXT_LEN), _p(VIS_LEN), _p(OUT), _p(WS), need if ws_bytes is None else ws_bytes,
            None], (keep_a, keep_g)


BAD_SIZES = [dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(T=1), dict(T=0), dict(T=-5), dict(V=0), dict(V=-2),
             dict(T=128, V=129), dict(T=257, V=1), dict(T=2, V=255), dict(T=1 << 20), dict(V=1 << 30), dict(n_layers=0),
             dict(n_layers=-1), dict(n_layers=MAX_TABLE + 1)]


def test_symbols_are_declared_exported_bound_and_callable_through_ops(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    assert callable(ops.selfattn_ours_row)
    assert callable(vb.SelfAttentionGenerator.generate_ours_padded_batch)
    assert callable(vb.GraphedGenerateOursPadded)
    assert vb.GraphedGenerateOursPadded is not vb.GraphedBaselinesBatch and "ours" not in vb.GraphedBaselinesBatch.METHODS


def test_the_declaration_cites_generate_ours(lib):
    with open(lib.HEADER_PATH) as fh:
        text = fh.read()
    at = text.index("mmx_selfattn_ours_row: generate_ours")
    assert "VisualBERT/mmf/models/transformers/backends/ExplanationGenerator.py:68-107" in text[at:at + 300]


def test_ops_refuse_host_tensors_and_mismatched_tables():
    import torch
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    x = torch.rand(1, 2, 5, 5)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.selfattn_ours_row([x, x], [x, x], n_text=3)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.selfattn_ours_row([x], [x], None, None, 3)
    with pytest.raises(MMXError):
        ops.selfattn_ours_row([], [], n_text=3)             # empty tables: refused before any device is asked for


@pytest.mark.parametrize("missing", [0, 1, 9, 10])
def test_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args, _keep = _args(lib)
    args[missing] = None
    assert handle.mmx_selfattn_ours_row(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("table", [0, 1])
@pytest.mark.parametrize("entry", [0, 2, 4])
def test_null_table_entries_are_refused(lib, table, entry):
    handle = lib.lib()
    args, keep = _args(lib)
    keep[table][entry] = None
    assert handle.mmx_selfattn_ours_row(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


def test_all_zero_arguments_are_refused(lib):
    handle = lib.lib()
    assert handle.mmx_selfattn_ours_row(None, None, 0, 0, 0, 0, 0, None, None, None, None, 0, None) < 0
    assert handle.mmx_last_error()
    assert handle.mmx_selfattn_ours_row_workspace_bytes(0, 0, 0, 0) == 0


@pytest.mark.parametrize("sizes", BAD_SIZES)
def test_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    """``B, H <= 0``, sizes outside ``T >= 2, V >= 1, T + V <= 256``, an empty table and one longer than the compiled maximum."""
    handle = lib.lib()
    args, _keep = _args(lib, **sizes)
    if "H" not in sizes:                                # the query takes no H; for everything else it answers 0
        assert handle.mmx_selfattn_ours_row_workspace_bytes(args[2], args[3], args[5], args[6]) == 0
    args[11] = 1 << 30                                  # (the refusal is about the size, not about the workspace)
    assert handle.mmx_selfattn_ours_row(*args) == EINVAL
    assert handle.mmx_last_error()


@pytest.mark.parametrize("B,n_layers,T,V", [(1 << 26, 32, 128, 128), (1 << 30, 1, 128, 128), (2147483647, 1, 2, 1),
                                            ((1 << 31) // 25 + 1, 1, 124, 100)])
def test_a_grid_beyond_one_dimension_is_refused(lib, B, n_layers, T, V):
    """``B x n_layers x ceil(N^2 / 2048)`` workgroups must fit a one-dimensional grid (2^31 - 1); the refusal comes before the
    workspace is looked at."""
    handle = lib.lib()
    strips = ((T + V) ** 2 + 2047) // 2048
    args, _keep = _args(lib, n_layers=n_layers, B=B, T=T, V=V, ws_bytes=(1 << 63) - 1)
    if B * n_layers * strips > (1 << 31) - 1:
        assert handle.mmx_selfattn_ours_row(*args) == EINVAL
        assert b"grid" in handle.mmx_last_error()
    else:                                               # the largest B of a single strip fits the grid: refused for its workspace
        args[11] = 16
        assert handle.mmx_selfattn_ours_row(*args) == EINVAL
        assert b"workspace" in handle.mmx_last_error()


def test_workspaces_smaller_than_the_query_are_refused(lib):
    handle = lib.lib()
    need = handle.mmx_selfattn_ours_row_workspace_bytes(5, 5, 12, 20)
    assert need > 0
    for short in (0, need - 1):
        args, _keep = _args(lib, ws_bytes=short)
        assert handle.mmx_selfattn_ours_row(*args) == EINVAL
        assert b"workspace" in handle.mmx_last_error()


def test_a_misaligned_workspace_is_refused(lib):
    handle = lib.lib()
    args, _keep = _args(lib)
    args[10] = C.c_void_p(PTR + STEP * WS + 8)
    args[11] += 16
    assert handle.mmx_selfattn_ours_row(*args) == EINVAL
    assert b"aligned" in handle.mmx_last_error()


@pytest.mark.parametrize("out", [9, 10])
@pytest.mark.parametrize("inp", ["attn0", "attn_last", "grad0", "grad_last", "text_len", "vis_len"])
def test_output_or_workspace_aliasing_an_input_is_refused(lib, out, inp):
    handle = lib.lib()
    args, _keep = _args(lib)
    where = {"attn0": ATTN0, "attn_last": ATTN0 + 4, "grad0": GRAD0, "grad_last": GRAD0 + 4, "text_len": TEXT_LEN,
             "vis_len": VIS_LEN}[inp]
    args[out] = C.c_void_p(PTR + STEP * where)
    assert handle.mmx_selfattn_ours_row(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_output_overlapping_a_slab_s_last_float_or_the_workspace_is_refused(lib):
    handle = lib.lib()
    for slot in (ATTN0 + 1, GRAD0 + 3):
        args, _keep = _args(lib)
        args[9] = C.c_void_p(PTR + STEP * slot + 4 * (5 * 4 * 32 * 32 - 1))
        assert handle.mmx_selfattn_ours_row(*args) == EINVAL
        assert b"alias" in handle.mmx_last_error()
    args, _keep = _args(lib)
    args[9] = args[10]
    assert handle.mmx_selfattn_ours_row(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()
    args, _keep = _args(lib)
    args[9] = C.c_void_p(PTR + STEP * WS + args[11] - 4)              # the workspace's last float
    assert handle.mmx_selfattn_ours_row(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_the_workspace_query_is_positive_and_monotone_in_the_batch(lib):
    handle = lib.lib()
    last = 0
    for B in (1, 2, 5, 32, 33, 256):
        need = handle.mmx_selfattn_ours_row_workspace_bytes(12, B, 24, 100)
        assert need > last and need >= 4 * B * 12 * 124 * 124
        last = need
    assert handle.mmx_selfattn_ours_row_workspace_bytes(1, 1, 2, 1) > 0
    assert handle.mmx_selfattn_ours_row_workspace_bytes(MAX_TABLE, 1, 128, 100) > 0
    assert handle.mmx_selfattn_ours_row_workspace_bytes(MAX_TABLE, 1, 128, 128) > 0
    for bad in ((0, 1, 24, 100), (MAX_TABLE + 1, 1, 24, 100), (1, 0, 24, 100), (1, 1, 1, 100), (1, 1, 24, 0), (1, 1, 200, 100)):
        assert handle.mmx_selfattn_ours_row_workspace_bytes(*bad) == 0
