"""CPU: the entries of the batched DETR baselines (``mmx_detr_cross_rows``, ``mmx_detr_rollout_rows`` and their workspace queries) are
declared, exported, bound and reachable through ``ops`` and the generator, and refuse bad arguments with ``MMX_EINVAL`` and a message
before any HIP call.  Every call here runs on made-up device addresses and every one of them is a REFUSAL: nothing in this file may
pass the argument checks (that a NULL gradient is accepted is shown on real buffers by the ``-m gpu`` suite)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_detr_cross_rows", "mmx_detr_cross_rows_workspace_bytes", "mmx_detr_rollout_rows", "mmx_detr_rollout_rows_workspace_bytes")
PTR = 0x7f0000000000            # made-up device addresses: a launch on them would fail differently
STEP = 1 << 28                  # further apart than any operand of the shapes below is long
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


def _cross_args(lib, K=5, H=4, Q=10, Ni=35, grad=True, shared=False, ws_bytes=None):
    """0 cross_attn, 1 cross_grad, 2 grad_bstride, 3 targets, 4 out, 5 K, 6 H, 7 Q, 8 Ni, 9 workspace, 10 workspace_bytes, 11 stream"""
    need = lib.lib().mmx_detr_cross_rows_workspace_bytes(K, H, Q, Ni)
    return [_p(0), _p(1) if grad else None, 0 if shared else H * Q * Ni, _p(3), _p(2), K, H, Q, Ni, _p(5),
            need if ws_bytes is None else ws_bytes, None]


def _ro_args(lib, n_enc=3, n_dec=2, K=5, H=4, Q=10, Ni=35, ws_bytes=None):
    """0 enc_table, 1 n_enc, 2 dec_table, 3 n_dec, 4 cross_attn, 5 targets, 6 out, 7 K, 8 H, 9 Q, 10 Ni, 11 workspace,
    12 workspace_bytes, 13 stream"""
    enc, keep_e = _table(10, n_enc)
    dec, keep_d = _table(50, n_dec)
    need = lib.lib().mmx_detr_rollout_rows_workspace_bytes(n_enc, n_dec, K, Q, Ni)
    return [enc, n_enc, dec, n_dec, _p(0), _p(3), _p(2), K, H, Q, Ni, _p(5), need if ws_bytes is None else ws_bytes, None], keep_e, keep_d


BAD_SIZES = [dict(Q=0), dict(Q=129), dict(Q=-1), dict(Ni=0), dict(Ni=2049), dict(Ni=-7), dict(H=0), dict(H=33), dict(H=-2), dict(K=0),
             dict(K=-3), dict(Q=1 << 20), dict(Ni=1 << 30)]
BAD_TABLES = [dict(n_enc=0), dict(n_dec=0), dict(n_enc=-1), dict(n_enc=MAX_TABLE + 1), dict(n_dec=MAX_TABLE + 1)]


def test_symbols_are_declared_exported_bound_and_callable(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2 and lib.ABI_VERSION == 2
    from transformer_mm_explainability_amd import detr_explainability as de
    from transformer_mm_explainability_amd import ops
    assert callable(ops.detr_raw_rows) and callable(ops.detr_gradcam_rows) and callable(ops.detr_rollout_rows)
    for method in ("generate_rollout_multi", "generate_raw_attn_multi", "generate_attn_gradcam_multi"):
        assert callable(getattr(de.Generator, method))
    assert de.GraphedBaselinesMulti.METHODS == ("rollout", "raw_attn", "attn_gradcam")
    assert lib.BASELINES_MAX_TABLE == MAX_TABLE and ops.DETR_BASELINES_MAX_TOKENS == 2048


def test_mask_generator_takes_the_option_and_defaults_to_the_per_query_route():
    import inspect
    from transformer_mm_explainability_amd import detr_explainability as de
    sig = inspect.signature(de.MaskGenerator.__init__)
    assert sig.parameters["batch_baselines"].default is False
    assert set(de.MaskGenerator._BASELINES_MULTI) == {"rollout", "raw_attn", "attn_gradcam"}
    assert set(de.MaskGenerator._BASELINES_MULTI) <= set(de.MaskGenerator._PER_QUERY)
    import torch.nn as nn
    with pytest.raises(ValueError):
        de.GraphedBaselinesMulti(nn.Identity(), None, "ours")


def test_the_truncated_backward_is_an_optional_argument():
    import inspect
    from transformer_mm_explainability_amd import detr_model
    for cls in (detr_model.Transformer, detr_model.DETRFromFeatures):
        assert inspect.signature(cls.backward_shared).parameters["stop_after_top_cross"].default is False


def test_ops_refuse_host_tensors():
    import torch
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    P, A, B, t = torch.rand(2, 3, 5), torch.rand(2, 5, 5), torch.rand(2, 3, 3), torch.tensor([0, 2])
    with pytest.raises(MMXError, match="no CPU path"):
        ops.detr_raw_rows(P, t)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.detr_gradcam_rows(P, P, t)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.detr_rollout_rows([A], [B], P, t)


@pytest.mark.parametrize("missing", [0, 3, 4, 9])
def test_cross_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args = _cross_args(lib)
    args[missing] = None
    assert handle.mmx_detr_cross_rows(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("missing", [0, 3])
def test_raw_form_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args = _cross_args(lib, grad=False)
    args[missing] = None
    assert handle.mmx_detr_cross_rows(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("missing", [0, 2, 4, 5, 6, 11])
def test_rollout_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args, _e, _d = _ro_args(lib)
    args[missing] = None
    assert handle.mmx_detr_rollout_rows(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("which,entry", [("enc", 0), ("enc", 2), ("dec", 0), ("dec", 1)])
def test_rollout_null_table_entries_are_refused(lib, which, entry):
    handle = lib.lib()
    args, keep_e, keep_d = _ro_args(lib)
    (keep_e if which == "enc" else keep_d)[entry] = None
    assert handle.mmx_detr_rollout_rows(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", BAD_SIZES)
def test_cross_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    handle = lib.lib()
    args = _cross_args(lib, **sizes)
    assert handle.mmx_detr_cross_rows_workspace_bytes(args[5], args[6], args[7], args[8]) == 0
    args[10] = 1 << 30                                  # (the refusal is about the size, not about the workspace)
    assert handle.mmx_detr_cross_rows(*args) == EINVAL
    assert handle.mmx_last_error()
    args[1] = None
    assert handle.mmx_detr_cross_rows(*args) == EINVAL


def test_a_gradient_stride_that_is_neither_zero_nor_a_slab_is_refused(lib):
    handle = lib.lib()
    args = _cross_args(lib)
    for bad in (1, args[2] - 1, args[2] + 1, -args[2], 2 * args[2]):
        args[2] = bad
        assert handle.mmx_detr_cross_rows(*args) == EINVAL
        assert b"grad_bstride" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", BAD_SIZES + BAD_TABLES)
def test_rollout_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    """Sizes outside the limits, an empty table and one longer than the compiled maximum."""
    handle = lib.lib()
    args, _e, _d = _ro_args(lib, **sizes)
    if "H" not in sizes:                                # the query takes no H; for everything else it answers 0
        assert handle.mmx_detr_rollout_rows_workspace_bytes(args[1], args[3], args[7], args[9], args[10]) == 0
    args[12] = 1 << 30
    assert handle.mmx_detr_rollout_rows(*args) == EINVAL
    assert handle.mmx_last_error()


def test_workspaces_smaller_than_the_query_are_refused(lib):
    handle = lib.lib()
    need = handle.mmx_detr_cross_rows_workspace_bytes(5, 4, 10, 35)
    for short in (0, need - 1):
        assert handle.mmx_detr_cross_rows(*_cross_args(lib, ws_bytes=short)) == EINVAL
        assert b"workspace" in handle.mmx_last_error()
    need = handle.mmx_detr_rollout_rows_workspace_bytes(3, 2, 5, 10, 35)
    for short in (0, need - 1):
        args, _e, _d = _ro_args(lib, ws_bytes=short)
        assert handle.mmx_detr_rollout_rows(*args) == EINVAL
        assert b"workspace" in handle.mmx_last_error()


def test_misaligned_workspaces_are_refused(lib):
    handle = lib.lib()
    args = _cross_args(lib)
    args[9] = C.c_void_p(PTR + STEP * 5 + 4)
    args[10] += 16
    assert handle.mmx_detr_cross_rows(*args) == EINVAL
    assert b"aligned" in handle.mmx_last_error()
    args, _e, _d = _ro_args(lib)
    args[11] = C.c_void_p(PTR + STEP * 5 + 8)
    args[12] += 16
    assert handle.mmx_detr_rollout_rows(*args) == EINVAL
    assert b"aligned" in handle.mmx_last_error()


@pytest.mark.parametrize("out", [4, 9])
@pytest.mark.parametrize("inp", [0, 1, 3])
def test_cross_output_or_workspace_aliasing_an_input_is_refused(lib, out, inp):
    handle = lib.lib()
    args = _cross_args(lib)
    args[out] = args[inp]
    assert handle.mmx_detr_cross_rows(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_cross_output_overlapping_a_slab_or_the_workspace_is_refused(lib):
    handle = lib.lib()
    args = _cross_args(lib)
    args[4] = C.c_void_p(PTR + 4 * (4 * 10 * 35 - 1))              # the probability slab's last float
    assert handle.mmx_detr_cross_rows(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()
    args = _cross_args(lib)
    args[4] = C.c_void_p(PTR + STEP + 4 * (5 * 4 * 10 * 35 - 1))   # the LAST sample's gradient slab: per-sample slabs are K long
    assert handle.mmx_detr_cross_rows(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()
    args = _cross_args(lib)
    args[4] = C.c_void_p(PTR + STEP * 5 + args[10] - 4)            # the workspace's last float
    assert handle.mmx_detr_cross_rows(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()
    args = _cross_args(lib, grad=False)
    args[4] = args[3]                                               # the raw form checks its output too
    assert handle.mmx_detr_cross_rows(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


@pytest.mark.parametrize("out", [6, 11])
@pytest.mark.parametrize("inp", ["enc0", "enc_last", "dec0", "dec_last", "cross", "targets"])
def test_rollout_output_or_workspace_aliasing_an_input_is_refused(lib, out, inp):
    handle = lib.lib()
    args, _e, _d = _ro_args(lib)
    where = {"enc0": PTR + STEP * 10, "enc_last": PTR + STEP * 12, "dec0": PTR + STEP * 50, "dec_last": PTR + STEP * 51,
             "cross": PTR, "targets": PTR + STEP * 3}[inp]
    args[out] = C.c_void_p(where)
    assert handle.mmx_detr_rollout_rows(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_rollout_output_aliasing_the_workspace_is_refused(lib):
    handle = lib.lib()
    args, _e, _d = _ro_args(lib)
    args[6] = args[11]
    assert handle.mmx_detr_rollout_rows(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_workspace_queries_are_positive_and_monotone_in_k(lib):
    handle = lib.lib()
    last_c = last_r = 0
    for K in (1, 2, 5, 16, 17, 100):
        c = handle.mmx_detr_cross_rows_workspace_bytes(K, 8, 100, 950)
        r = handle.mmx_detr_rollout_rows_workspace_bytes(6, 6, K, 100, 950)
        assert c > 0 and c >= last_c and c >= 4 * K * 8
        assert r > 0 and r >= last_r and r >= 4 * (6 * 950 * 950 + K * 950)
        last_c, last_r = c, r
    assert handle.mmx_detr_cross_rows_workspace_bytes(1, 1, 1, 1) > 0
    assert handle.mmx_detr_cross_rows_workspace_bytes(1, 32, 128, 2048) > 0
    assert handle.mmx_detr_rollout_rows_workspace_bytes(1, 1, 1, 1, 1) > 0
    assert handle.mmx_detr_rollout_rows_workspace_bytes(MAX_TABLE, MAX_TABLE, 1, 128, 2048) > 0
