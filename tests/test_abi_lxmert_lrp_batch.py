"""CPU: the entries of the batched LXMERT LRP methods (``mmx_lxmert_attr``, ``mmx_lxmert_attr_workspace_bytes``,
``mmx_head_minmax_live``) are declared, exported, bound and reachable through ``ops`` and the generators, and refuse bad arguments
with ``MMX_EINVAL`` and a message before any HIP call (every call here runs on made-up device addresses, on a machine without a
GPU)."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_lxmert_attr", "mmx_lxmert_attr_workspace_bytes", "mmx_head_minmax_live")
PTR = 0x7f0000000000            # made-up device addresses: a launch on them would fail differently
STEP = 1 << 26                  # further apart than any operand of the shapes below is long
EINVAL = -22
MAX_TABLE = 32
# positions in the argument list of mmx_lxmert_attr
TEXT_C, TEXT_G, N_TEXT, IMG_C, IMG_G, N_IMG, CROSS_C, CROSS_G, B_, H_, T_, I_, TEXT_LEN, R_TT, R_TI, R_II, WS, WS_BYTES, STREAM = range(19)


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


def _mm_args(B=5, H=4, Nq=12, Nk=20, flags=0):
    """cam, out, B, H, Nq, Nk, q_len, k_len, flags, stream"""
    return [_p(0), _p(2), B, H, Nq, Nk, _p(3), _p(4), flags, None]


def _at_args(lib, n_text=5, n_img=4, B=5, H=4, T=12, I=20, ws_bytes=None):
    """The argument list of ``mmx_lxmert_attr`` (positions above): cam tables at slots 10.. / 90.., gradient tables at 50.. / 130.."""
    tc, keep_tc = _table(10, n_text)
    tg, keep_tg = _table(50, n_text)
    ic, keep_ic = _table(90, n_img)
    ig, keep_ig = _table(130, n_img)
    need = lib.lib().mmx_lxmert_attr_workspace_bytes(n_text, n_img, B, T, I)
    args = [tc, tg, n_text, ic, ig, n_img, _p(0), _p(1), B, H, T, I, _p(2), _p(3), _p(4), _p(5), _p(6),
            need if ws_bytes is None else ws_bytes, None]
    return args, dict(text_c=keep_tc, text_g=keep_tg, img_c=keep_ic, img_g=keep_ig)


def test_symbols_are_declared_exported_bound_and_callable_through_ops(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2
    from transformer_mm_explainability_amd import lxmert_explainability as le
    from transformer_mm_explainability_amd import ops
    assert callable(ops.lxmert_transformer_attr) and callable(ops.head_minmax_live)
    for method in ("generate_transformer_attr_batch", "generate_partial_lrp_batch"):
        assert callable(getattr(le.GeneratorBaselines, method))
    use_lrp = inspect.signature(le.GeneratorOurs.generate_ours_batch).parameters["use_lrp"]
    assert use_lrp.default is False
    assert le.GraphedBaselinesBatch.METHODS == ("rollout", "raw_attn", "attn_gradcam")


def test_header_cites_the_reference_lines():
    text = open(os.path.join(ROOT, "include", "mmx_relevancy.h")).read()
    block = text[text.index(" * mmx_lxmert_attr:"):text.index("int mmx_head_minmax_live(")]
    assert ":373-460" in block and ":489-505" in block


def test_ops_refuse_host_tensors():
    import torch
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    x = torch.rand(1, 2, 3, 3)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.head_minmax_live(x)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.lxmert_transformer_attr([(x, x)], [(x, x)], (x, x))


def test_batched_lrp_methods_need_a_body_with_relprop_and_at_most_48_tokens():
    import torch
    from transformer_mm_explainability_amd import lxmert_explainability as le

    class NoRelprop(torch.nn.Module):
        def forward(self, **kw):
            raise AssertionError("must not run the body before checking for relprop")

    class TooLong(NoRelprop):
        def relprop(self, *a, **kw):
            raise AssertionError("must not run the LRP pass before checking the sizes")

    def usage(model):
        return type("Usage", (), {"model": model})()

    inputs = dict(input_ids=torch.zeros(2, 5, dtype=torch.long), visual_feats=torch.zeros(2, 7, 4))
    for call in (lambda m: le.GeneratorBaselines(usage(m)).generate_transformer_attr_batch(inputs),
                 lambda m: le.GeneratorBaselines(usage(m)).generate_partial_lrp_batch(inputs),
                 lambda m: le.GeneratorOurs(usage(m)).generate_ours_batch(inputs, use_lrp=True)):
        with pytest.raises(NotImplementedError, match="relprop"):
            call(NoRelprop())
    long_inputs = dict(input_ids=torch.zeros(2, 49, dtype=torch.long), visual_feats=torch.zeros(2, 7, 4))
    for call in (lambda m: le.GeneratorBaselines(usage(m)).generate_transformer_attr_batch(long_inputs),
                 lambda m: le.GeneratorBaselines(usage(m)).generate_partial_lrp_batch(long_inputs),
                 lambda m: le.GeneratorOurs(usage(m)).generate_ours_batch(long_inputs, use_lrp=True)):
        with pytest.raises(NotImplementedError, match="48"):
            call(TooLong())


def test_all_null_and_all_zero_arguments_are_refused(lib):
    handle = lib.lib()
    assert handle.mmx_head_minmax_live(None, None, 0, 0, 0, 0, None, None, 0, None) == EINVAL
    assert handle.mmx_last_error()
    assert handle.mmx_lxmert_attr(None, None, 0, None, None, 0, None, None, 0, 0, 0, 0, None, None, None, None, None, 0, None) == EINVAL
    assert handle.mmx_last_error()
    assert handle.mmx_lxmert_attr_workspace_bytes(0, 0, 0, 0, 0) == 0


@pytest.mark.parametrize("missing", [0, 1])
def test_minmax_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args = _mm_args()
    args[missing] = None
    assert handle.mmx_head_minmax_live(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("missing", [TEXT_C, TEXT_G, IMG_C, IMG_G, CROSS_C, CROSS_G, R_TT, R_TI, R_II, WS])
def test_attr_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args, _keep = _at_args(lib)
    args[missing] = None
    assert handle.mmx_lxmert_attr(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("which", ["text_c", "text_g", "img_c", "img_g"])
def test_attr_null_table_entries_are_refused(lib, which):
    handle = lib.lib()
    args, keep = _at_args(lib)
    keep[which][2] = None
    assert handle.mmx_lxmert_attr(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(Nq=0), dict(Nq=-2), dict(Nq=49), dict(Nk=0),
                                   dict(Nk=49), dict(Nk=1 << 20), dict(flags=2), dict(flags=0x80000000)])
def test_minmax_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    handle = lib.lib()
    assert handle.mmx_head_minmax_live(*_mm_args(**sizes)) == EINVAL
    assert handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(B=0), dict(B=-3), dict(H=0), dict(H=-1), dict(T=0), dict(T=49), dict(T=-5), dict(I=0),
                                   dict(I=49), dict(n_text=0), dict(n_text=-1), dict(n_img=0), dict(n_img=-2),
                                   dict(n_text=MAX_TABLE + 1), dict(n_img=MAX_TABLE + 1)])
def test_attr_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    """``B, H <= 0``, sizes outside 1..48, ``n_text < 1``, ``n_img < 1`` and tables longer than the compiled maximum."""
    handle = lib.lib()
    args, _keep = _at_args(lib, **sizes)
    if "H" not in sizes:                                # the query takes no H; for everything else it answers 0
        assert handle.mmx_lxmert_attr_workspace_bytes(args[N_TEXT], args[N_IMG], args[B_], args[T_], args[I_]) == 0
    args[WS_BYTES] = 1 << 30                            # (the refusal is about the size, not about the workspace)
    assert handle.mmx_lxmert_attr(*args) == EINVAL
    assert handle.mmx_last_error()


def test_attr_takes_tables_of_one(lib):
    assert lib.lib().mmx_lxmert_attr_workspace_bytes(1, 1, 1, 1, 1) > 0
    assert lib.lib().mmx_lxmert_attr_workspace_bytes(MAX_TABLE, MAX_TABLE, 1, 48, 48) > 0


def test_attr_workspace_smaller_than_the_query_is_refused(lib):
    handle = lib.lib()
    need = handle.mmx_lxmert_attr_workspace_bytes(5, 4, 5, 12, 20)
    for short in (0, need - 1):
        args, _keep = _at_args(lib, ws_bytes=short)
        assert handle.mmx_lxmert_attr(*args) == EINVAL
        assert b"workspace" in handle.mmx_last_error()


def test_attr_misaligned_workspace_is_refused(lib):
    handle = lib.lib()
    args, _keep = _at_args(lib)
    args[WS] = C.c_void_p(PTR + STEP * 6 + 4)
    args[WS_BYTES] += 16
    assert handle.mmx_lxmert_attr(*args) == EINVAL
    assert b"aligned" in handle.mmx_last_error()


@pytest.mark.parametrize("inp", [0, 6, 7])
def test_minmax_output_aliasing_an_input_is_refused(lib, inp):
    handle = lib.lib()
    args = _mm_args()
    args[1] = args[inp]
    assert handle.mmx_head_minmax_live(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_minmax_output_overlapping_the_slab_is_refused(lib):
    handle = lib.lib()
    args = _mm_args()
    args[1] = C.c_void_p(PTR + 4 * (5 * 4 * 12 * 20 - 1))         # the slab's last float
    assert handle.mmx_head_minmax_live(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


@pytest.mark.parametrize("out", [R_TT, R_TI, R_II, WS])
@pytest.mark.parametrize("inp", ["text_c0", "text_g_last", "img_c0", "img_g_last", "cross_c", "cross_g", "text_len"])
def test_attr_output_aliasing_an_input_is_refused(lib, out, inp):
    handle = lib.lib()
    args, _keep = _at_args(lib)
    where = {"text_c0": PTR + STEP * 10, "text_g_last": PTR + STEP * 54, "img_c0": PTR + STEP * 90, "img_g_last": PTR + STEP * 133,
             "cross_c": PTR, "cross_g": PTR + STEP * 1, "text_len": PTR + STEP * 2}[inp]
    args[out] = C.c_void_p(where)
    assert handle.mmx_lxmert_attr(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


@pytest.mark.parametrize("pair", [(R_TT, R_TI), (R_TT, R_II), (R_TI, R_II), (R_TT, WS), (R_TI, WS), (R_II, WS)])
def test_attr_outputs_aliasing_each_other_are_refused(lib, pair):
    handle = lib.lib()
    args, _keep = _at_args(lib)
    args[pair[1]] = args[pair[0]]
    assert handle.mmx_lxmert_attr(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_workspace_query_is_positive_and_monotone_in_the_batch(lib):
    handle = lib.lib()
    last = 0
    for B in (1, 2, 5, 32, 33, 256):
        need = handle.mmx_lxmert_attr_workspace_bytes(14, 9, B, 20, 36)
        assert need > 0 and need >= last and need >= 4 * B * 23 * 36 * 36
        last = need


def test_evaluator_offers_the_batch_lrp_flag():
    text = open(os.path.join(ROOT, "examples", "lxmert_perturbation_eval.py")).read()
    assert '"--batch-lrp"' in text and "choices=(0, 1), default=0" in text
