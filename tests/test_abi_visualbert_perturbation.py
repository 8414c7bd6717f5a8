"""CPU: the two entries of the batched VisualBERT perturbation test (``mmx_selfattn_perturb_regions``, ``mmx_selfattn_perturb_text``)
are declared, exported, bound and reachable through ``ops`` and ``VisualBertPerturbation``, and refuse bad arguments with ``MMX_EINVAL``
and a message before any HIP call.  Every call here runs on made-up device addresses and every one of them is a REFUSAL (the pattern of
``tests/test_abi_visualbert_baselines.py``); ``pad_rows`` is the inverse of ``unpad_row``."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mmx_selfattn_perturb_regions", "mmx_selfattn_perturb_text")
PTR = 0x7f0000000000            # made-up device addresses: a launch on them would fail differently
STEP = 1 << 28                  # further apart than any operand of the shapes below is long
EINVAL = -22


@pytest.fixture(scope="module")
def lib():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib


def _p(i):
    return C.c_void_p(PTR + STEP * i)


def _regions_args(B=5, T=12, V=20, E=96, G=4, R=None):
    """emb, cam, text_len, counts, x, mask, pooled, ranks, B, T, V, E, G, R, positive, stream"""
    return [_p(0), _p(1), _p(2), _p(3), _p(4), _p(5), _p(6), _p(7), B, T, V, E, G, B * G * T + 7 if R is None else R, 0, None]


def _text_args(B=5, T=12, V=20, S=9):
    """ids, segments, cam, text_len, counts, out_ids, out_segments, out_mask, new_len, B, T, V, S, positive, stream"""
    return [_p(0), _p(1), _p(2), _p(3), _p(4), _p(5), _p(6), _p(7), _p(8), B, T, V, S, 1, None]


def test_symbols_are_declared_exported_bound_and_callable(lib):
    handle = lib.lib()
    for name in NAMES:
        assert name in lib.header_symbols()
        assert name in lib._PROTOTYPES
        assert hasattr(handle, name)
    assert handle.mmx_abi_version() == 2
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    from transformer_mm_explainability_amd import visualbert_model as vm
    from transformer_mm_explainability_amd import visualbert_perturbation as vp
    assert callable(ops.selfattn_perturb_regions) and callable(ops.selfattn_perturb_text)
    for method in ("perturbation_image_batch", "perturbation_text_batch", "accuracy"):
        assert callable(getattr(vp.VisualBertPerturbation, method))
    assert callable(vm.VisualBERTForClassification.scores_packed) and callable(vb.pad_rows)
    assert vp.GraphedVisualBertPerturbation.MODALITIES == ("image", "text")


@pytest.mark.parametrize("missing", [0, 1, 2, 3, 4, 5, 6])
def test_regions_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args = _regions_args()
    args[missing] = None
    assert handle.mmx_selfattn_perturb_regions(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("missing", range(9))
def test_text_null_pointers_are_refused(lib, missing):
    handle = lib.lib()
    args = _text_args()
    args[missing] = None
    assert handle.mmx_selfattn_perturb_text(*args) == EINVAL
    assert b"null" in handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(T=2), dict(T=0), dict(T=24, V=233), dict(T=257, V=1), dict(V=0), dict(V=-4), dict(G=0), dict(G=65),
                                   dict(E=0), dict(E=-8), dict(B=-1), dict(B=0), dict(B=1 << 30), dict(B=(1 << 29) + 1),
                                   dict(E=(1 << 20) + 4), dict(R=0), dict(R=5 * 4 * 12 - 1),
                                   dict(R=5 * 4 * 32 + 1), dict(R=-1)])
def test_regions_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    handle = lib.lib()
    assert handle.mmx_selfattn_perturb_regions(*_regions_args(**sizes)) == EINVAL
    assert handle.mmx_last_error()


@pytest.mark.parametrize("sizes", [dict(T=2), dict(T=-1), dict(T=24, V=233), dict(T=257, V=1), dict(V=0), dict(S=0), dict(S=65), dict(S=-2),
                                   dict(B=-1), dict(B=0)])
def test_text_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    handle = lib.lib()
    assert handle.mmx_selfattn_perturb_text(*_text_args(**sizes)) == EINVAL
    assert handle.mmx_last_error()


@pytest.mark.parametrize("out", [4, 5, 6, 7])
@pytest.mark.parametrize("inp", [0, 1, 2, 3])
def test_regions_output_aliasing_an_input_is_refused(lib, out, inp):
    handle = lib.lib()
    args = _regions_args()
    args[out] = args[inp]
    assert handle.mmx_selfattn_perturb_regions(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_regions_outputs_overlapping_each_other_or_an_input_tail_are_refused(lib):
    handle = lib.lib()
    args = _regions_args()
    args[5] = args[4]                                               # mask on x
    assert handle.mmx_selfattn_perturb_regions(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()
    args = _regions_args()
    args[6] = C.c_void_p(PTR + 4 * (5 * 32 * 96 - 1))               # pooled on emb's last float
    assert handle.mmx_selfattn_perturb_regions(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


@pytest.mark.parametrize("out", [5, 6, 7, 8])
@pytest.mark.parametrize("inp", [0, 1, 2, 3, 4])
def test_text_output_aliasing_an_input_is_refused(lib, out, inp):
    handle = lib.lib()
    args = _text_args()
    args[out] = args[inp]
    assert handle.mmx_selfattn_perturb_text(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_text_outputs_overlapping_each_other_are_refused(lib):
    handle = lib.lib()
    args = _text_args()
    args[6] = C.c_void_p(PTR + STEP * 5 + 8 * (9 * 5 * 12 - 1))     # out_segments on out_ids' last element
    assert handle.mmx_selfattn_perturb_text(*args) == EINVAL
    assert b"alias" in handle.mmx_last_error()


def test_ops_refuse_host_tensors():
    import torch
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    B, T, V, E = 2, 4, 3, 8
    emb, cam = torch.rand(B, T + V, E), torch.rand(B, T + V)
    lens = torch.full((B,), 4, dtype=torch.int32)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.selfattn_perturb_regions(emb, cam, lens, torch.tensor([3, 0], dtype=torch.int32), B * (2 * T + 3), T)
    ids = torch.ones(B, T, dtype=torch.int64)
    with pytest.raises(MMXError, match="no CPU path"):
        ops.selfattn_perturb_text(ids, ids, cam, lens, torch.zeros(9, T, dtype=torch.int32))


def test_pad_rows_is_the_inverse_of_unpad_row():
    import torch
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    T, V, lens = 5, 4, [3, 5, 1]
    g = torch.Generator().manual_seed(0)
    padded = torch.rand(3, T + V, generator=g)
    for b, n in enumerate(lens):
        padded[b, n:T] = 0
    rows = [vb.unpad_row(padded, b, n, padded_text=T) for b, n in enumerate(lens)]
    back = vb.pad_rows(rows, lens, T)
    assert back.shape == (3, T + V) and torch.equal(back, padded)
    for b, n in enumerate(lens):
        assert torch.equal(vb.unpad_row(back, b, n, padded_text=T), rows[b])
    with pytest.raises(ValueError):
        vb.pad_rows(rows, lens[:2], T)                              # one length per row
    with pytest.raises(ValueError):
        vb.pad_rows(rows, [3, 4, 1], T)                             # a row that is not n + V wide
    with pytest.raises(ValueError):
        vb.pad_rows(rows, lens, 4)                                  # an item longer than the padded width
    with pytest.raises(ValueError):
        vb.pad_rows([], [], T)
    with pytest.raises(TypeError):
        vb.pad_rows(rows, lens)                                     # the padded text width is a required argument
