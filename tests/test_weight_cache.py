"""The per-parameter cache of derived GEMM weights (``ops._cached_weight`` behind ``_converted``, ``transposed_weight``,
``sign_split_weight`` and ``transposed_half_weight``) on CPU tensors: no library is loaded."""
import gc

import pytest
import torch

from transformer_mm_explainability_amd import ops

DERIVED = {
    "converted": (lambda w: ops._converted(w, torch.float16), lambda w: w.detach().to(torch.float16)),
    "transposed": (ops.transposed_weight, lambda w: w.detach().t().contiguous()),
    "sign_split": (ops.sign_split_weight, lambda w: torch.cat((w.detach().clamp(min=0), w.detach().clamp(max=0)), dim=1)),
    "sign_split_t": (lambda w: ops.sign_split_weight(w, transposed=True),
                     lambda w: torch.cat((w.detach().clamp(min=0), w.detach().clamp(max=0)), dim=1).t().contiguous()),
    "transposed_half": (ops.transposed_half_weight, lambda w: w.detach().t().to(torch.float16).contiguous()),
}


@pytest.mark.parametrize("name", sorted(DERIVED))
def test_cached_copy_follows_the_parameter(name):
    get, want = DERIVED[name]
    w = torch.nn.Parameter(torch.randn(8, 12, generator=torch.Generator().manual_seed(3)))
    first = get(w)
    assert torch.equal(first, want(w)) and first.is_contiguous()
    assert get(w) is first                              # untouched parameter: the same object
    with torch.no_grad():
        w.mul_(-2.0)
    second = get(w)
    assert second is not first and torch.equal(second, want(w))   # modified in place: a fresh copy of the new values
    assert get(w) is second


def test_transposed_sign_split_follows_its_source():
    w = torch.nn.Parameter(torch.randn(8, 12, generator=torch.Generator().manual_seed(4)))
    pn, pn_t = ops.sign_split_weight(w), ops.sign_split_weight(w, transposed=True)
    assert ops.sign_split_weight(w) is pn and ops.sign_split_weight(w, transposed=True) is pn_t
    assert pn_t.shape == (24, 8) and torch.equal(pn_t, pn.t())
    with torch.no_grad():
        w.neg_()
    pn2 = ops.sign_split_weight(w)                      # rebuilding the source drops the transposed copy ...
    assert pn2 is not pn and "pnT" not in ops._GEMM_WEIGHTS[id(w)]
    pn2_t = ops.sign_split_weight(w, transposed=True)   # ... and the next request builds it from the new source
    assert pn2_t is not pn_t and torch.equal(pn2_t, pn2.t()) and ops.sign_split_weight(w) is pn2


def test_all_copies_of_a_parameter_share_one_entry_that_dies_with_it():
    w = torch.nn.Parameter(torch.randn(8, 12))
    key = id(w)
    copies = [get(w) for get, _ in DERIVED.values()]
    assert set(ops._GEMM_WEIGHTS[key]) == {torch.float16, "t", "pn", "pnT", "t16"}
    del w
    gc.collect()
    assert key not in ops._GEMM_WEIGHTS and len(copies) == 5
