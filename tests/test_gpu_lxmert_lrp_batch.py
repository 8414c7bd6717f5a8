"""-m gpu: the four LRP methods of LXMERT on a padded batch of ragged questions (``GeneratorOurs.generate_ours_batch(use_lrp=True)``
with and without normalisation, ``GeneratorBaselines.generate_transformer_attr_batch`` / ``generate_partial_lrp_batch``) on the golden
LXMERT (``tests/golden/lxmert_model.npz``).  The batch is the one of ``tests/test_lxmert_lrp_batch_host.py``: the golden item at 9
tokens plus two truncations to 6 and 2 tokens with other ``visual_feats``, padded to 12.

* Item 0 against the reference's pass in float64 (the ``f64__`` entries of ``lxmert_model_lrp.npz``) with ``in_noise`` of
  ``tests/test_gpu_lrp.py`` -- ``LRP_FACTOR`` x the reference's own fp32-to-fp64 distance, the project's standing bar for this pass:
  the batch changes only the GEMM extents and the sum orders.
* Items 1 and 2 against the per-item methods on the unpadded item:
  ``|a - b| <= 3 (noise / top of that key in the golden file) max|b| + LRP_FLOOR max|b|`` -- each route is allowed 1.5 x the
  reference's own fp32-to-fp64 distance from the truth, so 3 x from each other.  This ASSUMES the truncated items are as noisy as
  the golden one; the measured ratios are printed and recorded (``tests/parity.py``), and ``tools/probe_lxmert_lrp_batch.py`` writes
  them to ``profiles/lxmert_lrp_batch_probe.txt``.
* ``index=None`` (the arg-max answer per sample, picked on the device) and given answer ids.
* Exact zeros beyond each question's length."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402
from test_gpu_lrp import LRP_FACTOR, LRP_FLOOR, in_noise  # noqa: E402
from test_lxmert_lrp_batch_host import TRUNCATIONS, ragged_batch  # noqa: E402

pytestmark = pytest.mark.gpu

# method -> ((golden key, attribute or position in the returned pair), ...)
KEYS = {"ours": (("R_t_t", 0), ("R_t_i", 1), ("R_i_i", "R_i_i"), ("R_i_t", "R_i_t")),
        "transformer_attr": (("transformer_attr_R_t_t", 0), ("transformer_attr_R_t_i", 1)),
        "partial_lrp": (("partial_lrp_R_t_t", 0), ("partial_lrp_R_t_i", 1))}


class ItemUsage:
    """The reference's ``ModelUsage`` for one unpadded item (lxmert/lxmert/perturbation.py:45-83)."""

    def __init__(self, model):
        self.model = model

    def forward(self, inputs):
        self.text_len, self.image_boxes_len = inputs["input_ids"].shape[1], inputs["visual_feats"].shape[1]
        return self.model(**inputs)


def _maps(method, gen, pair):
    return {key: (pair[where] if isinstance(where, int) else getattr(gen, where)).detach().clone() for key, where in KEYS[method]}


def run_batched(model, batch, index):
    from transformer_mm_explainability_amd import lxmert_explainability as le
    usage = type("Usage", (), {"model": model})()
    ours, base = le.GeneratorOurs(usage), le.GeneratorBaselines(usage)
    out = {"ours": _maps("ours", ours, ours.generate_ours_batch(batch, index=index, use_lrp=True))}
    out["transformer_attr"] = _maps("transformer_attr", base, base.generate_transformer_attr_batch(batch, index=index))
    out["transformer_attr"]["R_i_i"] = base.R_i_i.detach().clone()
    out["partial_lrp"] = _maps("partial_lrp", base, base.generate_partial_lrp_batch(batch, index=index))
    return out


def run_per_item(model, item, index):
    from transformer_mm_explainability_amd import lxmert_explainability as le
    usage = ItemUsage(model)
    ours, base = le.GeneratorOurs(usage), le.GeneratorBaselines(usage)
    out = {"ours": _maps("ours", ours, ours.generate_ours(item, index=index, use_lrp=True))}
    out["transformer_attr"] = _maps("transformer_attr", base, base.generate_transformer_attr(item, index=index))
    out["partial_lrp"] = _maps("partial_lrp", base, base.generate_partial_lrp(item, index=index))
    return out


def live(key, x, b, t):
    """Sample b's live block of a batched map (language extents cut to ``t``)."""
    x = x[b]
    if key.endswith("R_i_i"):
        return x
    if key.endswith("R_i_t"):
        return x[:, :t]
    return x[:t, :t] if key.endswith("R_t_t") else x[:t]


@pytest.fixture(scope="module")
def setup(golden):
    from test_gpu_generators import _lxmert_from_golden
    gm, g = golden("lxmert_model"), golden("lxmert_model_lrp")
    model, _usage = _lxmert_from_golden(gm)
    inputs = {k[4:]: torch.from_numpy(np.asarray(v)) for k, v in gm.items() if k.startswith("in__")}
    batch, items, index = ragged_batch(inputs, int(g["index"]))
    batch = {k: v.cuda() for k, v in batch.items()}
    items = [{k: v.cuda() for k, v in it.items()} for it in items]
    return model, g, batch, items, index


@pytest.fixture(scope="module", params=["argmax", "given"])
def results(request, setup):
    """``(g, batched maps, per-item maps of items 1 and 2)`` for ``index=None`` / given answer ids, computed once."""
    model, g, batch, items, index = setup
    given = request.param == "given"
    batched = run_batched(model, batch, torch.tensor(index, device="cuda") if given else None)
    per_item = {b: run_per_item(model, items[b], index[b] if given else None) for b in (1, 2)}
    return g, batched, per_item


@pytest.mark.parametrize("method", sorted(KEYS))
def test_item_0_is_within_the_references_noise(results, method):
    g, batched, _ = results
    for key, _where in KEYS[method]:
        in_noise(live(key, batched[method][key], 0, TRUNCATIONS[0]), g, key, "lxmert batched %s, item 0 of the padded batch" % key)


@pytest.mark.parametrize("method", sorted(KEYS))
def test_items_1_and_2_agree_with_the_per_item_methods(results, method):
    g, batched, per_item = results
    failures = []
    for key, _where in KEYS[method]:
        r64 = np.asarray(g["f64__" + key], dtype=np.float64)
        top = float(np.abs(r64).max())
        noise = float(np.abs(np.asarray(g[key], dtype=np.float64) - r64).max()) / top
        for b in (1, 2):
            a, want = live(key, batched[method][key], b, TRUNCATIONS[b]), per_item[b][method][key]
            assert a.shape == want.shape, (key, b)
            scale = float(want.abs().max())
            err, bound = float((a - want).abs().max()), 3.0 * noise * scale + LRP_FLOOR * scale
            parity.note("lxmert batched vs per-item %s item %d" % (key, b), err, bound, scale)
            print("%s item %d: |batched - per-item| %.3e  bound %.3e  ratio %.3f  (golden noise / top %.3e)"
                  % (key, b, err, bound, err / bound if bound else float("inf"), noise))
            if not err <= bound:
                failures.append((key, b, err, bound))
    assert not failures, failures


def test_ours_without_normalisation_agrees_with_the_per_item_method(setup):
    """``ours_with_lrp_no_normalization``: the same pass, the schedule without ``handle_residual``; the yardstick of ``R_t_t`` / ``R_t_i``."""
    from transformer_mm_explainability_amd import lxmert_explainability as le
    model, g, batch, items, index = setup
    gen = le.GeneratorOurs(type("Usage", (), {"model": model})())
    R_tt, R_ti = gen.generate_ours_batch(batch, use_lrp=True, normalize_self_attention=False)
    for b, t in enumerate(TRUNCATIONS):
        one = le.GeneratorOurs(ItemUsage(model))
        w_tt, w_ti = one.generate_ours(items[b], use_lrp=True, normalize_self_attention=False)
        for key, a, want in (("R_t_t", R_tt[b, :t, :t], w_tt), ("R_t_i", R_ti[b, :t], w_ti)):
            r64 = np.asarray(g["f64__" + key], dtype=np.float64)
            noise = float(np.abs(np.asarray(g[key], dtype=np.float64) - r64).max()) / float(np.abs(r64).max())
            scale = float(want.abs().max())
            err, bound = float((a - want).abs().max()), 3.0 * noise * scale + LRP_FLOOR * scale
            parity.note("lxmert batched vs per-item no-normalisation %s item %d" % (key, b), err, bound, scale)
            print("no-normalisation %s item %d: %.3e  bound %.3e" % (key, b, err, bound))
            assert err <= bound, (key, b, err, bound)


def test_exact_zeros_beyond_each_questions_length(results):
    _g, batched, _ = results
    for method, maps in batched.items():
        for key, x in maps.items():
            for b, t in enumerate(TRUNCATIONS):
                if key.endswith("R_t_t"):
                    assert not bool(x[b, t:].any()) and not bool(x[b, :, t:].any()), (method, key, b)
                    assert float(x[b, 0, 0]) == 0.0
                elif key.endswith("R_t_i"):
                    assert not bool(x[b, t:].any()), (method, key, b)
                elif key.endswith("R_i_t"):
                    assert not bool(x[b, :, t:].any()), (method, key, b)


def test_the_pass_never_takes_the_tape_path(setup, monkeypatch):
    """``forward_tape`` clears the LRP tapes: the LRP route stays on the module path whatever ``use_tape`` says."""
    from transformer_mm_explainability_amd import lxmert_explainability as le
    model, _g, batch, _items, _index = setup

    def boom(*a, **kw):
        raise AssertionError("the LRP route took the tape path")

    monkeypatch.setattr(type(model), "forward_tape", boom)
    usage = type("Usage", (), {"model": model})()
    gen = le.GeneratorOurs(usage)
    assert gen.use_tape
    gen.generate_ours_batch(batch, use_lrp=True)
    le.GeneratorBaselines(usage).generate_partial_lrp_batch(batch)
