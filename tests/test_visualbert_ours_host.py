"""CPU: the case table of the padded-batch ``generate_ours`` of VisualBERT (``tests/visualbert_ours_cases.py``) is fit for its purpose
-- a serial float32 emulation of the kernels' arithmetic stays inside the counted bound on every case and keeps exact zeros exact,
the clamp bites (and spares) at least 10 % of the live ``g * p`` entries, no product underflows (so float32 and float64 take the same
clamp decisions), and every mutant of the method is at least 2 x the bound away on every sample where it is another function -- and
the float64 restatement reproduces the row the reference's own ``generate_ours`` returned (``out`` of
tests/golden/visualbert_model.npz) on slabs of the oracle body loaded with the golden weights."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visualbert_ours_cases as cases  # noqa: E402


def test_the_case_table_covers_what_the_gpu_suite_needs():
    assert set(cases.SEEDS) == set(cases.CASES) and len(set(cases.CASES)) == len(cases.CASES)
    assert set(cases.OTHER_SEEDS) <= set(cases.CASES)
    main = [c for c in cases.CASES if c[3] == 5 and c[5] == 5]
    assert len(main) == 5 * 3 * 4
    assert {c[:2] for c in main} == {(3, 1), (8, 10), (24, 40), (28, 100), (128, 100)}
    assert {c[2] for c in main} == {1, 3, 12} and {c[4] for c in main} == {"null", "full", "ragged", "oob"}
    for L in (1, 2):
        assert len({c[:2] for c in cases.CASES if c[5] == L}) >= 2
    assert len({c[:2] for c in cases.CASES if c[3] == 1}) >= 2


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_seed_properties_mutants_and_the_float32_emulation(case):
    """One pass per case (the slabs are the expensive part)."""
    T, V, H, B, kind, L = case
    c = cases.make_case(*case, cases.SEEDS[case])
    t, v = c["t"], c["v"]
    assert len(c["attn"]) == len(c["grad"]) == L and all(g is not h for g, h in zip(c["grad"][1:], c["grad"]))
    for b in range(B):                                   # the padding of every gradient slab is PAD_GRAD, rows and columns
        dead = np.setdiff1d(np.arange(T + V), cases.live_index(T, t[b], v[b]))
        for g, p in zip(c["grad"], c["attn"]):
            assert (g[b][:, dead, :] == cases.PAD_GRAD).all() and (g[b][:, :, dead] == cases.PAD_GRAD).all()
            assert not p[b][:, :, dead].any()
    r = cases.seed_report(c)
    print("%s: clamped %.3f positive %.3f smallest |g p| %.3e mutants %s" % (cases.case_id(case), r["clamped"], r["positive"],
                                                                              r["min_product"], r["mutants"]))
    if H >= 3:
        assert r["clamped"] >= cases.MIN_SHARE and r["positive"] >= cases.MIN_SHARE, r
    assert r["min_product"] >= cases.FLT_MIN, r           # no product underflows
    for m, d in r["mutants"].items():
        expected = [b for b in range(B) if cases.can_differ(m, H, L, T, t[b])]
        assert (d is None) == (not expected), (m, d)
        if d is not None:
            assert d >= cases.MUTANT_FACTOR, "%s is only %.3g bounds away on some sample" % (m, d)
    assert r["mutants"]["c_is_t_minus_1"] is not None
    if H >= 3:
        assert r["mutants"]["clamp_after_sum"] is not None
    if L >= 2:
        assert r["mutants"]["ascending_layers"] is not None and r["mutants"]["no_identity"] is not None
    if kind in ("ragged", "oob") and B == 5:
        assert r["mutants"]["padded_extent"] is not None and r["mutants"]["prefix_live_set"] is not None

    ref, bound = cases.ours64(c["attn"], c["grad"], T, t, v)
    assert (ref >= 0).all() and ref.max() > 0
    got = cases.ours_f32(c["attn"], c["grad"], T, t, v)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float(cases.distance_in_bounds(got.astype(np.float64), ref, bound).max())
    print("%s: float32 emulation, worst error / bound %.3f" % (cases.case_id(case), worst))
    assert (err <= bound).all(), "|fp32 - fp64| exceeds the counted bound by %.3e" % float((err - bound).max())
    assert not got[ref == 0].any(), "an exact zero did not stay exact"
    for b in range(B):
        live = cases.live_index(T, t[b], v[b])
        assert ref[b, int(t[b]) - 2] == 0 and not np.delete(ref[b], live).any()


def test_slabs_are_shared_between_kinds_with_the_same_clamped_lengths():
    a = cases.make_case(8, 10, 3, 5, "ragged", 2, 1)
    b = cases.make_case(8, 10, 3, 5, "oob", 2, 1)
    assert a["attn"][0] is b["attn"][0] and np.array_equal(a["t"], b["t"]) and not np.array_equal(a["raw_t"], b["raw_t"])
    other = cases.make_case(8, 10, 3, 5, "ragged", 2, 2)
    assert not np.array_equal(a["grad"][0], other["grad"][0])


def test_the_bound_is_what_the_docstring_counts():
    assert cases.bound_factor(5, 228, 12) == pytest.approx(np.expm1(5 * 243 * 2.0 ** -24), rel=1e-15)
    assert cases.bound_factor(1, 4, 1) < 1e-6


def test_restatement_reproduces_the_reference_generator_on_the_oracle_body(golden):
    """``oracle/visualbert_torch.py`` with the golden weights gives the probability slabs of the golden item (unpadded: T = its 8
    real tokens) and, by autograd, their gradients for the arg-max answer; ``ours64`` (and the float32 emulation) on them is the
    row the reference's own ``SelfAttentionGenerator.generate_ours`` returned."""
    import torch
    from oracle import visualbert_torch as vt
    g = golden("visualbert_model")
    heads = int(g["dims"][1])
    sd = vt.prepare_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w__")})
    scores, probs = vt.forward(sd, heads, torch.from_numpy(g["input_ids"]), torch.from_numpy(g["input_mask"]),
                               torch.from_numpy(g["image_feature_0"]))
    grads = torch.autograd.grad(scores[0, int(scores[0].argmax())], probs)
    n = int(g["input_mask"].sum())
    V = g["image_feature_0"].shape[1]
    t, v = np.array([n]), np.array([V])
    P, G = [p.detach().numpy() for p in probs], [x.numpy() for x in grads]
    want = g["out"]
    assert want.shape == (1, n + V)
    for got in (cases.ours64(P, G, n, t, v)[0], cases.ours_f32(P, G, n, t, v).astype(np.float64)):
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5)
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max()
