"""CPU: the case table of the batched VisualBERT baselines (``tests/visualbert_baselines_cases.py``) is fit for its purpose -- the
stored seeds have the properties the GPU suite relies on, a float32 emulation (serial sums) of each method stays inside its counted
bound and inside the project's ``1e-4 x max|ref|``, out-of-range lengths mean their clamped values -- and the float64 restatements
reproduce the maps the reference's own generator returned (``rollout_out`` / ``raw_attn_out`` / ``gradcam_out`` of
tests/golden/visualbert_model.npz) on slabs of the oracle body loaded with the golden weights."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visualbert_baselines_cases as cases  # noqa: E402

RELMAX = 1e-4                   # tests/parity.py: the project's bound on a map, relative to its largest entry


def test_every_case_has_a_seed():
    assert set(cases.SEEDS) == set(cases.CASES) and len(cases.CASES) == 5 * 3 * 2 * 4
    assert set(cases.OTHER_SEEDS) <= set(cases.CASES)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_seed_properties_and_float32_emulations(case):
    """One pass per case (the slabs are the expensive part): the seed properties, then the serial-sum float32 emulation of every
    method against its counted bound and against ``1e-4 x max|ref|`` per sample."""
    T, V, H, B, kind = case
    c = cases.make_case(*case, cases.SEEDS[case], n_layers=max(cases.N_LAYERS))
    t, v = c["t"], c["v"]
    r = cases.seed_report(c)
    assert r["ratio"] >= cases.MIN_SPAN_OVER_E, r
    if H >= 3:
        assert r["clamped"] >= cases.MIN_SHARE and r["positive"] >= cases.MIN_SHARE, r
    assert r["row_ok"], r
    # the same GradCAM case whatever the table's length: the gradient and the last slab are drawn first
    d = cases.make_case(*case, cases.SEEDS[case], n_layers=1)
    assert np.array_equal(c["grad"], d["grad"]) and np.array_equal(c["attn"][-1], d["attn"][-1])

    def judge(label, got, ref, bound):
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all(), "%s: |fp32 - fp64| exceeds the counted bound by %.3e" % (label, float((err - bound).max()))
        for b in range(B):
            assert err[b].max() <= RELMAX * np.abs(ref[b]).max(), (label, b, float(err[b].max()), float(np.abs(ref[b]).max()))
        assert not got[ref == 0].any(), label + ": an exact zero did not stay exact"

    ref, bound = cases.raw64(c["attn"][-1], T, t, v)
    judge("raw attention", cases.raw_f32(c["attn"][-1], T, t, v), ref, bound)
    for L in cases.N_LAYERS:
        ref, bound = cases.rollout64(c["attn"][-L:], T, t, v)
        judge("rollout L=%d" % L, cases.rollout_f32(c["attn"][-L:], T, t, v), ref, bound)
    ref, bound = cases.gradcam64(c["attn"][-1], c["grad"], T, t, v)
    assert np.isfinite(bound).all() and bound.max() < 0.1
    judge("gradcam", cases.gradcam_f32(c["attn"][-1], c["grad"], T, t, v), ref, bound[:, None])


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[4] == "ragged" and c[3] == 5 and c[0] >= 8 and c[2] == 3], ids=cases.case_id)
def test_sums_over_the_padded_extent_would_be_seen(case):
    """The trap the live-set entry exists for: with the head weights summed over (and divided by) the padded N x N extent the GradCAM
    row moves by far more than its bound (the padding of the gradient slabs holds 1e3)."""
    T, V, H, B, _ = case
    c = cases.make_case(*case, cases.SEEDS[case])
    ref, bound = cases.gradcam64(c["attn"][-1], c["grad"], T, c["t"], c["v"])
    N = T + V
    for b in range(B):
        if c["t"][b] == T and c["v"][b] == V:
            continue
        idx, cb = cases.live_index(T, c["t"][b], c["v"][b]), int(c["t"][b]) - 2
        w = c["grad"][b].astype(np.float64).mean(axis=(1, 2))                       # over the padded extent
        cam = np.maximum((c["attn"][-1][b].astype(np.float64) * w[:, None, None]).mean(0), 0.0)[np.ix_(idx, idx)]
        with np.errstate(invalid="ignore", divide="ignore"):
            row = (cam[cb] - cam.min()) / (cam.max() - cam.min())
        row[cb] = 0.0
        assert not np.allclose(row, ref[b, idx], rtol=0, atol=bound[b], equal_nan=True), (b, N)


@pytest.mark.parametrize("T,V,B", [(3, 1, 1), (3, 1, 5), (24, 40, 5), (128, 100, 1), (128, 100, 5)])
def test_out_of_range_lengths_mean_their_clamped_values(T, V, B):
    raw_t, raw_v, t, v = cases.lengths(T, V, B, "oob")
    assert (raw_t < 2).any() or (raw_t > T).any()
    assert (raw_v < 1).any() or (raw_v > V).any()
    assert np.array_equal(np.clip(raw_t, 2, T), t) and np.array_equal(np.clip(raw_v, 1, V), v)
    rt, rv, st, sv = cases.lengths(T, V, B, "ragged")
    assert np.array_equal(rt, st) and np.array_equal(rv, sv) and st.min() >= 2 and st.max() <= T and sv.min() >= 1 and sv.max() <= V
    if B == 5:
        assert 2 in st and T in st and 1 in sv and V in sv
    assert cases.lengths(T, V, B, "null")[:2] == (None, None)


def test_all_clamped_sample_is_nan_off_its_own_column():
    """H = 1 with a negative head offset: the head weight is negative, the whole cam is clamped to zero, ``mx == mn`` and the live
    entries of the row are NaN, as in the per-item route -- but the row's own column and the padding stay zero."""
    c = cases.make_case(8, 10, 1, 5, "ragged", 1, negate=True)
    assert c["offsets"][0] < 0
    ref, _ = cases.gradcam64(c["attn"][-1], c["grad"], 8, c["t"], c["v"])
    emu = cases.gradcam_f32(c["attn"][-1], c["grad"], 8, c["t"], c["v"])
    for b in range(5):
        idx, cb = cases.live_index(8, c["t"][b], c["v"][b]), int(c["t"][b]) - 2
        others = np.delete(idx, cb)
        assert np.isnan(ref[b, others]).all() and np.isnan(emu[b, others]).all()
        assert ref[b, cb] == 0 and emu[b, cb] == 0
        dead = np.setdiff1d(np.arange(18), idx)
        assert not ref[b, dead].any() and not emu[b, dead].any()


def test_restatements_reproduce_the_reference_generator_on_the_oracle_body(golden):
    """``oracle/visualbert_torch.py`` with the golden weights gives the probability slabs of the golden item (unpadded: T = its 8
    real tokens) and, by autograd, their gradients for the arg-max answer; the float64 restatements on them are the maps the
    reference's own ``SelfAttentionGenerator`` returned."""
    import torch
    from oracle import visualbert_torch as vt
    g = golden("visualbert_model")
    heads = int(g["dims"][1])
    sd = vt.prepare_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w__")})
    scores, probs = vt.forward(sd, heads, torch.from_numpy(g["input_ids"]), torch.from_numpy(g["input_mask"]),
                               torch.from_numpy(g["image_feature_0"]))
    np.testing.assert_allclose(scores.detach().numpy(), g["scores"], rtol=0, atol=1e-5)
    grads = torch.autograd.grad(scores[0, int(scores[0].argmax())], probs)
    n = int(g["input_mask"].sum())
    V = g["image_feature_0"].shape[1]
    t, v = np.array([n]), np.array([V])
    P = [p.detach().numpy() for p in probs]
    assert P[0].shape == (1, heads, n + V, n + V)

    def check(got, want, what):
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-5, equal_nan=True, err_msg=what)
        fin = np.isfinite(want)
        if fin.any() and np.abs(want[fin]).max() > 0:
            assert np.abs(got[fin] - want[fin]).max() <= RELMAX * np.abs(want[fin]).max(), what

    check(cases.rollout64(P, n, t, v)[0], g["rollout_out"], "rollout")
    check(cases.raw64(P[-1], n, t, v)[0], g["raw_attn_out"], "raw attention")
    check(cases.gradcam64(P[-1], grads[-1].numpy(), n, t, v)[0], g["gradcam_out"], "gradcam")
    for emu, want in ((cases.rollout_f32(P, n, t, v), g["rollout_out"]), (cases.raw_f32(P[-1], n, t, v), g["raw_attn_out"]),
                      (cases.gradcam_f32(P[-1], grads[-1].numpy(), n, t, v), g["gradcam_out"])):
        check(emu.astype(np.float64), want, "float32 emulation")
