"""CPU: the case table of the batched LXMERT baselines (``tests/lxmert_baselines_cases.py``) is fit for its purpose -- every GradCAM
case has clamped AND positive entries inside its live blocks, the padded-batch trap (a gradient mean taken over the padded extent)
would be seen, out-of-range lengths mean their clamped values -- and the float64 restatement of rollout agrees with the oracle's own
fp32 ``compute_rollout_attention`` on the live sub-blocks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lxmert_baselines_cases as cases  # noqa: E402


def test_every_case_has_a_seed():
    assert set(cases.SEEDS) == set(cases.CASES) and len(cases.CASES) == 4 * 3 * 2 * 4


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_gradcam_cases_have_clamped_and_positive_entries_inside_the_live_blocks(case):
    c = cases.make_case(*case, cases.SEEDS[case])
    clamped, positive = cases.clamp_shares(c)
    assert clamped >= cases.MIN_SHARE and positive >= cases.MIN_SHARE, (clamped, positive)
    # the same case whatever the tables' lengths: the gradient and cross slabs are drawn first
    d = cases.make_case(*case, cases.SEEDS[case], n_text=5, n_img=4)
    assert all(np.array_equal(c[k], d[k]) for k in ("g_tt", "g_ti", "g_ti_k", "cross", "cross_k"))


@pytest.mark.parametrize("case", [c for c in cases.CASES if c[4] in ("ragged", "oob") and c[0] > 2 and c[3] == 5], ids=cases.case_id)
def test_a_mean_over_the_padded_extent_would_be_seen(case):
    """The trap the live-block entry exists for: with the head weights taken over the padded [Nq, Nk] extent the maps move by far
    more than any tolerance of the GPU suite (the padding of the gradient slabs holds 1e3)."""
    c = cases.make_case(*case, cases.SEEDS[case])
    T, I, H, B, _ = case
    want = cases.gradcam64(c["text"][-1], c["g_tt"], c["t"], c["t"], clamp=False)
    padded_w = cases.gradcam64(c["text"][-1][:, :, :, :], c["g_tt"], np.full(B, T), np.full(B, T), clamp=False)
    short = [b for b in range(B) if c["t"][b] < T]
    assert short
    for b in short:
        t = int(c["t"][b])
        assert np.abs(padded_w[b, :t, :t] - want[b, :t, :t]).max() > 1e-2


@pytest.mark.parametrize("T,B", [(2, 1), (2, 5), (17, 5), (48, 1), (48, 5)])
def test_out_of_range_lengths_mean_their_clamped_values(T, B):
    raw, clamped = cases.lengths(T, B, "oob")
    assert (raw < 1).any() or (raw > T).any()
    assert np.array_equal(np.clip(raw, 1, T), clamped)
    ragged, same = cases.lengths(T, B, "ragged")
    assert np.array_equal(ragged, same) and ragged.min() >= 1 and ragged.max() <= T
    if B == 5:
        assert 1 in ragged and T in ragged
    assert cases.lengths(T, B, "null")[0] is None


@pytest.mark.parametrize("n_text,n_img", [(2, 1), (5, 4)])
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_float64_rollout_agrees_with_the_oracle(shape, n_text, n_img):
    T, I = shape
    c = cases.make_case(T, I, 3, 5, "ragged", 0, n_text=n_text, n_img=n_img)
    R_tt, R_ti, R_ii = cases.rollout64(c["text"], c["img"], c["cross"], c["t"])
    o_tt, o_ti = cases.rollout_f32_oracle(c["text"], c["img"], c["cross"], c["t"])
    np.testing.assert_allclose(R_tt, o_tt, rtol=0, atol=2e-6)
    np.testing.assert_allclose(R_ti, o_ti, rtol=0, atol=2e-6)
    for b in range(5):
        t = int(c["t"][b])
        assert R_tt[b, 0, 0] == 0 and not R_tt[b, t:].any() and not R_tt[b, :, t:].any() and not R_ti[b, t:].any()
        np.testing.assert_allclose(R_ii[b].sum(-1), 1.0, atol=1e-12)        # a product of row-stochastic matrices


def test_float64_head_mean_and_gradcam_are_the_reference_formulas_on_an_unpadded_item():
    """On one unpadded item the restatements are the reference's lines verbatim (torch, float64)."""
    import torch
    c = cases.make_case(12, 20, 3, 1, "null", 0)
    P, G = torch.from_numpy(c["cross"]).double(), torch.from_numpy(c["g_ti"]).double()
    cam = P.reshape(-1, 12, 20)
    grad = G.reshape(-1, 12, 20).mean(dim=[1, 2], keepdim=True)
    want = (cam * grad).mean(0).clamp(min=0)
    np.testing.assert_allclose(cases.gradcam64(c["cross"], c["g_ti"], [12], [20])[0], want.numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(cases.head_mean64(c["cross"], [12], [20])[0], cam.mean(dim=0).numpy(), rtol=1e-13, atol=0)
