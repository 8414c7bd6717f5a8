"""CPU: the float64 restatement of ``tests/detr_baselines_cases.py`` -- the reference's matrix form of the three DETR baselines --
reproduces what the reference's own generator recorded in the fixtures, and the case table covers what it says it covers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detr_baselines_cases as cases  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _close(got, want):
    want = np.asarray(want, dtype=np.float64).reshape(got.shape)
    err = np.abs(got - want).max()
    assert err <= 1e-5 and err <= 1e-4 * np.abs(want).max(), (err, np.abs(want).max())


def test_the_restatement_reproduces_the_reference_generators_fixture():
    g = _load("detr_chain")                          # H = 4, Ni = 35, Q = 10, 3 + 3 layers, targets [2, 7]
    t = g["target_index"]
    enc, dec, cross = list(g["enc_attn"]), list(g["dself_attn"]), g["dcross_attn"][-1]
    _close(cases.rollout64(enc, dec, cross, t)[0], g["rollout_out"])
    _close(cases.raw64(cross, t)[0], g["raw_attn_out"])
    # one backward seeded on both queries: ONE gradient slab serves both rows
    _close(cases.gradcam64(cross, g["dcross_grad"][-1], t)[0], g["gradcam_out"])


@pytest.mark.parametrize("name", ["detr_chain_nonorm", "detr_chain_noself"])
def test_the_same_keys_of_the_other_chain_fixtures_where_present(name):
    g = _load(name)
    t = g["target_index"]
    enc, dec, cross = list(g["enc_attn"]), list(g["dself_attn"]), g["dcross_attn"][-1]
    checked = 0
    for key, fn in (("rollout_out", lambda: cases.rollout64(enc, dec, cross, t)[0]), ("raw_attn_out", lambda: cases.raw64(cross, t)[0]),
                    ("gradcam_out", lambda: cases.gradcam64(cross, g["dcross_grad"][-1], t)[0])):
        if key in g.files:
            _close(fn(), g[key])
            checked += 1
    assert checked == sum(k in g.files for k in ("rollout_out", "raw_attn_out", "gradcam_out"))
    ref, bound = cases.rollout64(enc, dec, cross, t)          # the restatement runs on these shapes whatever the fixture recorded
    assert ref.shape == (len(t), cross.shape[-1]) and (bound >= 0).all()


def test_the_row_form_agrees_with_the_matrix_form_in_float64():
    """The algebra the kernels rely on, step by step in float64: u = R_qq e_t bottom-up, s = u^T C, x <- w A + w top-down."""
    c = cases.make_case((65, 7, 8, 5, 6, 6))
    ref, _ = cases.rollout64(c["enc"], c["dec"], c["cross"], c["targets"])
    for k, t in enumerate(c["targets"]):
        y = np.zeros(c["Q"])
        y[t] = 1.0
        for b in c["dec"]:
            B = cases.head_mean64(b)
            y = (B @ y + y) / (1.0 + B.sum(-1))
        x = y @ cases.head_mean64(c["cross"])
        for a in reversed(c["enc"]):
            A = cases.head_mean64(a)
            w = x / (1.0 + A.sum(-1))
            x = w @ A + w
        assert np.abs(x - ref[k]).max() <= 1e-14


def test_the_case_table_covers_what_the_suite_promises():
    col = lambda i: {c[i] for c in cases.CASES}
    assert col(0) == {1, 2, 5, 63, 64, 65, 255, 257} and col(1) == {1, 2, 7, 100, 128}
    assert col(2) == {1, 3, 8} and col(3) == {1, 2, 5, 17} and col(4) == {1, 2, 6} and col(5) == {1, 2, 6}
    assert any(c[4] != c[5] for c in cases.CASES)
    zero = last = repeat = False
    for c in cases.CASES:
        t = cases.targets_of(c)
        assert t.shape == (c[3],) and t.min() >= 0 and t.max() <= c[1] - 1
        zero |= bool((t == 0).any())
        last |= bool((t == c[1] - 1).any()) and c[1] > 1
        repeat |= len(set(t.tolist())) < len(t)
    assert zero and last and repeat


def test_the_bounds_are_finite_positive_and_not_vacuous():
    for case in cases.CASES:
        c = cases.make_case(case)
        for ref, bound in (cases.raw64(c["cross"], c["targets"]), cases.rollout64(c["enc"], c["dec"], c["cross"], c["targets"]),
                           cases.gradcam64(c["cross"], c["grad"], c["targets"]),
                           cases.gradcam64(c["cross"], c["grad_shared"], c["targets"])):
            assert np.isfinite(bound).all() and (bound >= 0).all() and bound.max() <= 1e-3 * max(np.abs(ref).max(), 1e-30) + 1e-5
    # the GradCAM clamp bites and leaves something: both signs of head weights occur over the table
    pos = neg = 0
    for case in cases.CASES:
        c = cases.make_case(case)
        pre, _ = cases.gradcam64(c["cross"], c["grad"], c["targets"], clamp=False)
        pos += int((pre > 0).sum())
        neg += int((pre < 0).sum())
    assert pos > 100 and neg > 100
