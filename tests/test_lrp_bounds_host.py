"""CPU: the bounds, the inputs and the case tables of ``tests/lrp_bounds.py`` are sound before a kernel is held to them.

* At every row of both tables an fp32 restatement lies inside the bound of every output and has the reference's NaN pattern: the
  attention core in numpy float32 with the contraction in k-groups of 4 accumulated along the 64-key tiles, the rules with the
  two-stage tree of ``block_sum`` / ``partials_sum`` (trips per thread, xor-shuffle steps, four waves, partials per lane, the tree again).
* Every mutant (a deliberately wrong float64 reference: one realistic slip of a kernel) puts an output that a row STORES at >= 2x its
  bound in at least one row where it applies; in how many of those rows is printed.  (The one Add row of 64 x (2**18 + 1) elements is
  left out of the mutant sweeps: every path it takes is met by a smaller row.)
* Conditions on the inputs, asserted on the reference alone: ``offset``, ``zeros`` and ``eps`` rows have no unjudged element, ``randn``
  rows at most 2 % per output; the crafted elements of ``eps`` really take the ``den == 0`` branch.
* The tables hold every value the device test is asked to cover, with every (DP, phase).

The worst restatement error / bound and the median bound / |reference| per output and family are printed (past pytest's capture)."""
import numpy as np
import pytest

import lrp_bounds as lb

_cache = {}


def say(capsys, line):
    with capsys.disabled():
        print("\n  " + line, end="")


def core_of(c):
    if c["id"] not in _cache:
        x = lb.core_inputs(c)
        _cache[c["id"]] = (x, lb.core_ref(x, lb.scale_of(c), c["mode"], c["phase"], lb.with_scores(c)))
    return _cache[c["id"]]


def rule_of(c):
    if c["id"] not in _cache:
        x = lb.rule_inputs(c)
        _cache[c["id"]] = (x, lb.rule_ref(c, x))
    return _cache[c["id"]]


def heavy(c):
    return c["kind"] == "add" and c["batch"] * c["per"] > 4 * lb.CAP


def median_rel(val, bound):
    ok = np.isfinite(bound) & np.isfinite(val) & (val != 0)
    return float(np.median(bound[ok] / np.abs(val[ok]))) if ok.any() else 0.0


def test_an_fp32_restatement_of_every_core_row_is_inside_its_bounds(capsys):
    top, med, unj = {}, {}, {}
    for c in lb.core_cases():
        x, ref = core_of(c)
        got = lb.core_restatement(x, lb.scale_of(c), c["mode"], c["phase"], lb.with_scores(c))
        for n in lb.stored(c):
            fig = lb.ratio(got[n], ref[n], ref["e_" + n])
            assert np.array_equal(np.isnan(got[n]), np.isnan(ref[n])), (c["id"], n)
            assert fig <= 1.0, (c["id"], n, fig)
            key = (c["family"], n)
            top[key] = max(top.get(key, 0.0), fig)
            med.setdefault(key, []).append(median_rel(ref[n], ref["e_" + n]))
            unj[key] = max(unj.get(key, 0.0), lb.unjudged_share(ref["e_" + n]))
    for key in sorted(top):
        say(capsys, "lrp core restatement %-7s %-6s worst error / bound %.3f   median bound / |ref| %.2e ... %.2e   unjudged <= %.4f"
            % (key[0], key[1], top[key], min(med[key]), max(med[key]), unj[key]))


def test_unjudged_shares_of_the_core_families():
    """``offset``, ``zeros`` and ``eps``: none.  ``randn``: at most 2 % of an output."""
    seen = set()
    for c in lb.core_cases():
        _, ref = core_of(c)
        for n in lb.stored(c):
            share = lb.unjudged_share(ref["e_" + n])
            if c["family"] in ("offset", "zeros", "eps"):
                assert share == 0.0, (c["id"], n, share)
            if c["family"] == "randn":
                assert share <= 0.02, (c["id"], n, share)
        seen.add(c["family"])
    assert seen == set(lb.CORE_FAMILIES)


def test_the_eps_family_takes_the_den_equals_zero_branch():
    for c in lb.core_cases():
        if c["family"] != "eps":
            continue
        x, _ = core_of(c)
        a = lb.operand_a(x["q"], lb.scale_of(c), c["mode"])
        z = (a[:, c["Nq"] // 2, :, 0] * x["k"][:, c["Nk"] // 2, :, 0]).astype(lb.F32)
        assert (z == -lb.EPS).all() and (z + lb.EPS == 0).all()
        assert (x["o"][:, c["Nq"] - 1, 0, 0] == -lb.EPS).all()


def test_the_nan_of_a_nanrow_case_stays_inside_its_head():
    for c in lb.core_cases():
        if c["family"] != "nanrow":
            continue
        _, ref = core_of(c)
        for n in lb.stored(c):
            nan = np.isnan(ref[n])
            nan = nan if n == "cam_P" else np.transpose(nan, (0, 2, 1, 3))          # -> [B, H, ...]
            clean = np.ones(nan.shape[:2], bool)
            clean[0, 0] = clean[-1, -1] = False
            assert not nan[clean].any(), (c["id"], n)
        if c["phase"] & lb.VALUES:
            assert np.isnan(ref["cam_P"][0, 0, c["Nq"] // 2]).all()
        if c["phase"] & lb.SCORES_PHASE:
            assert np.isnan(ref["cam_k"][-1, :, -1]).all() and np.isnan(ref["cam_q"][-1, -1, -1]).all()


@pytest.mark.parametrize("mutant", sorted(lb.CORE_MUTANTS))
def test_every_core_mutant_is_outside_a_bound_by_2x(mutant, capsys):
    names, applies = lb.CORE_MUTANTS[mutant]
    hit, n, best = 0, 0, 0.0
    for c in lb.core_cases():
        outs = [m for m in names if m in lb.stored(c)]
        if not applies(c) or not outs or c["family"] == "nanrow":
            continue
        x, ref = core_of(c)
        wrong = lb.core_ref(x, lb.scale_of(c), c["mode"], c["phase"], lb.with_scores(c), mut=mutant)
        worst = max(lb.ratio(wrong[m], ref[m], ref["e_" + m]) for m in outs)
        n += 1
        hit += worst >= 2.0
        best = max(best, min(worst, 1e30))
    assert n > 0 and hit > 0, "core mutant %s survives in all of its %d rows (largest error / bound %.3g)" % (mutant, n, best)
    say(capsys, "lrp core mutant %-38s at >= 2x a bound in %3d of %3d rows, largest error / bound %.3g" % (mutant, hit, n, best))


def test_an_fp32_restatement_of_every_rule_row_is_inside_its_bounds(capsys):
    top, unj = {}, {}
    for c in lb.rule_cases():
        x, ref = rule_of(c)
        got = lb.rule_restatement(c, x)
        for n, (val, bound) in ref.items():
            fig = lb.ratio(got[n].reshape(val.shape), val, bound)
            assert np.array_equal(np.isnan(got[n].reshape(val.shape)), np.isnan(val)), (c["id"], n)
            assert fig <= 1.0, (c["id"], n, fig)
            key = (c["kind"], c["family"], n)
            top[key] = max(top.get(key, 0.0), fig)
            unj[key] = max(unj.get(key, 0.0), lb.unjudged_share(bound))
            if c["family"] == "positive":
                assert lb.unjudged_share(bound) == 0.0, (c["id"], n)            # the well-conditioned family is judged everywhere
    for key in sorted(top):
        say(capsys, "lrp rule restatement %-8s %-8s %-5s worst error / bound %.3f   unjudged <= %.4f" % (key + (top[key], unj[key])))


@pytest.mark.parametrize("mutant", sorted(lb.RULE_MUTANTS))
def test_every_rule_mutant_is_outside_a_bound_by_2x(mutant, capsys):
    applies = lb.RULE_MUTANTS[mutant]
    hit, n, best = 0, 0, 0.0
    for c in lb.rule_cases():
        if heavy(c) or not applies(c):
            continue
        x, ref = rule_of(c)
        wrong = lb.rule_ref(c, x, mut=mutant)
        worst = max(lb.ratio(wrong[m][0], ref[m][0], ref[m][1]) for m in ref)
        n += 1
        hit += worst >= 2.0
        best = max(best, min(worst, 1e30))
    assert n > 0 and hit > 0, "rule mutant %s survives in all of its %d rows (largest error / bound %.3g)" % (mutant, n, best)
    say(capsys, "lrp rule mutant %-32s at >= 2x a bound in %3d of %3d rows, largest error / bound %.3g" % (mutant, hit, n, best))


def test_the_sum_count_is_the_code_s():
    """trips + 24 at the 1024-block cap, trips + 21 up to 256 blocks; the counts the tables reach."""
    assert lb.n_adds(lb.CAP, 1024) == 25 and lb.n_adds(lb.CAP + 1, 1024) == 26 and lb.n_adds(2 * lb.CAP + 77, 1024) == 27
    assert lb.n_adds(3 * 65536 + 5, 256) == 4 + 21 and lb.n_adds(1, 1) == 22
    assert lb.grid_of(1) == 1 and lb.grid_of(257) == 2 and lb.grid_of(lb.CAP + 1) == 1024 and lb.rescale_grid([3 * 65536 + 5]) == 256
    # the restated tree adds what a float64 sum adds
    g = np.random.default_rng(0)
    x = np.abs(g.standard_normal(2 * lb.CAP + 77)).astype(lb.F32)
    s = float(lb.tree_sum32(x, 1024))
    assert abs(s - x.astype(np.float64).sum()) <= lb.n_adds(x.size, 1024) * lb.U * x.astype(np.float64).sum()


def test_safe_divide_special_values_in_fp32_are_torch_s():
    """The fp32 restatement of ``safe_divide`` has the bits of ``lrp.safe_divide`` (torch, fp32, CPU) on every pair of the special
    values -- zero, sign and NaN pattern included -- and the float64 form is within ``2 u |s| + 2**-126`` of it where it is finite."""
    import torch
    from transformer_mm_explainability_amd import lrp
    a, b = lb.special_pairs()
    want = lrp.safe_divide(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    got = lb.sd32(a, b)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.int32), want[ok].view(np.int32))
    s, _, _ = lb.sd(a, b)
    fin = np.isfinite(want) & np.isfinite(s)
    assert (np.abs(want[fin] - s[fin]) <= 2 * lb.U * np.abs(s[fin]) + lb.TINY).all()


def test_the_tables_hold_what_the_device_test_is_asked_to_cover():
    cases = lb.core_cases()
    assert len({c["id"] for c in cases}) == len(cases) and len(cases) <= 160
    for dp in (32, 64):
        for phase in lb.PHASES:
            rows = [c for c in cases if (32 if c["D"] <= 32 else 64) == dp and c["phase"] == phase and c["B"] == 2]
            assert {c["D"] for c in rows} == set(lb.DIMS[dp]), (dp, phase)
            assert {(c["Nq"], c["Nk"]) for c in rows} == set(lb.SHAPES), (dp, phase)
            assert {c["mode"] for c in rows} == {lb.Q_FIRST, lb.SCORES}
            assert {c["layout"] for c in rows} == set(lb.LAYOUTS)
            fams = set(lb.CORE_FAMILIES) - ({"eps"} if dp == 64 else set())
            assert {c["family"] for c in rows} == fams, (dp, phase, {c["family"] for c in rows})
    assert any((c["B"], c["H"], c["Nq"], c["Nk"], c["D"]) == (1, 8, 100, 950, 32) for c in cases)
    rules = lb.rule_cases()
    assert len({c["id"] for c in rules}) == len(rules)
    counts = {c["rows"] * c["n"] for c in rules if c["kind"] == "combine"}
    assert counts == {1, 255, 257, lb.CAP - 1, lb.CAP, lb.CAP + 1, 2 * lb.CAP + 77}
    assert all(1024 * 256 % c["n"] or c["n"] in (1, 64) for c in rules if c["kind"] == "combine")
    assert {(c["rows"], c["n_in"], c["n_out"]) for c in rules if c["kind"] == "linear"} == set(lb.LINEAR_SHAPES)
    assert {c["normalize"] for c in rules if c["kind"] == "linear"} == {True, False}
    adds = [c for c in rules if c["kind"] == "add" and c["per_sample"]]
    assert {(c["batch"], c["per"]) for c in adds} == {(b, p) for b in lb.ADD_BATCH for p in lb.ADD_PER}
    assert any(not c["per_sample"] for c in rules if c["kind"] == "add")
    assert {c["inputs"] for c in rules if c["kind"] == "clone"} == set(lb.CLONE_INPUTS)
    assert {c["branch"] for c in rules if c["kind"] == "rescale"} == {"taken", "pre_zero", "pre_nan", "post_nonzero"}
    assert any(c["sizes"][2] == 3 * 65536 + 5 and lb.rescale_grid(c["sizes"]) == 256 for c in rules if c["kind"] == "rescale")
    for fam in lb.RULE_FAMILIES:
        assert {c["kind"] for c in rules if c["family"] == fam} >= {"combine", "linear", "add", "clone"}, fam
