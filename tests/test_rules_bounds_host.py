"""CPU: the references, bounds, inputs and case tables of ``tests/rules_bounds.py`` are sound before a kernel is held to them.

* At every row of every table an fp32 restatement of the row's kernel lies inside the bound at every element, with the reference's NaN
  pattern, and its diag word inside the reference's interval (NaN iff the reference's).
* The row-sum condition of the division's bound, ``E_s <= 2**-10 |s|``, holds on every row that any eq. 8-9 of any case divides, and a
  bound is finite wherever its reference is.
* Every mutant (an fp32 restatement with ONE fault) puts an output at >= 2x its bound, or breaks the NaN pattern, in at least one case
  where it applies; in how many is printed.
* The old-rule check: which mutants the max-norm tolerances of ``tests/test_gpu_ops.py`` let through on ``plain`` inputs is COMPUTED and
  asserted to be exactly ``rules_bounds.OLD_RULE_BLIND``.  With gradients of 0.2 randn the head means are about 0.08 / n, not 0.01 / n:
  a fault of first order in A_bar moves an entry by 1e-4 and more and the old tolerance of 1e-5 sees it; what it lets through, at up to
  several hundred times the counted bound, is printed per mutant as the smallest error / old tolerance over the plain cases.
* The float64 references agree with the fp32 oracle (``oracle/relevancy_np.py``) to its own rounding.
* The tables reach the routes and edges they name.

The worst error / bound per kernel and family is printed (past pytest's capture)."""
import numpy as np
import pytest
from oracle import relevancy_np as onp

import rules_bounds as rb

NAMES = ("R_tt", "R_ti", "R_ii", "R_it")
_cache = {}


def say(capsys, line):
    with capsys.disabled():
        print("\n  " + line, end="")


def sched_of(c):
    if c["id"] not in _cache:
        x = rb.schedule_inputs(c)
        _cache[c["id"]] = (x, rb.schedule_ref(c, x))
    return _cache[c["id"]]


def detr_of(c):
    if c["id"] not in _cache:
        x = rb.detr_inputs(c)
        _cache[c["id"]] = (x, rb.detr_ref(c, x))
    return _cache[c["id"]]


def rule_of(c):
    if c["id"] not in _cache:
        x = rb.rule_inputs(c)
        _cache[c["id"]] = (x, rb.rule_ref(c, x))
    return _cache[c["id"]]


def bound_is_finite_where_the_reference_is(want, bound):
    return bool(np.isfinite(np.asarray(bound)[np.isfinite(want)]).all())


def sched_figure(got, ref):
    return max(rb.ratio(got[n], ref[n], ref["e_" + n[2:]]) for n in NAMES)


def test_an_fp32_restatement_of_every_schedule_case_is_inside_its_bound(capsys):
    top = {}
    for c in rb.schedule_cases():
        x, ref = sched_of(c)
        got = rb.schedule_restatement(c, x)
        for n in NAMES:
            assert np.array_equal(np.isnan(got[n]), np.isnan(ref[n])), (c["id"], n)
            assert bound_is_finite_where_the_reference_is(ref[n], ref["e_" + n[2:]]), (c["id"], n)
        f = sched_figure(got, ref)
        assert f <= 1.0, (c["id"], f)
        assert ref["margin"] <= rb.MARGIN_LIMIT, (c["id"], ref["margin"])
        assert (ref["diag"] is None) == (not c["normalize"])
        if ref["diag"] is not None:
            assert rb.diag_ok(got["diag"], ref["diag"]), (c["id"], got["diag"], ref["diag"])
        if c["family"] not in ("nan",) and c["n_lang"] and c["n_vis"]:
            assert rb.is_finite_case(ref, NAMES), c["id"]
        if c["family"] == "nan":                                    # the poison stays in sample 0
            assert np.isnan(ref["R_tt"][0]).any() or np.isnan(ref["R_ti"][0]).any()
            assert all(np.isfinite(ref[n][1:]).all() for n in NAMES), c["id"]
        tl = x["text_len"]
        if tl is not None:                                          # zeros beyond the sample's question
            for b in range(c["B"]):
                t = int(tl[b])
                assert not ref["R_tt"][b, t:].any() and not ref["R_tt"][b, :, t:].any() and not ref["R_ti"][b, t:].any() \
                    and not ref["R_it"][b, :, t:].any()
        key = (c["route"], c["family"])
        top[key] = max(top.get(key, 0.0), f)
    for k, v in sorted(top.items()):
        say(capsys, "schedule restatement %-9s %-7s worst error / bound %.3f" % (k[0], k[1], v))


def test_an_fp32_restatement_of_every_detr_and_rule_case_is_inside_its_bound(capsys):
    top = {}
    for c in rb.detr_cases():
        x, ref = detr_of(c)
        got = rb.detr_restatement(c, x)
        f = rb.ratio(got["s"], ref["s"], ref["e_s"])
        assert f <= 1.0, (c["id"], f)
        assert bound_is_finite_where_the_reference_is(ref["s"], ref["e_s"]), c["id"]
        assert ref["margin"] <= rb.MARGIN_LIMIT, (c["id"], ref["margin"])
        assert rb.diag_ok(got["diag"], ref["diag"]), (c["id"], got["diag"], ref["diag"])
        k, l, name = rb.detr_poison(c)
        if c["family"] == "nan_cross":                              # the layer is dropped for that sample: nothing is NaN
            assert np.isfinite(ref["s"]).all() and not ref["diag"][3], c["id"]
        elif c["family"] == "nan_self":                             # rules 6 / 7 have no scrub: that sample's row and the word are NaN
            assert ref["diag"][3] and np.isfinite(np.delete(ref["s"], k, 0)).all(), c["id"]
            assert np.isnan(ref["s"][k]).any() or l == 0, c["id"]
        else:
            assert np.isfinite(ref["s"]).all(), c["id"]
        top["detr " + c["family"]] = max(top.get("detr " + c["family"], 0.0), f)
    for c in rb.rule_cases():
        x, ref = rule_of(c)
        got = rb.rule_restatement(c, x)
        assert ref["margin"] <= rb.MARGIN_LIMIT, (c["id"], ref["margin"])
        for n, v in got.items():
            f = rb.ratio(v, *ref[n])
            assert f <= 1.0, (c["id"], n, f)
            assert bound_is_finite_where_the_reference_is(*ref[n]), (c["id"], n)
            top[c["op"] + " " + n] = max(top.get(c["op"] + " " + n, 0.0), f)
        if c["op"] == "mm" and c["nan_to_zero"]:
            assert np.isfinite(ref["sq"][0]).all(), c["id"]
    for k, v in sorted(top.items()):
        say(capsys, "restatement %-18s worst error / bound %.3f" % (k, v))


def mutant_figure(mutant, c):
    table = rb.MUTANTS[mutant][0]
    if table == "schedule":
        x, ref = sched_of(c)
        return sched_figure(rb.schedule_restatement(c, x, mutant), ref)
    if table == "detr":
        x, ref = detr_of(c)
        return rb.ratio(rb.detr_restatement(c, x, mutant)["s"], ref["s"], ref["e_s"])
    x, ref = rule_of(c)
    return max(rb.ratio(v, *ref[n]) for n, v in rb.rule_restatement(c, x, mutant).items())


TABLES = {"schedule": rb.schedule_cases, "detr": rb.detr_cases, "rule": rb.rule_cases}


@pytest.mark.parametrize("mutant", sorted(rb.MUTANTS))
def test_every_mutant_is_outside_a_bound(capsys, mutant):
    table, applies = rb.MUTANTS[mutant]
    rows = [c for c in TABLES[table]() if applies(c)]
    assert rows, mutant
    figs = [(mutant_figure(mutant, c), c["id"]) for c in rows]
    hit = [f for f in figs if f[0] >= 2.0]
    assert hit, (mutant, figs)
    say(capsys, "mutant %-40s at >= 2x a bound in %3d of %3d cases, e.g. %s (%.3g)" % (mutant, len(hit), len(rows), hit[0][1], hit[0][0]))


def test_what_the_old_tolerances_let_through_on_plain_inputs(capsys):
    blind = set()
    for mutant, (table, applies) in sorted(rb.MUTANTS.items()):
        if table != "schedule":
            continue
        least = None
        for c in rb.schedule_cases():
            if c["family"] != "plain" or not applies(c):
                continue
            x, ref = sched_of(c)
            wrong = rb.schedule_restatement(c, x, mutant)
            f = sched_figure(wrong, ref)
            if f < 2.0 or not rb.is_finite_case(ref, NAMES) or not rb.is_finite_case(wrong, NAMES):
                continue
            if all(rb.old_rule_passes(wrong[n], ref[n]) for n in NAMES):
                blind.add(mutant)
            with np.errstate(invalid="ignore"):
                rel = max(float(np.nanmax(np.abs(wrong[n] - ref[n]))) / (1e-5 * max(float(np.nanmax(np.abs(ref[n]))), 1.0)) for n in NAMES)
            if least is None or rel < least[0]:
                least = (rel, f, c["id"])
        if least:
            say(capsys, "old rule, plain: %-40s smallest error / old tolerance %.3g (at %.3g x the counted bound, %s)" % ((mutant,) + least))
    for mutant, (table, applies) in sorted(rb.MUTANTS.items()):      # DETR: ``2e-6 max |ref|``
        if table != "detr":
            continue
        for c in rb.detr_cases():
            if c["family"] != "plain" or not applies(c):
                continue
            x, ref = detr_of(c)
            wrong = rb.detr_restatement(c, x, mutant)["s"]
            f = rb.ratio(wrong, ref["s"], ref["e_s"])
            if f >= 2.0 and rb.old_rule_passes(wrong, ref["s"], "detr"):
                blind.add(mutant)
            say(capsys, "old rule, plain: %-40s error / old tolerance %.3g (at %.3g x the counted bound, %s)"
                % (mutant, float(np.abs(wrong - ref["s"]).max()) / (2e-6 * float(np.abs(ref["s"]).max())), f, c["id"]))
    assert blind == set(rb.OLD_RULE_BLIND), sorted(blind)
    # the restatement itself passes the old rule on every plain case
    for c in rb.schedule_cases():
        if c["family"] == "plain" and c["n_lang"] and c["n_vis"]:
            x, ref = sched_of(c)
            got = rb.schedule_restatement(c, x)
            assert all(rb.old_rule_passes(got[n], ref[n]) for n in NAMES), c["id"]


def test_the_float64_references_agree_with_the_fp32_oracle():
    for c in rb.schedule_cases():
        if c["family"] in ("nan", "ragged", "tiny", "hot") or not (c["n_lang"] and c["n_vis"]) or c["B"] > 2:
            continue
        x, ref = sched_of(c)
        for b in range(c["B"]):
            pick = lambda g: [(a[b], gr[b]) for a, gr in x[g]]      # noqa: E731
            layers = []
            for i in range(c["n_x"]):
                blk = {"lang_cross": pick("xlc")[i], "lang_self": pick("xls")[i]}
                if i < c["n_x"] - 1:
                    blk["img_cross"], blk["img_self"] = pick("xic")[i], pick("xis")[i]
                layers.append(blk)
            la, lg = zip(*pick("lang"))
            va, vg = zip(*pick("vis"))
            want = onp.lxmert_generate_ours_chain(list(la), list(lg), list(va), list(vg), layers, c["normalize"], c["self10"], return_all=True)
            for n, w in zip(NAMES, want):
                assert np.abs(ref[n][b] - w).max() <= 2e-5 * max(1.0, np.abs(w).max()), (c["id"], n)
    for c in rb.rule_cases():
        x, ref = rule_of(c)
        if c["op"] == "residual" and not c["identity_rows"]:
            want = np.stack([onp.handle_residual(r) for r in x["R"]])
            assert np.allclose(ref["out"][0], want, rtol=1e-5, atol=1e-7), c["id"]
            assert abs(ref["diag"][0] - float(np.diagonal(x["R"] - np.eye(c["N"], dtype=np.float32), axis1=1, axis2=2).min())) <= 1e-7
        elif c["op"] == "rollout":
            want = onp.compute_rollout_attention(x["layers"], 0, c["normalize"])
            assert np.allclose(ref["out"][0], want, rtol=1e-5, atol=1e-7), c["id"]
        elif c["op"] == "mm" and not c["nan_cam"]:
            if c["rule11"]:
                sq, ss = onp.apply_mm_attention_rules_lxmert(x["R_ss"], x["R_qq"], x["R_qs"], x["cam"], c["normalize"], c["self10"])
                assert np.allclose(ref["ss"][0], ss, rtol=1e-5, atol=1e-7, equal_nan=True), c["id"]
            elif c["nan_to_zero"]:
                sq = onp.apply_mm_attention_rules_detr(x["R_ss"], x["R_qq"], x["cam"], c["normalize"], c["self10"])
            else:
                continue
            assert np.allclose(ref["sq"][0], sq, rtol=1e-5, atol=1e-7, equal_nan=True), c["id"]


def test_the_tables_reach_the_routes_and_edges_they_name():
    cases = rb.schedule_cases()
    cells = {(c["family"], c["route"]) for c in cases}
    assert cells >= {(f, r) for f in rb.FAMILIES for r in rb.ROUTES}, sorted({(f, r) for f in rb.FAMILIES for r in rb.ROUTES} - cells)
    for c in cases:                                                  # the W rule, restated
        W = rb.CUS // c["B"]
        W = max(1, min(W, rb.nblk(c)))
        assert W == c["W"] and c["route"] == ("W=1" if W == 1 and rb.nblk(c) > 1 else "W=nblk" if W == rb.nblk(c) else "1<W<nblk")
        if c["B"] == 257:
            assert c["H"] <= 2 and c["T"] <= 6 and c["I"] <= 6 and c["route"] == "W=1"
    assert {c["B"] for c in cases} >= {1, 2, 40, 257}
    assert {c["H"] for c in cases} >= {1, 5, 6, 7, 12, 13}
    assert {c["T"] for c in cases} | {c["I"] for c in cases} >= {1, 3, 15, 16, 17, 31, 32, 33, 47, 48}
    assert {(c["T"] > c["I"]) - (c["T"] < c["I"]) for c in cases} == {-1, 0, 1}
    assert sum(1 for p in {(c["T"], c["I"]) for c in cases} if p[0] * p[1] % 4) >= 3
    layers = {(c["n_lang"], c["n_vis"], c["n_x"]) for c in cases}
    assert layers >= {(0, 2, 2), (2, 0, 2), (1, 1, 1), (3, 2, 3), (16, 16, 16)}
    assert all(c["T"] <= 5 and c["I"] <= 5 for c in cases if c["n_x"] == 16)
    assert any(not c["normalize"] and c["family"] != "tiny" for c in cases) and any(not c["self10"] for c in cases)
    assert {c["poison"] for c in cases if c["family"] == "nan"} >= {"lang", "xlc"}
    for c in cases:
        if c["family"] == "ragged":
            tl = rb.schedule_inputs(c)["text_len"]
            assert tl.min() == 1 and tl.max() == c["T"], c["id"]
    d = rb.detr_cases()
    assert {c["Q"] for c in d} == {1, 2, 15, 16, 17, 33, 100, 127, 128} | {5}
    assert {c["Ni"] for c in d} == {1, 3, 63, 64, 65, 130, 257}
    assert {c["H"] for c in d} >= {1, 3, 4, 5, 8} and {c["L"] for c in d} >= {1, 2, 6, 16} and {c["K"] for c in d} >= {1, 3}
    assert {c["shared"] for c in d} == {False, True} and {c["targets"] for c in d} == {"first", "last", "random"}
    assert {c["family"] for c in d} == set(rb.DETR_FAMILIES)
    r = rb.rule_cases()
    assert {c["N"] for c in r if c["op"] == "residual"} == {1, 2, 5, 63, 64, 65, 130}
    assert any(c["B"] * c["N"] % 4 for c in r if c["op"] == "residual")
    assert {c["L"] for c in r if c["op"] == "rollout"} == {1, 2, 3} and {c["B"] for c in r if c["op"] == "rollout"} == {1, 3}
    assert {(c["rule11"], c["nan_to_zero"]) for c in r if c["op"] == "mm"} >= {(True, False), (False, True)}
    assert any(c["Ns"] != c["Nq"] for c in r if c["op"] == "mm")
    assert {c["Ns"] for c in r if c["op"] == "mm"} | {c["Nq"] for c in r if c["op"] == "mm"} >= {1, 2, 5, 63, 64, 65, 130}
