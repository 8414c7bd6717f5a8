"""CPU: the bounds, the inputs and the case table of ``tests/attention_f32_bounds.py`` are sound before a kernel is held to them.

* At every row of the table an fp32 restatement of the row's kernel family (numpy float32, the family's own order of operations: the
  whole-head kernels' sequential in-lane sums and four-row tree, the tiled kernels' 64 lanes and ``expf``, the streaming kernels' 64-key
  tiles with a running maximum and rescaling, the one-sweep forward that rescales O itself) lies inside the bound of every output, and
  its NaN pattern (a fully masked query row) is the reference's.
* Every mutant (a deliberately wrong float64 reference: one realistic slip of a kernel) puts an output that a row STORES at >= 2x its
  bound in at least one row of the table; in how many of the rows where it applies is printed.
* The table reaches every ``(DP, NTK)`` instantiation of the whole-head dispatch for the capture forward, the no-slab forward and each
  backward form (plain, row mode, grouped row mode), every streaming and tiled path, and the routing edges -- computed from ``route``
  and the shapes.

The worst error / bound of every output and family is printed (past pytest's capture)."""
import numpy as np
import pytest

import attention_f32_bounds as fb

_cache = {}
BOUND = {"P": "e_P", "O": "e_O", "dP": "e_dP", "dq": "e_dq", "dk": "e_dk", "dv": "e_dv", "rel_out": "e_rel"}


def say(capsys, line):
    with capsys.disabled():
        print("\n  " + line, end="")


def fwd_routes(c):
    """The kernel families a forward row meets: its capture forward and, where another family serves it, its no-slab forward."""
    return [c["kernel"]] + ([c["kernel_noslab"]] if c["kernel_noslab"] != c["kernel"] else [])


def ref_of(c):
    """The reference of a case (forward rows: one per kernel family the row meets), computed once."""
    if c["id"] not in _cache:
        x = fb.case_inputs(c)
        if c["kind"] == "fwd":
            refs = {r: fb.fwd_ref(x["q"], x["k"], x["v"], fb.scale_of(c), c["mode"], x["mask"], r) for r in fwd_routes(c)}
            _cache[c["id"]] = (x, refs)
        else:
            P, o = fb.reference_forward_for(c, x)
            ref = fb.bwd_ref(x["q"], x["k"], x["v"], P, x["dO"], o, fb.scale_of(c), c["mode"], c["kernel"],
                             x["rel"] if c["rel"] else None, c["need"])
            _cache[c["id"]] = (x, P, o, ref)
    return _cache[c["id"]]


def bwd_outputs(c):
    """The outputs a backward row stores."""
    return [n for n in ("dP", "dq", "dk", "dv", "rel_out")
            if (n == "dP" and c["dprobs"]) or (n == "rel_out" and c["rel"]) or (n in ("dq", "dk", "dv") and c["need"])]


def test_an_fp32_restatement_of_every_forward_row_is_inside_its_bounds(capsys):
    top = {}
    for c in fb.fwd_cases():
        x, refs = ref_of(c)
        for r, ref in refs.items():
            P, O = fb.fwd_restatement(x["q"], x["k"], x["v"], fb.scale_of(c), c["mode"], x["mask"], r)
            figs = {"O": fb.ratio(O, ref["O"], ref["e_O"])}
            assert np.array_equal(np.isnan(O), np.isnan(ref["O"])), (c["id"], r)
            if P is not None:
                figs["P"] = fb.ratio(P, ref["P"], ref["e_P"])
                assert np.array_equal(np.isnan(P), np.isnan(ref["P"])), (c["id"], r)
            assert all(f <= 1.0 for f in figs.values()), (c["id"], r, c["family"], c["mask"], figs)
            for n, f in figs.items():
                top[(r, n)] = max(top.get((r, n), 0.0), f)
        if c["mask"] == "rowmasked" and c["family"] != "underflow":
            assert np.isnan(refs[c["kernel"]]["P"][:, :, c["Nq"] // 2]).all()             # the fully masked row is there
    say(capsys, "attention_f32 forward restatement worst error / bound: %s"
        % "  ".join("%s %s %.3f" % (k[0], k[1], v) for k, v in sorted(top.items())))


def test_an_fp32_restatement_of_every_backward_row_is_inside_its_bounds(capsys):
    top = {}
    for c in fb.bwd_cases():
        x, P, o, ref = ref_of(c)
        got = fb.bwd_restatement(x["q"], x["k"], x["v"], P, x["dO"], o, fb.scale_of(c), c["mode"], c["kernel"],
                                 x["rel"] if c["rel"] else None, c["need"])
        figs = {n: fb.ratio(got[n], ref[n], ref[BOUND[n]]) for n in bwd_outputs(c)}
        assert all(f <= 1.0 for f in figs.values()), (c["id"], c["family"], figs)
        for n, f in figs.items():
            top[(c["kernel"], n)] = max(top.get((c["kernel"], n), 0.0), f)
    say(capsys, "attention_f32 backward restatement worst error / bound: %s"
        % "  ".join("%s %s %.3f" % (k[0], k[1], v) for k, v in sorted(top.items())))


def test_the_summation_orders_are_really_different():
    """The sequential (whole-head), the 64-lane (tiled) and the tiled-with-rescale (streaming, one-sweep) restatements give different
    bits on one and the same row: the bounds are shown to hold for more than one order of the same sums."""
    c = next(c for c in fb.fwd_cases() if c["kernel"] == "split" and c["Nk"] > 128 and c["family"] == "randn")
    x, _ = ref_of(c)
    got = {r: fb.fwd_restatement(x["q"], x["k"], x["v"], fb.scale_of(c), c["mode"], x["mask"], r) for r in ("head", "tiled", "split", "stream1")}
    assert not np.array_equal(got["head"][0], got["split"][0]) and not np.array_equal(got["head"][0], got["tiled"][0])
    assert not np.array_equal(got["split"][1], got["stream1"][1])


@pytest.mark.parametrize("mutant", sorted(fb.FWD_MUTANTS))
def test_every_forward_mutant_is_outside_a_bound_by_2x(mutant, capsys):
    names, applies = fb.FWD_MUTANTS[mutant]
    hit, n, best = 0, 0, 0.0
    for c in fb.fwd_cases():
        if not applies(c):
            continue
        x, refs = ref_of(c)
        n += 1
        seen = False
        for r, ref in refs.items():
            wrong = fb.fwd_ref(x["q"], x["k"], x["v"], fb.scale_of(c), c["mode"], x["mask"], r, mut=mutant)
            stored = [m for m in names if not (m == "P" and r == "stream1")]              # (the one-sweep forward stores no P)
            worst = max(fb.ratio(wrong[m], ref[m], ref[BOUND[m]]) for m in stored)
            seen = seen or worst >= 2.0
            best = max(best, min(worst, 1e30))
        hit += seen
    assert n > 0 and hit > 0, "forward mutant %s survives in all of its %d rows (largest error / bound %.3g)" % (mutant, n, best)
    say(capsys, "attention_f32 forward mutant %-28s at >= 2x a bound in %3d of %3d rows, largest error / bound %.3g" % (mutant, hit, n, best))


@pytest.mark.parametrize("mutant", sorted(fb.BWD_MUTANTS))
def test_every_backward_mutant_is_outside_a_bound_by_2x(mutant, capsys):
    names, applies = fb.BWD_MUTANTS[mutant]
    hit, n, best = 0, 0, 0.0
    for c in fb.bwd_cases():
        stored = [m for m in names if m in bwd_outputs(c)]
        if not applies(c) or not stored:
            continue
        x, P, o, ref = ref_of(c)
        wrong = fb.bwd_ref(x["q"], x["k"], x["v"], P, x["dO"], o, fb.scale_of(c), c["mode"], c["kernel"],
                           x["rel"] if c["rel"] else None, c["need"], mut=mutant)
        worst = max(fb.ratio(wrong[m], ref[m], ref[BOUND[m]]) for m in stored)
        n += 1
        hit += worst >= 2.0
        best = max(best, min(worst, 1e30))
    assert n > 0 and hit > 0, "backward mutant %s survives in all of its %d rows (largest error / bound %.3g)" % (mutant, n, best)
    say(capsys, "attention_f32 backward mutant %-28s at >= 2x a bound in %3d of %3d rows, largest error / bound %.3g" % (mutant, hit, n, best))


def test_there_are_at_least_twenty_mutants():
    assert len(set(fb.FWD_MUTANTS) | {"bwd " + m for m in fb.BWD_MUTANTS}) >= 20


def test_the_table_reaches_every_instantiation_and_edge():
    cases = fb.all_cases()
    assert 200 <= len(cases) <= 280
    assert len({c["id"] for c in cases}) == len(cases)
    every = {(dp, ntk) for dp in (32, 64) for ntk in range(1, 9)}
    for form in ("fwd", "noslab", "bwd", "rel", "grouped"):
        assert fb.head_pairs(cases, form) == every, (form, sorted(every - fb.head_pairs(cases, form)))
    fwd = [c for c in cases if c["kind"] == "fwd"]
    bwd = [c for c in cases if c["kind"] == "bwd"]
    head_f = [c for c in fwd if c["kernel"] == "head"]
    assert {c["Nk"] for c in head_f} >= set(fb.LADDER) and {(c["Nq"], c["Nk"]) for c in head_f} >= set(fb.CROSS_HEAD)
    assert {c["D"] for c in head_f} == {4, 8, 20, 32, 36, 64} and {c["mode"] for c in head_f} == {0, 1}
    # the no-slab forward's two-workgroup split: NTK >= 7 with more than 8 query strips
    assert any(-(-c["Nk"] // 16) >= 7 and -(-c["Nq"] // 16) > 8 for c in head_f)
    # streaming forward: both option values; the small-grid kernel, the 64-row kernel and the one-sweep kernel all reached
    sf = [c for c in fwd if c["kernel"] in ("stream", "split")]
    assert {c["split"] for c in sf} == {0, 1} and {c["kernel"] for c in sf} == {"stream", "split"}
    assert {c["kernel_noslab"] for c in sf} == {"stream1", "split"}
    assert {c["Nk"] for c in sf if c["Nq"] == c["Nk"]} == set(fb.STREAM_N) and {(c["Nq"], c["Nk"]) for c in sf} >= set(fb.CROSS_STREAM)
    tf = [c for c in fwd if c["kernel"] == "tiled"]
    assert {c["D"] for c in tf} >= {6, 10, 20, 64} and {c["Nk"] for c in tf} >= {1, 17, 65, 130}
    # routing edges: a misaligned view of a whole-head shape goes to the tiled kernels, forward and backward; at NTK >= 7 with
    # Nq > 128 the forward stays whole-head while the backward streams
    assert any(c["misaligned"] and c["head"] and c["Nk"] <= 128 and c["D"] % 4 == 0 and c["kernel"] == "tiled" for c in fwd)
    assert any(c["misaligned"] and c["head"] and c["kernel"] == "tiled" for c in bwd)
    for Nq, Nk in ((129, 100), (256, 128)):
        assert any((c["Nq"], c["Nk"]) == (Nq, Nk) and c["kernel"] == "head" for c in fwd)
        assert any((c["Nq"], c["Nk"]) == (Nq, Nk) and c["head"] and c["kernel"] == "stream" for c in bwd)
    hb = [c for c in bwd if c["kernel"] == "head" and not c["rel"]]
    assert {c["Nk"] for c in hb if c["Nq"] == c["Nk"]} >= set(fb.LADDER)
    assert {c["o"] for c in hb} == {True, False} and {c["need"] for c in hb} == {True, False}
    sb = [c for c in bwd if c["kernel"] == "stream" and not c["rel"]]
    assert {c["o"] for c in sb} == {True, False} and {c["need"] for c in sb} == {True, False}
    for images in (0, 2):
        rows = [c for c in bwd if c["rel"] and c["images"] == images]
        assert {c["Nk"] for c in rows if c["kernel"] == "head"} >= {16, 17, 81, 128}
        assert {c["Nk"] for c in rows if c["kernel"] == "stream"} == {129, 200}
        assert {c["need"] for c in rows} == {True, False} and {c["dprobs"] for c in rows} == {True, False}
    assert any(c["shared"] for c in fwd) and any(c["shared"] for c in bwd)
    for fam in ("head", "stream", "tiled"):                         # every input family reaches every kernel family, both ways
        assert {c["family"] for c in fwd if c["kernel"] == fam or (fam == "stream" and c["kernel"] == "split")} == set(fb.FAMILIES), fam
        assert {c["family"] for c in bwd if c["kernel"] == fam} == set(fb.FAMILIES), fam
    assert {c["mask"] for c in fwd} == set(fb.MASKS)
