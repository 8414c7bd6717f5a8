"""CPU: the bounds, the inputs and the case table of ``tests/attention_bf16_bounds.py`` are sound before a kernel is held to them.

* An fp32 restatement of the bf16 matrix-core attention (numpy fp32 products of the bf16-rounded operands, numpy's accumulation order,
  libm's exp) lies inside the bound of every output at every case of the device test's table; so does the same restatement on torch's
  CPU fp32 ``matmul`` of the bf16-rounded operands, another accumulation order.  (torch's CPU bf16 ``matmul`` itself rounds its result
  to bf16, which the definition does not: it is not used.)
* Every mutant (a deliberately wrong float64 reference), at every case where it applies, puts at least one element of at least one of
  its named outputs at >= 2x its bound -- among the outputs the case really STORES (no dP without a dP slab), each judged in its stored
  type: an fp32 output by error / bound, a 16-bit output (rounded once to its type) by lying outside ``[rnd(v - 2b), rnd(v + 2b)]``.
* The near-tie allowance is conditioned: at every forward case at most 5 % of the entries of P may round either way; for dS the share is
  recorded only (the cancellation in ``dP - delta`` makes it input dependent -- the mutants are what guards dQ and dK).
* The table reaches every kernel family at a partial tile, at an exact tile multiple and with D below its padded width.

The worst error / bound of every output and every mutant's smallest detection ratio are printed (past pytest's capture)."""
import numpy as np
import pytest
import torch

import attention_bf16_bounds as ab

F32 = ab.F32
FWD_OUT = ("P", "O")
BWD_OUT = ("dP", "dq", "dk", "dv", "rel_out")
_cache = {}


def say(capsys, line):
    with capsys.disabled():
        print("\n  " + line, end="")


def torch_fp32_matmul(a, b):
    """torch's CPU fp32 product of the bf16-rounded operands (they pass through torch's bf16 type unchanged: they are bf16 numbers)."""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, F32)).to(torch.bfloat16).float()
    return torch.matmul(t(a), t(b)).numpy()


def fwd_of(c):
    """The reference forward of a case, computed once."""
    if c["id"] not in _cache:
        x = ab.case_inputs(c)
        if c["kind"] == "fwd":
            _cache[c["id"]] = (x, ab.fwd_ref(x["q"], x["k"], x["v"], ab.scale_of(c), c["mode"], x["mask"], c["slab"]))
        else:
            P, o = ab.reference_forward_for(c, x)
            rel = x["rel"] if c["rel"] else None
            _cache[c["id"]] = (x, P, o, ab.bwd_ref(x["q"], x["k"], x["v"], P, x["dO"], o, ab.scale_of(c), c["mode"], rel))
    return _cache[c["id"]]


def fwd_figures(c, got_slab, got_o, ref):
    return {"P": ab.judge(got_slab, ref["P"], ref["e_P"], c["slab"]), "O": ab.ratio(got_o, ref["O"], ref["e_O"])}


def bwd_outputs(c):
    """The outputs a case stores (no dP without a dP slab)."""
    return [n for n in BWD_OUT if (n == "dP" and c["dprobs"]) or (n == "rel_out" and c["rel"]) or (n in ("dq", "dk", "dv") and c["need"])]


def bwd_figures(c, got, ref, kinds=None):
    """``got``: dict of arrays; ``kinds``: the stored type per output (default fp32)."""
    kinds = kinds or {}
    bound = {"dP": "e_dP", "dq": "e_dq", "dk": "e_dk", "dv": "e_dv", "rel_out": "e_rel"}
    return {n: ab.judge(got[n], ref[n], ref[bound[n]], kinds.get(n, "f32")) for n in bwd_outputs(c) if got.get(n) is not None}


@pytest.mark.parametrize("impl", ["numpy fp32", "torch fp32 matmul of the bf16 operands"])
def test_an_fp32_restatement_of_the_forward_is_inside_the_bound(impl, capsys):
    mm = None if impl == "numpy fp32" else torch_fp32_matmul
    top = {}
    for c in ab.fwd_cases():
        x, ref = fwd_of(c)
        slab, o = ab.fwd_restatement(x["q"], x["k"], x["v"], ab.scale_of(c), c["mode"], x["mask"], c["slab"], matmul=mm)
        fig = fwd_figures(c, slab, o, ref)
        assert ab.passes(fig["P"], c["slab"]) and ab.passes(fig["O"]), (c["id"], fig)
        assert np.array_equal(np.isnan(o), np.isnan(ref["O"])) and np.array_equal(np.isnan(slab), np.isnan(ref["P"])), c["id"]
        key = c["kernel"]
        if c["slab"] == "f32":
            top[key + " P"] = max(top.get(key + " P", 0.0), fig["P"])
        top[key + " O"] = max(top.get(key + " O", 0.0), fig["O"])
    say(capsys, "attention_bf16 forward restatement (%s) worst error / bound: %s" % (impl, "  ".join("%s %.3f" % kv for kv in sorted(top.items()))))


@pytest.mark.parametrize("impl", ["numpy fp32", "torch fp32 matmul of the bf16 operands"])
def test_an_fp32_restatement_of_the_backward_is_inside_the_bound(impl, capsys):
    mm = None if impl == "numpy fp32" else torch_fp32_matmul
    top = {}
    for c in ab.bwd_cases():
        x, P, o, ref = fwd_of(c)
        got = ab.bwd_restatement(x["q"], x["k"], x["v"], P, x["dO"], o, ab.scale_of(c), c["mode"], x["rel"] if c["rel"] else None, matmul=mm)
        fig = bwd_figures(c, got, ref)
        assert all(ab.passes(v) for v in fig.values()), (c["id"], fig)
        # the 16-bit forms of the same results: rounded once, they lie in their intervals
        for n in ("dq", "dk", "dv"):
            if c["io_bf16"] and c["need"]:
                assert ab.outside_interval(ab.rne_bf16(got[n]), ref[n], ref["e_" + n], "bf16") == 0, (c["id"], n)
        if c["slab"] != "f32":
            assert ab.outside_interval(ab.slab_round(got["dP"], c["slab"]), ref["dP"], ref["e_dP"], c["slab"]) == 0, c["id"]
        for n, v in fig.items():
            top[(c["kernel"], n)] = max(top.get((c["kernel"], n), 0.0), v)
    say(capsys, "attention_bf16 backward restatement (%s) worst error / bound: %s"
        % (impl, "  ".join("%s %s %.3f" % (k[0], k[1], v) for k, v in sorted(top.items()))))


def test_the_near_tie_allowance_is_conditioned(capsys):
    """At most 5 % of the entries of P may round either way at every forward case (the counted bound), and under the issue's crude error
    at its three shapes; the dS share is recorded."""
    worst = 0.0
    for c in ab.fwd_cases():
        share = fwd_of(c)[1]["flagged"]
        assert share <= 0.05, (c["id"], c["family"], share)
        worst = max(worst, share)
    say(capsys, "attention_bf16 near-tie share of P, counted bound, worst over the forward cases: %.4f" % worst)
    for Nq, Nk, D in ((70, 130, 64), (65, 65, 32), (130, 130, 64)):
        x = ab.inputs("randn", 2, 2, ab.H, Nq, Nk, D)
        share = ab.crude_flag_share(x["q"], x["k"], x["v"], D ** -0.5, ab.Q_FIRST)
        assert share <= 0.05, (Nq, Nk, D, share)
        say(capsys, "attention_bf16 near-tie share of P, crude error, %dx%dx%d: %.4f" % (Nq, Nk, D, share))
    ds = {}
    for c in ab.bwd_cases():
        if c["need"]:
            ds.setdefault(c["kernel"], []).append(fwd_of(c)[3]["flagged_dS"])
    for k, v in sorted(ds.items()):
        say(capsys, "attention_bf16 near-tie share of dS (recorded) %s: median %.4f, worst %.4f" % (k, float(np.median(v)), max(v)))


BOUND = {"P": "e_P", "O": "e_O", "dP": "e_dP", "dq": "e_dq", "dk": "e_dk", "dv": "e_dv", "rel_out": "e_rel"}


def detection(wrong, ref, names, kinds):
    """A mutant's outputs against the reference, each in the type the device stores it in -> (is one of the named outputs at >= 2x its
    bound: an fp32 output by error / bound, a 16-bit output, rounded once to its type, by an element outside ``[rnd(v - 2b),
    rnd(v + 2b)]``; the largest fp32 error / bound over the named outputs, for the record)."""
    seen, top = False, 0.0
    for n in names:
        b = ref[BOUND[n]]
        r = ab.ratio(wrong[n], ref[n], b)
        top = max(top, r)
        if kinds[n] == "f32":
            seen = seen or r >= 2.0
        else:
            seen = seen or ab.outside_interval(ab.slab_round(wrong[n], kinds[n]), ref[n], 2 * b, kinds[n]) > 0
    return seen, top


@pytest.mark.parametrize("mutant", sorted(ab.FWD_MUTANTS))
def test_every_forward_mutant_is_outside_the_bound_by_2x(mutant, capsys):
    names, applies = ab.FWD_MUTANTS[mutant]
    low, n = None, 0
    for c in ab.fwd_cases():
        if not applies(c):
            continue
        x, ref = fwd_of(c)
        wrong = ab.fwd_ref(x["q"], x["k"], x["v"], ab.scale_of(c), c["mode"], x["mask"], c["slab"], mut=mutant)
        seen, r = detection(wrong, ref, names, {"P": c["slab"], "O": "f32"})
        assert seen, "forward mutant %s survives at %s (%s, mask %s): error / bound %.3g" % (mutant, c["id"], c["family"], c["mask"], r)
        low, n = (r if low is None else min(low, r)), n + 1
    assert n > 0
    say(capsys, "attention_bf16 forward mutant %-28s %3d cases, smallest error / bound %.3g" % (mutant, n, low))


@pytest.mark.parametrize("mutant", sorted(ab.BWD_MUTANTS))
def test_every_backward_mutant_is_outside_the_bound_by_2x(mutant, capsys):
    names, applies = ab.BWD_MUTANTS[mutant]
    low, n = None, 0
    for c in ab.bwd_cases():
        stored = [m for m in names if m in bwd_outputs(c)]
        if not applies(c) or not stored:                            # (none of its outputs is stored by this case)
            continue
        x, P, o, ref = fwd_of(c)
        wrong = ab.bwd_ref(x["q"], x["k"], x["v"], P, x["dO"], o, ab.scale_of(c), c["mode"], x["rel"] if c["rel"] else None, mut=mutant)
        io = "bf16" if c["io_bf16"] else "f32"
        seen, r = detection(wrong, ref, stored, {"dP": c["slab"], "dq": io, "dk": io, "dv": io, "rel_out": "f32"})
        assert seen, "backward mutant %s survives at %s (%s): error / bound %.3g" % (mutant, c["id"], c["family"], r)
        low, n = (r if low is None else min(low, r)), n + 1
    assert n > 0
    say(capsys, "attention_bf16 backward mutant %-28s %3d cases, smallest error / bound %.3g" % (mutant, n, low))


def test_the_table_reaches_every_kernel_family_at_its_edges():
    """A partial tile, an exact multiple of the tile and a head dim below its padded width, for each of the forward's two widths and the
    three backward generations (with both key sides of the third); every listed path of the issue has a row."""
    cases = ab.all_cases()
    assert 150 <= len(cases) <= 220
    assert len({c["id"] for c in cases}) == len(cases)
    padded = {"fwd32": 32, "fwd64": 64, "gen1": None, "gen2": 64, "gen3": 64, "gen4": 64}
    for fam, width in padded.items():
        rows = [c for c in cases if c["kernel"] == fam]
        assert any(c["Nk"] % 64 and c["Nk"] > 64 for c in rows), fam
        assert any(c["Nk"] % 64 == 0 for c in rows), fam
        if fam in ("gen3", "gen4"):
            assert all(c["D"] == 64 for c in rows)                  # these kernels exist at the full width only
        else:
            assert any(c["D"] < (width or (32 if c["D"] <= 32 else 64)) for c in rows), fam
    fwd = [c for c in cases if c["kind"] == "fwd"]
    assert {c["slab"] for c in fwd} == set(ab.SLABS) and {c["mode"] for c in fwd} == {0, 1} and {c["mask"] for c in fwd} == set(ab.MASKS)
    g1 = [c for c in cases if c["kernel"] == "gen1"]
    for pred in (lambda c: not c["o"], lambda c: c["o"] and not c["v2"], lambda c: c["D"] in (12, 20)):
        sub = [c for c in g1 if pred(c)]
        assert {(c["dprobs"], c["rel"], c["io_bf16"]) for c in sub} >= {(d, r, i) for d, r in ab.MODES3 for i in (False, True)}
    g2 = [c for c in cases if c["kernel"] == "gen2"]
    assert {c["D"] for c in g2} == {8, 40, 64} and {c["slab"] for c in g2} == set(ab.SLABS)
    assert {(c["rel"], c["need"], c["shared"], c["io_bf16"]) for c in g2} >= {(r, n, s, i) for r, n in ((False, True), (True, True), (True, False))
                                                                               for s in (False, True) for i in (False, True)}
    for fam in ("gen3", "gen4"):
        assert {c["need"] for c in cases if c["kernel"] == fam} == {True, False}
    # every input family reaches every kernel family it bears on: all five for the backward generations and the DP = 32 forward;
    # the DP = 64 forward (D = 40, 64) has no ``peaked`` row (its near-tie share of P passes the 5 % condition there, see ``_case``)
    for fam in padded:
        want = set(ab.FAMILIES) - ({"peaked"} if fam == "fwd64" else set())
        assert {c["family"] for c in cases if c["kernel"] == fam} >= want, fam
    peaked = [c for c in cases if c["kernel"] == "fwd32" and c["family"] == "peaked"]
    assert {(c["mode"], c["slab"]) for c in peaked} == {(m, s) for m in (0, 1) for s in ab.SLABS}
    assert any(c["Nk"] % 64 and c["Nk"] > 64 for c in peaked) and any(c["Nk"] % 64 == 0 for c in peaked)


def test_the_interval_check_sees_a_truncated_result():
    """A bf16 result rounded towards zero instead of to nearest is outside its interval somewhere; the rounded one nowhere."""
    c = next(c for c in ab.bwd_cases() if c["kernel"] == "gen2" and c["io_bf16"] and c["need"] and c["Nq"] >= 64)
    x, P, o, ref = fwd_of(c)
    got = ab.bwd_restatement(x["q"], x["k"], x["v"], P, x["dO"], o, ab.scale_of(c), c["mode"])
    assert ab.outside_interval(ab.rne_bf16(got["dv"]), ref["dv"], ref["e_dv"], "bf16") == 0
    assert ab.outside_interval(ab.trunc_bf16(got["dv"]), ref["dv"], ref["e_dv"], "bf16") > 0
