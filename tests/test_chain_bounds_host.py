"""CPU: the bounds, the inputs and the case tables of ``tests/chain_bounds.py`` are sound before a kernel is held to them.

* At every row of every table an fp32 restatement of the row's kernel (numpy float32 in the kernel's own order: heads summed in
  ascending order, the product accumulated in the k groups one MFMA instruction sums, the layer groups re-associated, the 32-row and
  4-row partials of the vector forms) lies inside the bound at every element, with the reference's NaN / inf pattern.
* Every mutant (an fp32 restatement with ONE defect) puts an output at >= 2x its bound in at least one row where it applies; in how
  many of them is printed.
* The mutant in which one 16-row block of a layer's product reads the updated R passes the tolerance ``tests/test_gpu_ops.py`` holds
  the chain to (``1e-5 + 1e-5 |ref|``, ``1e-4 max |ref|``) at a row where it is 100x outside the counted bound: why this file exists.
* The NaN / inf pattern of the ``nan`` and ``inf`` references is what ``torch.clamp`` / ``torch.bmm`` give on CPU float64.
* The tables reach every route and edge they name (a count over the tables, from ``chain_route`` and the shapes alone).

The worst error / bound per kernel and family is printed (past pytest's capture)."""
import numpy as np
import pytest
import torch

import chain_bounds as cb

_cache = {}


def say(capsys, line):
    with capsys.disabled():
        print("\n  " + line, end="")


def ref_of(c):
    if c["id"] not in _cache:
        x = cb.chain_inputs(c)
        _cache[c["id"]] = (x, cb.chain_ref(c, x))
    return _cache[c["id"]]


def outputs(c):
    return (("R", "e_R"), ("SQ", "e_SQ")) if c["M"] else (("R", "e_R"),)


def same_class(got, want):
    return np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) \
        and not np.isneginf(got).any()


def test_an_fp32_restatement_of_every_chain_row_is_inside_its_bound(capsys):
    top, med = {}, {}
    for c in cb.chain_cases():
        x, ref = ref_of(c)
        got = cb.chain_restatement(c, x)
        for n, e in outputs(c):
            f = cb.ratio(got[n], ref[n], ref[e])
            assert same_class(got[n], ref[n]), (c["id"], n)
            assert f <= 1.0, (c["id"], n, f)
            key = (c["kernel"] + (" grouped" if c["G"] > 1 else ""), c["family"])
            top[key] = max(top.get(key, 0.0), f)
            if c["family"] == "plain" and n == "R" and c["L"] > 1:
                med[c["kernel"]] = float(np.median(ref[e]))
        if c["G"] > 1 and c["family"] in cb.FINITE:                 # the re-association is exact in exact arithmetic
            assert np.allclose(ref["R_grouped"], ref["R"], rtol=1e-11, atol=1e-300), c["id"]
    for k, v in sorted(top.items()):
        say(capsys, "chain restatement %-14s %-11s worst error / bound %.3f" % (k[0], k[1], v))
    say(capsys, "chain median bound of R, plain rows: %s" % "  ".join("%s %.2e" % kv for kv in sorted(med.items())))


def test_an_fp32_restatement_of_every_bmm_row_is_inside_its_bound(capsys):
    top = {}
    for c in cb.bmm_cases():
        a, b, cin = cb.bmm_inputs(c)
        want, e = cb.bmm_ref(a, b, cin, c["trans_a"], c["nan"], c["bias_row"])
        got = cb.bmm_restatement(a, b, cin, c["trans_a"], c["nan"], "pair" if c["kernel"] == "tiles" else "slab4")
        f = cb.ratio(got, want, e)
        assert f <= 1.0, (c["id"], f)
        if c["nan"]:
            assert np.isfinite(want).all() and (want == 0).any()
        top[c["kernel"]] = max(top.get(c["kernel"], 0.0), f)
    say(capsys, "bmm restatement worst error / bound: %s" % "  ".join("%s %.3f" % kv for kv in sorted(top.items())))


def vec_pair(c, x, mut=None):
    """-> ``(restatement, reference, bound)`` of a vector-chain row."""
    if c["op"] == "matvec":
        return (cb.matvec_restatement(x["A"], x["v"], x["base"], mut),) + cb.matvec_ref(x["A"], x["v"], x["base"])
    if c["op"] == "vecmat":
        return (cb.vecmat_restatement(x["v"], x["A"], x["base"], mut),) + cb.vecmat_ref(x["v"], x["A"], x["base"])
    if c["op"] == "ahv":
        return (cb.ahv_restatement(x["v"], x["attn"][0], x["grad"][0], x["base"], mut),) + cb.ahv_ref(x["v"], x["attn"][0], x["grad"][0], x["base"])
    y = dict(x, R_init=None, R_sq_init=None)
    return (cb.chain_row_restatement(c, y, x["rows"], mut),) + cb.chain_row_ref(c, y, x["rows"])


def test_an_fp32_restatement_of_every_vector_and_head_mean_row_is_inside_its_bound(capsys):
    top = {}
    for c in cb.vec_cases():
        got, want, e = vec_pair(c, cb.vec_inputs(c))
        f = cb.ratio(got, want, e)
        assert f <= 1.0, (c["id"], f)
        top[c["op"]] = max(top.get(c["op"], 0.0), f)
    for c in cb.avg_cases():
        a, g = cb.avg_inputs(c)
        want, e = cb.abar_ref(a, g)
        f = cb.ratio(cb.abar32(a, g), want, e)
        assert f <= 1.0, (c["id"], f)
        top["avg_heads " + c["dtype"]] = max(top.get("avg_heads " + c["dtype"], 0.0), f)
    say(capsys, "vector chain / head mean restatement worst error / bound: %s" % "  ".join("%s %.3f" % kv for kv in sorted(top.items())))


def mutant_figure(mutant, c):
    table = cb.MUTANTS[mutant][0]
    if table == "chain":
        x, ref = ref_of(c)
        wrong = cb.chain_restatement(c, x, mutant)
        return max(cb.ratio(wrong[n], ref[n], ref[e]) for n, e in outputs(c))
    if table == "bmm":
        a, b, cin = cb.bmm_inputs(c)
        want, e = cb.bmm_ref(a, b, cin, c["trans_a"], c["nan"], c["bias_row"])
        return cb.ratio(cb.bmm_restatement(a, b, cin, c["trans_a"], c["nan"], mut=mutant), want, e)
    got, want, e = vec_pair(c, cb.vec_inputs(c), mutant)
    return cb.ratio(got, want, e)


TABLES = {"chain": cb.chain_cases, "bmm": cb.bmm_cases, "vec": cb.vec_cases}


@pytest.mark.parametrize("mutant", sorted(cb.MUTANTS))
def test_every_mutant_is_outside_a_bound_by_2x(mutant, capsys):
    table, applies = cb.MUTANTS[mutant]
    rows = [c for c in TABLES[table]() if applies(c)]
    if table == "chain" and len(rows) > 40:
        rows = rows[::len(rows) // 40 + 1]                          # (a spread of the rows it applies to is enough)
    hit, best = 0, 0.0
    for c in rows:
        f = mutant_figure(mutant, c)
        hit += f >= 2.0
        best = max(best, min(f, 1e30))
    assert rows and hit > 0, "mutant %s survives in all of its %d rows (largest error / bound %.3g)" % (mutant, len(rows), best)
    say(capsys, "chain mutant %-40s at >= 2x a bound in %3d of %3d rows, largest error / bound %.3g" % (mutant, hit, len(rows), best))


def test_there_are_thirteen_mutants():
    assert len(cb.MUTANTS) >= 13


def test_the_padding_head_mutant_shows_in_the_inf_family_only():
    """On finite inputs ``x * 0`` added to a non-negative sum changes no bit: the defect is invisible outside the ``inf`` rows."""
    c = next(c for c in cb.chain_small_cases() if c["family"] == "plain" and c["H"] % 4 and c["L"] > 1 and c["N"] >= 40)
    x, _ = ref_of(c)
    assert np.array_equal(cb.chain_restatement(c, x)["R"], cb.chain_restatement(c, x, "padding_head_weighted_by_zero")["R"])


def test_the_stale_block_mutant_passes_the_old_tolerance_100x_outside_the_bound(capsys):
    found = []
    for c in cb.chain_small_cases():
        if c["family"] != "plain" or c["L"] < 2 or c["N"] <= 16 or c["dtype"] != "f32":
            continue
        x, ref = ref_of(c)
        wrong = cb.chain_restatement(c, x, "row_block_reads_updated_R")["R"]
        f = cb.ratio(wrong, ref["R"], ref["e_R"])
        if f >= 100.0 and cb.old_rule_passes(wrong, ref["R"]):
            found.append((c["id"], f, float(np.abs(wrong - ref["R"]).max())))
    assert found
    say(capsys, "stale 16-row block passes 1e-5 + 1e-5 |ref| and 1e-4 max |ref| at: %s"
        % "  ".join("%s (error / bound %.0f, max error %.2e)" % t for t in found[:4]))


def torch_chain(x, B, N):
    """The definition in torch on CPU float64: ``clamp(min=0)``, ``mean`` over heads, ``bmm``."""
    R = torch.eye(N, dtype=torch.float64).expand(B, N, N) if x["R_init"] is None else torch.from_numpy(x["R_init"]).double()
    for a, g in zip(x["attn"], x["grad"]):
        A = (torch.from_numpy(g).double() * torch.from_numpy(a).double()).clamp(min=0).mean(1)
        R = R + torch.bmm(A, R)
    return R.numpy()


def test_the_nan_and_inf_pattern_of_the_reference_is_torchs():
    n = {"nan": 0, "inf": 0}
    for c in cb.chain_cases():
        if c["family"] not in n or c["kernel"] == "rows":
            continue
        x, ref = ref_of(c)
        want = torch_chain(x, c["B"], c["N"])
        assert same_class(ref["R"], want), c["id"]
        assert np.isfinite(ref["R"][1:]).all(), c["id"]             # the poison stays in sample 0
        l, h, i, j = cb.poison_at(c)
        if c["family"] == "inf":
            assert np.isposinf(ref["R"][0, i]).all() and np.isfinite(np.delete(ref["R"][0], i, 0)).all(), c["id"]
            assert c["H"] % 4 != 0 and l == c["L"] - 1 and h == c["H"] - 1
        else:
            assert np.isnan(ref["R"][0, i]).all()
        n[c["family"]] += 1
    assert min(n.values()) >= 10
    for c in cb.chain_large_cases():                                # the rows kernel's I + A_bar start: the same pattern
        if c["family"] in n and c["kernel"] == "rows":
            x, ref = ref_of(c)
            assert same_class(ref["R"], torch_chain(x, c["B"], c["N"])), c["id"]
    for c in cb.bmm_cases():
        if c["nan"]:
            a, b, cin = cb.bmm_inputs(c)
            want = torch.bmm(torch.from_numpy(a).double().transpose(1, 2) if c["trans_a"] else torch.from_numpy(a).double(),
                             torch.from_numpy(b).double())
            want = torch.nan_to_num(want + (torch.from_numpy(cin).double() if cin is not None else 0), nan=0.0).numpy()
            assert np.allclose(cb.bmm_ref(a, b, cin, c["trans_a"], True)[0], want, rtol=1e-12, atol=0)


def test_the_tables_reach_every_route_and_edge():
    small, large = cb.chain_small_cases(), cb.chain_large_cases()
    cases = small + large
    assert len({c["id"] for c in cases}) == len(cases)
    f32 = [c for c in small if c["dtype"] == "f32"]
    assert {c["N"] for c in small} == set(cb.NS) and {c["H"] for c in small} >= set(cb.HS)
    assert {c["L"] for c in small} >= {0, 1, 2, 3, 7, 12} and {c["B"] for c in small} == {1, 2, 3}
    assert {c["algo"] for c in small} == {1, 4, 5} and {c["groups"] for c in small} == {1, 2, 3, 4}
    assert {c["pipe"] for c in small} == {0, 1, 2, 4} and {c["cols_c"] for c in small if c["kernel"] == "cols"} == {0, 1, 2, 3}
    for kernel in ("fused", "cols", "groups"):
        rows = [c for c in f32 if c["kernel"] == kernel]
        assert {-(-c["N"] // 16) for c in rows} == set(range(1, 9)) or kernel == "groups", kernel
        assert {c["family"] for c in rows} == set(cb.FAMILIES), (kernel, {c["family"] for c in rows})
        assert {c["shared"] for c in rows} == {True, False} and {c["init"] for c in rows} == {True, False}
        assert any(c["misaligned"] for c in rows), kernel
    fused = [c for c in f32 if c["kernel"] == "fused"]
    assert {c["cpl"] for c in fused} == {0, 1, 2, 4} and {c["cpl"] for c in fused if c["G"] > 1} >= {0, 1, 2, 4}
    # the suspected defect: the pipelined loop with padding heads, fed an infinity
    assert {c["cpl"] for c in fused if c["family"] == "inf" and c["H"] % (4 // max(c["cpl"], 1)) and c["cpl"]} == {1, 2}
    assert any(c["cpl"] == 4 and c["family"] == "inf" for c in fused)
    # the cols threshold at 40, the pipeline threshold at N * N >= 1600, the groups kernel's LDS limit between 112 and 113
    assert any(c["N"] == 39 and c["algo"] == 4 and c["kernel"] == "fused" for c in f32)
    assert any(c["N"] == 40 and c["algo"] == 4 and c["kernel"] == "cols" for c in f32)
    assert any(c["N"] == 39 and c["pipe"] and c["cpl"] == 0 for c in fused) or any(c["N"] == 39 for c in fused)
    assert any(c["N"] == 40 and c["cpl"] for c in fused)
    assert any(c["N"] == 112 and c["kernel"] == "groups" for c in f32) and any(c["N"] == 113 and c["G"] > 1 and c["algo"] == 4 and c["kernel"] == "fused" for c in f32)
    groups = [c for c in f32 if c["kernel"] == "groups"]
    assert {c["G"] for c in groups} == {2, 3, 4} and any(c["L"] % c["G"] for c in groups)
    assert {-(-c["L"] // c["G"]) for c in groups} >= {1, 2, 3, 4, 6}                  # more than three images per group
    assert any(c["L"] == 7 and c["kernel"] == "cols" for c in f32)                  # wraps the ring of 6
    assert any(c["causal_flag"] for c in groups) and any(c["causal_flag"] for c in f32 if c["kernel"] == "cols")
    assert any(c["family"] == "causal" and not c["causal_flag"] for c in f32)
    assert sum(c["plan"] for c in small) >= 4
    assert {c["dtype"] for c in small if c["kernel"] == "fused"} == set(cb.DTYPES)
    assert any(c["dtype"] != "f32" and c["G"] > 1 for c in small) and any(c["dtype"] != "f32" and c["N"] * c["N"] % 4 for c in small)
    # N > 128
    assert {c["N"] for c in large} >= set(cb.NS_LONG) | {636, 639} and {c["M"] for c in large} == {0, 36}
    assert {c["kernel"] for c in large} == {"split", "rows"}
    assert any(c["N"] == 636 and c["kernel"] == "rows" for c in large) and any(c["N"] == 639 and c["rows"] and c["kernel"] == "split" for c in large)
    assert any(c["kernel"] == "rows" and not c["init"] for c in large) and any(c["kernel"] == "rows" and c["init"] for c in large)
    assert {c["bmm"] for c in large if c["kernel"] == "split"} >= {"bmm32", "tiles"}
    assert {c["dtype"] for c in large if c["kernel"] == "rows"} == set(cb.DTYPES)
    assert {c["family"] for c in large} == set(cb.FAMILIES)
    assert any(c["N"] <= 128 and c["M"] for c in large)
    # bmm
    bmm = cb.bmm_cases()
    assert {c["kernel"] for c in bmm} == {"bmm32", "bmm64", "tiles"}
    assert {(c["M"], c["N"], c["K"]) for c in bmm} >= {(1, 1, 1), (5, 7, 3), (31, 33, 32), (64, 64, 33), (65, 95, 17), (96, 96, 32), (100, 130, 47)}
    for key in ("trans_a", "cin", "nan", "bias_row"):
        assert any(c[key] for c in bmm) and any(not c[key] for c in bmm), key
    assert any(c["tiles"] == 0 and cb.bmm_kernel(c["batch"], c["M"], c["N"], c["K"]) == "tiles" for c in bmm)
    assert any(c["kernel"] == "tiles" and c["cin"] for c in bmm) and any(c["kernel"] == "tiles" and c["nan"] for c in bmm)
    # vector chain and head mean
    vec = cb.vec_cases()
    for op in ("matvec", "vecmat"):
        assert {c["N"] for c in vec if c["op"] == op} == {1, 3, 4, 5, 31, 32, 33, 64, 65, 130, 260}, op
    ahv = [c for c in vec if c["op"] == "ahv"]
    assert {c["H"] for c in ahv} == {1, 3, 12} and {c["dtype"] for c in ahv} == set(cb.DTYPES) and {c["B"] for c in ahv} == {1, 3}
    assert {c["base"] for c in ahv} == {True, False} and {c["shared"] for c in ahv} == {True, False}
    assert {c["N"] for c in ahv} >= {1, 5, 33, 65, 130, 260}
    assert {c["N"] for c in vec if c["op"] == "row"} == {77, 130}
    avg = cb.avg_cases()
    assert {(c["Nq"], c["Nk"]) for c in avg} >= {(1, 5), (33, 2), (9, 13)} and {c["dtype"] for c in avg} == set(cb.DTYPES)
    assert any(c["dtype"] != "f32" and c["Nq"] * c["Nk"] % 2 for c in avg) and any(c["shared"] for c in avg)
