"""-m gpu: the kernels that apply the bi-modal rules -- ``lxmert_schedule_v2_kernel`` (one launch on all three workgroups-per-sample
regimes, and the two-launch mode), the four kernels behind ``mmx_detr_decoder_rows`` and the per-rule entries on ``row_normalise_kernel``
(modes 0 / 1 / 2), ``copy_scrub_kernel`` and ``bmm_f32_kernel`` -- against the float64 references and the counted per-element bounds of
``tests/rules_bounds.py`` (proved on the CPU by ``tests/test_rules_bounds_host.py``).

Every element of every output is checked: error <= its bound, NaN exactly where the reference has NaN; entries beyond a sample's
``text_len`` are exactly zero; the diag word lies in the reference's interval and is NaN exactly when the reference's is; in the ``nan``
rows every sample but the poisoned one keeps the bits of the clean run; a second call gives the same bits (scratch, tickets and flags
are reset by the entry).  The two-launch mode of the schedule must give the bits of the one-launch mode (phase 1 sums the same heads in
the same order into the same scratch, phase 2 is the same code), and ``MMX_BM_SPLIT`` is put back to ``"0"`` explicitly -- the entry keeps
the last value it read.  Every input slab is carved out of a NaN-filled buffer with NaN margins on both sides (an over-read value that
reaches a result shows).  The worst error / bound per kernel, route and family is recorded (``parity.note``) and printed."""
import os

import numpy as np
import pytest
import torch

import rules_bounds as rb
from parity import note
from test_gpu_chain_bounds import bump, carve, chunks, same_bits
from test_gpu_rowwise_forward import host

pytestmark = pytest.mark.gpu

NAMES = ("R_tt", "R_ti", "R_ii", "R_it")


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    return _ops


def record(what, top):
    print("\nrules %s worst error / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(top.items()))))
    for k, v in top.items():
        note("rules_bounds %s %s" % (what, k), v, bound=1.0)


def nan_map(a):
    return np.isnan(host(a))


# ---------------------------------------------------------------------------------------------------------------------
# the LXMERT schedule
# ---------------------------------------------------------------------------------------------------------------------
def sched_on_device(x):
    d = {g: [(carve(a), carve(gr)) for a, gr in x[g]] for g in rb.GROUPS}
    d["text_len"] = None if x["text_len"] is None else torch.from_numpy(x["text_len"]).cuda()
    return d


def run_schedule(ops, c, d):
    """-> ``([R_tt, R_ti, R_ii, R_it], diag word or None)``."""
    out = ops.lxmert_schedule(*[d[g] for g in rb.GROUPS], apply_normalization=c["normalize"], apply_self_in_rule_10=c["self10"],
                              check_diag="defer", text_len=d["text_len"])
    torch.cuda.synchronize()
    return [m.clone() for m in out[:4]], (None if out[4] is None else out[4].clone())


def judge_schedule(c, x, ref, got, word, bad, what=""):
    figs = {n: rb.judge(host(g), ref[n], ref["e_" + n[2:]]) for n, g in zip(NAMES, got)}
    for n, f in figs.items():
        if not f <= 1.0:
            bad.append((c["id"] + what, n, f, "NaN at %d elements (reference %d)" % (nan_map(got[NAMES.index(n)]).sum(), np.isnan(ref[n]).sum())))
    if word is not None and not rb.diag_ok(float(word), ref["diag"]):
        bad.append((c["id"] + what, "diag word", float(word), ref["diag"]))
    if x["text_len"] is not None:
        for b in range(c["B"]):
            t = int(np.clip(x["text_len"][b], 1, c["T"]))
            beyond = [got[0][b, t:], got[0][b, :, t:], got[1][b, t:], got[3][b, :, t:]]
            if any(bool((m != 0).any()) for m in beyond):
                bad.append((c["id"] + what, "entries beyond text_len of sample %d" % b))
    return figs


@pytest.mark.parametrize("rows", chunks(rb.schedule_cases(), lambda c: c["route"]))
def test_the_schedule_meets_the_float64_bound(ops, rows):
    top, bad = {}, []
    for c in rows:
        x = rb.schedule_inputs(c)
        ref = rb.schedule_ref(c, x)
        d = sched_on_device(x)
        got, word = run_schedule(ops, c, d)
        # ops.lxmert_schedule asks the kernel for the word only with both flags on (without rule 10's self terms the normalised
        # matrices reach no output and the wrapper hands no word over); the per-rule entry publishes it in that branch too, and
        # test_mm_attention_rules_diag_word_keeps_a_positive_nan holds it there.  Where a word comes back it is judged below.
        assert (word is not None) == (c["normalize"] and c["self10"])
        figs = judge_schedule(c, x, ref, got, word, bad)
        print("%s W %d: %s  diag %s in %s" % (c["id"], c["W"], "  ".join("%s %.4g" % kv for kv in figs.items()),
                                             None if word is None else float(word), None if ref["diag"] is None else ref["diag"][1:]))
        for n, f in figs.items():
            bump(top, "%s %s" % (c["family"], n), f)
        got2, word2 = run_schedule(ops, c, d)
        if not (all(same_bits(a, b) for a, b in zip(got, got2)) and (word is None or same_bits(word, word2))):
            bad.append((c["id"], "second call"))
        if c["family"] == "nan":
            clean, _ = run_schedule(ops, c, sched_on_device(rb.schedule_inputs(c, poisoned=False)))
            if not all(same_bits(a[1:], b[1:]) for a, b in zip(got, clean)):
                bad.append((c["id"], "the poison left sample 0"))
    record("schedule " + rows[0]["route"], top)
    assert not bad, bad


def test_the_two_launch_mode_gives_the_bits_of_the_one_launch_mode(ops):
    """Once per family.  ``MMX_BM_SPLIT`` is read per call and the last value read stays: it is set back to ``"0"`` explicitly and a
    one-launch call afterwards must give the bits of the one before."""
    picked = {}
    for c in rb.schedule_cases():
        if c["family"] not in picked and c["route"] != "W=nblk":     # (with W = nblk phase 1 has the two-launch grid already)
            picked[c["family"]] = c
    assert set(picked) == set(rb.FAMILIES)
    top, bad = {}, []
    os.environ["MMX_BM_SPLIT"] = "0"
    try:
        for fam, c in sorted(picked.items()):
            x = rb.schedule_inputs(c)
            ref = rb.schedule_ref(c, x)
            d = sched_on_device(x)
            one, word1 = run_schedule(ops, c, d)
            os.environ["MMX_BM_SPLIT"] = "1"
            two, word2 = run_schedule(ops, c, d)
            os.environ["MMX_BM_SPLIT"] = "0"
            back, word3 = run_schedule(ops, c, d)
            figs = judge_schedule(c, x, ref, two, word2, bad, " two-launch")
            print("%s two-launch: %s" % (c["id"], "  ".join("%s %.4g" % kv for kv in figs.items())))
            for n, f in figs.items():
                bump(top, "%s %s" % (fam, n), f)
            if not (all(same_bits(a, b) for a, b in zip(one, two)) and (word1 is None or same_bits(word1, word2))):
                bad.append((c["id"], "two-launch != one-launch bits"))
            if not (all(same_bits(a, b) for a, b in zip(one, back)) and (word1 is None or same_bits(word1, word3))):
                bad.append((c["id"], "one-launch after MMX_BM_SPLIT=0"))
    finally:
        os.environ["MMX_BM_SPLIT"] = "0"
        c = picked["plain"]
        run_schedule(ops, c, sched_on_device(rb.schedule_inputs(c)))      # the entry has read "0" again, whatever happened above
    record("schedule two-launch", top)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# DETR decoder rows
# ---------------------------------------------------------------------------------------------------------------------
def detr_on_device(c, x):
    flat = lambda t: carve(t.reshape((-1,) + t.shape[2:]))                         # noqa: E731
    return {"self": [(flat(a), flat(g)) for a, g in x["self"]], "cross": [(flat(a), flat(g)) for a, g in x["cross"]],
            "targets": torch.from_numpy(x["targets"]).cuda()}


def run_detr(ops, c, d):
    s, word = ops.detr_decoder_rows(d["self"], d["cross"], d["targets"], shared_attn=c["shared"])
    torch.cuda.synchronize()
    return s.clone(), word.clone()


@pytest.mark.parametrize("rows", chunks(rb.detr_cases(), lambda c: "detr"))
def test_the_detr_decoder_rows_meet_the_float64_bound(ops, rows):
    top, bad = {}, []
    for c in rows:
        x = rb.detr_inputs(c)
        ref = rb.detr_ref(c, x)
        d = detr_on_device(c, x)
        s, word = run_detr(ops, c, d)
        f = rb.judge(host(s), ref["s"], ref["e_s"])
        print("%s: s %.4g  diag %r in %s" % (c["id"], f, float(word), ref["diag"][1:]))
        if not f <= 1.0:
            bad.append((c["id"], f, "NaN at %d elements (reference %d)" % (nan_map(s).sum(), np.isnan(ref["s"]).sum())))
        if not rb.diag_ok(float(word), ref["diag"]):
            bad.append((c["id"], "diag word", float(word), ref["diag"]))
        s2, word2 = run_detr(ops, c, d)
        if not (same_bits(s, s2) and same_bits(word, word2)):
            bad.append((c["id"], "second call"))
        if c["family"] in ("nan_self", "nan_cross"):
            k = rb.detr_poison(c)[0]
            clean, _ = run_detr(ops, c, detr_on_device(c, rb.detr_inputs(c, poisoned=False)))
            keep = [i for i in range(c["K"]) if i != k]
            if not same_bits(s[keep], clean[keep]):
                bad.append((c["id"], "the poison left sample %d" % k))
        bump(top, c["family"], f)
    record("detr rows", top)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the per-rule entries
# ---------------------------------------------------------------------------------------------------------------------
def run_rule(ops, c, x):
    """-> ``(dict of outputs, diag word or None)``."""
    if c["op"] == "residual":
        out, word = ops.handle_residual(carve(x["R"]), check_diag="defer")
        torch.cuda.synchronize()
        return {"out": out.clone()}, word.clone()
    if c["op"] == "rollout":
        out = ops.rollout_chain([carve(m) for m in x["layers"]], c["normalize"])
        torch.cuda.synchronize()
        return {"out": out.clone()}, None
    out = ops.mm_attention_rules(carve(x["R_ss"]), carve(x["R_qq"]), carve(x["cam"]), R_qs=carve(x["R_qs"]),
                                 apply_normalization=c["normalize"], apply_self_in_rule_10=c["self10"], nan_to_zero=c["nan_to_zero"])
    torch.cuda.synchronize()
    return ({"sq": out[0].clone(), "ss": out[1].clone()} if c["rule11"] else {"sq": out.clone()}), None


@pytest.mark.parametrize("rows", chunks(rb.rule_cases(), lambda c: c["op"]))
def test_the_per_rule_entries_meet_the_float64_bound(ops, rows):
    top, bad = {}, []
    for c in rows:
        x = rb.rule_inputs(c)
        ref = rb.rule_ref(c, x)
        got, word = run_rule(ops, c, x)
        figs = {n: rb.judge(host(v).reshape(ref[n][0].shape), *ref[n]) for n, v in got.items()}
        print("%s%s%s%s%s: %s" % (c["id"], "" if c["normalize"] else " no eq. 8-9", "" if c["self10"] else " no self terms",
                                  " rule 11" if c["rule11"] else "", " nan_to_zero" if c["nan_to_zero"] else "",
                                  "  ".join("%s %.4g" % kv for kv in figs.items())))
        for n, f in figs.items():
            if not f <= 1.0:
                bad.append((c["id"], n, f))
            bump(top, n, f)
        if word is not None and not rb.diag_ok(float(word), ref["diag"]):
            bad.append((c["id"], "diag word", float(word), ref["diag"]))
        got2, word2 = run_rule(ops, c, x)
        if not (all(same_bits(got[n], got2[n]) for n in got) and (word is None or same_bits(word, word2))):
            bad.append((c["id"], "second call"))
    record("entry " + rows[0]["op"], top)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the diag word keeps a NaN, whatever its sign bit and whenever it arrives
# ---------------------------------------------------------------------------------------------------------------------
def positive_nan(t):
    """``float("nan")``: 0x7fc00000, the sign bit clear -- what most arithmetic NaNs are."""
    v = torch.tensor(float("nan"), dtype=torch.float32)
    assert int(v.view(torch.int32)) == 0x7fc00000
    return v.to(t.device)


@pytest.mark.parametrize("batch,N,row", [(1, 5, 2), (3, 64, 33), (2, 130, 64), (3, 130, 1), (3, 130, 128)])
def test_handle_residual_diag_word_keeps_a_positive_nan(ops, batch, N, row):
    """``row_normalise_kernel`` publishes ``min diag(R - I)`` with one atomic per row: rows with a positive excess arrive before AND after
    the NaN row, and the word must end as NaN (the reference's ``assert diag.min() >= 0`` fails on a NaN diagonal)."""
    rng = np.random.default_rng(N * 10 + row)
    R = torch.from_numpy(rb._relevancy(rng, batch, N)).cuda()
    R[batch // 2, row, row] = positive_nan(R)
    for _ in range(3):                                              # (three launches: three arrival orders, no more)
        out, word = ops.handle_residual(R, check_diag="defer")
        assert torch.isnan(word).all(), float(word)
    with pytest.raises(AssertionError):
        ops.handle_residual(R, check_diag=True)
    clean = torch.from_numpy(rb._relevancy(rng, batch, N)).cuda()
    assert float(ops.handle_residual(clean, check_diag="defer")[1]) >= 0


@pytest.mark.parametrize("where", ["R_ss", "R_qq"])
@pytest.mark.parametrize("Ns,Nq", [(5, 7), (65, 130), (130, 64)])
def test_mm_attention_rules_diag_word_keeps_a_positive_nan(ops, where, Ns, Nq):
    c = rb._rule(77, "mm", Ns=Ns, Nq=Nq, rule11=True)
    x = rb.rule_inputs(c)
    t = {k: torch.from_numpy(v).cuda() for k, v in x.items()}
    ops.mm_attention_rules(t["R_ss"], t["R_qq"], t["cam"], R_qs=t["R_qs"])          # clean: no assert
    n = Ns if where == "R_ss" else Nq
    t[where][n // 2, n // 2] = positive_nan(t[where])
    for self10 in (True, False):                                     # the reference asserts before it looks at apply_self_in_rule_10
        with pytest.raises(AssertionError):
            ops.mm_attention_rules(t["R_ss"], t["R_qq"], t["cam"], R_qs=t["R_qs"], apply_self_in_rule_10=self10)
    ops.mm_attention_rules(t["R_ss"], t["R_qq"], t["cam"], R_qs=t["R_qs"], apply_normalization=False)   # no eq. 8-9: no assert


def test_schedule_and_detr_diag_words_keep_a_positive_nan(ops):
    c = rb._sched(78, 3, 5, 17, 7, 2, 2, 2)
    x = rb.schedule_inputs(c)
    x["lang"][0][1][1, 0, 8, 8] = np.nan                             # a middle row of sample 1: diag(R_tt) of that row is NaN
    d = sched_on_device(x)
    got, word = run_schedule(ops, c, d)
    assert torch.isnan(word).all() and not torch.isnan(got[0][0]).any() and not torch.isnan(got[0][2]).any()
    with pytest.raises(AssertionError):
        ops.lxmert_schedule(*[d[g] for g in rb.GROUPS], check_diag=True)
    c = rb._detr(79, 3, 3, 33, 65, 3)
    x = rb.detr_inputs(c)
    x["self"][1][1][1, 0, 16, 16] = np.nan
    s, word = run_detr(ops, c, detr_on_device(c, x))
    assert torch.isnan(word).all() and not (float(word) >= 0)
    assert torch.isfinite(s[0]).all() and torch.isfinite(s[2]).all()
