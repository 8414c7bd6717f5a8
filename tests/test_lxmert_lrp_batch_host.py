"""CPU: what the GPU suites of the batched LXMERT LRP methods rest on (``tests/test_gpu_lxmert_lrp_batch_ops.py``,
``tests/test_gpu_lxmert_lrp_batch.py``).

1. The stored seeds have the two properties ``tests/lxmert_lrp_batch_cases.py`` promises (conditions, checked here).
2. The float64 restatements ``attr64`` / ``minmax64`` reproduce what the REFERENCE's generator returned on the trios of
   ``tests/golden/lxmert_chain_lrp.npz`` (``tattr_*``, ``plrp_*``) to 1e-6.
3. The per-element error bounds of the op-level GPU suite are proved the way ``tests/test_chain_bounds_host.py`` does it: an fp32
   numpy emulation of the kernels' arithmetic stays inside them in forward, reversed and pairwise summation orders, and each of
   eight wrong implementations is at least TWICE a bound away from the restatement on some element of some case.  The mutants:

     clamp after the head sum                 A_bar = max(0, mean_h(G_h C_h))
     divide by H over the padded extent       A_bar is formed on the whole padded block and the chain runs on it (the 1e6 products of
                                              the padding reach the live block from the second step on)
     mean taken over the padded extent        R_ti keeps the head mean of the padded query rows
     chain order reversed                     the tables are walked from their last entry
     A_bar . R without the + R
     R_tt[0, 0] not zeroed
     R_ti as a product                        R_ti = R_tt^T (A_bar(cross) R_ii), the line the reference has commented out (:450)
     min / max over the padded extent         the extremes of the min-max step include the padding

4. The premise of the whole route: with the stand-in capture op and the oracle's attention core, a padded ragged batch leaves every
   attention module's LRP cam equal to the item's own pass on the live block and EXACTLY zero at padded language rows and columns."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lxmert_lrp_batch_cases as cases  # noqa: E402
from oracle import lrp_torch as lrp_oracle  # noqa: E402
from test_bert_lrp_host import cpu_body, lxmert_cams, lxmert_from_golden, within_reference_noise  # noqa: E402,F401

F32 = np.float32


# ---------------------------------------------------------------------------------------- 1. the seeds
@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_seeds_have_both_properties(case):
    c = cases.make_case(*case, cases.SEEDS[case])
    neg, pos = cases.clamp_shares(c)
    assert neg >= cases.MIN_SHARE and pos >= cases.MIN_SHARE, (neg, pos)
    assert cases.min_span(c) >= cases.MIN_SPAN
    nan = cases.make_case(*case, cases.SEEDS[case], pad=np.nan)        # the live values do not depend on the padding
    for (c0, g0), (c1, g1) in zip(c["text"] + c["img"] + [c["cross"]], nan["text"] + nan["img"] + [nan["cross"]]):
        keep = ~np.isnan(c1)
        assert np.array_equal(c0[keep], c1[keep]) and np.array_equal(g0[keep], g1[keep]) and bool((c0[~keep] == cases.PAD).all())


def test_case_table_covers_the_tables_and_the_evaluator_shape():
    assert len(cases.CASES) == len(cases.SHAPES) * len(cases.HEADS) * len(cases.BATCHES) * len(cases.KINDS) * 2 + 1
    assert cases.CASES[-1] == (20, 36, 12, 5, "ragged", 14, 9)
    assert {(c[5], c[6]) for c in cases.CASES[:-1]} == {(1, 1), (5, 4)}


# ---------------------------------------------------------------------------------------- 2. the restatements on the golden trios
def golden_tables(g):
    """``(text, img, cross)`` pair tables of ``lxmert_chain_lrp.npz`` in the order the C entry takes them; every slab ``[1, H, q, k]``."""
    def pairs(prefix, sl=slice(None)):
        return list(zip(g[prefix + "_cam"][sl], g[prefix + "_grad"][sl]))
    text = pairs("lang") + pairs("x_lang_self")
    img = pairs("vis") + pairs("x_img_self", slice(0, -1))
    return text, img, (g["x_lang_cross_cam"][-1], g["x_lang_cross_grad"][-1])


def test_restatements_reproduce_the_reference_on_the_golden_trios(golden):
    g = golden("lxmert_chain_lrp")
    text, img, cross = golden_tables(g)
    T, I = cross[0].shape[-2:]
    R_tt, R_ti, _ = cases.attr64(text, img, cross, [T])
    np.testing.assert_allclose(R_tt[0], g["tattr_R_t_t"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(R_ti[0], g["tattr_R_t_i"], rtol=0, atol=1e-6)
    p_tt = cases.minmax64(g["x_lang_self_cam"][-1], [T], [T], zero_cls=True)
    p_ti = cases.minmax64(cross[0], [T], [I])
    np.testing.assert_allclose(p_tt[0], g["plrp_R_t_t"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(p_ti[0], g["plrp_R_t_i"], rtol=0, atol=1e-6)


def test_minmax_restatement_on_the_degenerate_rows():
    for name, cam, q_len, k_len in cases.degenerate_minmax():
        out = cases.minmax64(cam, q_len, k_len)
        q, k = int(q_len[1]), int(k_len[1])
        assert np.isnan(out[1, :q, :k]).all(), name
        assert not np.isnan(out[0]).any() and not out[1, q:].any() and not out[1, :, k:].any(), name
        assert cases.minmax64(cam, q_len, k_len, zero_cls=True)[1, 0, 0] == 0.0, name


# ---------------------------------------------------------------------------------------- 3. the bounds: fp32 emulation, mutants
def _sum32(terms, order):
    terms = list(terms)
    if order == "reversed":
        terms = terms[::-1]
    if order == "pairwise":
        while len(terms) > 1:
            terms = [(terms[i] + terms[i + 1]).astype(F32) if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        return terms[0]
    acc = terms[0]
    for x in terms[1:]:
        acc = (acc + x).astype(F32)
    return acc


def _abar32(C, G, order):
    return (_sum32([np.maximum((G[h] * C[h]).astype(F32), F32(0)) for h in range(C.shape[0])], order) / F32(C.shape[0])).astype(F32)


def _step32(A, R, order):
    prod = _sum32([(A[:, k, None] * R[None, k, :]).astype(F32) for k in range(A.shape[1])], order)
    return (R + prod).astype(F32)


def attr32(c, order):
    B, T, I = c["B"], c["T"], c["I"]
    R_tt, R_ti, R_ii = np.zeros((B, T, T), F32), np.zeros((B, T, I), F32), np.zeros((B, I, I), F32)
    for b in range(B):
        t = int(c["t"][b])
        r, ri = np.eye(t, dtype=F32), np.eye(I, dtype=F32)
        for cm, g in c["text"]:
            r = _step32(_abar32(cm[b, :, :t, :t], g[b, :, :t, :t], order), r, order)
        for cm, g in c["img"]:
            ri = _step32(_abar32(cm[b], g[b], order), ri, order)
        R_tt[b, :t, :t], R_ii[b] = r, ri
        R_tt[b, 0, 0] = 0
        R_ti[b, :t] = _abar32(c["cross"][0][b, :, :t], c["cross"][1][b, :, :t], order)
    return R_tt, R_ti, R_ii


def minmax32(cam, q_len, k_len, order):
    B, H, Nq, Nk = cam.shape
    out = np.zeros((B, Nq, Nk), F32)
    for b in range(B):
        q, k = int(q_len[b]), int(k_len[b])
        m = (_sum32([cam[b, h, :q, :k] for h in range(H)], order) / F32(H)).astype(F32)
        with np.errstate(invalid="ignore"):                              # a one-entry block: 0 / 0
            out[b, :q, :k] = ((m - m.min()).astype(F32) / F32(m.max() - m.min())).astype(F32)
    return out


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_fp32_emulation_stays_inside_the_bounds_in_three_orders(case):
    c = cases.make_case(*case, cases.SEEDS[case])
    ref = cases.attr64(c["text"], c["img"], c["cross"], c["t"])
    bounds = cases.attr_bounds(c, ref)
    for order in ("forward", "reversed", "pairwise"):
        for name, got, want, bound in zip(("R_tt", "R_ti", "R_ii"), attr32(c, order), ref, bounds):
            assert bool((np.abs(got.astype(np.float64) - want) <= bound).all()), (order, name)
            assert not got[want == 0].any(), (order, name)
        for name, cam, _rq, q, _rk, k, _cls in cases.minmax_maps(c):
            want = cases.minmax64(cam, q, k)
            ok = ~np.isnan(want)                                         # (a one-entry block is NaN: no bound there)
            bound = cases.minmax_bound(cam, q, k, want)
            got = minmax32(cam, q, k, order).astype(np.float64)
            assert bool((np.abs(got - want)[ok] <= bound[ok]).all()), (order, name)


def _abar64(C, G, clamp_after_sum=False):
    prod = G.astype(np.float64) * C.astype(np.float64)
    return np.maximum(prod.mean(axis=0), 0.0) if clamp_after_sum else np.maximum(prod, 0.0).mean(axis=0)


def attr_mutant(c, mutant):
    """``attr64`` with ONE thing wrong (module docstring)."""
    B, T, I = c["B"], c["T"], c["I"]
    R_tt, R_ti, R_ii = np.zeros((B, T, T)), np.zeros((B, T, I)), np.zeros((B, I, I))
    cas = mutant == "clamp after the head sum"
    for b in range(B):
        t = int(c["t"][b])
        n = T if mutant == "divide by H over the padded extent" else t
        r, ri = np.eye(n), np.eye(I)
        text, img = (c["text"][::-1], c["img"][::-1]) if mutant == "chain order reversed" else (c["text"], c["img"])
        for cm, g in text:
            prod = _abar64(cm[b, :, :n, :n], g[b, :, :n, :n], cas) @ r
            r = prod if mutant == "A_bar . R without the + R" else r + prod
        for cm, g in img:
            prod = _abar64(cm[b], g[b], cas) @ ri
            ri = prod if mutant == "A_bar . R without the + R" else ri + prod
        rows = T if mutant == "mean taken over the padded extent" else t
        a_cross = _abar64(c["cross"][0][b, :, :rows], c["cross"][1][b, :, :rows], cas)
        R_ti[b, :rows] = r[:t, :t].T @ (a_cross @ ri) if mutant == "R_ti as a product" else a_cross
        R_tt[b, :t, :t], R_ii[b] = r[:t, :t], ri
        if mutant != "R_tt[0, 0] not zeroed":
            R_tt[b, 0, 0] = 0.0
    return R_tt, R_ti, R_ii


ATTR_MUTANTS = ("clamp after the head sum", "divide by H over the padded extent", "mean taken over the padded extent",
                "chain order reversed", "A_bar . R without the + R", "R_tt[0, 0] not zeroed", "R_ti as a product")


@pytest.fixture(scope="module")
def worst_mutant_ratios():
    """{mutant: the largest |mutant - float64| / bound over every element of every case} (a zero bound with a difference: inf)."""
    worst = {m: 0.0 for m in ATTR_MUTANTS + ("min / max over the padded extent",)}

    def ratio(diff, bound):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(diff > 0, diff / bound, 0.0)
        return float(np.nanmax(r))

    for case in cases.CASES:
        c = cases.make_case(*case, cases.SEEDS[case])
        ref = cases.attr64(c["text"], c["img"], c["cross"], c["t"])
        bounds = cases.attr_bounds(c, ref)
        for m in ATTR_MUTANTS:
            for got, want, bound in zip(attr_mutant(c, m), ref, bounds):
                worst[m] = max(worst[m], ratio(np.abs(got - want), bound))
        for _name, cam, _rq, q, _rk, k, _cls in cases.minmax_maps(c):
            want = cases.minmax64(cam, q, k)
            full_q, full_k = np.full(c["B"], cam.shape[2]), np.full(c["B"], cam.shape[3])
            padded = cases.minmax64(cam, full_q, full_k)                 # the extremes of the whole padded block
            for b in range(c["B"]):
                padded[b, int(q[b]):], padded[b, :, int(k[b]):] = 0.0, 0.0
            ok = ~np.isnan(want)
            bound = cases.minmax_bound(cam, q, k, want)
            worst["min / max over the padded extent"] = max(worst["min / max over the padded extent"],
                                                            ratio(np.abs(padded - want)[ok], bound[ok]))
    return worst


@pytest.mark.parametrize("mutant", ATTR_MUTANTS + ("min / max over the padded extent",))
def test_each_mutant_is_at_least_twice_a_bound_on_some_case(worst_mutant_ratios, mutant):
    assert worst_mutant_ratios[mutant] >= 2.0, "%s: at most %.3g x a bound on every case" % (mutant, worst_mutant_ratios[mutant])


# ---------------------------------------------------------------------------------------- 4. the premise: a padded batch is sound
PADDED_T = 12
TRUNCATIONS = (9, 6, 2)         # the golden item, then two truncations of it with other visual features
ANSWERS = (None, 3, 5)          # item 0: the golden answer


def ragged_batch(inputs, index0):
    """``(batch, items, index)``: the three-item batch padded to ``PADDED_T`` and the same items alone, unpadded."""
    gen = torch.Generator().manual_seed(11)
    items = []
    for n, t in enumerate(TRUNCATIONS):
        it = {k: v.clone() for k, v in inputs.items()}
        for k in ("input_ids", "attention_mask", "token_type_ids"):
            it[k] = it[k][:, :t].clone()
        if n:
            it["visual_feats"] = torch.randn(inputs["visual_feats"].shape, generator=gen)
        items.append(it)
    batch = {k: torch.cat([it[k] for it in items]) for k in ("visual_feats", "visual_pos")}
    for k in ("input_ids", "attention_mask", "token_type_ids"):
        batch[k] = torch.zeros(len(items), PADDED_T, dtype=inputs[k].dtype)
        for b, it in enumerate(items):
            batch[k][b, :it[k].shape[1]] = it[k][0]
    return batch, items, [index0 if a is None else a for a in ANSWERS]


def live_block(name, cam, b, t):
    """Sample b's live block of a batch cam ``[B, H, Nq, Nk]`` -> ``[1, H, q, k]`` (language extents cut to ``t``)."""
    rows = t if ("lang" in name or name[0] == "l" or name.endswith("_cross")) else cam.shape[2]
    cols = t if ("lang" in name or name[0] == "l" or name.endswith("_cross_copy")) else cam.shape[3]
    return cam[b:b + 1, :, :rows, :cols], rows, cols


def _relprop_cams(model, inputs, index):
    out = model(**inputs).question_answering_score
    one_hot = torch.zeros_like(out).scatter_(1, torch.as_tensor(index).reshape(-1, 1), 1.0)
    model.zero_grad()
    torch.sum(one_hot * out).backward()
    model.relprop(one_hot.clone(), alpha=1, core=lrp_oracle.core)
    return {name: m.get_attn_cam().detach().clone() for name, m in lxmert_cams(model).items()}


def test_padded_ragged_batch_gives_the_per_item_cams_on_the_live_block(golden, cpu_body):
    gm, g = golden("lxmert_model"), golden("lxmert_model_lrp")
    model, inputs = lxmert_from_golden(gm)
    batch, items, index = ragged_batch(inputs, int(g["index"]))
    alone = [_relprop_cams(model, it, [index[b]]) for b, it in enumerate(items)]
    both = _relprop_cams(model, batch, index)
    # items 1 and 2 have no float64 pass of their own and are not the golden item: their yardstick is the reference's WORST relative
    # fp32-to-fp64 distance over the golden item's cams (what the pass is uncertain by, module docstring of test_bert_lrp_host.py),
    # with the factor and floor of within_reference_noise
    noise = 0.0
    for name in both:
        r64 = np.asarray(g["f64__cam__" + name], dtype=np.float64)
        top = float(np.abs(r64).max())
        if top > 0:
            noise = max(noise, float(np.abs(np.asarray(g["cam__" + name], dtype=np.float64) - r64).max()) / top)
    for name, cam in both.items():
        key = "cam__" + name
        for b, t in enumerate(TRUNCATIONS):
            blk, rows, cols = live_block(name, cam, b, t)
            assert blk.shape == alone[b][name].shape, (name, b)
            if b == 0:
                within_reference_noise(blk, g, key, what="%s of item 0 in the padded batch" % name)
            want = alone[b][name]
            scale = float(want.abs().max())
            assert float((blk - want).abs().max()) <= 4.0 * noise * scale + 1e-5 * scale, (name, b)
            assert not bool(cam[b, :, rows:].any()) and not bool(cam[b, :, :, cols:].any()), "%s: item %d is not zero in its padding" % (name, b)
