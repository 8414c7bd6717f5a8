"""Shared by the suites of the batched LXMERT LRP methods: the case table, the slabs of a case and float64 restatements of
transformer attribution (lxmert/lxmert/src/ExplanationGenerator.py:373-460 with ``avg_heads`` :18-23) and of the per-map step of
partial LRP (:489-505) for a padded batch, each sample on its LIVE block only.

A case is ``(T, I, H, B, kind, n_text, n_img)``: the tables of ``tests/lxmert_baselines_cases.py`` times two table lengths, plus the
evaluator's shape.  LRP cams are not probabilities: the cam slabs are signed ``randn * 1e-2``, the gradients ``randn``, and outside each
live block BOTH slabs hold ``pad`` (1e3: their product, 1e6, would pass the clamp; the GPU suite also runs ``pad = NaN``).

``SEEDS`` holds, per case, a seed (``find_seed``, first fit from 0) for which
  * rule 5's per-head products ``G_h * C_h`` have at least 10 % clamped and at least 10 % positive entries inside the live blocks, and
  * ``max m - min m >= 1e-2 * max|m|`` on every live block of more than one entry of the three head-mean maps the min-max entry is
    checked on,
so that neither the clamp nor the min-max bound makes a comparison vacuous (tests/test_lxmert_lrp_batch_host.py asserts both)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lxmert_baselines_cases import BATCHES, HEADS, KINDS, SHAPES, image_lengths, lengths  # noqa: E402,F401

TABLES = ((1, 1), (5, 4))
EVALUATOR_CASE = (20, 36, 12, 5, "ragged", 14, 9)
PAD = 1e3
MIN_SHARE = 0.10
MIN_SPAN = 1e-2
U = 2.0 ** -24

CASES = [(T, I, H, B, kind, nt, ni) for (T, I) in SHAPES for H in HEADS for B in BATCHES for kind in KINDS for (nt, ni) in TABLES]
CASES.append(EVALUATOR_CASE)


def case_id(c):
    return "T%d_I%d_H%d_B%d_%s_nt%d_ni%d" % c


def _pair(rng, B, H, Nq, Nk, q_live, k_live, pad):
    c = (rng.standard_normal((B, H, Nq, Nk)) * 1e-2).astype(np.float32)
    g = rng.standard_normal((B, H, Nq, Nk)).astype(np.float32)
    for b in range(B):
        for s in (c, g):
            s[b, :, int(q_live[b]):, :] = pad
            s[b, :, :, int(k_live[b]):] = pad
    return c, g


def make_case(T, I, H, B, kind, n_text, n_img, seed, pad=PAD):
    """The slabs of a case (numpy, fp32) and its lengths: ``text`` / ``img`` lists of ``(cam, grad)``, ``cross`` one pair, and
    ``cross_k`` a cross cam under ragged key lengths ``k_len`` as well (the min-max entry takes the two lengths independently).  The
    live values do not depend on ``pad``."""
    rng = np.random.default_rng(seed)
    raw, t = lengths(T, B, kind)
    full_i = np.full(B, I, dtype=np.int32)
    k_len = image_lengths(I, B)
    case = dict(T=T, I=I, H=H, B=B, kind=kind, raw=raw, t=t, k_len=k_len, full_i=full_i)
    case["cross"] = _pair(rng, B, H, T, I, t, full_i, pad)
    case["cross_k"] = _pair(rng, B, H, T, I, t, k_len, pad)[0]
    case["text"] = [_pair(rng, B, H, T, T, t, t, pad) for _ in range(n_text)]
    case["img"] = [_pair(rng, B, H, I, I, full_i, full_i, pad) for _ in range(n_img)]
    return case


# ---------------------------------------------------------------------------------------- float64 restatements
def abar64(C, G):
    """``avg_heads`` (:18-23) of one sample's live block ``[H, q, k]``: the clamp per head, then the head mean."""
    return np.maximum(G.astype(np.float64) * C.astype(np.float64), 0.0).mean(axis=0)


def attr64(text, img, cross, t_len):
    """``(R_tt [B, T, T], R_ti [B, T, I], R_ii [B, I, I])`` of :373-460, sample b on its leading ``t_len[b]`` tokens."""
    B, H, T, I = cross[0].shape
    R_tt, R_ti, R_ii = np.zeros((B, T, T)), np.zeros((B, T, I)), np.zeros((B, I, I))
    for b in range(B):
        t = int(t_len[b])
        r = np.eye(t)                                                   # :383
        for c, g in text:
            r = r + abar64(c[b, :, :t, :t], g[b, :, :t, :t]) @ r        # :411, :435, :457
        ri = np.eye(I)                                                  # :385
        for c, g in img:
            ri = ri + abar64(c[b], g[b]) @ ri                           # :420, :441
        R_tt[b, :t, :t] = r
        R_tt[b, 0, 0] = 0.0                                             # :459
        R_ii[b] = ri
        R_ti[b, :t] = abar64(cross[0][b, :, :t], cross[1][b, :, :t])    # :451
    return R_tt, R_ti, R_ii


def minmax64(cam, q_len, k_len, zero_cls=False):
    """``(m - min m) / (max m - min m)``, ``m = mean_h cam[b, h]`` on the live block (:493, :498, :502-503), zeros outside it.  numpy's
    ``min`` / ``max`` spread a NaN like torch's, and ``max == min`` leaves 0 / 0 = NaN.  ``zero_cls``: ``out[b, 0, 0] = 0`` last (:505)."""
    B, H, Nq, Nk = cam.shape
    out = np.zeros((B, Nq, Nk), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            q, k = int(q_len[b]), int(k_len[b])
            m = cam[b, :, :q, :k].astype(np.float64).mean(axis=0)
            out[b, :q, :k] = (m - m.min()) / (m.max() - m.min())
            if zero_cls:
                out[b, 0, 0] = 0.0
    return out


def minmax_maps(case):
    """The three maps the min-max entry is checked on: ``(name, cam, raw q_len, q, raw k_len, k, zero_cls)``; a raw length of ``None``
    means no array is handed over."""
    raw, t = case["raw"], case["t"]
    return [("self", case["text"][-1][0], raw, t, raw, t, True),
            ("cross", case["cross"][0], raw, t, None, case["full_i"], False),
            ("cross ragged keys", case["cross_k"], raw, t, case["k_len"], case["k_len"], False)]


# ---------------------------------------------------------------------------------------- error bounds (per element, u = 2^-24)
def attr_bounds(case, ref):
    """Every operand of the chain is non-negative, so the bounds are relative to the float64 value: ``expm1(n (len + H + 3) u)`` per
    chain (per step: ``H + 1`` roundings of A_bar, ``len`` of the product's sum, one of the add) and ``expm1((H + 3) u)`` for R_ti."""
    H, I, B = case["H"], case["I"], case["B"]
    R_tt, R_ti, R_ii = ref
    b_tt = np.stack([math.expm1(len(case["text"]) * (int(case["t"][b]) + H + 3) * U) * R_tt[b] for b in range(B)])
    b_ii = math.expm1(len(case["img"]) * (I + H + 3) * U) * R_ii
    b_ti = math.expm1((H + 3) * U) * R_ti
    return b_tt, b_ti, b_ii


def minmax_bound(cam, q_len, k_len, ref):
    """``2 e (1 + |out|) / (max - min) + 3 u |out|`` with ``e = (H + 1) u max_block(mean_h |cam|)``: numerator and denominator are each
    off by at most ``2 e``, then one subtraction, one more and the division round.  NaN (no bound) where the restatement is NaN."""
    B, H, Nq, Nk = cam.shape
    out = np.zeros((B, Nq, Nk), dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(B):
            q, k = int(q_len[b]), int(k_len[b])
            blk = cam[b, :, :q, :k].astype(np.float64)
            m = blk.mean(axis=0)
            e = (H + 1) * U * np.abs(blk).mean(axis=0).max()
            a = np.abs(ref[b, :q, :k])
            out[b, :q, :k] = 2.0 * e * (1.0 + a) / (m.max() - m.min()) + 3.0 * U * a
    return out


# ---------------------------------------------------------------------------------------- seeds
def clamp_shares(case):
    """``(clamped, positive)`` shares of rule 5's per-head products over the live entries of every pair of the case."""
    neg = pos = live = 0
    for pairs, ql, kl in ((case["text"], case["t"], case["t"]), (case["img"], case["full_i"], case["full_i"]),
                          ([case["cross"]], case["t"], case["full_i"])):
        for c, g in pairs:
            for b in range(case["B"]):
                q, k = int(ql[b]), int(kl[b])
                prod = g[b, :, :q, :k].astype(np.float64) * c[b, :, :q, :k].astype(np.float64)
                neg += int((prod < 0).sum())
                pos += int((prod > 0).sum())
                live += prod.size
    return neg / live, pos / live


def min_span(case):
    """The smallest ``(max m - min m) / max|m|`` over the live blocks of more than one entry of ``minmax_maps``."""
    worst = np.inf
    for _name, cam, _rq, q_len, _rk, k_len, _cls in minmax_maps(case):
        for b in range(case["B"]):
            q, k = int(q_len[b]), int(k_len[b])
            if q * k > 1:
                m = cam[b, :, :q, :k].astype(np.float64).mean(axis=0)
                worst = min(worst, (m.max() - m.min()) / np.abs(m).max())
    return worst


def find_seed(case, first=0, tries=200):
    for seed in range(first, first + tries):
        c = make_case(*case, seed)
        neg, pos = clamp_shares(c)
        if neg >= MIN_SHARE and pos >= MIN_SHARE and min_span(c) >= MIN_SPAN:
            return seed
    raise AssertionError("no seed with the two properties for %s" % (case,))


# {case: seed}: ``python tests/lxmert_lrp_batch_cases.py`` (find_seed over CASES, first fit from 0) prints the cases whose first fit
# is not 0 -- there is none: signed cams times ``randn`` gradients put about half the products on either side of the clamp
SEEDS = {c: 0 for c in CASES}


# ---------------------------------------------------------------------------------------- degenerate rows of the min-max entry
def degenerate_minmax():
    """``(name, cam [B, H, Nq, Nk], q_len, k_len)`` by hand: a constant live block (max == min), a one-entry block (t = 1 with
    k_len = 1) and one NaN inside a live block; sample 0 of each is an ordinary block, so a NaN must not leave its sample."""
    rng = np.random.default_rng(7)
    H, Nq, Nk = 3, 5, 7
    out = []
    base = (rng.standard_normal((2, H, Nq, Nk)) * 1e-2).astype(np.float32)
    const = base.copy()
    const[1, :, :3, :4] = 0.25
    out.append(("constant block", const, np.array([5, 3], np.int32), np.array([7, 4], np.int32)))
    out.append(("one-entry block", base.copy(), np.array([4, 1], np.int32), np.array([6, 1], np.int32)))
    nan = base.copy()
    nan[1, 2, 1, 2] = np.nan
    out.append(("NaN in the live block", nan, np.array([5, 3], np.int32), np.array([7, 4], np.int32)))
    return out


if __name__ == "__main__":
    for c in CASES:
        s = find_seed(c)
        if s:
            print("    %r: %d," % (c, s))
