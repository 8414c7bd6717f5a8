"""Shared by the suites of the padded-batch ``generate_ours`` of VisualBERT (``mmx_selfattn_ours_row``): the case table, the slabs of a
case, a float64 restatement of VisualBERT/mmf/models/transformers/backends/ExplanationGenerator.py:83-97 for a padded batch -- each
sample on its COMPACTED live set, the full matrix chain, row c -- the counted error bound of the kernels, a serial float32 emulation
of their arithmetic and the mutants the data must be able to tell from the method.

A case is ``(T, V, H, B, kind, L)``: the first five as in ``tests/visualbert_baselines_cases.py`` (whose shapes, head counts, length
kinds and slab makers are imported, not restated), ``L`` the number of layers.  Every layer has its own probability slab (a softmax
over the LIVE keys: exact zeros at padded key columns, ordinary rows at padded queries) and its own gradient slab (``randn + c_h``,
``|c_h|`` in [0.5, 1.5], sign + - + ... over h, ``PAD_GRAD`` = 1e3 at every padded row and column).

The method, per sample on its live set (n = t + v entries, c = t - 2):

    A_l = (sum_h max(0, G_l[h] * P_l[h])) / H          the clamp per head, BEFORE the sum (rule 5, :91-92)
    R   = (I + A_{L-1}) ... (I + A_0)                  R += A_l R from layer 0 up (:93)
    out = R[c] with out[c] = 0                         (:94-97)

Bound, with u = 2^-24:  |err| <= expm1(L (N + H + 3) u) ref, elementwise.  Per layer: one rounding per product g * p, H - 1 additions
and one division for A_l, and at most n + 1 operations on any path of the row update x <- x + x . A_l (n products-and-additions of
the dot product in any association, one addition of x): at most N + H + 2 roundings, N + H + 3 allowed.  Every term is non-negative
after the clamp, so the relative errors compound as (1 +- u)^k for ANY summation order and an exact zero stays an exact zero.  A
float32 product has the sign of the exact product as long as it does not underflow (``min_product`` is asserted to be normal), so the
kernel and the float64 restatement take the same clamp decisions.

``SEEDS`` holds, per case, a seed for which at least 10 % of the live ``g * p`` entries are clamped and at least 10 % positive
(H >= 3) and every mutant that can differ from the method on a sample does so by at least ``MUTANT_FACTOR`` x the bound
(``find_seed`` searches on the CPU; tests/test_visualbert_ours_host.py asserts the properties)."""
import functools

import numpy as np

from visualbert_baselines_cases import (HEADS, KINDS, PAD_GRAD, SHAPES, U, _grad_slab, _softmax_slab, gamma, head_offsets, lengths,
                                        live_index)

MIN_SHARE = 0.10
MUTANT_FACTOR = 2.0
FLT_MIN = float(np.finfo(np.float32).tiny)          # the smallest normal float32
B_MAIN, L_MAIN = 5, 5
F = np.float32

# every shape x head count x length kind at B = 5, L = 5; then L in {1, 2} and B = 1 at N = 64 (one full wave of columns) and at
# N = 228 (the real limit)
CASES = [(T, V, H, B_MAIN, kind, L_MAIN) for (T, V) in SHAPES for H in HEADS for kind in KINDS]
CASES += [(T, V, H, B, "ragged", L) for (T, V, H) in ((24, 40, 3), (128, 100, 12)) for (B, L) in ((5, 1), (5, 2), (1, 5), (1, 2))]
CASES += [(T, V, H, 1, "oob", 1) for (T, V, H) in ((24, 40, 3), (128, 100, 12))]


def case_id(c):
    return "T%d_V%d_H%d_B%d_%s_L%d" % c


@functools.lru_cache(maxsize=2)
def _slabs(T, V, H, B, t_key, v_key, seed, n_layers):
    """The slabs depend on the CLAMPED lengths only: "null" and "full", and "ragged" and "oob", share them."""
    rng = np.random.default_rng(seed)
    t, v = np.array(t_key, dtype=np.int32), np.array(v_key, dtype=np.int32)
    offsets = head_offsets(rng, H)
    attn = [_softmax_slab(rng, B, H, T, V, t, v) for _ in range(n_layers)]
    grad = [_grad_slab(rng, B, H, T, V, t, v, offsets) for _ in range(n_layers)]
    return offsets, attn, grad


def make_case(T, V, H, B, kind, n_layers, seed):
    """The slabs of a case (numpy, fp32; cached: treat them as read-only) and its lengths."""
    raw_t, raw_v, t, v = lengths(T, V, B, kind)
    offsets, attn, grad = _slabs(T, V, H, B, tuple(int(x) for x in t), tuple(int(x) for x in v), seed, n_layers)
    return dict(T=T, V=V, N=T + V, H=H, B=B, L=n_layers, kind=kind, raw_t=raw_t, raw_v=raw_v, t=t, v=v, offsets=offsets, attn=attn,
                grad=grad)


def _compact(slab, b, idx):
    return slab[b][:, idx][:, :, idx].astype(np.float64)


def bound_factor(L, N, H):
    return float(np.expm1(L * (N + H + 3) * U))


# ---------------------------------------------------------------------------------------- the float64 restatement and its mutants
MUTANTS = ("clamp_after_sum", "ascending_layers", "padded_extent", "prefix_live_set", "c_is_t_minus_1", "no_identity")


def _row64(P, G, b, idx, c, mutant=None):
    """Row ``c`` of the full matrix chain on the index set ``idx`` of sample b, its own column zeroed."""
    H = P[0].shape[1]
    mats = []
    for p, g in zip(P, G):
        prod = _compact(g, b, idx) * _compact(p, b, idx)             # exact: 24 x 24 bits fit a float64
        if mutant == "clamp_after_sum":
            mats.append(np.maximum(prod.sum(axis=0) / H, 0.0))
        else:
            mats.append(np.maximum(prod, 0.0).sum(axis=0) / H)
    if mutant == "ascending_layers":
        mats = mats[::-1]
    eye = np.eye(idx.size)
    R = eye.copy()
    for A in mats:
        R = A @ R if mutant == "no_identity" else R + A @ R
    row = R[c].copy()
    row[c] = 0.0
    return row


def ours64(P, G, T, t, v):
    """``(ref, bound)``, both ``[B, N]``: :83-97 on each sample's compacted live set, scattered back to the padded layout."""
    B, H, N, _ = P[0].shape
    ref = np.zeros((B, N))
    for b in range(B):
        idx = live_index(T, t[b], v[b])
        ref[b, idx] = _row64(P, G, b, idx, int(t[b]) - 2)
    return ref, bound_factor(len(P), N, H) * ref


def can_differ(mutant, H, L, T, t_b):
    """Whether ``mutant`` is another function than the method on a sample of ``t_b`` text tokens.  The padded-extent mutants differ
    through the text padding only: the probabilities are exact zeros at padded key columns and ``PAD_GRAD`` is finite, so a padded
    REGION never receives relevance and a sum that includes it adds exact zeros."""
    if mutant == "clamp_after_sum":
        return H >= 3
    if mutant in ("ascending_layers", "no_identity"):
        return L >= 2                                    # (one layer: e_c A and e_c (I + A) differ at column c only, which is zeroed)
    if mutant in ("padded_extent", "prefix_live_set"):
        return int(t_b) < T
    return True


def mutant64(mutant, P, G, T, t, v):
    """``[B, N]``: the method with one mistake, in float64.

    clamp_after_sum    max(0, mean_h(g p)) instead of mean_h max(0, g p)
    ascending_layers   the row vector carried through layer 0 first: (I + A_0) ... (I + A_{L-1})
    padded_extent      the lengths ignored: every sum over all N rows and columns, row T - 2
    prefix_live_set    the live set taken as the leading n positions (the text padding sits in the MIDDLE of the sequence)
    c_is_t_minus_1     the row of [SEP], not of the token in front of it
    no_identity        R <- A_l R (the residual term dropped)"""
    B, H, N, _ = P[0].shape
    out = np.zeros((B, N))
    for b in range(B):
        idx, c = live_index(T, t[b], v[b]), int(t[b]) - 2
        if mutant == "padded_extent":
            idx, c = np.arange(N), T - 2
        elif mutant == "prefix_live_set":
            idx = np.arange(idx.size)
        elif mutant == "c_is_t_minus_1":
            c = int(t[b]) - 1
        out[b, idx] = _row64(P, G, b, idx, c, mutant)
    return out


def distance_in_bounds(got, ref, bound):
    """``[B]``: max over a sample's entries of |got - ref| / bound (an entry that differs where the bound is zero counts as inf)."""
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, np.where(bound > 0, err / bound, np.inf))
    return ratio.max(axis=1)


# ---------------------------------------------------------------------------------------- float32 emulation (serial sums)
def ours_f32(P, G, T, t, v):
    B, H, N, _ = P[0].shape
    out = np.zeros((B, N), dtype=F)
    for b in range(B):
        idx, c = live_index(T, t[b], v[b]), int(t[b]) - 2
        x = np.zeros(idx.size, dtype=F)
        x[c] = 1
        for p, g in zip(reversed(P), reversed(G)):
            A = np.zeros((idx.size, idx.size), dtype=F)
            for h in range(H):
                A = A + np.maximum(g[b, h][idx][:, idx] * p[b, h][idx][:, idx], F(0))
            A = A / F(H)
            y = np.zeros(idx.size, dtype=F)
            for i in range(idx.size):
                y = y + x[i] * A[i]
            x = x + y
        x[c] = 0
        out[b, idx] = x
    return out


# ---------------------------------------------------------------------------------------- seeds
def seed_report(case):
    """What the host test asserts about a case's data: the clamped and the positive share of the live ``g * p`` entries, the smallest
    non-zero |float32 product| among them, and per mutant the smallest distance (in bounds) over the samples on which it can differ
    (``None`` when there is no such sample)."""
    T, H, L, t, v = case["T"], case["H"], case["L"], case["t"], case["v"]
    neg = pos = live = 0
    smallest = np.inf
    for p, g in zip(case["attn"], case["grad"]):
        for b in range(case["B"]):
            idx = live_index(T, t[b], v[b])
            prod = g[b][:, idx][:, :, idx] * p[b][:, idx][:, :, idx]                   # float32, as the kernel forms it
            neg += int((prod < 0).sum())
            pos += int((prod > 0).sum())
            live += prod.size
            exact = g[b][:, idx][:, :, idx].astype(np.float64) * p[b][:, idx][:, :, idx].astype(np.float64)
            if (exact != 0).any():
                smallest = min(smallest, float(np.abs(prod[exact != 0]).min()))
    ref, bound = ours64(case["attn"], case["grad"], T, t, v)
    mutants = {}
    for m in MUTANTS:
        where = [b for b in range(case["B"]) if can_differ(m, H, L, T, t[b])]
        if where:
            mutants[m] = float(distance_in_bounds(mutant64(m, case["attn"], case["grad"], T, t, v), ref, bound)[where].min())
        else:
            mutants[m] = None
    return dict(clamped=neg / live, positive=pos / live, min_product=smallest, mutants=mutants)


def report_fits(r, H):
    shares = H < 3 or (r["clamped"] >= MIN_SHARE and r["positive"] >= MIN_SHARE)
    return shares and r["min_product"] >= FLT_MIN and all(d is None or d >= MUTANT_FACTOR for d in r["mutants"].values())


def find_seed(T, V, H, B, kind, L, first=1, tries=50):
    for seed in range(first, first + tries):
        if report_fits(seed_report(make_case(T, V, H, B, kind, L, seed)), H):
            return seed
    raise AssertionError("no seed fits %s" % ((T, V, H, B, kind, L),))


# {case: seed} where the first fit from 1 is not 1, written by ``python tests/visualbert_ours_cases.py``
OTHER_SEEDS = {
}
SEEDS = {c: OTHER_SEEDS.get(c, 1) for c in CASES}


if __name__ == "__main__":
    for c in CASES:
        s = find_seed(*c)
        if s != 1:
            print("    %r: %d," % (c, s))
