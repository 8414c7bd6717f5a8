"""Shared by the suites of the batched VisualBERT baselines: the case table, the slabs of a case, float64 restatements of the three
methods for a padded batch written from their definitions (VisualBERT/mmf/models/transformers/backends/ExplanationGenerator.py:155-166
raw attention, :168-180 with :5-17 rollout, :200-211 attention GradCAM), each sample on its COMPACTED live set, the counted error
bounds of the kernels and float32 emulations (serial sums) of the kernels' arithmetic.

A case is ``(T, V, H, B, kind)``: padded text width, regions, heads, batch and the kind of length arrays --

    "null"    no length arrays (every sample is full)
    "full"    arrays that say T and V for every sample
    "ragged"  different lengths; at B = 5 text_len = [2, T, (T+2)//2, max(2, T-1), min(T, 3)] and
              vis_len = [V, 1, (V+1)//2, max(1, V-1), min(V, 2)]
    "oob"     as "ragged" with out-of-range entries (0 and T + 7 where "ragged" has 2 and T, V + 7 and 0 where it has V and 1; at
              B = 1: T + 7 and V + 7): the kernels clamp to 2..T and 1..V

The sequence of a padded sample is [T text positions | V regions]; its live index set is ``[0, t) u [T, T + v)`` -- the text padding
sits in the MIDDLE -- and every method returns row ``c = t - 2`` of its map, zero at ``c`` and outside the live set.

Slabs are what a masked body leaves behind: probability rows are a softmax over the LIVE keys (exact zeros at padded key columns,
ordinary rows at padded queries); gradients are ``randn + c_h`` with ``|c_h|`` in [0.5, 1.5] and alternating sign over h (pure ``randn``
makes the head weights ~ 0 and every GradCAM bound vacuous), set to 1e3 at every padded row and column, so that a sum taken over the
padded extent -- or divided by it -- is off by orders of magnitude.

Bounds, computed in float64 from the case's own data with u = 2^-24 and gamma(k) = k u / (1 - k u):

    raw attention   |err| <= gamma(H) ref                              elementwise (H - 1 additions and one division of non-negatives)
    rollout         |err| <= expm1(L (N + H + 2) u) ref                elementwise: every term is non-negative, so this holds for any
                                                                       summation order, and exact zeros stay exact
    GradCAM         dw_h = gamma(n^2) mean_live |G_h|                  (any summation order of the n^2 terms, then one division)
                    E = max over L x L of [(1/H) sum_h P_h dw_h + gamma(H + 2) (1/H) sum_h P_h (|w_h| + dw_h)]
                    |err| <= 4 E / (span - 2 E) + 4 u                  span = mx - mn of the float64 cam

``SEEDS`` holds, per case, a seed for which every GradCAM sample has ``span >= 100 E``, for H >= 3 at least 10 % of the live cam is
clamped and at least 10 % positive, and every sample with n >= 8 has a positive entry off ``c`` in row ``c`` (``find_seed`` searches
on the CPU; tests/test_visualbert_baselines_host.py asserts the properties), so neither the clamp nor the bound can make a
comparison vacuous."""
import functools

import numpy as np

SHAPES = ((3, 1), (8, 10), (24, 40), (28, 100), (128, 100))    # the smallest | N < 64 | N = 64 | N = 128 | N = 228, the real limit
HEADS = (1, 3, 12)
BATCHES = (1, 5)
KINDS = ("null", "full", "ragged", "oob")
N_LAYERS = (1, 2, 5)
PAD_GRAD = 1e3
MIN_SHARE = 0.10
MIN_SPAN_OVER_E = 100.0
U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def lengths(T, V, B, kind):
    """``(raw_t, raw_v, t, v)``: the int32 arrays handed to the kernels (``None`` for "null") and what they mean after the clamp."""
    if kind in ("null", "full"):
        t, v = np.full(B, T, dtype=np.int32), np.full(B, V, dtype=np.int32)
        return (None, None, t, v) if kind == "null" else (t.copy(), v.copy(), t, v)
    if B == 5:
        t = np.array([2, T, (T + 2) // 2, max(2, T - 1), min(T, 3)], dtype=np.int32)
        v = np.array([V, 1, (V + 1) // 2, max(1, V - 1), min(V, 2)], dtype=np.int32)
    else:
        t, v = np.full(B, (T + 2) // 2, dtype=np.int32), np.full(B, (V + 1) // 2, dtype=np.int32)
    if kind == "ragged":
        return t.copy(), v.copy(), t, v
    raw_t, raw_v = t.copy(), v.copy()
    if B == 5:
        raw_t[0], raw_t[1] = 0, T + 7                  # clamped to 2 and T
        raw_v[0], raw_v[1] = V + 7, 0                  # clamped to V and 1
        return raw_t, raw_v, t, v
    raw_t[:], raw_v[:] = T + 7, V + 7
    return raw_t, raw_v, np.full(B, T, dtype=np.int32), np.full(B, V, dtype=np.int32)


def live_index(T, t, v):
    return np.concatenate((np.arange(int(t)), T + np.arange(int(v))))


def _softmax_slab(rng, B, H, T, V, t, v):
    N = T + V
    logits = (rng.standard_normal((B, H, N, N)) * 2.0).astype(np.float32).astype(np.float64)
    out = np.zeros((B, H, N, N), dtype=np.float64)
    for b in range(B):
        idx = live_index(T, t[b], v[b])
        z = logits[b][:, :, idx]
        e = np.exp(z - z.max(-1, keepdims=True))
        out[b][:, :, idx] = e / e.sum(-1, keepdims=True)
    return out.astype(np.float32)


def head_offsets(rng, H):
    """``c_h``: |c_h| in [0.5, 1.5], sign + - + ... over h."""
    return rng.uniform(0.5, 1.5, H) * np.where(np.arange(H) % 2 == 0, 1.0, -1.0)


def _grad_slab(rng, B, H, T, V, t, v, offsets):
    N = T + V
    g = (rng.standard_normal((B, H, N, N)) + offsets[None, :, None, None]).astype(np.float32)
    for b in range(B):
        dead = np.ones(N, dtype=bool)
        dead[live_index(T, t[b], v[b])] = False
        g[b][:, dead, :] = PAD_GRAD
        g[b][:, :, dead] = PAD_GRAD
    return g


@functools.lru_cache(maxsize=4)
def make_case(T, V, H, B, kind, seed, n_layers=1, negate=False):
    """The slabs of a case (numpy, fp32) and its lengths: ``attn`` a table of ``n_layers`` probability slabs -- ``attn[-1]`` with ``grad``
    is what raw attention and GradCAM read -- drawn so that one seed means the same GradCAM case for every table length.  ``negate``
    flips the head offsets (H = 1: every head weight negative, the whole cam clamped).  Cached: treat the arrays as read-only."""
    rng = np.random.default_rng(seed)
    raw_t, raw_v, t, v = lengths(T, V, B, kind)
    offsets = head_offsets(rng, H) * (-1.0 if negate else 1.0)
    case = dict(T=T, V=V, N=T + V, H=H, B=B, kind=kind, raw_t=raw_t, raw_v=raw_v, t=t, v=v, offsets=offsets)
    case["grad"] = _grad_slab(rng, B, H, T, V, t, v, offsets)
    last = _softmax_slab(rng, B, H, T, V, t, v)
    case["attn"] = [_softmax_slab(rng, B, H, T, V, t, v) for _ in range(n_layers - 1)] + [last]
    return case


def _compact(slab, b, idx):
    return slab[b][:, idx][:, :, idx].astype(np.float64)


# ---------------------------------------------------------------------------------------- float64 restatements and bounds
def raw64(P, T, t, v):
    """``(ref, bound)``, both ``[B, N]``: :155-166 on each sample's compacted live set, scattered back to the padded layout."""
    B, H, N, _ = P.shape
    ref = np.zeros((B, N))
    for b in range(B):
        idx, c = live_index(T, t[b], v[b]), int(t[b]) - 2
        row = _compact(P, b, idx).mean(axis=0)[c]
        row[c] = 0.0
        ref[b, idx] = row
    return ref, gamma(H) * ref


def rollout64(layers, T, t, v):
    """``(ref, bound)``: :168-180 with :5-17 (add I, NO row normalisation, left-multiplied), the full product, row c."""
    B, H, N, _ = layers[0].shape
    ref = np.zeros((B, N))
    for b in range(B):
        idx, c = live_index(T, t[b], v[b]), int(t[b]) - 2
        mats = [_compact(m, b, idx).sum(axis=0) / H + np.eye(idx.size) for m in layers]
        joint = mats[0]
        for m in mats[1:]:
            joint = m @ joint
        row = joint[c].copy()
        row[c] = 0.0
        ref[b, idx] = row
    return ref, np.expm1(len(layers) * (N + H + 2) * U) * ref


def gradcam64(P, G, T, t, v, details=False):
    """``(ref, bound)``: :200-211 on the compacted live block, min-max normalised, row c; ``bound`` is ``[B]``, one figure per sample.
    ``details``: also the per-sample dicts (``pre`` the map before the clamp, ``cam``, ``span``, ``E``)."""
    B, H, N, _ = P.shape
    ref, bound, info = np.zeros((B, N)), np.zeros(B), []
    for b in range(B):
        idx, c = live_index(T, t[b], v[b]), int(t[b]) - 2
        p, g = _compact(P, b, idx), _compact(G, b, idx)
        n = idx.size
        w = g.mean(axis=(1, 2))
        pre = (p * w[:, None, None]).mean(axis=0)
        cam = np.maximum(pre, 0.0)
        mn, mx = cam.min(), cam.max()
        span = mx - mn
        dw = gamma(n * n) * np.abs(g).mean(axis=(1, 2))
        E = float(((p * dw[:, None, None]).sum(0) / H + gamma(H + 2) * (p * (np.abs(w) + dw)[:, None, None]).sum(0) / H).max())
        with np.errstate(invalid="ignore", divide="ignore"):
            row = (cam[c] - mn) / span
            bound[b] = 4.0 * E / (span - 2.0 * E) + 4.0 * U if span > 2.0 * E else np.inf
        row[c] = 0.0
        ref[b, idx] = row
        info.append(dict(pre=pre, cam=cam, span=span, E=E, c=c, n=n))
    return (ref, bound, info) if details else (ref, bound)


# ---------------------------------------------------------------------------------------- float32 emulations (serial sums)
F = np.float32


def raw_f32(P, T, t, v):
    B, H, N, _ = P.shape
    out = np.zeros((B, N), dtype=F)
    for b in range(B):
        idx, c = live_index(T, t[b], v[b]), int(t[b]) - 2
        s = np.zeros(idx.size, dtype=F)
        for h in range(H):
            s = s + P[b, h, c, idx]
        s = s / F(H)
        s[c] = 0
        out[b, idx] = s
    return out


def rollout_f32(layers, T, t, v):
    B, H, N, _ = layers[0].shape
    out = np.zeros((B, N), dtype=F)
    for b in range(B):
        idx, c = live_index(T, t[b], v[b]), int(t[b]) - 2
        x = np.zeros(idx.size, dtype=F)
        x[c] = 1
        for m in reversed(layers):
            A = np.zeros((idx.size, idx.size), dtype=F)
            for h in range(H):
                A = A + m[b, h][idx][:, idx]
            A = A / F(H)
            y = np.zeros(idx.size, dtype=F)
            for i in range(idx.size):
                y = y + x[i] * A[i]
            x = x + y
        x[c] = 0
        out[b, idx] = x
    return out


def gradcam_f32(P, G, T, t, v):
    B, H, N, _ = P.shape
    out = np.zeros((B, N), dtype=F)
    for b in range(B):
        idx, c = live_index(T, t[b], v[b]), int(t[b]) - 2
        n = idx.size
        acc = np.zeros((n, n), dtype=F)
        for h in range(H):
            w = np.cumsum(G[b, h][idx][:, idx].ravel(), dtype=F)[-1] / F(n * n)       # (a float32 cumsum is a serial sum)
            acc = acc + P[b, h][idx][:, idx] * w
        cam = np.maximum(acc / F(H), F(0))
        mn, mx = cam.min(), cam.max()
        with np.errstate(invalid="ignore", divide="ignore"):
            row = (cam[c] - mn) / (mx - mn)
        row[c] = 0
        out[b, idx] = row
    return out


# ---------------------------------------------------------------------------------------- seeds
def seed_report(case):
    """What the host test asserts about a case's GradCAM data: the smallest ``span / E`` over the samples, the clamped and positive
    shares of the live cam, and whether every sample with n >= 8 has a positive entry off c in row c."""
    _ref, _bound, info = gradcam64(case["attn"][-1], case["grad"], case["T"], case["t"], case["v"], details=True)
    ratio = min(d["span"] / d["E"] for d in info)
    neg = sum(int((d["pre"] < 0).sum()) for d in info)
    pos = sum(int((d["pre"] > 0).sum()) for d in info)
    live = sum(d["pre"].size for d in info)
    row_ok = all(bool((np.delete(d["cam"][d["c"]], d["c"]) > 0).any()) for d in info if d["n"] >= 8)
    return dict(ratio=ratio, clamped=neg / live, positive=pos / live, row_ok=row_ok)


def seed_fits(case):
    r = seed_report(case)
    shares = case["H"] < 3 or (r["clamped"] >= MIN_SHARE and r["positive"] >= MIN_SHARE)
    return r["ratio"] >= MIN_SPAN_OVER_E and shares and r["row_ok"]


def find_seed(T, V, H, B, kind, first=1, tries=50):
    for seed in range(first, first + tries):
        if seed_fits(make_case(T, V, H, B, kind, seed)):
            return seed
    raise AssertionError("no seed fits %s" % ((T, V, H, B, kind),))


CASES = [(T, V, H, B, kind) for (T, V) in SHAPES for H in HEADS for B in BATCHES for kind in KINDS]

# {case: seed} where the first fit from 1 is not 1, written by ``python tests/visualbert_baselines_cases.py``
OTHER_SEEDS = {
}
SEEDS = {c: OTHER_SEEDS.get(c, 1) for c in CASES}


def case_id(c):
    return "T%d_V%d_H%d_B%d_%s" % c


if __name__ == "__main__":
    for c in CASES:
        s = find_seed(*c)
        if s != 1:
            print("    %r: %d," % (c, s))
