"""Shared by the suites of the batched LXMERT baselines: the case table, the slabs of a case and a float64 restatement of the three
methods for a padded batch, written from their definitions (lxmert/lxmert/src/ExplanationGenerator.py:508-540 raw attention,
:542-593 attention GradCAM, :595-665 with :5-15 rollout), each sample on its LIVE block only.

A case is ``(T, I, H, B, kind)``: padded text / image sizes, heads, batch and the kind of length array --

    "null"    no length array (every sample is full)
    "full"    an array that says T for every sample
    "ragged"  different lengths, t = 1 and t = T among them at B = 5
    "oob"     as "ragged" with out-of-range entries (0 and T + 7 at B = 5, T + 7 at B = 1): the kernels clamp to 1..T

Slabs are what a masked body leaves behind: probability rows are a softmax over the LIVE keys (exact zeros at padded key columns,
ordinary rows at padded queries), gradients are ``randn`` with 1e3 at padded key columns and padded query rows, so that a mean taken
over the padded extent -- or divided by it -- is off by orders of magnitude.  ``SEEDS`` holds, per case, a seed for which the float64
GradCAM maps have at least 10 % clamped and at least 10 % positive entries inside the live blocks (``find_seed`` searched them on the
CPU; tests/test_lxmert_baselines_host.py asserts the property), so the clamp cannot make a comparison vacuous."""
import numpy as np

from oracle import relevancy_np

SHAPES = ((2, 3), (12, 20), (17, 36), (48, 48))     # below one 16 x 16 tile | no multiple of 16 | crossing 16 and 32 | the limit
HEADS = (1, 3, 12)
BATCHES = (1, 5)
KINDS = ("null", "full", "ragged", "oob")
N_TEXT = (2, 5)
N_IMG = (1, 4)
PAD_GRAD = 1e3
MIN_SHARE = 0.10


def lengths(T, B, kind):
    """``(raw, clamped)``: the int32 array handed to the kernels (``None`` for "null") and what it means after the clamp."""
    if kind in ("null", "full"):
        full = np.full(B, T, dtype=np.int32)
        return (None if kind == "null" else full), full
    ragged = np.array([1, T, (T + 1) // 2, max(1, T - 1), min(T, 3)], dtype=np.int32) if B == 5 else \
        np.full(B, (T + 1) // 2, dtype=np.int32)
    if kind == "ragged":
        return ragged, ragged.copy()
    raw = ragged.copy()
    if B == 5:
        raw[0], raw[1] = 0, T + 7                    # clamped to 1 and T: the same live blocks as "ragged"
        return raw, ragged.copy()
    raw[:] = T + 7
    return raw, np.full(B, T, dtype=np.int32)


def image_lengths(I, B):
    """Ragged KEY lengths of the cross slab (the head-mean entry takes the two lengths independently)."""
    return np.array([I, 1, (I + 1) // 2, max(1, I - 1), min(I, 2)], dtype=np.int32)[:B] if B == 5 else \
        np.full(B, max(1, I - 1), dtype=np.int32)


def _softmax_slab(rng, B, H, Nq, Nk, k_live):
    logits = rng.standard_normal((B, H, Nq, Nk)) * 2.0
    out = np.zeros((B, H, Nq, Nk), dtype=np.float64)
    for b in range(B):
        k = int(k_live[b])
        e = np.exp(logits[b, :, :, :k] - logits[b, :, :, :k].max(-1, keepdims=True))
        out[b, :, :, :k] = e / e.sum(-1, keepdims=True)
    return out.astype(np.float32)


def _grad_slab(rng, B, H, Nq, Nk, q_live, k_live):
    g = rng.standard_normal((B, H, Nq, Nk)).astype(np.float32)
    for b in range(B):
        g[b, :, int(q_live[b]):, :] = PAD_GRAD
        g[b, :, :, int(k_live[b]):] = PAD_GRAD
    return g


def make_case(T, I, H, B, kind, seed, n_text=2, n_img=1):
    """The slabs of a case (numpy, fp32) and its lengths.  ``text[-1]`` / ``cross`` with ``g_tt`` / ``g_ti`` are the last x-layer's
    language self-attention and cross-attention with their gradients; ``cross_k`` / ``g_ti_k`` the same kind of slab under ragged
    key lengths ``k_len`` as well."""
    rng = np.random.default_rng(seed)
    raw, t = lengths(T, B, kind)
    full_i = np.full(B, I, dtype=np.int32)
    k_len = image_lengths(I, B)
    case = dict(T=T, I=I, H=H, B=B, kind=kind, raw=raw, t=t, k_len=k_len)
    case["g_tt"] = _grad_slab(rng, B, H, T, T, t, t)
    case["g_ti"] = _grad_slab(rng, B, H, T, I, t, full_i)
    case["g_ti_k"] = _grad_slab(rng, B, H, T, I, t, k_len)
    case["cross"] = _softmax_slab(rng, B, H, T, I, full_i)
    case["cross_k"] = _softmax_slab(rng, B, H, T, I, k_len)
    case["text"] = [_softmax_slab(rng, B, H, T, T, t) for _ in range(n_text)]        # (the gradient slabs come first: one seed
    case["img"] = [_softmax_slab(rng, B, H, I, I, full_i) for _ in range(n_img)]     #  means the same GradCAM case for every table)
    return case


# ---------------------------------------------------------------------------------------- float64 restatement
def head_mean64(P, q_len, k_len, zero_cls=False):
    B, H, Nq, Nk = P.shape
    out = np.zeros((B, Nq, Nk), dtype=np.float64)
    for b in range(B):
        q, k = int(q_len[b]), int(k_len[b])
        out[b, :q, :k] = P[b, :, :q, :k].astype(np.float64).mean(axis=0)
        if zero_cls:
            out[b, 0, 0] = 0.0
    return out


def gradcam64(P, G, q_len, k_len, zero_cls=False, clamp=True):
    """``clamp(mean_h(P[b, h] * w[b, h]), 0)``, ``w[b, h]`` = the mean of ``G[b, h]`` over the live block (:542-547 on the unpadded
    item).  ``clamp=False`` returns the values before the clamp (the host test counts their signs)."""
    B, H, Nq, Nk = P.shape
    out = np.zeros((B, Nq, Nk), dtype=np.float64)
    for b in range(B):
        q, k = int(q_len[b]), int(k_len[b])
        w = G[b, :, :q, :k].astype(np.float64).mean(axis=(1, 2), keepdims=True)
        pre = (P[b, :, :q, :k].astype(np.float64) * w).mean(axis=0)
        out[b, :q, :k] = np.maximum(pre, 0.0) if clamp else pre
        if zero_cls:
            out[b, 0, 0] = 0.0
    return out


def _rollout_product64(mats):
    """compute_rollout_attention (:5-15) in float64: add I, divide by the row sums, left-multiply."""
    n = mats[0].shape[-1]
    aug = [m + np.eye(n) for m in mats]
    aug = [m / m.sum(axis=-1, keepdims=True) for m in aug]
    joint = aug[0]
    for m in aug[1:]:
        joint = m @ joint
    return joint


def rollout64(text, img, cross, t_len):
    """``(R_tt [B, T, T], R_ti [B, T, I], R_ii [B, I, I])`` of :595-665, sample b on its leading ``t_len[b]`` tokens."""
    B, H, T, I = cross.shape
    R_tt, R_ti, R_ii = np.zeros((B, T, T)), np.zeros((B, T, I)), np.zeros((B, I, I))
    for b in range(B):
        t = int(t_len[b])
        cams_t = [m[b, :, :t, :t].astype(np.float64).mean(axis=0) for m in text]
        cams_i = [m[b].astype(np.float64).mean(axis=0) for m in img]
        cam_ti = cross[b, :, :t, :].astype(np.float64).mean(axis=0)
        r_prime = _rollout_product64(cams_t[:-1])
        R_ii[b] = _rollout_product64(cams_i)
        R_ti[b, :t] = r_prime.T @ (cam_ti @ R_ii[b])
        R_tt[b, :t, :t] = _rollout_product64(cams_t)
        R_tt[b, 0, 0] = 0.0
    return R_tt, R_ti, R_ii


def rollout_f32_oracle(text, img, cross, t_len):
    """The same in the oracle's own fp32 arithmetic (``oracle.relevancy_np.compute_rollout_attention``): the host test checks the
    float64 restatement above against it."""
    B, H, T, I = cross.shape
    R_tt, R_ti = np.zeros((B, T, T), np.float32), np.zeros((B, T, I), np.float32)
    for b in range(B):
        t = int(t_len[b])
        cams_t = [m[b, :, :t, :t].mean(axis=0) for m in text]
        cams_i = [m[b].mean(axis=0) for m in img]
        r_prime = relevancy_np.compute_rollout_attention(cams_t[:-1])
        r_ii = relevancy_np.compute_rollout_attention(cams_i)
        R_ti[b, :t] = r_prime.T @ (cross[b, :, :t, :].mean(axis=0) @ r_ii)
        R_tt[b, :t, :t] = relevancy_np.compute_rollout_attention(cams_t)
        R_tt[b, 0, 0] = 0.0
    return R_tt, R_ti


# ---------------------------------------------------------------------------------------- GradCAM seeds
def gradcam_maps64(case, clamp=True):
    """The three GradCAM maps the op-level suite checks: language self-attention (q = k = t, [CLS] entry zeroed), cross-attention
    (q = t, every key) and the cross slab under ragged key lengths."""
    full_i = np.full(case["B"], case["I"], dtype=np.int32)
    return (gradcam64(case["text"][-1], case["g_tt"], case["t"], case["t"], zero_cls=True, clamp=clamp),
            gradcam64(case["cross"], case["g_ti"], case["t"], full_i, clamp=clamp),
            gradcam64(case["cross_k"], case["g_ti_k"], case["t"], case["k_len"], clamp=clamp))


def clamp_shares(case):
    """``(clamped, positive)`` shares of the live entries of the case's GradCAM maps before the clamp."""
    pre = gradcam_maps64(case, clamp=False)
    full_i = np.full(case["B"], case["I"], dtype=np.int32)
    neg = pos = live = 0
    for m, (ql, kl) in zip(pre, ((case["t"], case["t"]), (case["t"], full_i), (case["t"], case["k_len"]))):
        for b in range(case["B"]):
            blk = m[b, :int(ql[b]), :int(kl[b])]
            neg += int((blk < 0).sum())
            pos += int((blk > 0).sum())
            live += blk.size
    return neg / live, pos / live


def find_seed(T, I, H, B, kind, first=0, tries=200):
    for seed in range(first, first + tries):
        neg, pos = clamp_shares(make_case(T, I, H, B, kind, seed))
        if neg >= MIN_SHARE and pos >= MIN_SHARE:
            return seed
    raise AssertionError("no seed with >= 10 %% clamped and >= 10 %% positive GradCAM entries for %s" % ((T, I, H, B, kind),))


# {(T, I, H, B, kind): seed}, written by ``python tests/lxmert_baselines_cases.py`` (find_seed over CASES, first fit from 0)
SEEDS = {
    (2, 3, 1, 1, 'null'): 0, (2, 3, 1, 1, 'full'): 0, (2, 3, 1, 1, 'ragged'): 0, (2, 3, 1, 1, 'oob'): 0,
    (2, 3, 1, 5, 'null'): 0, (2, 3, 1, 5, 'full'): 0, (2, 3, 1, 5, 'ragged'): 0, (2, 3, 1, 5, 'oob'): 0,
    (2, 3, 3, 1, 'null'): 0, (2, 3, 3, 1, 'full'): 0, (2, 3, 3, 1, 'ragged'): 0, (2, 3, 3, 1, 'oob'): 0,
    (2, 3, 3, 5, 'null'): 0, (2, 3, 3, 5, 'full'): 0, (2, 3, 3, 5, 'ragged'): 0, (2, 3, 3, 5, 'oob'): 0,
    (2, 3, 12, 1, 'null'): 0, (2, 3, 12, 1, 'full'): 0, (2, 3, 12, 1, 'ragged'): 0, (2, 3, 12, 1, 'oob'): 0,
    (2, 3, 12, 5, 'null'): 0, (2, 3, 12, 5, 'full'): 0, (2, 3, 12, 5, 'ragged'): 0, (2, 3, 12, 5, 'oob'): 0,
    (12, 20, 1, 1, 'null'): 0, (12, 20, 1, 1, 'full'): 0, (12, 20, 1, 1, 'ragged'): 1, (12, 20, 1, 1, 'oob'): 0,
    (12, 20, 1, 5, 'null'): 0, (12, 20, 1, 5, 'full'): 0, (12, 20, 1, 5, 'ragged'): 0, (12, 20, 1, 5, 'oob'): 0,
    (12, 20, 3, 1, 'null'): 0, (12, 20, 3, 1, 'full'): 0, (12, 20, 3, 1, 'ragged'): 0, (12, 20, 3, 1, 'oob'): 0,
    (12, 20, 3, 5, 'null'): 0, (12, 20, 3, 5, 'full'): 0, (12, 20, 3, 5, 'ragged'): 0, (12, 20, 3, 5, 'oob'): 0,
    (12, 20, 12, 1, 'null'): 0, (12, 20, 12, 1, 'full'): 0, (12, 20, 12, 1, 'ragged'): 0, (12, 20, 12, 1, 'oob'): 0,
    (12, 20, 12, 5, 'null'): 0, (12, 20, 12, 5, 'full'): 0, (12, 20, 12, 5, 'ragged'): 0, (12, 20, 12, 5, 'oob'): 0,
    (17, 36, 1, 1, 'null'): 4, (17, 36, 1, 1, 'full'): 4, (17, 36, 1, 1, 'ragged'): 0, (17, 36, 1, 1, 'oob'): 4,
    (17, 36, 1, 5, 'null'): 0, (17, 36, 1, 5, 'full'): 0, (17, 36, 1, 5, 'ragged'): 0, (17, 36, 1, 5, 'oob'): 0,
    (17, 36, 3, 1, 'null'): 0, (17, 36, 3, 1, 'full'): 0, (17, 36, 3, 1, 'ragged'): 0, (17, 36, 3, 1, 'oob'): 0,
    (17, 36, 3, 5, 'null'): 0, (17, 36, 3, 5, 'full'): 0, (17, 36, 3, 5, 'ragged'): 0, (17, 36, 3, 5, 'oob'): 0,
    (17, 36, 12, 1, 'null'): 0, (17, 36, 12, 1, 'full'): 0, (17, 36, 12, 1, 'ragged'): 0, (17, 36, 12, 1, 'oob'): 0,
    (17, 36, 12, 5, 'null'): 0, (17, 36, 12, 5, 'full'): 0, (17, 36, 12, 5, 'ragged'): 0, (17, 36, 12, 5, 'oob'): 0,
    (48, 48, 1, 1, 'null'): 0, (48, 48, 1, 1, 'full'): 0, (48, 48, 1, 1, 'ragged'): 1, (48, 48, 1, 1, 'oob'): 0,
    (48, 48, 1, 5, 'null'): 0, (48, 48, 1, 5, 'full'): 0, (48, 48, 1, 5, 'ragged'): 0, (48, 48, 1, 5, 'oob'): 0,
    (48, 48, 3, 1, 'null'): 0, (48, 48, 3, 1, 'full'): 0, (48, 48, 3, 1, 'ragged'): 0, (48, 48, 3, 1, 'oob'): 0,
    (48, 48, 3, 5, 'null'): 0, (48, 48, 3, 5, 'full'): 0, (48, 48, 3, 5, 'ragged'): 0, (48, 48, 3, 5, 'oob'): 0,
    (48, 48, 12, 1, 'null'): 0, (48, 48, 12, 1, 'full'): 0, (48, 48, 12, 1, 'ragged'): 0, (48, 48, 12, 1, 'oob'): 0,
    (48, 48, 12, 5, 'null'): 0, (48, 48, 12, 5, 'full'): 0, (48, 48, 12, 5, 'ragged'): 0, (48, 48, 12, 5, 'oob'): 0,
}

CASES = [(T, I, H, B, kind) for (T, I) in SHAPES for H in HEADS for B in BATCHES for kind in KINDS]


def case_id(c):
    return "T%d_I%d_H%d_B%d_%s" % c


if __name__ == "__main__":
    for c in CASES:
        print("    %r: %d," % (c, find_seed(*c)))
