"""Float64 references, counted per-element bounds, input families, mutants and the case tables for the LRP relprop kernels: the
attention core of ``csrc/attention_lrp.hip`` (``attn_lrp_q_kernel<32|64>``, ``attn_lrp_kv_kernel<32|64>``) and the nine rule kernels
of ``csrc/lrp_kernels.hip`` behind ``ops.lrp_linear`` / ``lrp_add`` / ``lrp_clone`` / ``lrp_mha_rescale``.  CPU only (numpy), on top of
``tests/rowwise_bounds.py`` and ``tests/attention_bf16_bounds.py`` (imported, not changed): ``tests/test_lrp_bounds_host.py`` proves the
bounds and the mutants here, ``tests/test_gpu_lrp_bounds.py`` holds the kernels to them.

Reference.  Float64 of ``oracle/lrp_torch.core`` and of ``lrp.py``'s formulas on the operands as handed in; the one rounding the
kernels make on an input is applied where they make it: ``A = fp32(q scale)`` in SCALE_Q_FIRST (attention_lrp.hip:83-84 / 149, 162;
SCALE_SCORES: A = q, ``scale`` is not read).  The constant is ``c = fp32(1e-9)``.

``safe_divide(a, b)`` (mmx_common.h) with errors ``e_a``, ``e_b`` on its arguments.  The kernel computes ``den = fl(b + c)``, takes
``c`` when that is 0, then ``fl(a / den)``, and gives 0 where ``b == 0``.  Its bound is an interval, not a first-order truncation:

    e_den = e_b + u (|den| + e_b)
    e_den < |den|:   e_s = (|a| + e_a) / (|den| - e_den) - |a| / |den| + 2 u |s| + 2**-126
    otherwise the element is UNJUDGED (infinite bound); so is one with ``e_b > 0`` and ``|b| <= e_b`` (the ``b == 0`` branch may or
    may not be the one the kernel takes).  An infinite denominator gives an exact 0, and so does ``b == 0`` with ``e_b == 0``.

An unjudged ``S1[i, j]`` makes row i of ``cam_q`` and row j of ``cam_k`` unjudged.

Products.  A dot product of n fp32 terms on the fp32 MFMA or in FMA code, in any order and grouping, errs by at most
``(n + 1) u sum |a b|``; operand errors are carried linearly:

    S     = safe_divide(cam_O, O)                      e_S   = the interval form with e_a = e_b = 0
    dp    = S V^T                                      e_dp  = e_S |V|^T + (D + 1) u |S| |V|^T
    cam_P = P dp / 2                                   e_camP = P e_dp / 2 + 2 u |cam_P|
    cam_V = V (P^T S) / 2                              e_camV = |V| (P^T e_S + (Nq + 1) u P^T |S|) / 2 + 2 u |cam_V|
    Z     = A K^T                                      e_Z   = (D + 1) u |A| |K|^T   (D = 1: the one product's own rounding error)
    S1    = safe_divide(cam_P or cam_scores, Z)        e_S1  = the interval form with (e_camP or 0, e_Z)
    cam_Q = A (S1 K) / 2                               e_camQ = |A| (e_S1 |K| + (Nk + 1) u |S1| |K|) / 2 + 2 u |cam_Q|
    cam_K = K (S1^T A) / 2                             e_camK = |K| (e_S1^T |A| + (Nq + 1) u |S1|^T |A|) / 2 + 2 u |cam_K|

The library GEMMs inside ``lrp_linear`` get the same any-order bound with n = 2 in (Z, whose terms are all >= 0: ``sum |a b| = Z``)
and n = out (Y).

Sums of the Linear normalisation, the Add rule and the q / k rescale.  Counted from the code: a term passes the per-thread trips of
the grid-stride loop (lrp_kernels.hip:77-90, 136-144, 184-188), six shuffle steps and four waves (``block_sum``, :31-44), then
``ceil(nparts / 256)`` partials per lane, six steps and four waves again (``partials_sum``, :105-108):

    n_adds = trips + 6 + 4 + ceil(nparts / 256) + 6 + 4        (= trips + 24 at the 1024-block cap, trips + 21 up to 256 blocks)
    e_sum  = sum e_term + n_adds u sum |term|

never ``N u``.  The ratios ``safe_divide(sum R, sum out)`` etc. go through the interval form; a product of two uncertain factors is
``|x| e_y + |y| e_x + e_x e_y + u |x y|``.  Results below the normal range get ``2**-126``."""
import numpy as np

from attention_bf16_bounds import Q_FIRST, SCORES, TINY, bh, f64
from rowwise_bounds import F32, U
from rowwise_bounds import _ratio as ratio

__all__ = ["Q_FIRST", "SCORES", "F32", "U", "TINY", "ratio"]

EPS = F32(1e-9)
C = float(EPS)
VALUES, SCORES_PHASE = 1, 2                  # _lib.LRP_VALUES / LRP_SCORES
FUSED = VALUES | SCORES_PHASE
THREADS, MAX_BLOCKS = 256, 1024              # kLrpThreads, kLrpMaxBlocks
CAP = THREADS * MAX_BLOCKS                   # 262 144 threads: one trip of the capped grid
QUIET = dict(invalid="ignore", over="ignore", divide="ignore", under="ignore")


def _abt(a, b):
    return np.matmul(a, np.swapaxes(b, -1, -2))


def _atb(a, b):
    return np.matmul(np.swapaxes(a, -1, -2), b)


def back(t):
    """``[B, H, N, D]`` -> ``[B, N, H, D]``."""
    return np.ascontiguousarray(np.transpose(t, (0, 2, 1, 3)))


# ---------------------------------------------------------------------------------------------------------------------
# safe_divide
# ---------------------------------------------------------------------------------------------------------------------
def sd(a, b, e_a=0.0, e_b=0.0, mut=None):
    """Float64 ``safe_divide`` -> ``(s, e_s, unjudged)``.  ``e_s`` is finite (0 where unjudged or where s is not finite)."""
    a, b = np.broadcast_arrays(f64(a), f64(b))
    e_a, e_b = np.broadcast_to(f64(e_a), a.shape), np.broadcast_to(f64(e_b), a.shape)
    with np.errstate(**QUIET):
        den = b + (0.0 if mut == "epsilon_missing" else C)
        den = np.where(den == 0, C, den)
        s = a / den
        if mut != "zero_mask_missing":
            s = np.where(b != 0, s, s * 0.0)
        aden = np.abs(den)
        e_den = e_b + U * (aden + e_b)
        unj = ((e_den >= aden) | ((e_b > 0) & (np.abs(b) <= e_b))) & np.isfinite(den)
        e = tiny((np.abs(a) + e_a) / (aden - e_den) - np.abs(a) / aden + 2 * U * np.abs(s))
        e = np.where(unj | ~np.isfinite(e) | ~np.isfinite(s) | ((b == 0) & (e_b == 0)), 0.0, e)       # b == 0 exactly: an exact zero
    return s, e, unj


def sd32(a, b):
    """The kernels' ``safe_divide`` in numpy fp32, comparison form (a NaN denominator stays NaN)."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(**QUIET):
        den = (np.where(b < EPS, EPS, b) + np.where(b > EPS, EPS, b)).astype(F32)
        den = (den + np.where(den == 0, EPS, F32(0))).astype(F32)
        return ((a / den).astype(F32) * np.where(b != 0, F32(1), F32(0))).astype(F32)


def tiny(bound):
    """``bound + 2**-126`` where the bound is not 0: each form below is 0 only where the kernel's result is exact (a zero factor, an
    all-zero sum), and an exact zero must stay one for the ``b == 0`` branch of the next ``safe_divide``."""
    return bound + TINY * (bound > 0)


def mul_bound(x, e_x, y, e_y):
    return tiny(np.abs(x) * e_y + np.abs(y) * e_x + e_x * e_y + U * np.abs(x * y))


# ---------------------------------------------------------------------------------------------------------------------
# attention core: inputs
# ---------------------------------------------------------------------------------------------------------------------
CORE_FAMILIES = ("randn", "offset", "zeros", "tiny", "eps", "nanrow")
H = 3


def core_inputs(c):
    """The operands of a core case: ``q [B, Nq, H, D]``, ``k v [B, Nk, H, D]``, ``probs [B, H, Nq, Nk]`` (a softmax of the scores),
    ``o = fp32(P V)``, ``cam_o``, ``cam_scores``.  ``offset``: q, k = 3 + randn / 8 (every score far from 0); ``zeros`` (on the offset
    base): an all-zero q row, an all-zero k row, +0 and -0 in ``o``, a zero column of v; ``tiny``: q, k x 2**-20; ``eps`` (D = 1, offset
    base): q = 1 at one query and k = -c at one key, so that their score is -c exactly, and one ``o`` = -c; ``nanrow`` (offset base):
    one NaN in ``o`` of (b, h) = (0, 0) and one NaN in q of the last (b, h)."""
    B, Hh, Nq, Nk, D, fam = c["B"], c["H"], c["Nq"], c["Nk"], c["D"], c["family"]
    g = np.random.default_rng(1000 + c["seed"])
    q, k, v = (g.standard_normal((B, n, Hh, D)).astype(F32) for n in (Nq, Nk, Nk))
    if fam in ("offset", "zeros", "eps", "nanrow"):
        q, k = (q / F32(8) + F32(3)).astype(F32), (k / F32(8) + F32(3)).astype(F32)
    if fam == "tiny":
        q, k = np.ldexp(q, -20).astype(F32), np.ldexp(k, -20).astype(F32)
    iq, ik = Nq // 2, Nk // 2
    if fam == "zeros":
        q[:, iq] = 0.0
        k[:, ik] = 0.0
        v[..., D // 2] = 0.0
    if fam == "eps":
        assert D == 1
        q[:, iq] = 1.0
        k[:, ik] = -EPS
    s = _abt(bh(q), bh(k)) / np.sqrt(D)
    if fam == "tiny":
        s = s * 2.0 ** 40
    e = np.exp(s - s.max(-1, keepdims=True))
    probs = (e / e.sum(-1, keepdims=True)).astype(F32)
    o = back(np.matmul(f64(probs), bh(v))).astype(F32)
    cam_o = (g.standard_normal((B, Nq, Hh, D)) * 0.1).astype(F32)
    cam_scores = (g.standard_normal((B, Hh, Nq, Nk)) * 0.01).astype(F32)
    if fam == "zeros":
        o[:, 0, :, 0] = 0.0
        o[:, Nq - 1, :, D - 1] = -0.0
    if fam == "eps":
        o[:, Nq - 1, 0, 0] = -EPS
    if fam == "nanrow":
        o[0, iq, 0, D // 2] = np.nan
        q[B - 1, Nq - 1, Hh - 1, 0] = np.nan
    return {"q": q, "k": k, "v": v, "probs": probs, "o": o, "cam_o": cam_o, "cam_scores": cam_scores}


def operand_a(q, scale, mode):
    q = np.asarray(q, F32)
    with np.errstate(**QUIET):
        return q if mode == SCORES else (q * F32(scale)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# attention core: reference and restatement
# ---------------------------------------------------------------------------------------------------------------------
CORE_OUT = ("cam_P", "cam_q", "cam_k", "cam_v")


def core_ref(x, scale, mode, phase, with_scores=False, mut=None):
    """Float64 core -> dict of the outputs the phase stores (``cam_P [B, H, Nq, Nk]``; ``cam_q cam_k cam_v [B, N, H, D]``) and their
    bounds ``e_*`` (``inf`` where unjudged).  ``with_scores``: ``cam_scores`` is what the scores phase divides."""
    q, k, v = x["q"], x["k"], x["v"]
    B, Nq, Hh, D = q.shape
    Nk = k.shape[1]
    a32 = operand_a(q, scale, mode)
    if mut == "scale_applied_in_scores_mode" and mode == SCORES:
        a32 = operand_a(q, scale, Q_FIRST)
    A, K, V = bh(a32), bh(k), bh(v)
    out = {}
    values, scores = bool(phase & VALUES), bool(phase & SCORES_PHASE)
    cam_p = e_cam_p = None
    with np.errstate(**QUIET):
        if values or mut == "cam_P_fed_despite_cam_scores":
            S, e_S, _ = sd(bh(x["cam_o"]), bh(x["o"]), mut=mut)
            P = f64(x["probs"])
            dp = _abt(S, V)
            e_dp = _abt(e_S, np.abs(V)) + (D + 1) * U * _abt(np.abs(S), np.abs(V))
            cam_p = P * dp / 2
            e_cam_p = tiny(P * e_dp / 2 + 2 * U * np.abs(cam_p))
        if values:
            nq = 64 * ((Nq - 1) // 64) if mut == "last_query_tile_left_out_on_key_side" else Nq
            cam_v = V * _atb(P[:, :, :nq], S[:, :, :nq]) / 2
            e_cam_v = tiny(np.abs(V) * (_atb(P, e_S) + (Nq + 1) * U * _atb(P, np.abs(S))) / 2 + 2 * U * np.abs(cam_v))
            if mut == "half_missing":
                cam_v = cam_v * 2
            out.update(cam_P=cam_p, e_cam_P=e_cam_p, cam_v=back(cam_v), e_cam_v=back(e_cam_v))
        if scores:
            Az = bh(q) if (mut == "Z_from_unscaled_q" and mode == Q_FIRST) else A
            Kz = np.roll(K, 1, 1) if mut == "neighbouring_heads_k" else K
            Z = _abt(Az, Kz)
            if mut == "padded_lane_not_zeroed":                     # lane D of the padded tile = column 0 of the next head in memory
                Z = Z + np.roll(A, -1, 1)[..., :1] * np.swapaxes(np.roll(K, -1, 1)[..., :1], -1, -2)
            if D == 1:
                e_Z = np.abs(f64(Z.astype(F32)) - Z)
            else:
                e_Z = (D + 1) * U * _abt(np.abs(A), np.abs(K))
            if with_scores and mut != "cam_P_fed_despite_cam_scores":
                cam_s, e_cam_s = f64(x["cam_scores"]), 0.0
            else:
                cam_s, e_cam_s = cam_p, e_cam_p
            S1, e_S1, unj = sd(cam_s, Z, e_cam_s, e_Z, mut=mut)
            nk = {"last_key_left_out": Nk - 1, "last_64_tile_left_out": 64 * ((Nk - 1) // 64)}.get(mut, Nk)
            nq = 64 * ((Nq - 1) // 64) if mut == "last_query_tile_left_out_on_key_side" else Nq
            cam_q = A * np.matmul(S1[..., :nk], K[:, :, :nk]) / 2
            e_cam_q = tiny(np.abs(A) * (np.matmul(e_S1, np.abs(K)) + (Nk + 1) * U * np.matmul(np.abs(S1), np.abs(K))) / 2
                           + 2 * U * np.abs(cam_q))
            cam_k = K * _atb(S1[:, :, :nq], A[:, :, :nq]) / 2
            e_cam_k = tiny(np.abs(K) * (_atb(e_S1, np.abs(A)) + (Nq + 1) * U * _atb(np.abs(S1), np.abs(A))) / 2
                           + 2 * U * np.abs(cam_k))
            if mut == "half_missing" and not values:
                cam_k = cam_k * 2
            e_cam_q = np.where(unj.any(-1)[..., None], np.inf, e_cam_q)
            e_cam_k = np.where(unj.any(-2)[..., None], np.inf, e_cam_k)
            out.update(cam_q=back(cam_q), e_cam_q=back(e_cam_q), cam_k=back(cam_k), e_cam_k=back(e_cam_k))
    return out


def _mm(a, b):
    with np.errstate(**QUIET):
        return np.matmul(np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)).astype(F32)


def mm_groups(a, b, group=4):
    """``a @ b`` in fp32 with the contraction taken in k-groups of 4 (one ``v_mfma_f32_16x16x4_f32`` each) that are accumulated one
    after the other: the 64-key tiles of the kernels are sixteen such groups in a row, on one accumulator."""
    acc = np.zeros(a.shape[:-1] + (b.shape[-1],), F32)
    with np.errstate(**QUIET):
        for t in range(0, a.shape[-1], group):
            acc = (acc + _mm(a[..., t:t + group], b[..., t:t + group, :])).astype(F32)
    return acc


def core_restatement(x, scale, mode, phase, with_scores=False):
    """The core in numpy fp32 in the kernels' order -> dict of fp32 outputs."""
    t = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 1, 3))).astype(F32)
    T = lambda a: np.swapaxes(a, -1, -2)
    A, K, V = t(operand_a(x["q"], scale, mode)), t(x["k"]), t(x["v"])
    half = F32(0.5)
    out = {}
    cam_p = None
    with np.errstate(**QUIET):
        if phase & VALUES:
            S = sd32(t(x["cam_o"]), t(x["o"]))
            P = np.asarray(x["probs"], F32)
            cam_p = ((P * mm_groups(S, T(V))).astype(F32) * half).astype(F32)
            out["cam_P"] = cam_p
            out["cam_v"] = back(((V * mm_groups(T(P), S)).astype(F32) * half).astype(F32))
        if phase & SCORES_PHASE:
            S1 = sd32(np.asarray(x["cam_scores"], F32) if with_scores else cam_p, mm_groups(A, T(K)))
            out["cam_q"] = back(((A * mm_groups(S1, K)).astype(F32) * half).astype(F32))
            out["cam_k"] = back(((K * mm_groups(T(S1), A)).astype(F32) * half).astype(F32))
    return out


def unjudged_share(bound):
    return float(np.isinf(bound).mean())


# ---------------------------------------------------------------------------------------------------------------------
# attention core: mutants and the case table
# ---------------------------------------------------------------------------------------------------------------------
def _scores(c):
    return bool(c["phase"] & SCORES_PHASE)


def _values(c):
    return bool(c["phase"] & VALUES)


CORE_MUTANTS = {
    "last_key_left_out": (("cam_q",), lambda c: _scores(c) and c["Nk"] > 1),
    "last_64_tile_left_out": (("cam_q",), lambda c: _scores(c) and c["Nk"] > 64),
    "last_query_tile_left_out_on_key_side": (("cam_k", "cam_v"), lambda c: c["Nq"] > 64),
    "half_missing": (("cam_k", "cam_v"), lambda c: True),
    "Z_from_unscaled_q": (("cam_q", "cam_k"), lambda c: _scores(c) and c["mode"] == Q_FIRST and c["D"] > 1),
    "scale_applied_in_scores_mode": (("cam_q", "cam_k"), lambda c: _scores(c) and c["mode"] == SCORES and c["family"] == "tiny"),
    "padded_lane_not_zeroed": (("cam_q", "cam_k"), lambda c: _scores(c) and c["D"] not in (32, 64)),
    "neighbouring_heads_k": (("cam_q", "cam_k"), lambda c: _scores(c)),
    "cam_P_fed_despite_cam_scores": (("cam_q", "cam_k"), lambda c: c["phase"] == SCORES_PHASE),
    "epsilon_missing": (("cam_P", "cam_q", "cam_k", "cam_v"), lambda c: c["family"] in ("tiny", "eps")),
    "zero_mask_missing": (("cam_P", "cam_q", "cam_k", "cam_v"), lambda c: c["family"] in ("zeros", "eps")),
}

DIMS = {32: (1, 4, 20, 32), 64: (33, 40, 64)}
SHAPES = ((1, 1), (16, 16), (17, 15), (15, 17), (64, 64), (65, 63), (63, 65), (130, 70), (5, 130), (130, 1), (1, 130))
RAGGED = ((17, 15), (15, 17), (65, 63), (63, 65), (130, 70), (5, 130))
PHASES = (FUSED, VALUES, SCORES_PHASE)
LAYOUTS = ("bnhd", "bhnd", "packed", "padded_o")     # packed: q / k / v are slices of one [B, N, 3, H, D]; padded_o: o, cam_o row stride > H D
SCORES_MODE_SCALE = 0.37                             # SCALE_SCORES never reads it: the bits of scale = 1


def scale_of(c):
    return c["D"] ** -0.5 if c["mode"] == Q_FIRST else SCORES_MODE_SCALE


def stored(c):
    """The outputs a core row stores."""
    return [n for n in CORE_OUT if (_values(c) if n in ("cam_P", "cam_v") else _scores(c))]


def with_scores(c):
    return c["phase"] == SCORES_PHASE


def _core_case(n, Nq, Nk, D, phase, **kw):
    fams = ("offset", "randn", "zeros", "tiny", "nanrow")
    c = {"B": 2, "H": H, "Nq": Nq, "Nk": Nk, "D": D, "phase": phase, "mode": n % 2, "family": fams[n % 5],
         "layout": LAYOUTS[n % 4], "seed": n}
    if D == 1 and n % 3 != 2:
        c["family"] = "eps"
    c.update(kw)
    if c["layout"] == "packed" and Nq != Nk:
        c["layout"] = "bhnd" if n % 8 < 4 else "bnhd"
    c["id"] = "%s-%dx%dx%d-%s-%d" % ({FUSED: "fused", VALUES: "values", SCORES_PHASE: "scores"}[phase], Nq, Nk, D, c["family"], n)
    return c


def core_cases():
    """Every D, every (Nq, Nk), both scale modes, every layout and every family with every (DP, phase): no full cross product."""
    out, n = [], 0
    for dp in (32, 64):
        dims = DIMS[dp]
        for phase in PHASES:
            rows = list(SHAPES) + [SHAPES[(3 * j + dp // 32) % len(SHAPES)] for j in range(13)]
            for i, (Nq, Nk) in enumerate(rows):
                out.append(_core_case(n, Nq, Nk, dims[(i + i // len(dims)) % len(dims)], phase))
                n += 1
    out.append(_core_case(n, 100, 950, 32, FUSED, B=1, H=8, family="randn", mode=Q_FIRST, layout="bnhd"))       # DETR's cross attention
    return out


# ---------------------------------------------------------------------------------------------------------------------
# rules: sums
# ---------------------------------------------------------------------------------------------------------------------
def grid_of(n, cap=MAX_BLOCKS):
    """``lrp_grid``."""
    return int(min(cap, max(1, -(-n // THREADS))))


def trips_of(n, grid):
    return -(-n // (grid * THREADS))


def n_adds(n, grid):
    """The additions a term of an n-element sum passes on a ``grid``-block launch (module docstring)."""
    return trips_of(n, grid) + 6 + 4 + -(-grid // THREADS) + 6 + 4


def sum_ref(x, e_x, grid, mut=None):
    """Float64 sum of the flat ``x`` as the two-stage reduction of a ``grid``-block launch sees it -> ``(sum, e_sum)``."""
    x = f64(x).reshape(-1)
    keep = x
    if mut == "second_trip_dropped_from_sum":
        keep = x[:grid * THREADS]
    elif mut == "partials_beyond_256_dropped":
        keep = x[(np.arange(x.size) // THREADS) % grid < 256]
    with np.errstate(**QUIET):
        s = keep.sum()
        e_terms = float(np.sum(e_x)) if np.ndim(e_x) else float(e_x) * x.size
        e = tiny(e_terms + n_adds(x.size, grid) * U * np.abs(x).sum())
    return s, e


def _block_tree(v):
    """``block_sum``: xor-shuffle steps 32 ... 1 inside each wave of 64, then the four waves in index order.  ``v [..., 256]``."""
    v = v.reshape(v.shape[:-1] + (4, 64))
    with np.errstate(**QUIET):
        w = 64
        while w > 1:
            w //= 2
            v = (v[..., :w] + v[..., w:2 * w]).astype(F32)
        s = np.zeros(v.shape[:-2], F32)
        for i in range(4):
            s = (s + v[..., i, 0]).astype(F32)
    return s


def tree_sum32(x, grid):
    """The two-stage fp32 sum of the rule kernels: thread t of block b adds its elements in trip order, the block tree, then lane t
    adds the partials t, t + 256, ... and the block tree again."""
    x = np.asarray(x, F32).reshape(-1)
    step = grid * THREADS
    trips = max(1, trips_of(x.size, grid))
    pad = np.zeros(trips * step, F32)
    pad[:x.size] = x
    with np.errstate(**QUIET):
        acc = np.zeros(step, F32)
        for t in range(trips):
            acc = (acc + pad[t * step:(t + 1) * step]).astype(F32)
        partial = _block_tree(acc.reshape(grid, THREADS))
        lanes = -(-grid // THREADS)
        p = np.zeros(lanes * THREADS, F32)
        p[:grid] = partial
        acc = np.zeros(THREADS, F32)
        for j in range(lanes):
            acc = (acc + p[j * THREADS:(j + 1) * THREADS]).astype(F32)
        return _block_tree(acc[None])[0]


# ---------------------------------------------------------------------------------------------------------------------
# rules: references and restatements
# ---------------------------------------------------------------------------------------------------------------------
def split_signs(X):
    X = np.asarray(X, F32)
    with np.errstate(**QUIET):
        return np.concatenate((np.where(X < 0, F32(0), X), np.where(X > 0, F32(0), X)), axis=-1)


def combine_ref(XX, Y, e_Y, R, mut=None):
    """``mmx_lrp_linear_combine`` on ``XX Y [rows, 2 n]``: ``out = XX_p Y_p + XX_n Y_n``, times ``safe_divide(sum R, sum out)`` when R
    is given -> ``(out, e_out)``; ``e_out`` is inf everywhere where the ratio is unjudged."""
    XX, Y = f64(XX), f64(Y)
    rows, n = XX.shape[0], XX.shape[1] // 2
    with np.errstate(**QUIET):
        tp, tn = XX[:, :n] * Y[:, :n], XX[:, n:] * Y[:, n:]
        out = tp + tn
        e_Y = np.broadcast_to(f64(e_Y), Y.shape)
        e_out = tiny(np.abs(XX[:, :n]) * e_Y[:, :n] + np.abs(XX[:, n:]) * e_Y[:, n:] + 2 * U * (np.abs(tp) + np.abs(tn)))
        if R is None:
            return out, e_out
        grid = grid_of(rows * n)
        s_out, e_s_out = sum_ref(out, e_out, grid, mut)
        r = f64(R).reshape(-1)
        if mut == "sum_R_over_rows_n_in":
            r = r[:rows * n]
        s_r, e_s_r = sum_ref(r, 0.0, grid)
        kf, e_k, unj = sd(s_r, s_out, e_s_r, e_s_out)
        res = out * kf
        e_res = mul_bound(out, e_out, kf, e_k)
        if unj:
            e_res = np.full_like(e_res, np.inf)
    return res, e_res


def linear_ref(R, X, W, normalize, mut=None):
    """``ops.lrp_linear`` on ``R [rows, out]``, ``X [rows, in]``, ``W [out, in]`` -> ``(out, e_out)``."""
    XX, WW = f64(split_signs(X)), f64(split_signs(W))               # [rows, 2 in], [out, 2 in]
    n_in, n_out = X.shape[1], W.shape[0]
    with np.errstate(**QUIET):
        Z = _abt(XX, WW)                                            # every term >= 0: sum |a b| = Z
        e_Z = (2 * n_in + 1) * U * _abt(np.abs(XX), np.abs(WW))
        S, e_S, unj = sd(f64(R), Z, 0.0, e_Z)
        Y = np.matmul(S, WW)
        e_Y = np.matmul(e_S, np.abs(WW)) + (n_out + 1) * U * np.matmul(np.abs(S), np.abs(WW))
        e_Y = np.where(unj.any(-1)[:, None], np.inf, e_Y)
        out, e_out = combine_ref(XX, Y, np.where(np.isinf(e_Y), 0.0, e_Y), R if normalize else None, mut)
        bad = unj.any(-1)
        if bad.any():
            e_out = np.full_like(e_out, np.inf) if normalize else np.where(bad[:, None], np.inf, e_out)
    return out, e_out


def combine_restatement(XX, Y, R):
    XX, Y = np.asarray(XX, F32), np.asarray(Y, F32)
    rows, n = XX.shape[0], XX.shape[1] // 2
    with np.errstate(**QUIET):
        out = ((XX[:, :n] * Y[:, :n]).astype(F32) + (XX[:, n:] * Y[:, n:]).astype(F32)).astype(F32)
        if R is None:
            return out
        grid = grid_of(rows * n)
        kf = sd32(tree_sum32(R, grid), tree_sum32(out, grid))
        return (out * kf).astype(F32)


def linear_restatement(R, X, W, normalize):
    XX, WW = split_signs(X), split_signs(W)
    S = sd32(R, _mm(XX, WW.T))
    return combine_restatement(XX, _mm(S, WW), R if normalize else None)


def _share_chain(sa, e_sa, sb, e_sb, tot, e_tot):
    """``x_a = safe_divide(|s_a| / (|s_a| + |s_b|) tot, s_a)`` and ``x_b`` likewise -> ``((x_a, e_a, unj_a), (x_b, e_b, unj_b))``."""
    with np.errstate(**QUIET):
        den = np.abs(sa) + np.abs(sb)
        e_den = e_sa + e_sb + U * den
        res = []
        for s, e_s in ((sa, e_sa), (sb, e_sb)):
            r1, e_r1, u1 = sd(np.abs(s), den, e_s, e_den)
            f = r1 * tot
            e_f = mul_bound(r1, e_r1, tot, e_tot)
            xf, e_x, u2 = sd(f, s, e_f, e_s)
            res.append((xf, e_x, u1 | u2))
    return res


def _add_split(R, a, b):
    """The first half of the Add rule on one sample -> ``(ra, e_ra, rb, e_rb, any unjudged)``."""
    R, a, b = f64(R), f64(a), f64(b)
    ab = a + b
    s, e_s, unj = sd(R, ab, 0.0, U * np.abs(ab))
    ra, rb = a * s, b * s
    return ra, tiny(np.abs(a) * e_s + U * np.abs(ra)), rb, tiny(np.abs(b) * e_s + U * np.abs(rb)), bool(unj.any())


def add_ref(R, a, b, batch, mut=None):
    """``ops.lrp_add`` on flat ``[batch, per]`` operands -> ``(ra, e_ra, rb, e_rb)``; a sample whose ratios are unjudged is inf."""
    R, a, b = (np.asarray(t).reshape(batch, -1) for t in (R, a, b))
    grid = grid_of(R.shape[1])
    out_a, out_b, be_a, be_b = (np.empty(R.shape) for _ in range(4))
    with np.errstate(**QUIET):
        whole = None
        if mut == "sample_sums_over_whole_batch":
            ra, e_ra, rb, e_rb, _ = _add_split(R, a, b)
            whole = [sum_ref(ra, e_ra, grid), sum_ref(rb, e_rb, grid), sum_ref(R, 0.0, grid)]
        for i in range(batch):
            ra, e_ra, rb, e_rb, unj = _add_split(R[i], a[i], b[i])
            sums = whole or [sum_ref(ra, e_ra, grid, mut), sum_ref(rb, e_rb, grid, mut), sum_ref(R[i], 0.0, grid, mut)]
            (xa, e_xa, ua), (xb, e_xb, ub) = _share_chain(sums[0][0], sums[0][1], sums[1][0], sums[1][1], sums[2][0], sums[2][1])
            out_a[i], out_b[i] = ra * xa, rb * xb
            be_a[i] = np.inf if (ua or unj) else mul_bound(ra, e_ra, xa, e_xa)
            be_b[i] = np.inf if (ub or unj) else mul_bound(rb, e_rb, xb, e_xb)
    return out_a, be_a, out_b, be_b


def add_restatement(R, a, b, batch):
    R, a, b = (np.asarray(t, F32).reshape(batch, -1) for t in (R, a, b))
    grid = grid_of(R.shape[1])
    with np.errstate(**QUIET):
        s = sd32(R, (a + b).astype(F32))
        ra, rb = (a * s).astype(F32), (b * s).astype(F32)
        for i in range(batch):
            sa, sb, tot = (tree_sum32(t[i], grid) for t in (ra, rb, R))
            den = (np.abs(sa) + np.abs(sb)).astype(F32)
            fa, fb = (sd32(np.abs(sa), den) * tot).astype(F32), (sd32(np.abs(sb), den) * tot).astype(F32)
            ra[i], rb[i] = (ra[i] * sd32(fa, sa)).astype(F32), (rb[i] * sd32(fb, sb)).astype(F32)
    return ra, rb


def clone_ref(Rs, X, mut=None):
    """``ops.lrp_clone``: ``X sum_i safe_divide(R_i, X)`` -> ``(out, e_out)``."""
    X = f64(X)
    Rs = list(Rs)[:7] if (mut == "eighth_clone_input_dropped" and len(Rs) == 8) else list(Rs)
    with np.errstate(**QUIET):
        c, e_c, mag = 0.0, 0.0, 0.0
        for r in Rs:
            s, e_s, _ = sd(f64(r), X)
            c, e_c, mag = c + s, e_c + e_s, mag + np.abs(s)
        e_c = e_c + (len(Rs) - 1) * U * mag
        out = X * c
        e_out = tiny(np.abs(X) * e_c + U * np.abs(out))
    return out, e_out


def clone_restatement(Rs, X):
    X = np.asarray(X, F32)
    with np.errstate(**QUIET):
        c = sd32(Rs[0], X)
        for r in Rs[1:]:
            c = (c + sd32(r, X)).astype(F32)
        return (X * c).astype(F32)


def rescale_grid(sizes):
    return grid_of(max(sizes), cap=256)


def rescale_taken(v_pre, v_post, mut=None):
    """``all_zero(v_post) & ~all_zero(v_pre)``: -0 is zero, a NaN is not."""
    v_pre, v_post = np.asarray(v_pre), np.asarray(v_post)
    pre_nonzero = bool((v_pre != 0).any())
    if mut == "nan_counted_as_zero":
        pre_nonzero = bool(((v_pre != 0) & ~np.isnan(v_pre)).any())
    if mut == "rescale_when_v_pre_all_zero":
        pre_nonzero = True
    return bool((v_post == 0).all()) and pre_nonzero


def rescale_ref(v_pre, v_post, cam_k, cam_q, cam_o, mut=None):
    """``ops.lrp_mha_rescale`` -> ``(taken, cam_k, e_k, cam_q, e_q)``; not taken: the inputs' own values and zero bounds."""
    k, q, o = f64(cam_k), f64(cam_q), f64(cam_o)
    if not rescale_taken(v_pre, v_post, mut):
        return False, k, np.zeros_like(k), q, np.zeros_like(q)
    grid = rescale_grid([np.size(t) for t in (v_pre, v_post, cam_k, cam_q, cam_o)])
    (sk, e_sk), (sq, e_sq), (so, e_so) = (sum_ref(t, 0.0, grid) for t in (k, q, o))
    (xk, e_xk, uk), (xq, e_xq, uq) = _share_chain(sk, e_sk, sq, e_sq, so, e_so)
    with np.errstate(**QUIET):
        e_k = np.full_like(k, np.inf) if uk else mul_bound(k, 0.0, xk, e_xk)
        e_q = np.full_like(q, np.inf) if uq else mul_bound(q, 0.0, xq, e_xq)
        return True, k * xk, e_k, q * xq, e_q


def rescale_restatement(v_pre, v_post, cam_k, cam_q, cam_o):
    k, q = np.asarray(cam_k, F32).copy(), np.asarray(cam_q, F32).copy()
    if not rescale_taken(v_pre, v_post):
        return k, q
    grid = rescale_grid([np.size(t) for t in (v_pre, v_post, cam_k, cam_q, cam_o)])
    sk, sq, so = (tree_sum32(t, grid) for t in (k, q, cam_o))
    with np.errstate(**QUIET):
        den = (np.abs(sk) + np.abs(sq)).astype(F32)
        kf, qf = (sd32(np.abs(sk), den) * so).astype(F32), (sd32(np.abs(sq), den) * so).astype(F32)
        return (k * sd32(kf, sk)).astype(F32), (q * sd32(qf, sq)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# rules: inputs, mutants and the case table
# ---------------------------------------------------------------------------------------------------------------------
RULE_FAMILIES = ("positive", "signed", "special")
COUNTS = ((1, 1), (15, 17), (1, 257), (513, 511), (4096, 64), (4033, 65), (6169, 85))       # rows x n = 1, 255, 257, 2**18 - 1, 2**18,
#                                                                                             2**18 + 1, 2 * 2**18 + 77
LINEAR_SHAPES = ((1, 1, 1), (15, 12, 7), (128, 512, 1024), (129, 512, 8), (128, 516, 8), (2049, 128, 8))
ADD_PER = (1, 257, CAP + 1)
ADD_BATCH = (1, 2, 64)
CLONE_INPUTS = (1, 2, 7, 8)
SUBNORMAL = F32(2.0 ** -140)


def _relevance(g, shape, family):
    r = (g.standard_normal(shape) * 0.05).astype(F32)
    return np.abs(r) if family == "positive" else r


def specials(t, g, with_inf=True):
    """A subnormal, an inf and a NaN at three distinct places of the flat ``t`` (as many as fit)."""
    flat = t.reshape(-1)
    at = g.choice(flat.size, size=min(3, flat.size), replace=False)
    for i, val in zip(at, (SUBNORMAL, F32(np.nan), F32(np.inf) if with_inf else SUBNORMAL)):
        flat[i] = val


def rule_inputs(c):
    """The operands of a rule case.  Every family: exact zeros on both sides of the sign split (column 0 of X), an all-zero row of X,
    ``a + b == 0`` at some elements.  ``positive``: R > 0 (the ratios are well conditioned: conservation makes the sums agree);
    ``signed``: R of both signs; ``special``: signed plus a subnormal, an inf and a NaN element."""
    g = np.random.default_rng(5000 + c["seed"])
    fam, kind = c["family"], c["kind"]
    if kind == "combine":
        rows, n = c["rows"], c["n"]
        XX = split_signs(g.standard_normal((rows, n)).astype(F32))
        Y = np.abs(g.standard_normal((rows, 2 * n))).astype(F32) * np.where(XX < 0, F32(-1), F32(1))    # XX Y >= 0, as in the rule
        if fam != "positive":
            Y = (Y * np.sign(g.standard_normal((rows, 2 * n))).astype(F32)).astype(F32)
        XX[rows // 2] = 0.0
        R = _relevance(g, (rows, c["m"]), fam)
        if fam == "special":
            specials(Y, g, with_inf=False)
        return {"XX": XX, "Y": Y, "R": R}
    if kind == "linear":
        rows, n_in, n_out = c["rows"], c["n_in"], c["n_out"]
        X = g.standard_normal((rows, n_in)).astype(F32)
        X[:, 0] = 0.0
        X[rows // 2] = 0.0
        W = (g.standard_normal((n_out, n_in)) * 0.1).astype(F32)
        W.reshape(-1)[::7] = 0.0
        R = _relevance(g, (rows, n_out), fam)
        if fam == "special":
            X[0, n_in - 1] = SUBNORMAL
            R[0, 0] = SUBNORMAL
            if rows > 2:
                X[rows - 1, n_in // 2] = np.nan
        return {"R": R, "X": X, "W": W}
    if kind == "add":
        shape = (c["batch"], c["per"])
        a, b = g.standard_normal(shape).astype(F32), g.standard_normal(shape).astype(F32)
        R = _relevance(g, shape, fam)
        if fam == "positive":
            a, b = np.abs(a), np.abs(b)
        b[:, ::5] = -a[:, ::5]                                      # a + b == 0
        a[:, ::11] = 0.0
        if c["per"] > 3:
            b[:, 3] = -EPS - a[:, 3]                                # a + b == -c (where fp32 can hold it): den == 0
        if fam == "special":
            for t in (a, b, R):
                specials(t[c["batch"] - 1], g)
        return {"R": R, "a": a, "b": b}
    if kind == "clone":
        X = g.standard_normal(c["n"]).astype(F32)
        X[::9] = 0.0
        X[1::9] = -EPS
        Rs = [_relevance(g, c["n"], fam) for _ in range(c["inputs"])]
        if fam == "special":
            specials(X, g)
            specials(Rs[-1], g)
        return {"X": X, "Rs": Rs}
    if kind == "rescale":
        sizes = c["sizes"]
        v_pre, v_post, cam_k, cam_q, cam_o = (_relevance(g, n, fam) for n in sizes)
        if c["branch"] != "post_nonzero":
            v_post[:] = 0.0
            v_post[::3] = -0.0
        if c["branch"] == "pre_zero":
            v_pre[:] = 0.0
        if c["branch"] == "pre_nan":
            v_pre[:] = 0.0
            v_pre[sizes[0] // 2] = np.nan
        return {"v_pre": v_pre, "v_post": v_post, "cam_k": cam_k, "cam_q": cam_q, "cam_o": cam_o}
    raise KeyError(kind)


def sum_len(c):
    """The number of terms of a row's longest two-stage sum (0: the row sums nothing)."""
    if c["kind"] == "combine":
        return c["rows"] * c["n"] if c["m"] else 0
    if c["kind"] == "add":
        return c["per"] if c["per_sample"] else c["batch"] * c["per"]
    return 0


def add_batch(c):
    return c["batch"] if c["per_sample"] else 1


RULE_MUTANTS = {
    "second_trip_dropped_from_sum": lambda c: sum_len(c) > CAP and c["family"] == "positive",
    "partials_beyond_256_dropped": lambda c: sum_len(c) > 256 * THREADS and c["family"] == "positive",
    "sum_R_over_rows_n_in": lambda c: c["family"] == "positive" and (c["kind"] == "combine" and c["m"] > c["n"]
                                                                      or c["kind"] == "linear" and c["normalize"] and c["n_out"] > c["n_in"]),
    "sample_sums_over_whole_batch": lambda c: c["kind"] == "add" and add_batch(c) > 1 and c["family"] == "positive",
    "eighth_clone_input_dropped": lambda c: c["kind"] == "clone" and c["inputs"] == 8,
    "rescale_when_v_pre_all_zero": lambda c: c["kind"] == "rescale" and c["branch"] == "pre_zero",
    "nan_counted_as_zero": lambda c: c["kind"] == "rescale" and c["branch"] == "pre_nan",
}


def rule_cases():
    out, n = [], 0

    def add(kind, **kw):
        nonlocal n
        c = dict(kind=kind, seed=n, family=RULE_FAMILIES[n % 3])
        c.update(kw)
        c["id"] = "%s-%d-%s" % (kind, n, c["family"])
        out.append(c)
        n += 1

    for rows, nn in COUNTS:                                         # mmx_lrp_linear_combine on an arena, normalise on and off
        for fam in ("positive", "signed"):
            add("combine", rows=rows, n=nn, m=nn + 3, family=fam)
        add("combine", rows=rows, n=nn, m=0, family="special")
    for rows, n_in, n_out in LINEAR_SHAPES:
        for normalize in (True, False):
            for fam in (("positive", "signed") if normalize else ("signed", "special")):
                add("linear", rows=rows, n_in=n_in, n_out=n_out, normalize=normalize, family=fam)
    for batch in ADD_BATCH:                                         # per sample; the largest (64 x (2**18 + 1)) in one family only
        for per in ADD_PER:
            for fam in (RULE_FAMILIES if batch * per <= 4 * CAP else ("positive",)):
                add("add", batch=batch, per=per, per_sample=True, family=fam)
    for batch, per in ((2, 257), (2, CAP + 1), (64, 257), (3, CAP)):       # whole tensor: one sample of batch x per elements
        for fam in ("positive", "signed"):
            add("add", batch=batch, per=per, per_sample=False, family=fam)
    for inputs in CLONE_INPUTS:
        for nn, fam in ((1, "signed"), (257, "special"), (CAP + 1, "positive")):
            add("clone", inputs=inputs, n=nn, family=fam)
    sizes = (1000, 257, 3 * 65536 + 5, 70000, 4097)                 # v_pre, v_post, cam_k (three trips of the 256-block grid), cam_q, cam_o
    for branch in ("taken", "pre_zero", "pre_nan", "post_nonzero"):
        for fam in ("positive", "signed"):
            add("rescale", sizes=sizes, branch=branch, family=fam)
    add("rescale", sizes=(1, 1, 1, 1, 1), branch="taken", family="positive")
    return out


def rule_ref(c, x, mut=None):
    """-> dict name -> ``(value, bound)`` of a rule case."""
    kind = c["kind"]
    if kind == "combine":
        out, e = combine_ref(x["XX"], x["Y"], 0.0, x["R"] if c["m"] else None, mut)
        return {"out": (out, e)}
    if kind == "linear":
        out, e = linear_ref(x["R"], x["X"], x["W"], c["normalize"], mut)
        return {"out": (out, e)}
    if kind == "add":
        ra, ea, rb, eb = add_ref(x["R"], x["a"], x["b"], add_batch(c), mut)
        return {"ra": (ra, ea), "rb": (rb, eb)}
    if kind == "clone":
        out, e = clone_ref(x["Rs"], x["X"], mut)
        return {"out": (out, e)}
    _taken, k, ek, q, eq = rescale_ref(x["v_pre"], x["v_post"], x["cam_k"], x["cam_q"], x["cam_o"], mut)
    return {"cam_k": (k, ek), "cam_q": (q, eq)}


def rule_restatement(c, x):
    kind = c["kind"]
    if kind == "combine":
        return {"out": combine_restatement(x["XX"], x["Y"], x["R"] if c["m"] else None)}
    if kind == "linear":
        return {"out": linear_restatement(x["R"], x["X"], x["W"], c["normalize"])}
    if kind == "add":
        ra, rb = add_restatement(x["R"], x["a"], x["b"], add_batch(c))
        return {"ra": ra, "rb": rb}
    if kind == "clone":
        return {"out": clone_restatement(x["Rs"], x["X"])}
    k, q = rescale_restatement(x["v_pre"], x["v_post"], x["cam_k"], x["cam_q"], x["cam_o"])
    return {"cam_k": k, "cam_q": q}


# the special-value table of safe_divide: every pair (a, b) of these
SPECIALS = (0.0, -0.0, 1.0, -1.0, float(EPS), -float(EPS), 2e-9, -2e-9, float(SUBNORMAL), -float(SUBNORMAL), 2.0 ** -126, 3.0e38,
            -3.0e38, 1e-30, 0.1, float("inf"), float("-inf"), float("nan"))


def special_pairs():
    a, b = np.meshgrid(np.array(SPECIALS, F32), np.array(SPECIALS, F32), indexing="ij")
    return a.reshape(-1).copy(), b.reshape(-1).copy()
