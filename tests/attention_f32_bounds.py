"""Float64 references, counted rounding bounds, input families, mutants and the case table for the EXACT-fp32 attention kernels: the
whole-head kernels of ``csrc/attention_head.hip``, the streaming kernels of ``csrc/attention_stream.hip`` (``attn_fwd_stream_kernel``,
the small-grid ``attn_fwd_split_kernel``, the one-sweep ``attn_fwd_stream1_kernel``, ``attn_bwd_q_stream_kernel`` /
``attn_bwd_kv_stream_kernel`` without ``MM``) and the tiled kernels of ``csrc/attention_kernels.hip``.  CPU only (numpy), on top of
``tests/attention_bf16_bounds.py`` and ``tests/rowwise_bounds.py`` (imported, not changed): ``tests/test_attention_f32_bounds_host.py``
proves the bounds and the mutants here, ``tests/test_gpu_attention_f32.py`` holds the kernels to them.

Reference.  Float64 of the kernels' DEFINITION on the operands as handed in; the one rounding the kernels make on an input is applied
where they make it (``scale`` is the fp32 number the C ABI receives):

    forward   A = fp32(q scale)  (SCALE_Q_FIRST: attention_head.hip:135/349, attention_stream.hip:99/272, attention_kernels.hip:27/52)
              or  q  (SCALE_SCORES: S is divided by ``scale`` after the product: head:397, stream:296, tiled:69)
              S = A K^T (/ scale) (+ mask),  P = softmax(S),  O = P V          (a fully masked row: NaN in P and O, as torch.softmax)
    backward  a function of (q, k, v, slab P, dO, optional O)
              dP = dO V^T
              delta = rowsum(dO O) where the kernel takes it from O -- the streaming query side only, attention_stream.hip:760-777;
                      sum_k P dP everywhere else (stream:779-802, head:522-528/563 and tiled:176-185 never read O)
              dS = P (dP - delta) m          m = 1, or 1 / scale in SCALE_SCORES
              dQ = (dS K) (scale or 1),   dK = dS^T A,   dV = P^T dO
              row mode:  rel_out = rel + (1 / H) sum_h sum_q rel[q] max(P dP, 0)[q, key]
              shared forward (one q / k / v / P for every dO) and grouped row mode (target t explains image t % M): the same per
              target on the operands of its image

Bounds, per element, to first order in ``u = 2**-24``.  No operand is re-rounded, so every output is in the exact-operand class of
the bf16 module: no boundary allowances, no flagged shares.  A dot product of n fp32 terms on the fp32 MFMA or in FMA code errs by at
most ``(n + 1) u sum |a_i b_i|`` in any order and grouping (zeros of the padding add nothing).

* ``S``: ``e_S = u ((D + 1) sum_d |A K| (/ scale) + |S_unmasked| [SCORES: the division] + |S| [mask: its addition])``.
* ``P = exp(S - max) / sum``.  The maximum is an exact selection among the computed scores and cancels between numerator and sum.  With
  ``x = S - max``, every family:  ``e_P = P (e_S + sum_j P_j e_S[j] + u (cx |x| + cx sum_j P_j |x_j| + cP)) + 2**-126``.
  - whole-head (head:390-422): the subtraction ``u |x|``; ``exp_fast`` (head:46) = v_exp_f32 of ``x log2(e)``: the product ``u |x|``,
    the fp32 constant's own error ``0.23 u |x|`` and v_exp_f32's 1 ulp ``2 u`` -- ``cx = 2.25``.  The sum passes ``4 NTK`` in-lane
    additions (head:405-413) and the two of the four-row all-reduce (head:56-64); then ``1 / sum`` (head:415) and one product (head:420):
    ``cP = 2 + 1 [numerator] + 2 + 4 NTK + 2 + 1 [sum] = 4 NTK + 8``, ``NTK = ceil(Nk / 16)``.
  - streaming (stream:304-337 / 572-623, then 343-356 / 640-651), ``nt = ceil(Nk / 64)``: a term of the sum is taken relative to a
    running maximum and rescaled once per tile and once at the merge (the split kernel: per wave, then across the four waves) by
    ``exp_fast(old - new)``; the exponents of these factors add up to ``x`` (``cx = 2.25`` again), each of at most ``nt + 1`` factors
    costs its ``exp_fast`` (2) and its product (1), the term passes at most ``4 nt + 8`` additions; then the reciprocal and the
    product:  ``cP = 2 + 1 + 2 + 3 (nt + 1) + 4 nt + 8 + 1 = 7 nt + 17``.
  - tiled (kernels:78-103): ``expf`` (1 ulp: 2 u) of the rounded difference -- ``cx = 1``; a lane adds ``nt`` terms, six shuffle steps,
    one division:  ``cP = 2 + 1 + 2 + nt + 6 = nt + 11``.
* ``O``: ``e_O = sum_k e_P |V| + (Nk + 1) u sum_k |P V|``.  The one-sweep no-slab forward (stream:434-485) never forms P: the
  unnormalised terms and O are rescaled per tile (``3 nt``), the row sum is ``5 nt + 4`` additions away and O is multiplied by its
  reciprocal at the end: the same form with ``cP = 11 nt + 11`` and ``Nk + 3`` for ``Nk + 1``.
* ``dP``: ``(D + 1) u sum_d |dO V|``.   ``dV``: ``(Nq + 1) u sum_q |P dO|``.
* ``delta`` from O: ``(D + 1) u sum_d |dO O|``; by the sweep: ``sum_k P e_dP + (Nk + 1) u sum_k |P dP|``.
* ``e_dS = P m (e_dP + e_delta) + 4 u |dS|``  (the subtraction, the product, the division -- stream:809/829: the rounded reciprocal
  and its product).
* ``e_dQ = (sum_k e_dS |K| + (Nk + 1) u sum_k |dS K|) (scale or 1) + u |dQ| [Q_FIRST]``,
  ``e_dK = sum_q e_dS |A| + (Nq + 1) u sum_q |dS A|``.
* ``rel_out``: a term ``rel[q] max(P dP, 0)`` carries ``|rel[q]| (P e_dP + u |P dP|)`` and its own product; it passes ``n_rel``
  additions -- whole-head (head:538-546, kernels:478-487): 4 on DPP, ``ceil(Nq / 16)`` waves, H heads; streaming (stream:733-741,
  817-820): 4, 16 partial rows, ``H ceil(Nq / 64)`` rows -- the rounded ``1 / H`` and its product, the final addition:
  ``e_rel = (1 / H) sum_h sum_q |rel[q]| (P e_dP + (n_rel + 4) u |P dP|) + u |rel_out|``.

Results below the normal range get the ``2**-126`` term the bf16 module uses.  The bounds rest on three hardware properties that are
taken from the comments at ``attention_stream.hip:37-40`` and the vendor's documentation, not measured here: v_exp_f32's 1 ulp, the
fp32 MFMA rounding each product and each addition to nearest, and its keeping subnormal operands and results."""
import numpy as np

from attention_bf16_bounds import Q_FIRST, SCORES, TINY, bh, f64, inputs, judge, make_mask, passes, ratio, rne_bf16, scale_of
from rowwise_bounds import F32, U

__all__ = ["Q_FIRST", "SCORES", "TINY", "F32", "U", "bh", "judge", "passes", "ratio", "scale_of"]

FAMILIES = ("randn", "peaked", "small", "poscode", "underflow")
MASKS = ("none", "causal", "keypad", "rowmasked")
H = 3
LOG2E = F32(1.4426950408889634)


def _abt(a, b):
    return np.matmul(a, np.swapaxes(b, -1, -2))


def _atb(a, b):
    return np.matmul(np.swapaxes(a, -1, -2), b)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def family_inputs(family, Bq, B, Nq, Nk, D, seed=0):
    """``attention_bf16_bounds.inputs`` (seeded ``randn`` / ``peaked``: q and k x 4) and on top of it ``small`` (every operand
    x 2**-20, exactly), ``poscode`` (q and k = 3 + randn / 8: a shared offset, every score near 9 sqrt(D)) and ``underflow`` (plain
    operands; its mask does the work, see ``mask_of``)."""
    x = inputs("peaked" if family == "peaked" else "randn", Bq, B, H, Nq, Nk, D, seed)
    if family == "small":
        for n in ("q", "k", "v", "dO"):
            x[n] = np.ldexp(x[n], -20).astype(F32)
    elif family == "poscode":
        for n in ("q", "k"):
            x[n] = (x[n] / F32(8) + F32(3)).astype(F32)
    return x


def mask_of(kind, family, Bq, Nq, Nk):
    """The additive mask of a case.  ``underflow`` (the family) overrides the kind: a key-padding mask ``[B, 1, Nk]`` of -10000 on all
    but the LAST 3 + b keys of sample b.  ``keypad`` is the bf16 module's plus a soft bias of -3 on key 0."""
    if family == "underflow":
        m = np.zeros((Bq, 1, Nk), F32)
        for b in range(Bq):
            m[b, 0, :max(0, Nk - 3 - b)] = -10000.0
        return m
    m = make_mask(kind, Bq, Nq, Nk)
    if kind == "keypad" and Nk > 2:
        m[:, 0, 0] = -3.0
    return m


def _mask4(mask):
    if mask is None:
        return None
    m = f64(mask)
    return m[None, None] if m.ndim == 2 else m[:, None]


def operand_a(q, scale, mode):
    q = np.asarray(q, F32)
    return q if mode == SCORES else (q * F32(scale)).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def fwd_consts(route, Nk):
    """``(cx, cP, cO)`` of a kernel family (module docstring)."""
    nt, ntk = -(-Nk // 64), -(-Nk // 16)
    return {"head": (2.25, 4 * ntk + 8, Nk + 1), "stream": (2.25, 7 * nt + 17, Nk + 1), "split": (2.25, 7 * nt + 17, Nk + 1),
            "stream1": (2.25, 11 * nt + 11, Nk + 3), "tiled": (1.0, nt + 11, Nk + 1)}[route]


def _d_padded(c):
    return c["D"] % 16 != 0


def fwd_ref(q, k, v, scale, mode, mask, route, mut=None):
    """Float64 forward on ``q [B, Nq, H, D]``, ``k v [B, Nk, H, D]`` -> dict of ``P [B, H, Nq, Nk]``, ``O [B, Nq, H, D]`` and the
    bounds ``e_P e_O`` of the kernel family ``route``."""
    B, Nq, Hh, D = q.shape
    Nk = k.shape[1]
    sc = float(F32(scale))
    A = bh(operand_a(q, scale, mode))
    if mut == "scale_rounded_to_bf16":
        sc = float(rne_bf16(np.array([scale], F32))[0])
    if mut == "scale_slip_1e-6":
        sc = sc * (1 + 1e-6)
    if mut in ("scale_rounded_to_bf16", "scale_slip_1e-6") and mode == Q_FIRST:
        A = bh(q) * sc
    K, V = bh(k), bh(v)
    raw = _abt(A, K)
    if mut == "padded_column":                                      # lane D of the padded tile = column 0 of the next head in memory
        raw = raw + np.roll(A, -1, 1)[..., :1] * np.swapaxes(np.roll(K, -1, 1)[..., :1], -1, -2)
    absraw = _abt(np.abs(A), np.abs(K))
    m4 = _mask4(mask)
    if m4 is not None and mut == "mask_row_off_by_one" and m4.shape[2] > 1:
        m4 = m4[:, :, np.minimum(np.arange(Nq) + 1, Nq - 1)]
    if m4 is not None and mut == "mask_of_sample_0":
        m4 = m4[:1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        S0 = raw / sc if mode == SCORES else raw
        if m4 is not None and mut == "mask_before_division" and mode == SCORES:
            S = (raw + m4) / sc
        else:
            S = S0 if m4 is None else S0 + m4
        mx = S[..., :16].max(-1, keepdims=True) if mut == "max_over_first_tile" else S.max(-1, keepdims=True)
        x = S - mx                                                  # a fully masked row: -inf - -inf = NaN, like torch.softmax
        E = np.exp(x * (1 + 2.0 ** -20)) if mut == "exp_slope_off_2**-20" else np.exp(x)
        if mut == "max_over_first_tile":
            E = np.where(x > 88.72, np.inf, E)                      # fp32's exp overflows there
        if mut == "last_key_left_out_of_sum":
            den = E[..., :-1].sum(-1, keepdims=True)
        elif mut == "last_tile_left_out_of_sum":
            den = E[..., :16 * ((Nk - 1) // 16)].sum(-1, keepdims=True)
        else:
            den = E.sum(-1, keepdims=True)
        P = E / den
        cx, cP, cO = fwd_consts(route, Nk)
        live = P > 0
        e_S = U * ((D + 1) * absraw * (1.0 / sc if mode == SCORES else 1.0) + (np.abs(S0) if mode == SCORES else 0.0)
                   + (np.abs(S) if m4 is not None else 0.0))
        e_S = np.where(live, e_S, 0.0)
        ax = np.where(live, np.abs(x), 0.0)
        e_P = P * (e_S + (P * e_S).sum(-1, keepdims=True) + U * (cx * ax + cx * (P * ax).sum(-1, keepdims=True) + cP)) + TINY
        Vo = np.roll(V, -1, 1) if mut == "O_reads_next_head_of_V" else V
        if mut == "O_without_last_key":
            O = np.matmul(P[..., :-1], Vo[..., :-1, :])
        else:
            O = np.matmul(P, Vo)
        e_O = np.matmul(e_P, np.abs(V)) + U * cO * np.matmul(np.abs(P), np.abs(V)) + TINY
    return {"S": S, "P": P, "O": np.transpose(O, (0, 2, 1, 3)), "e_P": e_P, "e_O": np.transpose(e_O, (0, 2, 1, 3))}


# ---- fp32 restatements: numpy float32, each family's own order of operations -------------------------------------------
def _mm(a, b):
    return np.matmul(np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)).astype(F32)


def _mm_tiles(a, b, tile=64):
    """``a @ b`` with the contraction cut into ``tile``-wide pieces that are accumulated one after the other in fp32."""
    n = a.shape[-1]
    acc = np.zeros(a.shape[:-1] + (b.shape[-1],), F32)
    for t in range(0, n, tile):
        acc = (acc + _mm(a[..., t:t + tile], b[..., t:t + tile, :])).astype(F32)
    return acc


def exp_fast32(x):
    """``exp_fast`` of the kernels: fp32 2**(x log2 e)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.exp2((np.asarray(x, F32) * LOG2E).astype(F32)).astype(F32)


def seqsum(x, axis=-1):
    """One fp32 accumulator, the terms added one after the other."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.take(np.cumsum(x, axis=axis, dtype=F32), -1, axis=axis)


def _tree(x):
    """Pairwise fp32 sum of the last axis (a power of two: the lanes of a DPP / shuffle reduction)."""
    with np.errstate(invalid="ignore", over="ignore"):
        while x.shape[-1] > 1:
            x = (x[..., 0::2] + x[..., 1::2]).astype(F32)
    return x


def _pad(x, mult, fill):
    n = x.shape[-1]
    out = np.full(x.shape[:-1] + (-(-n // mult) * mult,), fill, F32)
    out[..., :n] = x
    return out


def head_rowsum(X):
    """The whole-head kernels' row sum: lane group g adds its keys 16 t + 4 g + r in the order (t, r), then the four groups are added
    in two steps -> ``[..., 1]``."""
    X = _pad(X, 16, 0.0)
    ntk = X.shape[-1] // 16
    X = np.moveaxis(X.reshape(X.shape[:-1] + (ntk, 4, 4)), -2, -3).reshape(X.shape[:-1] + (4, ntk * 4))
    return _tree(seqsum(X))


def lanes_rowsum(X, lanes):
    """``lanes`` lanes, lane i adding the elements i, i + lanes, ... one after the other, then a tree over the lanes -> ``[..., 1]``."""
    X = _pad(X, lanes, 0.0)
    return _tree(seqsum(X.reshape(X.shape[:-1] + (X.shape[-1] // lanes, lanes)), axis=-2))


def fwd_restatement(q, k, v, scale, mode, mask, route):
    """The forward in numpy fp32 in the order of the kernel family ``route`` -> ``(P or None, O)``: ``head`` one maximum, sequential
    in-lane sums and a tree; ``tiled`` 64 lanes and ``expf``; ``stream`` / ``split`` 64-key tiles with a lane-local running maximum and
    rescaling; ``stream1`` one sweep in which O itself is rescaled."""
    t = lambda x: np.ascontiguousarray(np.transpose(x, (0, 2, 1, 3)))
    A, K, V = t(operand_a(q, scale, mode)), t(np.asarray(k, F32)), t(np.asarray(v, F32))
    Nk = K.shape[-2]
    ninf = F32(-np.inf)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        S = _mm(A, np.swapaxes(K, -1, -2))
        if mode == SCORES:
            S = (S / F32(scale)).astype(F32)
        m4 = _mask4(mask)
        if m4 is not None:
            S = (S + m4.astype(F32)).astype(F32)
        if route == "head":
            E = exp_fast32(S - S.max(-1, keepdims=True))
            P = (E * (F32(1) / head_rowsum(E)).astype(F32)).astype(F32)
            O = _mm(P, V)
        elif route == "tiled":
            E = np.exp((S - S.max(-1, keepdims=True)).astype(F32)).astype(F32)
            P = (E / lanes_rowsum(E, 64)).astype(F32)
            O = _mm_tiles(P, V)
        elif route in ("stream", "split"):
            X = _pad(S, 64, ninf)
            nt = X.shape[-1] // 64
            X = X.reshape(X.shape[:-1] + (nt, 4, 16))               # [tile, sub-tile, lane]
            m = np.full(S.shape[:-1] + (16,), ninf, F32)
            l = np.zeros_like(m)
            for ti in range(nt):
                sv = X[..., ti, :, :]
                mn = np.maximum(m, sv.max(-2))
                base = np.where(mn == ninf, F32(0), mn)
                l = (l * exp_fast32(m - base)).astype(F32)
                for j in range(4):
                    l = (l + exp_fast32(sv[..., j, :] - base)).astype(F32)
                m = mn
            mall = m.max(-1, keepdims=True)
            base = np.where(mall == ninf, F32(0), mall)
            linv = (F32(1) / _tree((l * exp_fast32(m - base)).astype(F32))).astype(F32)
            P = (exp_fast32(S - base) * linv).astype(F32)
            O = _mm_tiles(P, V)
        elif route == "stream1":
            X = _pad(S, 64, ninf)
            Vp = np.zeros(V.shape[:-2] + (X.shape[-1], V.shape[-1]), F32)
            Vp[..., :Nk, :] = V
            m = np.full(S.shape[:-1] + (1,), ninf, F32)
            l = np.zeros(S.shape[:-1] + (16,), F32)
            O = np.zeros(S.shape[:-1] + (V.shape[-1],), F32)
            for ti in range(X.shape[-1] // 64):
                sv = X[..., 64 * ti:64 * ti + 64]
                mn = np.maximum(m, sv.max(-1, keepdims=True))
                base = np.where(mn == ninf, F32(0), mn)
                alpha = exp_fast32(m - base)
                p = exp_fast32(sv - base)
                l = (l * alpha + seqsum(p.reshape(p.shape[:-1] + (4, 16)), axis=-2)).astype(F32)
                O = ((O * alpha).astype(F32) + _mm(p, Vp[..., 64 * ti:64 * ti + 64, :])).astype(F32)
                m = mn
            P = None
            O = (O * (F32(1) / _tree(l)).astype(F32)).astype(F32)
        else:
            raise KeyError(route)
    return P, np.transpose(O, (0, 2, 1, 3))


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def target_map(Bq, B, mut=None):
    """Which forward (image) target t of ``B`` reads: t % Bq -- the identity per sample, 0 for the shared forward, the K-major order
    of the grouped row mode."""
    idx = np.arange(B) % Bq
    if mut == "grouped_row_points_to_image_0":
        idx[-1] = 0
    return idx


def n_rel(route, Nq, Hh):
    return 4 + -(-Nq // 16) + Hh if route == "head" else 4 + 16 + Hh * -(-Nq // 64)


def bwd_ref(q, k, v, P, d_o, o, scale, mode, route, rel=None, need=True, mut=None):
    """Float64 backward.  ``q k v [Bq, N, H, D]``, ``P [Bq, H, Nq, Nk]`` fp32, ``d_o [B, Nq, H, D]``, ``o [Bq, Nq, H, D]`` fp32 or None
    (read by the streaming family alone), ``rel [B, Nq]`` or None -> dict of ``dP [B, H, Nq, Nk]``, ``dq dk dv [B, N, H, D]``,
    ``rel_out [B, Nk]`` and the bounds ``e_*``."""
    B, Nq, Hh, D = d_o.shape
    Nk = k.shape[1]
    sc = float(F32(scale))
    idx = target_map(q.shape[0], B, mut)
    A, Qr, K, V = bh(operand_a(q, scale, mode))[idx], bh(q)[idx], bh(k)[idx], bh(v)[idx]
    Pw = f64(np.asarray(P, F32))[idx]
    dO = bh(np.roll(d_o, 1, 0) if mut == "sample_reads_previous_dO" else d_o)
    if mut == "head_reads_next_head_of_P":
        Pw = np.roll(Pw, -1, 1)
    if mut == "last_key_dropped":
        Pw = Pw.copy()
        Pw[..., -1] = 0
    dP = _abt(dO, V)
    if mut == "padded_column":
        dP = dP + np.roll(dO, -1, 1)[..., :1] * np.swapaxes(np.roll(V, -1, 1)[..., :1], -1, -2)
    e_dP = U * (D + 1) * _abt(np.abs(dO), np.abs(V)) + TINY
    if o is not None and route == "stream" and need:
        O = bh(o)[idx]
        terms = dO * O
        if mut == "delta_off_by_one_term":
            terms = terms[..., :-1]
        delta = terms.sum(-1, keepdims=True)
        e_delta = U * (D + 1) * np.abs(dO * O).sum(-1, keepdims=True)
    else:
        terms = Pw * dP
        if mut == "delta_off_by_one_term":
            terms = terms[..., :-1]
        delta = terms.sum(-1, keepdims=True)
        e_delta = (Pw * e_dP).sum(-1, keepdims=True) + U * (Nk + 1) * np.abs(Pw * dP).sum(-1, keepdims=True)
    if mut == "delta_of_neighbouring_head":
        delta = np.roll(delta, 1, 1)
    if mut == "delta_of_neighbouring_row":
        delta = np.roll(delta, 1, 2)
    m = 1.0 / sc if mode == SCORES else 1.0
    mm_ = {"dS_inverse_scale_twice": m * m, "dS_without_inverse_scale": 1.0}.get(mut, m)
    dS = Pw * (dP - delta) * mm_
    e_dS = Pw * m * (e_dP + e_delta) + 4 * U * np.abs(Pw * (dP - delta) * m) + TINY
    out = {"dP": dP, "e_dP": e_dP}
    if need:
        mul = sc if mode == Q_FIRST and mut != "dQ_without_scale" else 1.0
        dQ = np.matmul(dS, K) * mul
        e_dQ = (np.matmul(e_dS, np.abs(K)) + U * (Nk + 1) * np.matmul(np.abs(dS), np.abs(K))) * mul \
            + (U * np.abs(dQ) if mode == Q_FIRST else 0.0) + TINY
        Ak = Qr if mut == "dK_with_unscaled_q" else A
        dK = _atb(dS, Ak)
        e_dK = _atb(e_dS, np.abs(A)) + U * (Nq + 1) * _atb(np.abs(dS), np.abs(A)) + TINY
        dV = _atb(Pw, dO)
        e_dV = U * (Nq + 1) * _atb(np.abs(Pw), np.abs(dO)) + TINY
        for name, val in (("dq", dQ), ("e_dq", e_dQ), ("dk", dK), ("e_dk", e_dK), ("dv", dV), ("e_dv", e_dV)):
            out[name] = np.transpose(val, (0, 2, 1, 3))
    if rel is not None:
        r = f64(rel)
        prod = Pw * dP
        term = prod if mut == "row_product_not_clamped" else np.maximum(prod, 0.0)
        w = r[:, None, None, :] if mut == "rel_indexed_by_key" else r[:, None, :, None]
        if mut == "clamp_after_head_mean":
            acc = (r[:, :, None] * np.maximum(prod.mean(1), 0.0)).sum(1) * Hh
        else:
            acc = (w * term).sum((1, 2))
        out["rel_out"] = r + acc / (Hh + 1 if mut == "mean_over_H_plus_1" else Hh)
        nr = n_rel(route, Nq, Hh)
        out["e_rel"] = (np.abs(r)[:, None, :, None] * (Pw * e_dP + (nr + 4) * U * np.abs(prod))).sum((1, 2)) / Hh \
            + U * np.abs(out["rel_out"]) + TINY
    return out


def bwd_restatement(q, k, v, P, d_o, o, scale, mode, route, rel=None, need=True):
    """The backward in numpy fp32 in the order of the kernel family ``route`` -> dict of fp32 ``dP (dq dk dv) (rel_out)``."""
    t = lambda x: np.ascontiguousarray(np.transpose(x, (0, 2, 1, 3))).astype(F32)
    T = lambda x: np.swapaxes(x, -1, -2)
    B, Nq, Hh, D = d_o.shape
    idx = target_map(q.shape[0], B)
    A, K, V, dO = t(operand_a(q, scale, mode))[idx], t(k)[idx], t(v)[idx], t(d_o)
    Pw = np.asarray(P, F32)[idx]
    mm = _mm if route == "head" else _mm_tiles
    dP = _mm(dO, T(V))
    out = {"dP": dP}
    if need:
        if o is not None and route == "stream":
            delta = seqsum((dO * t(o)[idx]).astype(F32))[..., None]
        elif route == "head":
            delta = head_rowsum((Pw * dP).astype(F32))
        else:
            delta = lanes_rowsum((Pw * dP).astype(F32), 16 if route == "stream" else 64)
        dS = (Pw * (dP - delta).astype(F32)).astype(F32)
        if mode == SCORES:
            dS = (dS * (F32(1) / F32(scale))).astype(F32) if route == "stream" else (dS / F32(scale)).astype(F32)
        dq = mm(dS, K)
        if mode == Q_FIRST:
            dq = (dq * F32(scale)).astype(F32)
        for n, a in (("dq", dq), ("dk", mm(T(dS), A)), ("dv", mm(T(Pw), dO))):
            out[n] = np.transpose(a, (0, 2, 1, 3))
    if rel is not None:
        r = np.asarray(rel, F32)
        term = (r[:, None, :, None] * np.maximum((Pw * dP).astype(F32), F32(0))).astype(F32)
        part = seqsum(seqsum(term, axis=2), axis=1)                 # the queries of a head, then the heads
        out["rel_out"] = (r + (part * (F32(1) / F32(Hh))).astype(F32)).astype(F32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# mutants: name -> (the outputs it must move, where it applies: case -> bool).  Each is one realistic slip of a kernel; each must
# put an output that a case stores at >= 2x its bound in at least one row of the table (the host test asserts it and prints in how
# many of the rows where it applies).
# ---------------------------------------------------------------------------------------------------------------------
def _has_2d_mask(c):
    return c["family"] != "underflow" and c["mask"] in ("causal", "rowmasked")


def _has_batch_mask(c):
    return c["family"] == "underflow" or c["mask"] == "keypad"


FWD_MUTANTS = {
    "last_key_left_out_of_sum": (("P", "O"), lambda c: c["Nk"] > 1),
    "last_tile_left_out_of_sum": (("P", "O"), lambda c: c["Nk"] > 16),
    "max_over_first_tile": (("P", "O"), lambda c: c["Nk"] > 16),
    "mask_before_division": (("P", "O"), lambda c: c["mode"] == SCORES and _has_batch_mask(c) and c["family"] != "underflow"),
    "mask_row_off_by_one": (("P", "O"), _has_2d_mask),
    "mask_of_sample_0": (("P", "O"), lambda c: _has_batch_mask(c) and c["Bq"] > 1),
    "scale_rounded_to_bf16": (("P", "O"), lambda c: c["Nk"] > 1 and c["D"] not in (4, 16, 64)),     # (there the scale IS a bf16 number)
    "scale_slip_1e-6": (("P", "O"), lambda c: c["Nk"] > 1),
    "exp_slope_off_2**-20": (("P", "O"), lambda c: c["Nk"] > 1),
    "padded_column": (("P", "O"), lambda c: _d_padded(c) and c["Nk"] > 1),
    "O_without_last_key": (("O",), lambda c: c["Nk"] > 1),
    "O_reads_next_head_of_V": (("O",), lambda c: True),
}
BWD_MUTANTS = {
    "last_key_dropped": (("dq", "dk", "dv", "rel_out"), lambda c: True),
    "delta_off_by_one_term": (("dq", "dk"), lambda c: c["need"]),
    "delta_of_neighbouring_head": (("dq", "dk"), lambda c: c["need"]),
    "delta_of_neighbouring_row": (("dq", "dk"), lambda c: c["need"] and c["Nq"] > 1),
    "dS_inverse_scale_twice": (("dq", "dk"), lambda c: c["need"] and c["mode"] == SCORES),
    "dS_without_inverse_scale": (("dq", "dk"), lambda c: c["need"] and c["mode"] == SCORES),
    "dQ_without_scale": (("dq",), lambda c: c["need"] and c["mode"] == Q_FIRST),
    "dK_with_unscaled_q": (("dk",), lambda c: c["need"] and c["mode"] == Q_FIRST),
    "padded_column": (("dP", "dq", "dk", "rel_out"), _d_padded),
    "head_reads_next_head_of_P": (("dq", "dk", "dv", "rel_out"), lambda c: True),
    "sample_reads_previous_dO": (("dP", "dv", "rel_out"), lambda c: True),
    "row_product_not_clamped": (("rel_out",), lambda c: c["rel"]),
    "clamp_after_head_mean": (("rel_out",), lambda c: c["rel"]),
    "mean_over_H_plus_1": (("rel_out",), lambda c: c["rel"]),
    "rel_indexed_by_key": (("rel_out",), lambda c: c["rel"]),
    "grouped_row_points_to_image_0": (("dP", "dq", "dk", "dv", "rel_out"), lambda c: c["images"] > 0),
}


# ---------------------------------------------------------------------------------------------------------------------
# the case table (shared by the host proof and the device test)
# ---------------------------------------------------------------------------------------------------------------------
LADDER = (1, 15, 16, 17, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128)          # every NTK = ceil(N / 16), both sides of the edges
CROSS_HEAD = ((1, 5), (17, 96), (129, 100), (256, 128), (250, 81))
STREAM_N = (63, 64, 65, 129, 130, 200)
CROSS_STREAM = ((5, 200), (200, 5), (70, 130))
DIMS32, DIMS64 = (4, 8, 20, 32), (36, 64)
ROW_N_HEAD = (16, 17, 33, 49, 65, 81, 97, 128)                                         # row mode: NTK = 1 ... 8
ROW_N_STREAM = (129, 200)


def head_lds_ok(Nq, Nk, D):
    """``bwd_head_lds`` <= 160 KiB and no NTK >= 7 with more than 8 query strips (attention_head.hip:689-694, 824)."""
    dp, ntk, ntq = (32 if D <= 32 else 64), -(-Nk // 16), -(-Nq // 16)
    lds = 4 * max(ntk * 16 * (2 * dp + 12), ntq * 16 * (ntk * 16 + 4 + dp + 4))
    return lds <= 160 * 1024 and not (ntk >= 7 and ntq > 8)


def route(c, noslab=False):
    """Which kernel family a case must reach, by the rules of ``attn_fwd_head_try`` / ``attn_bwd_head_try`` (attention_head.hip:773-855),
    ``attn_fwd_stream_try`` / ``attn_bwd_stream_try`` (attention_stream.hip:1141-1191) and the dispatch of attention_kernels.hip:365-368,
    623-641: ``head`` | ``stream`` | ``split`` (the small-grid forward) | ``stream1`` (the one-sweep no-slab forward) | ``tiled``."""
    Nq, Nk, D = c["Nq"], c["Nk"], c["D"]
    vec = D % 4 == 0 and D <= 64 and not c["misaligned"]
    head = c["head"] and vec and Nk <= 128 and Nq <= 256
    if c["kind"] == "bwd":
        head = head and head_lds_ok(Nq, Nk, D)
    if head:
        return "head"
    if c["stream"] and vec:
        if c["kind"] == "bwd":
            return "stream"
        small_grid = c["split"] and -(-Nq // 64) * c["H"] * c["Bq"] < 160 and Nk > 64
        return "split" if small_grid else ("stream1" if noslab else "stream")
    return "tiled"


def _case(kind, Nq, Nk, D, i, **kw):
    c = {"kind": kind, "Nq": Nq, "Nk": Nk, "D": D, "H": H, "shared": False, "images": 0, "mode": i % 2, "mask": "none",
         "family": FAMILIES[i % len(FAMILIES)], "head": 1, "stream": 1, "split": 1, "misaligned": False, "o": True, "need": True,
         "dprobs": True, "rel": False, "seed": i}
    c.update(kw)
    c["Bq"], c["B"] = (1, 2) if c["shared"] else ((c["images"], 2 * c["images"]) if c["images"] else (2, 2))
    if kind == "fwd":
        c["B"] = c["Bq"]
    c["kernel"] = route(c)
    if kind == "fwd":
        c["kernel_noslab"] = route(c, noslab=True)
    c["id"] = "%s-%s-%dx%dx%d-%d" % (kind, c["kernel"], Nq, Nk, D, i)
    return c


def fwd_cases():
    out = []
    n = 0
    for i, N in enumerate(LADDER):                                  # whole-head: every (DP, NTK), capture + no-slab
        for j, D in enumerate((DIMS32[i % 4], DIMS64[i % 2])):
            out.append(_case("fwd", N, N, D, n, mask=MASKS[(i + j) % 4], shared=n % 7 == 3))
            n += 1
    for i, (Nq, Nk) in enumerate(CROSS_HEAD):
        for j, D in enumerate((DIMS32[(i + 1) % 4], DIMS64[(i + 1) % 2])):
            out.append(_case("fwd", Nq, Nk, D, n, mask=("none", "keypad", "rowmasked")[(i + j) % 3]))
            n += 1
    for i, (Nq, Nk, D) in enumerate(((17, 17, 4), (49, 49, 20), (81, 81, 64), (113, 113, 32), (128, 128, 36), (250, 81, 8))):
        out.append(_case("fwd", Nq, Nk, D, n, family="peaked", mask="causal" if i == 1 else "none"))
        n += 1
    n = 100
    for split in (1, 0):                                            # streaming: the small-grid kernel and the 64-row kernels
        for i, (Nq, Nk) in enumerate(tuple((N, N) for N in STREAM_N) + CROSS_STREAM):
            for j, D in enumerate((DIMS32[(i + split) % 4], DIMS64[(i + split) % 2])):
                mask = MASKS[(i + j + split) % 4] if Nq == Nk else ("none", "keypad", "rowmasked")[(i + j) % 3]
                out.append(_case("fwd", Nq, Nk, D, n, head=0, split=split, mask=mask, shared=n % 5 == 2))
                n += 1
    n = 200
    for i, D in enumerate((6, 10, 20, 64)):                         # tiled
        for j, N in enumerate((1, 17, 65, 130)):
            out.append(_case("fwd", N, N, D, n, head=0, stream=0, mask=MASKS[(i + j) % 4]))
            n += 1
    out.append(_case("fwd", 33, 33, 8, n, misaligned=True, family="randn"))          # whole-head eligible but for the view: tiled
    out.append(_case("fwd", 70, 130, 64, n + 1, misaligned=True, family="peaked", mask="keypad"))
    return out


def bwd_cases():
    out = []
    n = 300
    for i, N in enumerate(LADDER):                                  # whole-head: plain, every (DP, NTK); with / without o, need_dqkv
        for j, D in enumerate((DIMS32[(i + 1) % 4], DIMS64[(i + 1) % 2])):
            out.append(_case("bwd", N, N, D, n, o=(i + j) % 2 == 0, need=n % 6 != 5, shared=n % 7 == 3))
            n += 1
    for i, (Nq, Nk) in enumerate(CROSS_HEAD):                       # (129, 100), (256, 128), (250, 81) at D > 32: streaming
        for j, D in enumerate((DIMS32[i % 4], DIMS64[i % 2])):
            out.append(_case("bwd", Nq, Nk, D, n, o=(i + j) % 2 == 1))
            n += 1
    n = 400
    for images in (0, 2):                                           # row mode and grouped row mode
        for i, N in enumerate(ROW_N_HEAD + ROW_N_STREAM):
            for j, D in enumerate((DIMS32[(i + images) % 4], DIMS64[(i + images) % 2])):
                out.append(_case("bwd", N, N, D, n, rel=True, images=images, dprobs=(i + j) % 3 == 0, need=n % 4 != 1,
                                 o=(i + j) % 2 == 0, shared=images == 0 and n % 5 == 0))
                n += 1
    n = 500
    for i, (Nq, Nk) in enumerate(tuple((N, N) for N in STREAM_N) + CROSS_STREAM):        # streaming, with and without o
        for j, has_o in enumerate((True, False)):
            out.append(_case("bwd", Nq, Nk, (DIMS32 + DIMS64)[(i + 3 * j) % 6], n, head=0, o=has_o, need=n % 7 != 6,
                             shared=n % 5 == 2))
            n += 1
    n = 600
    for i, (N, D) in enumerate(((1, 6), (17, 10), (65, 20), (130, 64), (17, 64), (65, 6), (130, 10), (33, 20))):         # tiled
        out.append(_case("bwd", N, N, D, n, head=0, stream=0, o=i % 2 == 0, need=i != 5))
        n += 1
    out.append(_case("bwd", 33, 33, 8, n, misaligned=True, family="randn"))
    return out


def all_cases():
    return fwd_cases() + bwd_cases()


def case_inputs(c):
    """The operands of a case and its forward mask (the backward's P is the reference forward under the same mask: the ``underflow``
    family hands the backward whole key tiles of exact zeros)."""
    x = family_inputs(c["family"], c["Bq"], c["B"], c["Nq"], c["Nk"], c["D"], c["seed"])
    kind = c["mask"] if c["kind"] == "fwd" else "none"
    x["mask"] = mask_of(kind, c["family"], c["Bq"], c["Nq"], c["Nk"])
    return x


def reference_forward_for(c, x):
    """What the backward of a case is fed: the REFERENCE's P and O rounded to fp32 (``o`` None where the case runs without)."""
    f = fwd_ref(x["q"], x["k"], x["v"], scale_of(c), c["mode"], x["mask"], "head")
    return f["P"].astype(F32), (f["O"].astype(F32) if c["o"] else None)


def head_pairs(cases, form):
    """The ``(DP, NTK)`` instantiations of the whole-head dispatch that the rows of one form reach: ``fwd`` | ``noslab`` | ``bwd`` |
    ``rel`` | ``grouped`` -- from ``route`` and the shapes alone."""
    got = set()
    for c in cases:
        pair = (32 if c["D"] <= 32 else 64, -(-c["Nk"] // 16))
        if form in ("fwd", "noslab"):
            if c["kind"] == "fwd" and (c["kernel_noslab"] if form == "noslab" else c["kernel"]) == "head":
                got.add(pair)
        elif c["kind"] == "bwd" and c["kernel"] == "head":
            mine = "grouped" if c["images"] else ("rel" if c["rel"] else "bwd")
            if mine == form:
                got.add(pair)
    return got
