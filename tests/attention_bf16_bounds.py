"""Float64 references, counted rounding bounds, input families, mutants and the case table for the bf16 matrix-core attention
(``mma_bf16=True``): the ``MM`` instantiations of ``csrc/attention_stream.hip`` (forward, first-generation backward),
``csrc/attention_bf16.hip`` (second generation), ``csrc/attention_bf16_v3.hip`` (third-generation query side, third- and
fourth-generation key sides) and their ``MMX_ATTN_IO_BF16`` epilogues.  CPU only (numpy), on top of ``tests/rowwise_bounds.py`` and
``tests/rowwise_backward_bounds.py`` (imported, not changed): ``tests/test_attention_bf16_bounds_host.py`` proves the bounds and the
mutants here, ``tests/test_gpu_attention_bf16.py`` holds the kernels to them.

Reference.  Float64 of the kernels' DEFINITION on the operands as handed in; every rounding the kernels make is applied once, where
they make it (``rne`` = to the nearest bf16, ties to even; ``scale`` is the fp32 number the C ABI receives):

    forward   A  = rne(fp32(q scale))  (SCALE_Q_FIRST)  or  rne(q)  (SCALE_SCORES: S is divided by ``scale`` after the product)
              Kb = rne(k), Vb = rne(v),  S = A Kb^T (/ scale) (+ mask),  P = softmax(S),  slab <- P rounded once to the slab type
              O  = rne(P) Vb             (the fp32 P, not the slab's)
    backward  a function of (q, k, v, slab P, dO, optional O): Pw = the slab P widened to fp32, Pb = rne(Pw), dOb = rne(dO)
              dP = dOb Vb^T              (stored rounded once to the slab type; never stored in row mode)
              delta = rowsum(dO O)       from the dO and the O handed in;  without O:  delta = sum_k Pw dP
              dS = Pw (dP - delta) m     m = 1, or fp32(1 / scale) in SCALE_SCORES
              dQ = (rne(dS) Kb) (scale or 1),   dK = rne(dS)^T A,   dV = Pb^T dOb
              row mode:  rel_out = rel + (1 / H) sum_h sum_q rel[q] max(Pw dP, 0)[q, key]
              bf16 gradient I/O: dq, dk, dv are those fp32 results rounded once

Bounds, per element, to first order in ``u = 2**-24``.  A product of two bf16 numbers is exact in fp32, so an MFMA dot product of n
terms errs only in its additions: at most n of them in any order and grouping, ``n u sum |a_i b_i|`` (zeros of the padding add
nothing).  Two classes of outputs.

Exact-operand outputs (every MFMA operand is a deterministic rounding of an input):

* ``S``: D additions, in SCALE_SCORES the division (1) and with a mask its addition (1):
  ``e_S = u (D sum_d |A Kb| (/ scale) + |S_unmasked| [SCORES] + |S| [mask])``.
* ``P = exp(S - max) / sum``.  The maximum is an exact selection among the computed scores and cancels between numerator and sum.
  A numerator carries ``e_S`` (an absolute error of the exponent is a relative one of the value), the subtraction ``u |x|``
  (``x = S - max``), ``exp_fast``: the product with log2(e) ``u |x|`` and v_exp_f32's 1 ulp ``2 u`` (attention_stream.hip:37-40).
  The sum, ``nt = ceil(Nk / 64)`` key tiles: a term is taken relative to the running maximum and rescaled once per tile and once at the
  merge by ``exp_fast(old - new)`` -- the exponents of these factors add up to ``x``, each factor costs its subtraction, its
  ``exp_fast`` and its multiplication: ``3 u |x| + 4 (nt + 1) u`` with the term's own ``2 u``; it passes at most ``4 nt + 4`` additions
  (four per tile, the 16-lane merge).  Then the reciprocal (1) and the product with it (1):
  ``e_P = P (e_S + sum_j P_j e_S[j] + u (2 |x| + 3 sum_j P_j |x_j| + 8 nt + 16)) + 2**-126``  (``2**-126``: results below the normal
  range).
* ``dP``: D additions, ``e_dP = D u sum_d |dOb Vb|``.  ``dV``: Nq additions, ``e_dV = Nq u sum_q |Pb dOb|``.
* ``delta`` from O: D products (1 each) and D - 1 additions, ``e_delta = D u sum_d |dO O|``; by the sweep: the error of every dP, the
  product (1) and Nk - 1 additions, ``e_delta = sum_k Pw e_dP + Nk u sum_k |Pw dP|``.
* ``rel_out``: a term ``rel[q] max(Pw dP, 0)`` carries ``|rel[q]| (Pw e_dP + u |Pw dP|)`` and its own product (1); it passes at most
  ``Nq + H ceil(Nq / 64) + 4`` additions (the lane's queries, the partial rows), the rounded ``1 / H`` and its product (2), the final
  addition (1):  ``e_rel = (1 / H) sum_h sum_q |rel[q]| (Pw e_dP + (n_rel + 4) u |Pw dP|) + u |rel_out|``.

Re-rounded outputs (one operand is computed in fp32 and THEN rounded to bf16; an fp32-level error can move it across a rounding
boundary).  With ``e`` the counted fp32 bound of the intermediate ``x``, the bf16 operand may differ from the reference's only where
``rne(x - e) != rne(x + e)``, and then by at most ``gap = rne(x + e) - rne(x - e)``:

* ``e_dS = Pw m (e_dP + e_delta) + 3 u |dS|``  (the subtraction and the two products).
* ``O``:  ``e_O = Nk u sum_k |rne(P) Vb| + gap(P, e_P) |Vb|``.
* ``dQ``: ``e_dQ = (Nk u sum_k |rne(dS) Kb| + gap(dS, e_dS) |Kb|) (scale or 1) + u |dQ| [Q_FIRST]``.
* ``dK``: ``e_dK = Nq u sum_q |rne(dS) A| + gap(dS, e_dS)^T |A|``.

A 16-bit output (a bf16 / fp16 slab of P or dP, bf16 dq / dk / dv) with float64 value ``v`` and fp32 bound ``b`` is right iff
``rnd(v - b) <= got <= rnd(v + b)`` in the stored type (rounding is monotone), as the bf16 QuickGELU backward is judged.

Exact scaling.  The backward is linear in dO and every rounding commutes with a power of two inside the normal range: dP, dq, dk, dv of
``2**s dO`` are ``2**s`` times those of ``dO`` bit for bit (fp16 slabs aside, for their range)."""
import math

import numpy as np

import rowwise_bounds as rb
from rowwise_backward_bounds import bf16_bits, rne_bf16, trunc_bf16
from rowwise_bounds import F32, U

__all__ = ["bf16_bits", "rne_bf16", "trunc_bf16", "U", "F32"]

Q_FIRST, SCORES = 0, 1                      # _lib.SCALE_Q_FIRST / SCALE_SCORES
TILE = 64
TINY = 2.0 ** -126
FAMILIES = ("randn", "prerounded", "peaked", "small", "poscode")
MASKS = ("none", "causal", "keypad", "rowmasked")
SLABS = ("f32", "f16", "bf16")


def f64(a):
    return None if a is None else np.asarray(a, np.float64)


def slab_round(a, slab):
    """float64 or fp32 -> the slab type's nearest number (rounded once from the type given), as fp32."""
    if slab == "f32":
        with np.errstate(over="ignore", invalid="ignore"):
            return np.asarray(a).astype(F32)
    if slab == "bf16":
        return rne_bf16(a)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a).astype(np.float16).astype(F32)


def _abt(a, b):
    return np.matmul(a, np.swapaxes(b, -1, -2))


def _ab(a, b):
    return np.matmul(a, b)


def _atb(a, b):
    return np.matmul(np.swapaxes(a, -1, -2), b)


def bh(x):
    """``[B, N, H, D]`` -> ``[B, H, N, D]`` float64."""
    return np.transpose(f64(x), (0, 2, 1, 3))


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def make_mask(kind, B, Nq, Nk):
    """The additive mask of one kind (fp32), or None."""
    if kind == "none":
        return None
    if kind == "causal":
        assert Nq == Nk
        return np.triu(np.full((Nq, Nk), -np.inf, F32), 1)
    if kind == "keypad":                                            # key padding [B, 1, Nk]: sample b loses its last 1 + b keys (never all)
        m = np.zeros((B, 1, Nk), F32)
        for b in range(B):
            m[b, 0, max(1, Nk - 1 - b):] = -10000.0
        return m
    if kind == "rowmasked":                                         # forward only: one fully masked query row (NaN like torch.softmax)
        m = np.zeros((Nq, Nk), F32)
        m[Nq // 2] = -np.inf
        if Nk > 1:
            m[0, Nk - 1] = -np.inf
        return m
    raise KeyError(kind)


def inputs(family, Bq, B, H, Nq, Nk, D, seed=0):
    """One seeded operand set: ``q [Bq, Nq, H, D]``, ``k v [Bq, Nk, H, D]``, ``dO [B, Nq, H, D]``, ``rel [B, Nq]``, all fp32.  ``Bq = 1``
    with ``B > 1`` is the shared forward.  Plain ``randn`` is NOT representable in bf16: the kernels' own rounding is under test."""
    rng = np.random.default_rng([FAMILIES.index(family), Bq, B, H, Nq, Nk, D, seed])
    q, k, v = (rng.standard_normal((Bq, n, H, D)).astype(F32) for n in (Nq, Nk, Nk))
    d_o = rng.standard_normal((B, Nq, H, D)).astype(F32)
    rel = rng.random((B, Nq)).astype(F32)
    if family == "prerounded":
        q, k, v, d_o = (rne_bf16(t) for t in (q, k, v, d_o))
    elif family == "peaked":
        q, k = (q * 4).astype(F32), (k * 4).astype(F32)
    elif family == "small":
        d_o = np.ldexp(d_o, -20).astype(F32)
    elif family == "poscode":                                       # exact in bf16, a function of (row, column) alone
        d = np.arange(D)[None, None, None, :]
        v = np.broadcast_to(1.0 + (d % 7) / 8.0 + (np.arange(Nk)[None, :, None, None] % 64) / 64.0, v.shape).astype(F32)
        d_o = np.broadcast_to(1.0 + (d % 5) / 8.0 + ((3 * np.arange(Nq)[None, :, None, None]) % 64) / 64.0, d_o.shape).astype(F32)
        rel = np.broadcast_to(1.0 + (np.arange(Nq)[None, :] % 32) / 32.0, rel.shape).astype(F32)
    return {"q": q, "k": k, "v": v, "dO": np.ascontiguousarray(d_o), "rel": np.ascontiguousarray(rel)}


def _mask4(mask, B):
    """-> broadcastable to ``[B, H, Nq, Nk]`` float64, or None."""
    if mask is None:
        return None
    m = f64(mask)
    return m[None, None] if m.ndim == 2 else m[:, None]


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def operand_a(q, scale, mode, mut=None):
    if mode == SCORES:
        return rne_bf16(q)
    if mut == "q_rounded_before_scale":
        return rne_bf16((rne_bf16(q) * F32(scale)).astype(F32))
    return rne_bf16((np.asarray(q, F32) * F32(scale)).astype(F32))


def _gap(x, e):
    """Where may ``rne(x)`` move under an error ``e``, and by how much at most: ``rne(x + e) - rne(x - e)`` (0 where it cannot)."""
    with np.errstate(invalid="ignore", over="ignore"):
        g = f64(rne_bf16(x + e)) - f64(rne_bf16(x - e))
    return np.where(np.isfinite(g), g, 0.0)


def fwd_ref(q, k, v, scale, mode, mask=None, slab="f32", mut=None):
    """Float64 forward on ``q [B, Nq, H, D]``, ``k v [B, Nk, H, D]`` -> dict of ``S P [B, H, Nq, Nk]``, ``slab`` (P in the slab type, as
    fp32), ``O [B, Nq, H, D]`` and the bounds ``e_S e_P e_O`` with ``flagged`` (the share of P that may round either way)."""
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    sc = float(F32(scale))
    A = bh(operand_a(q, scale, mode, mut))
    Kb = bh(trunc_bf16(k) if mut == "k_truncated" else rne_bf16(k))
    Vb = bh(trunc_bf16(v) if mut == "v_truncated" else rne_bf16(v))
    raw = _abt(A, Kb)
    if mut == "padded_column":                                      # column D of the padded tile = column 0 of the next head in memory
        raw = raw + np.roll(A, -1, 1)[..., :1] * np.swapaxes(np.roll(Kb, -1, 1)[..., :1], -1, -2)
    absraw = _abt(np.abs(A), np.abs(Kb))
    S0 = raw / sc if mode == SCORES else raw
    m4 = _mask4(mask, B)
    if m4 is not None and mut == "mask_ignored_on_last_tile":
        m4 = np.broadcast_to(m4, (B, 1) + S0.shape[2:]).copy() if m4.shape[1] == 1 else m4.copy()
        m4[..., TILE * ((Nk - 1) // TILE):] = 0.0
    S = S0 if m4 is None else S0 + m4
    if mut == "last_key_dropped":
        S = S.copy()
        S[..., -1] = -np.inf
    if mut == "last_partial_tile_dropped":
        S = S.copy()
        S[..., TILE * (Nk // TILE):] = -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        mx = S.max(-1, keepdims=True)
        x = S - mx                                                  # a fully masked row: -inf - -inf = NaN, like torch.softmax
        E = np.exp(x)
        P = E / E.sum(-1, keepdims=True)
        e_S = U * (D * absraw * (1.0 / sc if mode == SCORES else 1.0) + (np.abs(S0) if mode == SCORES else 0.0)
                   + (np.abs(S) if m4 is not None else 0.0))
        live = P > 0
        e_S = np.where(live, e_S, 0.0)
        ax = np.where(live, np.abs(x), 0.0)
        nt = -(-Nk // TILE)
        e_P = P * (e_S + (P * e_S).sum(-1, keepdims=True) + U * (2 * ax + 3 * (P * ax).sum(-1, keepdims=True) + 8 * nt + 16)) + TINY
    Pslab = slab_round(P, slab)
    Pop = f64(rne_bf16(Pslab if mut == "O_from_slab_P" else P))
    with np.errstate(invalid="ignore", over="ignore"):
        O = _ab(Pop, Vb)
        gap = _gap(P, e_P)
        e_O = U * Nk * _ab(np.abs(Pop), np.abs(Vb)) + _ab(gap, np.abs(Vb)) + TINY
    pos = np.isfinite(P) & (P > 0)                                  # (an exact zero -- a masked key -- has nothing to round)
    with np.errstate(invalid="ignore", over="ignore"):
        share = float((_gap(P, e_P - TINY)[pos] != 0).mean()) if pos.any() else 0.0
    return {"S": S, "P": P, "slab": Pslab, "O": np.transpose(O, (0, 2, 1, 3)), "e_S": e_S, "e_P": e_P,
            "e_O": np.transpose(e_O, (0, 2, 1, 3)), "flagged": share}


def fwd_restatement(q, k, v, scale, mode, mask=None, slab="f32", matmul=None):
    """The forward in fp32 numpy: the same rounding places, numpy's own accumulation order, libm's exp -> ``(slab P, O)``.
    ``matmul(a, b)``: another fp32-accumulating product of bf16 numbers (default ``np.matmul`` on fp32)."""
    mm = matmul or (lambda a, b: np.matmul(a.astype(F32), b.astype(F32)))
    t = lambda x: np.ascontiguousarray(np.transpose(x, (0, 2, 1, 3)))
    A, Kb, Vb = t(operand_a(q, scale, mode)), t(rne_bf16(k)), t(rne_bf16(v))
    with np.errstate(invalid="ignore", over="ignore"):
        S = mm(A, np.swapaxes(Kb, -1, -2)).astype(F32)
        if mode == SCORES:
            S = (S / F32(scale)).astype(F32)
        m4 = _mask4(mask, q.shape[0])
        if m4 is not None:
            S = (S + m4.astype(F32)).astype(F32)
        E = np.exp((S - S.max(-1, keepdims=True)).astype(F32)).astype(F32)
        P = (E * (F32(1) / E.sum(-1, keepdims=True, dtype=F32)).astype(F32)).astype(F32)
        O = mm(rne_bf16(P), Vb).astype(F32)
    return slab_round(P, slab), np.transpose(O, (0, 2, 1, 3))


def crude_flag_share(q, k, v, scale, mode):
    """The near-tie share of P under the deliberately crude error of the issue: D + 1 roundings on S, twice that on the row maximum,
    ``1.2e-7 |s - max|`` for the exp, ``Nk + 8`` on the sum."""
    r = fwd_ref(q, k, v, scale, mode)
    D, Nk = q.shape[-1], k.shape[1]
    absraw = _abt(np.abs(bh(operand_a(q, scale, mode))), np.abs(bh(rne_bf16(k))))
    eS = (D + 1) * U * absraw
    e = r["P"] * (eS + 2 * eS.max(-1, keepdims=True) + 1.2e-7 * np.abs(r["S"] - r["S"].max(-1, keepdims=True)) + (Nk + 8) * U)
    return float((_gap(r["P"], e) != 0).mean())


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def bwd_ref(q, k, v, P_slab, d_o, o, scale, mode, rel=None, mut=None):
    """Float64 backward.  ``q k v [Bq, N, H, D]`` (``Bq = 1``: shared forward), ``P_slab [Bq, H, Nq, Nk]`` (numbers of the slab type, as
    fp32), ``d_o [B, Nq, H, D]`` (fp32, or bf16 numbers as fp32), ``o [Bq, Nq, H, D]`` fp32 or None, ``rel [B, Nq]`` or None -> dict of
    ``dP [B, H, Nq, Nk]``, ``dq dk dv [B, N, H, D]``, ``rel_out [B, Nk]`` and the bounds ``e_*``, with ``flagged_dS``."""
    B, Nq, H, D = d_o.shape
    Nk = k.shape[1]
    sc = float(F32(scale))
    A = bh(operand_a(q, scale, mode, mut))
    Kb = bh(trunc_bf16(k) if mut == "k_truncated" else rne_bf16(k))
    Vb = bh(trunc_bf16(v) if mut == "v_truncated" else rne_bf16(v))
    if mut == "sample_reads_previous_dO":
        d_o = np.roll(d_o, 1, 0)
    dO = bh(d_o)
    dOb = bh(trunc_bf16(d_o) if mut == "dO_truncated" else rne_bf16(d_o))
    Ps = np.asarray(P_slab, F32)
    if mut == "head_reads_next_head_of_P":
        Ps = np.roll(Ps, -1, 1)
    if mut == "last_key_dropped":
        Ps = Ps.copy()
        Ps[..., -1] = 0
    if mut == "last_partial_tile_dropped":
        Ps = Ps.copy()
        Ps[..., TILE * (Nk // TILE):] = 0
    Pw, Pb = f64(Ps), f64(rne_bf16(Ps))
    dP = _abt(dOb, Vb)
    if mut == "padded_column":
        dP = dP + np.roll(dOb, -1, 1)[..., :1] * np.swapaxes(np.roll(Vb, -1, 1)[..., :1], -1, -2)
    e_dP = U * D * _abt(np.abs(dOb), np.abs(Vb)) + TINY
    by_o = (o is not None) != (mut in ("delta_by_sweep_with_o", "delta_from_o_without_o"))
    if mut == "delta_from_o_without_o":
        o = np.transpose(_ab(Pb, Vb), (0, 2, 1, 3)).astype(F32)     # what a forward would hand in
    if by_o:
        O = bh(o)
        dOd = dOb if mut == "delta_from_rounded_dO" else dO
        delta = (dOd * O).sum(-1, keepdims=True)
        e_delta = U * D * (np.abs(dOd) * np.abs(O)).sum(-1, keepdims=True)
    else:
        delta = (Pw * dP).sum(-1, keepdims=True)
        e_delta = (Pw * e_dP).sum(-1, keepdims=True) + U * Nk * np.abs(Pw * dP).sum(-1, keepdims=True)
    m = float(F32(1) / F32(scale)) if mode == SCORES and mut != "dS_without_inverse_scale" else 1.0
    dS = Pw * (dP - delta) * m
    e_dS = Pw * m * (e_dP + e_delta) + 3 * U * np.abs(dS) + TINY
    dSb = f64(rne_bf16(dS))
    gap = _gap(dS, e_dS)
    mul = sc if mode == Q_FIRST and mut != "dQ_without_scale" else 1.0
    aK, aA = np.abs(Kb), np.abs(A)
    dQ = _ab(dSb, Kb) * mul
    e_dQ = (U * Nk * _ab(np.abs(dSb), aK) + _ab(gap, aK)) * mul \
        + (U * np.abs(dQ) if mode == Q_FIRST else 0.0) + TINY
    dK = _atb(dSb, A)
    e_dK = U * Nq * _atb(np.abs(dSb), aA) + _atb(gap, aA) + TINY
    dV = _atb(Pb, dOb)
    e_dV = U * Nq * _atb(np.abs(Pb), np.abs(dOb)) + TINY
    nz = dS != 0
    out = {"dP": dP, "e_dP": e_dP, "flagged_dS": float((_gap(dS, e_dS - TINY)[nz] != 0).mean()) if nz.any() else 0.0}
    for name, val in (("dq", dQ), ("e_dq", e_dQ), ("dk", dK), ("e_dk", e_dK), ("dv", dV), ("e_dv", e_dV)):
        out[name] = np.transpose(val, (0, 2, 1, 3))
    if rel is not None:
        r = f64(rel)
        prod = Pw * dP
        term = prod if mut == "row_product_not_clamped" else np.maximum(prod, 0.0)
        if mut == "rel_indexed_by_key":
            w = r[:, None, None, :]
        else:
            w = r[:, None, :, None]
        acc = (w * term).sum((1, 2))
        out["rel_out"] = r + (acc if mut == "heads_summed_not_averaged" else acc / H)
        n_rel = Nq + H * (-(-Nq // TILE)) + 4
        out["e_rel"] = (np.abs(r)[:, None, :, None] * (Pw * e_dP + (n_rel + 4) * U * np.abs(prod))).sum((1, 2)) / H \
            + U * np.abs(out["rel_out"]) + TINY
    return out


def bwd_restatement(q, k, v, P_slab, d_o, o, scale, mode, rel=None, matmul=None):
    """The backward in fp32 numpy: the same rounding places, numpy's accumulation order -> dict of fp32 ``dP dq dk dv (rel_out)``."""
    mm = matmul or (lambda a, b: np.matmul(a.astype(F32), b.astype(F32)))
    t = lambda x: np.ascontiguousarray(np.transpose(x, (0, 2, 1, 3))).astype(F32)
    T = lambda x: np.swapaxes(x, -1, -2)
    H = q.shape[2]
    A, Kb, Vb, dO, dOb = t(operand_a(q, scale, mode)), t(rne_bf16(k)), t(rne_bf16(v)), t(d_o), t(rne_bf16(d_o))
    Pw = np.asarray(P_slab, F32)
    Pb = rne_bf16(Pw)
    dP = mm(dOb, T(Vb)).astype(F32)
    if o is not None:
        delta = (dO * t(o)).astype(F32).sum(-1, keepdims=True, dtype=F32)
    else:
        delta = (Pw * dP).astype(F32).sum(-1, keepdims=True, dtype=F32)
    dS = (Pw * (dP - delta).astype(F32)).astype(F32)
    if mode == SCORES:
        dS = (dS * (F32(1) / F32(scale))).astype(F32)
    dSb = rne_bf16(dS)
    dq = mm(dSb, Kb).astype(F32)
    if mode == Q_FIRST:
        dq = (dq * F32(scale)).astype(F32)
    out = {"dP": dP, "dq": dq, "dk": mm(T(dSb), A).astype(F32), "dv": mm(T(Pb), dOb).astype(F32)}
    out = {n: (a if n == "dP" else np.transpose(a, (0, 2, 1, 3))) for n, a in out.items()}
    if rel is not None:
        r = np.asarray(rel, F32)
        term = (r[:, None, :, None] * np.maximum((Pw * dP).astype(F32), F32(0))).astype(F32)
        out["rel_out"] = (r + (term.sum((1, 2), dtype=F32) * (F32(1) / F32(H))).astype(F32)).astype(F32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# judging
# ---------------------------------------------------------------------------------------------------------------------
def ratio(got, want, bound):
    """Worst error / bound over every element (``rowwise_bounds._ratio``: a one-sided NaN / inf is infinitely wrong)."""
    return rb._ratio(got, want, bound)


def outside_interval(got, want, bound, kind):
    """A 16-bit output: how many elements lie outside ``[rnd(v - b), rnd(v + b)]`` of the stored type (``kind``: ``bf16`` / ``f16``); a
    NaN must meet a NaN."""
    got = np.asarray(got, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = slab_round(want - bound, kind), slab_round(want + bound, kind)
        nan = np.isnan(want)
        ok = np.where(nan, np.isnan(got), (lo <= got) & (got <= hi))
    return int((~ok).sum())


def judge(got, want, bound, kind="f32"):
    """-> the figure of one output: error / bound for an fp32 output (right iff ``<= 1``), the number of elements outside their
    interval for a 16-bit one (right iff 0)."""
    if kind == "f32":
        return ratio(got, want, bound)
    return float(outside_interval(got, want, bound, kind))


def passes(figure, kind="f32"):
    return figure <= 1.0 if kind == "f32" else figure == 0


# ---------------------------------------------------------------------------------------------------------------------
# mutants: name -> (side, the outputs it must move, where it applies: case -> bool)
# ---------------------------------------------------------------------------------------------------------------------
def _partial(c):
    """Is there a last PARTIAL 64-key tile next to a whole one?  (Up to 64 keys the one tile holds every key: dropping it leaves no
    softmax at all, NaN everywhere -- not a subtle error, and ``last_key_dropped`` covers the short shapes.)"""
    return c["Nk"] % TILE != 0 and c["Nk"] > TILE


def _same_delta(c):
    return c["slab"] == "bf16" and (c["io_bf16"] or c["family"] in ("prerounded", "poscode"))


def _d_padded(c):
    return c["D"] in (8, 20, 40) and c["H"] > 1


FWD_MUTANTS = {
    "last_key_dropped": (("P", "O"), lambda c: c["Nk"] > 1 and c["mask"] != "keypad"),           # (key padding already removes the last key)
    "last_partial_tile_dropped": (("P", "O"), lambda c: _partial(c) and not (c["mask"] == "keypad" and c["Nk"] % TILE <= 2)),   # (all padded)
    "k_truncated": (("P", "O"), lambda c: c["family"] not in ("prerounded",) and c["Nk"] > 1),           # (one key: P = 1 whatever S is)
    "v_truncated": (("O",), lambda c: c["family"] not in ("prerounded", "poscode")),
    "q_rounded_before_scale": (("P", "O"), lambda c: c["mode"] == Q_FIRST and c["D"] in (8, 32) and c["family"] != "prerounded"
                               and c["Nk"] > 1),
    "O_from_slab_P": (("O",), lambda c: c["slab"] == "f16" and c["Nk"] > 1),
    "mask_ignored_on_last_tile": (("P", "O"), lambda c: c["mask"] in ("causal", "keypad") and c["Nk"] > 1),
    "padded_column": (("P", "O"), lambda c: _d_padded(c) and c["Nk"] > 1),
}
BWD_MUTANTS = {
    "last_key_dropped": (("dq", "dk", "dv", "rel_out"), lambda c: True),
    "last_partial_tile_dropped": (("dq", "dk", "dv", "rel_out"), _partial),
    # (v enters dP, and through it dS and the row product: seen in whatever the case stores)
    "v_truncated": (("dP", "dq", "dk", "rel_out"), lambda c: c["family"] not in ("prerounded", "poscode")),
    "k_truncated": (("dq",), lambda c: c["need"] and c["family"] != "prerounded" and c["Nk"] > 1),   # (one key: dS = 0, dq = 0)
    "q_rounded_before_scale": (("dk",), lambda c: c["need"] and c["mode"] == Q_FIRST and c["D"] in (8, 32)
                               and c["family"] != "prerounded" and c["Nk"] > 1),
    "dO_truncated": (("dP", "dv"), lambda c: c["family"] not in ("prerounded", "poscode") and not c["io_bf16"]),
    # (a bf16 slab with a bf16 dO: Pw = Pb and dO = dOb, so rowsum(dO O) and sum_k Pw dP are the same number up to O's fp32 rounding)
    "delta_by_sweep_with_o": (("dq", "dk"), lambda c: c["o"] and c["need"] and c["Nk"] > 1 and not _same_delta(c)),
    "delta_from_o_without_o": (("dq", "dk"), lambda c: not c["o"] and c["need"] and c["Nk"] > 1 and not _same_delta(c)),
    "delta_from_rounded_dO": (("dq", "dk"), lambda c: c["o"] and c["need"] and not c["io_bf16"]
                              and c["family"] not in ("prerounded", "poscode") and c["Nk"] > 1),
    "dS_without_inverse_scale": (("dq", "dk"), lambda c: c["mode"] == SCORES and c["need"] and c["Nk"] > 1),
    "dQ_without_scale": (("dq",), lambda c: c["mode"] == Q_FIRST and c["need"] and c["Nk"] > 1),
    "row_product_not_clamped": (("rel_out",), lambda c: c["rel"] and c["family"] != "poscode"),     # (v, dO > 0: nothing to clamp)
    "heads_summed_not_averaged": (("rel_out",), lambda c: c["rel"]),
    "rel_indexed_by_key": (("rel_out",), lambda c: c["rel"] and c["Nq"] > 1),
    "head_reads_next_head_of_P": (("dq", "dk", "dv", "rel_out"), lambda c: c["H"] > 1 and c["Nk"] > 1      # (one key: P = 1 in every head;
                                  and not (c["family"] == "poscode" and not c["need"])),       # poscode: dP is the same in every head, the head SUM stays)
    "sample_reads_previous_dO": (("dP", "dv", "rel_out"), lambda c: c["B"] > 1 and c["family"] != "poscode"),
    "padded_column": (("dP", "dq", "dk", "rel_out"), _d_padded),
}
# (Where a mutant is the same operation as the reference it does not apply: the predicates above carry every such exemption with its
# reason.  Wherever a mutant applies it must be at 2x a bound: there is no further exemption.)


# ---------------------------------------------------------------------------------------------------------------------
# the case table (shared by the host proof and the device test)
# ---------------------------------------------------------------------------------------------------------------------
SELF_N = (1, 15, 16, 17, 33, 63, 64, 65, 97, 128, 129, 130)
CROSS = ((70, 130), (130, 70), (5, 200), (200, 5))
DIMS = (8, 12, 20, 32, 40, 64)
H = 3


def _case(kind, Nq, Nk, D, i, **kw):
    c = {"kind": kind, "Nq": Nq, "Nk": Nk, "D": D, "H": H, "B": 2, "shared": False, "slab": "f32", "mode": Q_FIRST, "mask": "none",
         "family": FAMILIES[i % len(FAMILIES)], "o": True, "v2": 1, "v3": 3, "dprobs": True, "rel": False, "need": True,
         "io_bf16": False, "packed": bool(i % 2), "seed": i}
    c.update(kw)
    # FORWARD rows only: the S bound grows with D sum |A Kb|, 16-fold under ``peaked``, and the near-tie share of P it allows is 1.5 % at
    # D = 8, 2.5 % at 12, 4.9 % at 20 and 9 % at 32 -- past the 5 % the allowance on rne(P) is conditioned on.  So a round-robin row that
    # would be peaked beyond D = 12 is ``randn``, and the forward's peaked rows are the explicit ones of ``PEAKED_FWD`` (D = 8 and 12:
    # the DP = 32 instantiations; the DP = 64 forward, D = 40 and 64, has none).  In the backward P is an input: no downgrade there.
    if kind == "fwd" and c["family"] == "peaked" and D > 12:
        c["family"] = "randn"
    if c["shared"]:
        c["B"] = 3
    c["Bq"] = 1 if c["shared"] else c["B"]
    c["kernel"] = route(c)
    c["id"] = "%s-%dx%dx%d-%s" % (c["kernel"], Nq, Nk, D, i)
    return c


def route(c):
    """Which kernels serve a case, by the rules of ``attn_fwd_stream_try`` / ``attn_bwd_bf16_v3_try`` / ``attn_bwd_bf16_try`` /
    ``attn_bwd_stream_try`` (the operands of the table satisfy their 16-byte alignment tests)."""
    if c["kind"] == "fwd":
        return "fwd%d" % (32 if c["D"] <= 32 else 64)
    if (c["v3"] and c["io_bf16"] and c["rel"] and c["o"] and not c["dprobs"] and c["D"] == 64 and c["slab"] == "bf16"
            and c["mode"] == Q_FIRST and c["Nq"] == c["Nk"] and c["shared"]):
        return "gen3" if c["v3"] == 2 else "gen4"                   # third-generation query side; key side: third / fourth generation
    if c["v2"] and c["o"] and c["D"] % 8 == 0:
        return "gen2"
    return "gen1"


# The forward under ``peaked`` (q and k x 4: |s - max| up to ~100, P over many binades down to fp32's subnormals, 16-bit slabs flushing
# the small entries; the ``2 |x| + 3 sum P |x|`` terms of e_P at work): both scale modes x the three slabs, a partial tile, exact
# multiples, a cross shape, a causal mask.
PEAKED_FWD = ((65, 65, 8, "f32", Q_FIRST, "none"), (130, 130, 12, "bf16", SCORES, "none"), (130, 130, 8, "f16", Q_FIRST, "causal"),
              (64, 64, 12, "f32", SCORES, "none"), (128, 128, 8, "bf16", Q_FIRST, "none"), (64, 64, 8, "f16", SCORES, "keypad"),
              (70, 130, 12, "f16", Q_FIRST, "none"), (17, 17, 12, "bf16", Q_FIRST, "none"))


def fwd_cases():
    """Forward: DP 32 and 64, the three slabs, both scale modes, every mask kind, self and cross shapes."""
    out = []
    for i, N in enumerate(SELF_N):
        for j in range(3):
            n = 3 * i + j
            out.append(_case("fwd", N, N, DIMS[(i + 2 * j) % 6], n, slab=SLABS[(i + j) % 3], mode=(i + j) % 2, mask=MASKS[(n + i + (n % 5 == 0)) % 4]))
    for i, (Nq, Nk) in enumerate(CROSS):
        for j in range(2):
            n = 100 + 2 * i + j
            out.append(_case("fwd", Nq, Nk, DIMS[(2 * i + 3 * j + 1) % 6], n, slab=SLABS[(i + j) % 3], mode=j,
                             mask=("none", "keypad", "rowmasked")[(i + j) % 3]))
    for i, (Nq, Nk, D, slab, mode, mask) in enumerate(PEAKED_FWD):
        out.append(_case("fwd", Nq, Nk, D, 150 + i, family="peaked", slab=slab, mode=mode, mask=mask))
    return out


MODES3 = ((True, False), (True, True), (False, True))               # (dprobs slab, rel_row)


def gen1_cases():
    """First-generation backward (``attn_bwd_q_stream_kernel<MM>`` / ``attn_bwd_kv_stream_kernel<MM>``): ``o=None`` (delta by sweep),
    option ``attn_bf16_v2`` = 0 with ``o``, D % 8 != 0 -- each with / without a dP slab, with / without ``rel_row``, fp32 and bf16 dO."""
    out = []
    n = 200
    for variant, dims in (("no_o", (8, 32, 40, 64)), ("v2_off", (8, 32, 64, 40)), ("d12_20", (12, 20))):
        for vi, N in enumerate((17, 64, 65, 130) if variant != "d12_20" else (16, 63, 129, 33)):
            for mi, (dp, rel) in enumerate(MODES3):
                for io in (False, True):
                    D = dims[(vi + mi) % len(dims)]
                    kw = dict(o=variant != "no_o", v2=0 if variant == "v2_off" else 1, dprobs=dp, rel=rel, io_bf16=io,
                              slab=SLABS[(vi + mi + io) % 3], mode=(vi + mi) % 2, shared=(vi + io) % 2 == 1)
                    out.append(_case("bwd", N, N, D, n, **kw))
                    n += 1
    for i, (Nq, Nk) in enumerate(CROSS):                            # cross shapes: outside row mode
        out.append(_case("bwd", Nq, Nk, (12, 20, 32, 64)[i], n, o=i % 2 == 0, v2=0, io_bf16=i >= 2, slab=SLABS[i % 3], mode=i % 2))
        n += 1
    return out


def gen2_cases():
    """Second-generation backward (``attention_bf16.hip``): ``o`` given, D in {8, 40, 64}, the three slabs, fp32 and bf16 dO; plain, row
    mode, row mode with ``need_dqkv=False``; per-sample and shared forward."""
    out = []
    n = 400
    for ni, N in enumerate((1, 15, 33, 64, 65, 97, 128, 130)):
        for mi, (dp, rel, need) in enumerate(((True, False, True), (False, True, True), (False, True, False))):
            for io in (False, True):
                D = (8, 40, 64)[(ni + mi + io) % 3]
                slab = SLABS[(ni + mi) % 3]
                shared = (ni + mi + io) % 2 == 0
                # (shared + bf16 slab + bf16 dO + row mode + D = 64 + Q_FIRST is the third generation's: keep these on SCALE_SCORES)
                mode = SCORES if (shared and slab == "bf16" and io and rel and D == 64) else (ni + io) % 2
                out.append(_case("bwd", N, N, D, n, dprobs=dp, rel=rel, need=need, io_bf16=io, slab=slab, shared=shared, mode=mode))
                n += 1
    for i, (Nq, Nk) in enumerate(CROSS):
        out.append(_case("bwd", Nq, Nk, (8, 40, 64, 40)[i], n, io_bf16=i % 2 == 1, slab=SLABS[(i + 1) % 3], mode=i % 2, shared=i >= 2))
        n += 1
    return out


def gen3_cases():
    """Third generation (``attention_bf16_v3.hip``) at ``attn_bf16_v3`` = 2 (third-generation key side) and 3 (fourth-generation key
    side, 32 keys per wave): shared forward, bf16 slab, bf16 dO, row mode, D = 64, SCALE_Q_FIRST, no dP slab; ``need_dqkv`` both ways."""
    out = []
    n = 600
    for mode3 in (2, 3):
        for ni, N in enumerate(SELF_N):
            for need in ((True, False) if ni % 2 == 0 else (True,)):
                out.append(_case("bwd", N, N, 64, n, v3=mode3, shared=True, slab="bf16", io_bf16=True, rel=True, dprobs=False, need=need))
                n += 1
    return out


def bwd_cases():
    return gen1_cases() + gen2_cases() + gen3_cases()


def all_cases():
    return fwd_cases() + bwd_cases()


def scale_of(c):
    """The ``scale`` argument: the multiplier D**-0.5 in SCALE_Q_FIRST, the divisor sqrt(D) in SCALE_SCORES."""
    return c["D"] ** -0.5 if c["mode"] == Q_FIRST else math.sqrt(c["D"])


def case_inputs(c):
    """The operands of a case (``inputs`` + its mask); a bf16 dO holds bf16 numbers as fp32."""
    x = inputs(c["family"], c["Bq"], c["B"], c["H"], c["Nq"], c["Nk"], c["D"], c["seed"])
    if c["io_bf16"]:
        x["dO"] = rne_bf16(x["dO"])
    x["mask"] = make_mask(c["mask"], c["Bq"], c["Nq"], c["Nk"]) if c["kind"] == "fwd" else None
    return x


def reference_forward_for(c, x):
    """What the backward of a case is fed: the REFERENCE's P rounded to the slab type and its O as fp32 (``o`` None where the case runs
    without)."""
    f = fwd_ref(x["q"], x["k"], x["v"], scale_of(c), c["mode"], None, c["slab"])
    return f["slab"], (f["O"].astype(F32) if c["o"] else None)
