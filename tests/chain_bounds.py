"""Float64 references, counted rounding bounds, input families, mutants and the case tables for the kernels of the self-attention
relevancy chain  ``R <- R + A_bar_l . R``,  ``A_bar_l = mean_h clamp(G_l * A_l, 0)``:  ``avg_heads_kernel``, ``self_chain_fused_kernel``
(plain and software-pipelined stream loop), ``self_chain_groups_kernel``, ``self_chain_cols_kernel``, the one-launch-per-layer kernel of
``csrc/relevancy_chain_rows.hip``, the split path on ``bmm_f32_kernel<32 / 64>`` and ``bmm_f32_tiles_kernel``, and the vector chain
(``chain_matvec``, ``chain_vecmat_*``, ``avg_heads_vecmat_*``).  CPU only (numpy), on top of ``tests/rowwise_bounds.py`` and
``tests/attention_bf16_bounds.py`` (imported, not changed): ``tests/test_chain_bounds_host.py`` proves the bounds and the mutants here,
``tests/test_gpu_chain_bounds.py`` holds the kernels to them.  The fp16-mode chain (``mmx_relevancy_self_chain_half``) is not judged here.

Reference.  Float64 of the DEFINITION on the operands as handed in (16-bit slabs convert exactly to fp32: nothing is re-rounded):

    A_bar = (1 / H) sum_h max(G A, 0)      NaN propagates like torch.clamp;  the chain is sequential in layer order from R_0 = I or the
    given R_init (R_sq likewise when M > 0).   Vector forms: base + A y, base + x A, base + x A_bar; relevancy_chain_row is the row of R.

Bounds, per element, to first order in ``u = 2**-24``, each with the ``2**-126`` term for results below the normal range.  A dot product
of n fp32 terms on the fp32 MFMA or in FMA code errs by at most ``(n + 1) u sum |a_i b_i|`` in any order and grouping (zeros of the
padding add nothing).

* ``A_bar``: every term is >= 0, so sum |terms| = H A_bar.  One product, H in-order additions (the first one, onto 0, is exact) and the division (avg_heads_kernel in
  relevancy_kernels.hip; reduce_chunk and the pipelined loop's consume in relevancy_chain_fused.hip; consume in chain_stream.h;
  stream_block in relevancy_chain_rows.hip):  ``e_A = (H + 2) u A_bar``.  The 16-bit element-wise
  tail of each has the same count.
* one layer, ``P = A_bar |R|`` in float64:  ``E' = E + A_bar E + e_A |R| + (N + 1) u P + u |R'|`` -- the propagated error of R, the
  error of A_bar, the product of N terms on v_mfma_f32_16x16x4_f32 (chain_tile_product in chain_matrix.h for the three N <= 128
  kernels; 32x32x2 in the rows kernel's multiply and in bmm_f32_tiles.hip; bmm_f32_kernel in relevancy_kernels.hip) and the addition
  ``R + (A_bar . R)`` (each kernel's layer loop; the Cin addition of the product kernels' epilogues).
* layer groups (G > 1: the hand-off + combine sections of self_chain_fused_kernel and self_chain_groups_kernel): each ``P_g = prod (I + A_bar_l)`` carries its own ``E_g`` by the recurrence
  above (group 0 starts at R_init); the combine ``acc <- P_g . acc`` (no addition) adds
  ``|P_g| e_acc + E_g |acc| + (N + 1) u |P_g| |acc|``.  The reference stays the sequential chain: the bound licenses the re-association.
* ``bmm`` (mmx_bmm_f32: both general tile sizes, trans_a, Cin, the bias row behind mmx_linear_f32, the tiles kernel):
  ``(K + 1) u sum_k |a b|``, plus ``u |C|`` for the Cin addition (the epilogues of bmm_f32_kernel and bmm_f32_tiles_kernel).  nan_to_zero: a NaN of the reference is 0.
* split path and rows kernel: the one-layer recurrence with these pieces.  The rows kernel's first layer from the identity is
  ``I + A_bar`` (chain_rows_layer_kernel, R_in == nullptr): no product, ``e_A`` and the addition ``u |R'|`` (exact off the diagonal, where it adds 0).
* ``chain_matvec`` (chain_matvec_kernel): a term passes its product, at most 4 additions per chunk step of its lane
  (``ceil((N / 4) / 64)`` steps; the tail element adds one more), six shuffle steps, then the base:  ``(4 steps + 8) u sum |A y| + u |out|``.
* ``chain_vecmat`` (chain_vecmat_partial_kernel, chain_vecmat_reduce_kernel): product, up to 32 additions in the row chunk, ``ceil(N / 32)`` in the chunk sum, then the base:
  ``(33 + ceil(N / 32)) u sum |x A| + u |out|``.
* ``avg_heads_vecmat`` (avg_heads_vecmat_partial_kernel, avg_heads_vecmat_reduce_kernel): ``e_A |x|`` on every term, the product with x,
  three additions of the four rows in LDS, ``ceil(N / 4)`` in the chunk sum, the base:  ``sum_r |x_r| e_A + (4 + ceil(N / 4)) u sum |x A_bar| + u |out|``.
* ``relevancy_chain_row``: N <= 128 the row of the fused chain's bound; longer, ``x <- x + x A_bar_l`` from the top layer down with
  ``e' = e + e A_bar + |x| e_A + (33 + ceil(N / 32)) u |x| A_bar + u |x'|``.

The bounds rest on the hardware properties ``tests/attention_f32_bounds.py`` states and does not measure either: the fp32 MFMA rounds
each product and each addition to nearest, it keeps subnormal operands and results, and its zero padding contributes exact zeros.

Input families (all seeded): ``plain`` softmax of randn, gradients 0.05 randn (the generators' regime) | ``hot`` gradients x 100, R grows
by orders of magnitude | ``peaked`` softmax of 8 randn | ``signed_init`` R_init = randn | ``causal`` softmax under the -inf upper
triangle, gradients finite and large above the diagonal | ``tiny`` gradients x 2**-100 | ``nan`` one NaN gradient in sample 0 |
``inf`` one +inf gradient on a positive probability in head H - 1 of sample 0, H % 4 != 0, every other gradient positive, in the LAST
layer.  (Why the last layer and positive gradients: an infinity that is in R when another product follows meets exact zeros -- of the
identity, of a clamped product, of the MFMA tiles' padding -- and 0 * inf = NaN, where and whether depends on the association; with the
infinity entering in the last product on all-positive operands its place is decided by the real operands alone: row i of R is +inf.
With layer groups the last group holds two layers for the same reason: alone, its ``I + A_bar_L`` would multiply the identity's zeros.)"""
import numpy as np

from attention_bf16_bounds import TINY, judge, ratio, slab_round
from rowwise_bounds import F32, U

__all__ = ["F32", "U", "TINY", "judge", "ratio"]

FAMILIES = ("plain", "hot", "peaked", "signed_init", "causal", "tiny", "nan", "inf")
FINITE = FAMILIES[:6]
DTYPES = ("f32", "f16", "bf16")
CUS = 256                                   # compute units of an MI355X: the grid rule of bmm_f32_tiles_try (bmm_f32_tiles.hip:200)


def f64(a):
    return np.asarray(a, np.float64)


def _al(n):
    return (n + 255) // 256 * 256


# ---------------------------------------------------------------------------------------------------------------------
# routes: which kernel a chain case must reach (chain_route in relevancy_chain.hip)
# ---------------------------------------------------------------------------------------------------------------------
def groups_lds_ok(nt, per):
    """``groups_lds_bytes`` <= 160 KiB (``self_chain_groups_applies`` in relevancy_chain_groups.hip)."""
    return 4 * (max(per, 3) * nt * 16 * (nt * 16 + 4) + per * nt + 8) <= 160 * 1024


def pipe_cpl(N, H, pipe):
    """Chunks per lane of the fused kernel's pipelined stream loop, 0 = the plain loop (the work split, the pipelined form's condition and
    ``run_cpl`` in self_chain_fused_kernel; the N * N >= 1600 rule of mmx_relevancy_self_chain_flags)."""
    NN, nt = N * N, -(-N // 16)
    if not pipe or NN < 1600 or nt >= 16:
        return 0
    nchunks, LT, ML = (NN + 3) // 4, 1024 - nt * 64, nt * 64
    full = nchunks // LT
    split = full >= 1 and nchunks - full * LT <= ML
    stream_end = full * LT if split else nchunks
    if not (stream_end * 4 <= NN and stream_end > 0):
        return 0
    nws = LT // 64
    if pipe >= 4 and stream_end >= nws * 256:
        return 4
    if pipe >= 2 and stream_end >= nws * 128:
        return 2
    return 1


def bmm_kernel(batch, M, N, K, trans_a=False, tiles=1):
    """``launch_bmm`` (relevancy_kernels.hip) and ``bmm_f32_tiles_try`` (bmm_f32_tiles.hip) on 256 compute units."""
    w64 = -(-N // 64) * -(-M // 64) * batch
    if tiles and not trans_a and M >= 96 and N >= 96 and K >= 32 and w64 >= CUS:
        return "tiles"
    return "bmm64" if w64 >= 1024 else "bmm32"


def chain_route(c):
    """-> ``(kernel, G, cpl, bmm)``: ``fused`` | ``cols`` | ``groups`` | ``split`` | ``rows``; the group count (1 outside the N <= 128
    kernels), the pipelined loop's chunks per lane (fused only, 0 = plain loop) and the product kernel of the split path.  An independent
    restatement of ``chain_route`` in csrc/relevancy_chain.hip (with ``chain_groups`` already applied: ``c["groups"]``), the tests' reference
    for the dispatcher."""
    N, H, L, B, M = c["N"], c["H"], c["L"], c["B"], c["M"]
    nt = -(-N // 16)
    f32 = c["dtype"] == "f32"
    if nt <= 8 and M == 0:
        G = 1 if L < 2 else min(c["groups"], L)
        if c["algo"] != 1 and f32 and L >= 1 and (c["algo"] == 5 or (N >= 40 and G == 1)):
            return "cols", 1, 0, None
        if G > 1 and c["algo"] != 1 and f32 and L >= G and groups_lds_ok(nt, -(-L // G)):
            return "groups", G, 0, None
        return "fused", G, (pipe_cpl(N, H, c["pipe"]) if f32 else 0), None
    bk = bmm_kernel(B, N, N, N)
    if c["rows"] and M == 0 and 128 < N <= 636:
        return "rows", 1, 0, None
    return "split", 1, 0, bk


def workspace_bytes(c):
    """What ``mmx_self_chain_workspace_bytes`` must answer for the route (``chain_workspace_bytes`` in relevancy_chain.hip)."""
    N, B, M = c["N"], c["B"], c["M"]
    if -(-N // 16) <= 8 and M == 0:
        return 0 if c["kernel"] == "cols" or c["G"] == 1 else _al(4 * B) + _al(4 * B * c["G"] * N * N)
    return 2 * _al(4 * B * N * N) + (_al(4 * B * N * M) if M else 0)


def group_spans(L, G):
    per = -(-L // G)
    return [(min(L, g * per), min(L, g * per + per)) for g in range(G)]


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _softmax32(s):
    with np.errstate(invalid="ignore"):
        e = np.exp(s - s.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(F32)


def poison_at(c):
    """``(layer, head, row, col)`` of the NaN / inf gradient of sample 0."""
    N, L, H = c["N"], c["L"], c["H"]
    layer = L - 1 if c["family"] == "inf" or c["seed"] % 2 == 0 else 0
    return layer, H - 1, min(1, N - 1), min(2, N - 1)


def chain_inputs(c, poisoned=True):
    """-> dict ``attn`` / ``grad``: lists of fp32 arrays ``[B or 1, H, N, N]`` / ``[B, H, N, N]`` holding values of the slab type,
    ``R_init [B, N, N]`` or None, ``R_sq_init [B, N, M]`` or None."""
    rng = np.random.default_rng(1000 + c["seed"])
    N, H, L, B, M, fam = c["N"], c["H"], c["L"], c["B"], c["M"], c["family"]
    Ba = 1 if c["shared"] else B
    attn, grad = [], []
    upper = np.triu(np.ones((N, N), bool), 1)
    for _ in range(L):
        s = rng.standard_normal((Ba, H, N, N)) * (8.0 if fam == "peaked" else 1.0)
        if fam == "causal":
            s = np.where(upper, -np.inf, s)
        g = rng.standard_normal((B, H, N, N)) * 0.05
        if fam == "hot":
            g = g * 100.0
        elif fam == "causal":
            g = np.where(upper, g * 1000.0, g)
        elif fam == "inf":
            g = np.abs(g) + 2.0 ** -10
        g = g.astype(F32)
        if fam == "tiny":
            g = np.ldexp(g, -100).astype(F32)
        attn.append(slab_round(_softmax32(s), c["dtype"]))
        grad.append(slab_round(g, c["dtype"]))
    if poisoned and fam in ("nan", "inf") and L:
        l, h, i, j = poison_at(c)
        grad[l][0, h, i, j] = np.nan if fam == "nan" else np.inf
        assert attn[l][0, h, i, j] > 0
    R0 = SQ0 = None
    if c["init"]:
        if fam == "signed_init":
            R0 = rng.standard_normal((B, N, N)).astype(F32)
        else:
            R0 = (np.eye(N) + rng.random((B, N, N)) * 0.1 + 2.0 ** -10).astype(F32)
    if M:
        SQ0 = (rng.standard_normal((B, N, M)) if fam == "signed_init" else rng.random((B, N, M)) * 0.1).astype(F32)
    return {"attn": attn, "grad": grad, "R_init": R0, "R_sq_init": SQ0}


# ---------------------------------------------------------------------------------------------------------------------
# float64 references and bounds
# ---------------------------------------------------------------------------------------------------------------------
def abar_ref(a, g):
    """``a [B or 1, H, Nq, Nk]``, ``g [B, H, Nq, Nk]`` -> ``(A_bar, e_A)`` float64 ``[B, Nq, Nk]``."""
    Hh = g.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        x = f64(g) * f64(a)
        x = np.where(x < 0, 0.0, x)                 # a NaN is not < 0: it stays, like torch.clamp(min=0)
        A = x.sum(1) / Hh
        return A, (Hh + 2) * U * A + TINY


def _step(A, eA, R, E, n):
    """One layer ``R' = R + A R`` and its bound."""
    with np.errstate(invalid="ignore", over="ignore"):
        aR = np.abs(R)
        Rn = R + np.matmul(A, R)
        En = E + np.matmul(A, E) + np.matmul(eA, aR) + (n + 1) * U * np.matmul(A, aR) + U * np.abs(Rn) + TINY
    return Rn, En


def _eye(B, N):
    return np.broadcast_to(np.eye(N), (B, N, N)).copy()


def chain_ref(c, x):
    """-> dict ``R e_R`` (and ``SQ e_SQ`` when M > 0) ``[B, N, N]`` / ``[B, N, M]`` float64: the sequential chain and the bound of the
    route ``c["kernel"]``, plus ``A`` / ``e_A``: the per-layer head means."""
    N, B, L = c["N"], c["B"], c["L"]
    As = [abar_ref(a, g) for a, g in zip(x["attn"], x["grad"])]
    R0 = _eye(B, N) if x["R_init"] is None else f64(x["R_init"])
    zero = np.zeros((B, N, N))
    R, E = R0, zero
    seq = []
    for l, (A, eA) in enumerate(As):
        if c["kernel"] == "rows" and l == 0 and x["R_init"] is None:
            Rn = _step(A, eA, R, E, N)[0]           # the VALUE is the definition's (A_bar . I: a NaN takes its whole row along)
            with np.errstate(invalid="ignore"):
                R, E = Rn, eA + U * np.abs(Rn) * np.eye(N) + TINY
        else:
            R, E = _step(A, eA, R, E, N)
        seq.append(R)
    out = {"R": R, "e_R": E, "A": [a for a, _ in As], "e_A": [e for _, e in As]}
    if c["G"] > 1:
        acc = e = None
        for g, (l0, l1) in enumerate(group_spans(L, c["G"])):
            P, Eg = (R0 if g == 0 else _eye(B, N)), zero
            for A, eA in As[l0:l1]:
                P, Eg = _step(A, eA, P, Eg, N)
            if g == 0:
                acc, e = P, Eg
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    aP, aacc = np.abs(P), np.abs(acc)
                    e = np.matmul(aP, e) + np.matmul(Eg, aacc) + (N + 1) * U * np.matmul(aP, aacc) + TINY
                    acc = np.matmul(P, acc)
        out["e_R"] = e
        out["R_grouped"] = acc
    if c["M"]:
        SQ, Es = f64(x["R_sq_init"]), np.zeros((B, N, c["M"]))
        for A, eA in As:
            SQ, Es = _step(A, eA, SQ, Es, N)
        out["SQ"], out["e_SQ"] = SQ, Es
    return out


def bmm_ref(a, b, cin=None, trans_a=False, nan_to_zero=False, bias_row=False):
    """``op(a) b (+ cin)`` float64 and its bound; ``cin`` is ``[batch, M, N]`` or, ``bias_row``, ``[N]``."""
    A = np.swapaxes(f64(a), -1, -2) if trans_a else f64(a)
    Bm = f64(b)
    K = A.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        C = np.matmul(A, Bm)
        e = (K + 1) * U * np.matmul(np.abs(A), np.abs(Bm)) + TINY
        if cin is not None:
            C = C + f64(cin)
            e = e + U * np.abs(C)
        if nan_to_zero:
            C = np.where(np.isnan(C), 0.0, C)
            e = np.where(np.isfinite(e), e, TINY)
    return C, e


def matvec_ref(A, y, base):
    N = A.shape[-1]
    steps = -(-(N // 4) // 64)
    s = np.einsum("bij,bj->bi", f64(A), f64(y))
    out = f64(base) + s
    return out, (4 * steps + 8) * U * np.einsum("bij,bj->bi", np.abs(f64(A)), np.abs(f64(y))) + U * np.abs(out) + TINY


def vecmat_consts(N):
    return 33 + -(-N // 32)


def vecmat_ref(x, A, base):
    N = A.shape[-1]
    out = f64(base) + np.einsum("bi,bij->bj", f64(x), f64(A))
    return out, vecmat_consts(N) * U * np.einsum("bi,bij->bj", np.abs(f64(x)), np.abs(f64(A))) + U * np.abs(out) + TINY


def ahv_ref(x, a, g, base):
    N = g.shape[-1]
    A, eA = abar_ref(a, g)
    ax = np.abs(f64(x))
    with np.errstate(invalid="ignore"):
        out = f64(base) + np.einsum("bi,bij->bj", f64(x), A)
        e = np.einsum("bi,bij->bj", ax, eA) + (4 + -(-N // 4)) * U * np.einsum("bi,bij->bj", ax, A) + U * np.abs(out) + TINY
    return out, e


def chain_row_ref(c, x, rows):
    """Row ``rows[b]`` of the chain: N <= 128 picked from ``chain_ref``; longer, the vector recurrence's bound on the same reference."""
    N, B = c["N"], c["B"]
    pick = np.arange(B)
    if N <= 128:
        r = chain_ref(c, x)
        return r["R"][pick, rows], r["e_R"][pick, rows]
    As = [abar_ref(a, g) for a, g in zip(x["attn"], x["grad"])]
    v = np.zeros((B, N))
    v[pick, rows] = 1.0
    e = np.zeros((B, N))
    k = vecmat_consts(N)
    for A, eA in reversed(As):
        av = np.abs(v)
        vn = v + np.einsum("bi,bij->bj", v, A)
        e = e + np.einsum("bi,bij->bj", e, A) + np.einsum("bi,bij->bj", av, eA) + k * U * np.einsum("bi,bij->bj", av, A) \
            + U * np.abs(vn) + TINY
        v = vn
    return v, e


# ---------------------------------------------------------------------------------------------------------------------
# fp32 restatements: numpy float32 in each kernel's own order of operations; ``mut`` plants ONE defect (the mutants below)
# ---------------------------------------------------------------------------------------------------------------------
def _f(x):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.asarray(x).astype(F32)


def abar32(a, g, mut=None, causal_flag=False):
    """Heads summed in ascending order in one fp32 accumulator, then the division."""
    a, g = np.asarray(a, F32), np.asarray(g, F32)
    B, Hh, Nq, Nk = g.shape
    NN = Nq * Nk
    if mut == "shared_forward_read_with_sample_stride" and a.shape[0] == 1 and B > 1:
        a = np.concatenate([a, np.full((B - 1,) + a.shape[1:], np.nan, F32)])      # what lies behind the one shared slab: the NaN margin
    s = np.zeros((B, Nq, Nk), F32)
    flat = np.arange(NN).reshape(Nq, Nk)
    ragged = flat >= 4 * (NN // 4)
    dead = np.zeros((Nq, Nk), bool)
    if mut == "causal_skip_drops_straddling_chunk" and causal_flag:
        p0 = (flat // 4) * 4                                        # the chunk's first element: above the diagonal, the chunk wraps
        r0, c0 = p0 // Nk, p0 % Nk
        dead = (c0 > r0) & (c0 + 3 >= Nk)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if mut == "clamp_after_head_mean":
            for h in range(Hh):
                s = _f(s + _f(g[:, h] * a[:, h]))
            m = _f(s / F32(Hh))
            return np.where(m < 0, F32(0), m)
        for h in range(Hh):
            t = _f(g[:, h] * a[:, h])
            t = np.where(t < 0, F32(0), t)
            if mut == "last_head_dropped_in_ragged_chunk" and h == Hh - 1 and Hh > 1:
                t = np.where(ragged, F32(0), t)
            t = np.where(dead, F32(0), t)
            s = _f(s + t)
        if mut == "padding_head_weighted_by_zero" and Hh % 4:
            t = _f(g[:, Hh - 1] * a[:, Hh - 1])
            s = _f(s + _f(np.where(t < 0, F32(0), t) * F32(0)))     # the clamped duplicate of head H - 1, times w = 0
        return _f(s / F32(Hh))


def k_groups(n, how):
    """The contraction index in the groups one MFMA instruction sums: ``mfma16`` k = 16 t + 4 q + r per (t, r)
    (chain_tile_product in chain_matrix.h); ``slab4`` four consecutive k (bmm_f32_kernel); ``pair`` {8 j + t, 8 j + 4 + t}
    (v_mfma_f32_32x32x2_f32: bmm_f32_tiles.hip:151-166, relevancy_chain_rows.hip:229-235)."""
    out = []
    if how == "mfma16":
        for t in range(-(-n // 16)):
            for r in range(4):
                out.append([k for k in (16 * t + 4 * q + r for q in range(4)) if k < n])
    elif how == "slab4":
        out = [list(range(k, min(k + 4, n))) for k in range(0, n, 4)]
    else:
        for j in range(-(-n // 8)):
            for t in range(4):
                out.append([k for k in (8 * j + t, 8 * j + 4 + t) if k < n])
    return [np.array(g) for g in out if g]


def mm32(a, b, how="mfma16", mut=None):
    """``a @ b`` in fp32, the contraction summed group by group into one accumulator."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if mut == "product_operands_rounded_to_bf16":
        a, b = slab_round(a, "bf16"), slab_round(b, "bf16")
    acc = np.zeros(a.shape[:-1] + (b.shape[-1],), F32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for idx in k_groups(a.shape[-1], how):
            acc = _f(acc + _f(np.matmul(a[..., idx], b[..., idx, :])))
    return acc


def _layer32(A, R, how, mut=None, stale=False):
    with np.errstate(invalid="ignore", over="ignore"):
        Rn = _f(R + mm32(A, R, how, mut))
        if stale and R.shape[-2] > 16:              # rows 16 .. 31 of the product read rows 0 .. 15 of the UPDATED R
            mix = R.copy()
            mix[..., :16, :] = Rn[..., :16, :]
            Rn[..., 16:32, :] = _f(R[..., 16:32, :] + mm32(A[..., 16:32, :], mix, how))
    return Rn


def chain_restatement(c, x, mut=None):
    """The chain of a case in fp32 in the order of its route -> dict ``R`` (``SQ``)."""
    N, B, L, G = c["N"], c["B"], c["L"], c["G"]
    As = [abar32(a, g, mut, c["causal_flag"]) for a, g in zip(x["attn"], x["grad"])]
    eye = np.broadcast_to(np.eye(N, dtype=F32), (B, N, N)).copy()
    R0 = eye if x["R_init"] is None else np.asarray(x["R_init"], F32)
    how = {"split": "pair" if c["bmm"] == "tiles" else "slab4", "rows": "pair"}.get(c["kernel"], "mfma16")
    stale_at = L - 1 if mut == "row_block_reads_updated_R" else -1
    out = {}
    if G > 1:
        parts = []
        for g, (l0, l1) in enumerate(group_spans(L, G)):
            P = R0 if (g == 0 or mut == "R_init_applied_by_every_group") else eye
            for l in range(l0, l1):
                P = _layer32(As[l], P, how, mut, l == stale_at)
            parts.append(P)
        acc = parts[0]
        for P in parts[1:]:
            acc = mm32(acc, P, how, mut) if mut == "group_combine_in_wrong_order" else mm32(P, acc, how, mut)
        out["R"] = acc
    else:
        R = R0
        for l, A in enumerate(As):
            if c["kernel"] == "rows" and l == 0 and x["R_init"] is None:
                bad = ~np.isfinite(A)               # rows:159-: I + A_bar, NaN where ANOTHER element of the row is NaN / inf (0 * inf)
                R = np.where(bad.sum(-1, keepdims=True) - bad > 0, F32(np.nan), _f(A + eye))
            else:
                R = _layer32(A, R, how, mut, l == stale_at)
        out["R"] = R
    if c["M"]:
        SQ = np.asarray(x["R_sq_init"], F32)
        for A in As:
            SQ = _layer32(A, SQ, "slab4", mut)
        out["SQ"] = SQ
    return out


def bmm_restatement(a, b, cin=None, trans_a=False, nan_to_zero=False, how="slab4", mut=None):
    A = np.swapaxes(np.asarray(a, F32), -1, -2) if trans_a else np.asarray(a, F32)
    Bm = np.asarray(b, F32)
    K = A.shape[-1]
    if mut == "last_K_slab_dropped" and K % 32 and K > 32:
        A, Bm = A[..., :32 * (K // 32)], Bm[..., :32 * (K // 32), :]
    C = mm32(A, Bm, how)
    with np.errstate(invalid="ignore", over="ignore"):
        if cin is not None:
            C = _f(np.asarray(cin, F32) + C)
            if mut == "Cin_added_twice":
                C = _f(np.asarray(cin, F32) + C)
        if nan_to_zero:
            C = np.where(np.isnan(C), F32(0), C)
    return C


def _tree(x):
    while x.shape[-1] > 1:
        x = _f(x[..., 0::2] + x[..., 1::2])
    return x[..., 0]


def matvec_restatement(A, y, base, mut=None):
    """Lane l: chunks l, l + 64, ... of four products each, then its tail element; the xor butterfly; the base."""
    A, y, base = np.asarray(A, F32), np.asarray(y, F32), np.asarray(base, F32)
    B, N, _ = A.shape
    n4 = N // 4
    t = _f(A * y[:, None, :])
    lanes = np.zeros((B, N, 64), F32)
    for j in range(n4):
        q = t[..., 4 * j:4 * j + 4]
        lanes[..., j % 64] = _f(lanes[..., j % 64] + _f(_f(_f(q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]))
    if mut != "matvec_tail_dropped":
        for j in range(4 * n4, N):
            lanes[..., j - 4 * n4] = _f(lanes[..., j - 4 * n4] + t[..., j])
    return _f(base + _tree(lanes))


def vecmat_restatement(x, A, base, mut=None):
    """32-row partials, each one accumulator over its rows; the partials added in order; the base."""
    x, A, base = np.asarray(x, F32), np.asarray(A, F32), np.asarray(base, F32)
    B, N, _ = A.shape
    chunks = -(-N // 32)
    s = np.zeros((B, N), F32)
    for ch in range(chunks):
        if mut == "vecmat_partial_dropped" and ch == chunks - 1 and chunks > 1:
            continue
        acc = np.zeros((B, N), F32)
        for r in range(32 * ch, min(N, 32 * ch + 32)):
            acc = _f(acc + _f(A[:, r, :] * x[:, r, None]))
        s = _f(s + acc)
    return _f(base + s)


def ahv_restatement(x, a, g, base, mut=None):
    """The head mean times x per row, four rows added in LDS, the 4-row partials added in order, the base."""
    x, base = np.asarray(x, F32), np.asarray(base, F32)
    A = abar32(a, g, mut)
    B, N, _ = A.shape
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = _f(A * x[:, :, None])
        s = np.zeros((B, N), F32)
        for ch in range(-(-N // 4)):
            rows = [v[:, r] if r < N else np.zeros((B, N), F32) for r in range(4 * ch, 4 * ch + 4)]
            s = _f(s + _f(_f(_f(rows[0] + rows[1]) + rows[2]) + rows[3]))
        return _f(base + s)


def chain_row_restatement(c, x, rows, mut=None):
    N, B = c["N"], c["B"]
    pick = np.arange(B)
    if N <= 128:
        return chain_restatement(c, x, mut)["R"][pick, rows]
    v = np.zeros((B, N), F32)
    v[pick, rows] = 1.0
    for a, g in zip(reversed(x["attn"]), reversed(x["grad"])):
        v = vecmat_restatement(v, abar32(a, g, mut), v, mut)
    return v


def old_rule_passes(got, ref):
    """The tolerance ``tests/test_gpu_ops.py`` holds the chain to: ``1e-5 + 1e-5 |ref|`` per element and ``1e-4 max |ref|``."""
    err = np.abs(f64(got) - f64(ref))
    return bool((err <= 1e-5 + 1e-5 * np.abs(ref)).all() and err.max() <= 1e-4 * np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------------
# mutants: name -> (table, where it applies: case -> bool).  Each is an fp32 restatement with ONE defect and must put a stored output
# at >= 2x its bound in at least one row where it applies.
# ---------------------------------------------------------------------------------------------------------------------
def _finite(c):
    return c["family"] in FINITE


MUTANTS = {
    "last_head_dropped_in_ragged_chunk": ("chain", lambda c: _finite(c) and c["N"] * c["N"] % 4 and c["H"] > 1 and c["L"] > 0),
    "clamp_after_head_mean": ("chain", lambda c: _finite(c) and c["H"] > 1 and c["L"] > 0),
    "row_block_reads_updated_R": ("chain", lambda c: _finite(c) and c["N"] > 16 and c["L"] > 1 and c["kernel"] != "rows"),
    "group_combine_in_wrong_order": ("chain", lambda c: _finite(c) and c["G"] > 1),
    "R_init_applied_by_every_group": ("chain", lambda c: _finite(c) and c["G"] > 1 and c["init"]),
    "shared_forward_read_with_sample_stride": ("chain", lambda c: _finite(c) and c["shared"] and c["B"] > 1 and c["L"] > 0),
    "causal_skip_drops_straddling_chunk": ("chain", lambda c: c["causal_flag"] and c["N"] % 4 and c["N"] > 4 and c["L"] > 0),
    "product_operands_rounded_to_bf16": ("chain", lambda c: _finite(c) and c["L"] > 1 and c["N"] > 1),
    "padding_head_weighted_by_zero": ("chain", lambda c: c["family"] == "inf"),
    "last_K_slab_dropped": ("bmm", lambda c: c["K"] % 32 and c["K"] > 32),
    "Cin_added_twice": ("bmm", lambda c: c["cin"] and not c["nan"]),
    "vecmat_partial_dropped": ("vec", lambda c: c["op"] == "vecmat" and c["N"] > 32),
    "matvec_tail_dropped": ("vec", lambda c: c["op"] == "matvec" and c["N"] % 4),
}


# ---------------------------------------------------------------------------------------------------------------------
# case tables (shared by the host proof and the device test)
# ---------------------------------------------------------------------------------------------------------------------
NS = (1, 5, 15, 16, 17, 33, 39, 40, 50, 77, 96, 97, 112, 113, 127, 128)      # every NT = ceil(N / 16); 96 is NT = 6
HS = (1, 3, 5, 8, 12)
NS_LONG = (129, 130, 160, 197, 255, 260)


def _chain(i, N, H, L, B, **kw):
    c = {"kind": "chain", "N": N, "H": H, "L": L, "B": B, "M": 0, "family": "plain", "dtype": "f32", "algo": 4, "groups": 1, "pipe": 4,
         "cols_c": 0, "rows": 0, "shared": False, "init": False, "causal_flag": False, "misaligned": False, "plan": False, "seed": i}
    c.update(kw)
    if c["family"] == "signed_init" or c["L"] == 0:
        c["init"] = True
    if c["family"] == "tiny" and c["dtype"] == "f16":
        c["dtype"] = "bf16"                         # (2**-100 is no fp16 number)
    if c["family"] in ("nan", "inf"):
        c["B"] = max(c["B"], 2)
    if c["plan"]:
        c["init"] = False
    c["kernel"], c["G"], c["cpl"], c["bmm"] = chain_route(c)
    c["id"] = "%s%s-%dx%dx%dx%d-%s-%s-%d" % (c["kernel"], ("-g%d" % c["G"]) if c["G"] > 1 else "", L, B, H, N, c["family"], c["dtype"], i)
    return c


def chain_small_cases():
    out = []
    n = 0
    Ls = (1, 2, 3, 7, 12, 2)
    for i, N in enumerate(NS):                                      # every NT, every algo, one group
        for j, algo in enumerate((1, 4, 5)):
            k = i + j
            L = Ls[(i + 2 * j) % 6]
            if N >= 97 and L == 12 and k % 2:
                L = 7
            out.append(_chain(n, N, HS[k % 5], L, (1, 2, 3)[k % 3], algo=algo, family=FINITE[k % 6], pipe=(4, 0, 1, 2)[k % 4],
                              cols_c=(0, 1, 2, 3)[k % 4] if algo == 5 else 0, shared=k % 4 == 1, init=k % 5 == 2,
                              causal_flag=FINITE[k % 6] == "causal" and i % 2 == 0, misaligned=k % 3 == 2))
            n += 1
    n = 100
    for i, N in enumerate((17, 33, 50, 77, 96, 112, 113, 128)):    # layer groups: both kernels, L % G != 0, the LDS limit at 112 / 113
        for j, G in enumerate((2, 3, 4)):
            for a, algo in enumerate((1, 4)):
                k = i + j + a
                L = (2, 3, 5, 7, 12)[(i + j) % 5]
                if L < G:
                    L = G + 1
                if N >= 112 and L == 12:
                    L = 7
                out.append(_chain(n, N, HS[(k + 1) % 5], L, (2, 1, 3)[k % 3], algo=algo, groups=G, family=FINITE[(k + 2) % 6],
                                  pipe=(4, 2, 1, 0)[k % 4], shared=k % 4 == 2, init=k % 3 == 0,
                                  causal_flag=FINITE[(k + 2) % 6] == "causal" and j % 2 == 0, misaligned=k % 5 == 4))
                n += 1
    out.append(_chain(n, 77, 8, 12, 2, groups=2, family="causal", causal_flag=True))          # six images per group
    out.append(_chain(n + 1, 77, 3, 12, 1, groups=3, family="hot"))                            # four images per group
    out.append(_chain(n + 2, 50, 12, 12, 3, groups=2, algo=1, family="plain", init=True))
    n = 200
    for i, N in enumerate((5, 16, 39, 50, 77, 128)):               # no layers: R_init comes back
        out.append(_chain(n, N, 1, 0, (1, 2, 3)[i % 3], algo=(1, 4, 5)[i % 3], family=("plain", "signed_init")[i % 2]))
        n += 1
    for i, (N, H, L, B, G) in enumerate(((50, 12, 3, 2, 1), (77, 8, 4, 3, 2), (17, 3, 2, 1, 1), (128, 5, 2, 2, 1), (113, 3, 3, 2, 2))):
        out.append(_chain(n, N, H, L, B, groups=G, plan=True, family=("plain", "causal")[i % 2], causal_flag=i % 2 == 1))
        n += 1
    n = 300
    for i, N in enumerate((5, 15, 17, 33, 39, 50, 77, 97, 113, 128)):      # 16-bit slabs: the fused kernel's plain loop
        for j, dt in enumerate(("f16", "bf16")):
            k = i + j
            out.append(_chain(n, N, HS[(k + 2) % 5], (2, 3, 1, 7)[k % 4], (2, 3, 1)[k % 3], dtype=dt, family=FINITE[(k + 1) % 6],
                              groups=(1, 2, 1, 3)[k % 4], shared=k % 3 == 0, init=k % 4 == 3, misaligned=k % 4 == 1))
            n += 1
    n = 400
    # NaN / inf: every N <= 128 kernel; the pipelined loop at 1, 2 and 4 chunks per lane, with padding heads (H % (4 / CPL) != 0)
    poison = ((50, 3, 4, 1), (50, 5, 1, 1), (77, 5, 4, 1), (77, 3, 2, 1), (77, 3, 1, 1), (128, 3, 2, 1), (128, 5, 1, 1), (113, 3, 4, 1),
              (113, 3, 4, 2), (97, 5, 2, 3), (40, 3, 1, 1), (33, 3, 4, 1), (17, 5, 0, 2), (127, 7, 2, 1), (96, 3, 4, 1))
    for i, (N, H, pipe, G) in enumerate(poison):
        for fam in ("nan", "inf"):
            for algo in (1, 4):
                if algo == 4 and fam == "inf" and i % 2:
                    continue
                out.append(_chain(n, N, H, 2 * G, 2 + i % 2, algo=algo, groups=G, pipe=pipe, family=fam,
                                  init=i % 4 == 3, shared=i % 5 == 4))
                n += 1
    return out


def chain_large_cases():
    out = []
    n = 500
    for i, N in enumerate(NS_LONG):
        for j, M in enumerate((0, 36)):
            for rows in (0, 1):
                k = i + j + rows
                fam = FAMILIES[(2 * i + j + 3 * rows) % 7]          # every family but inf (below)
                out.append(_chain(n, N, (2, 3, 1, 5)[k % 4], (2, 3, 1)[k % 3], (2, 1)[k % 2], M=M, rows=rows, family=fam,
                                  dtype=DTYPES[k % 3], shared=k % 4 == 3, init=k % 3 == 1, misaligned=k % 5 == 2))
                n += 1
    out.append(_chain(n, 636, 2, 2, 1, rows=1))
    out.append(_chain(n + 1, 639, 2, 2, 1, rows=1))                 # past the rows kernel's limit: the split path
    out.append(_chain(n + 2, 130, 1, 2, 29))                        # 9 x 29 workgroups: the product on the tiles kernel
    out.append(_chain(n + 3, 50, 3, 2, 2, M=36, family="hot"))      # a second right-hand side at N <= 128: the split path
    for i, (N, rows, dt) in enumerate(((130, 0, "f32"), (197, 1, "f32"), (160, 1, "bf16"), (129, 0, "f16"))):
        out.append(_chain(n + 4 + i, N, 3, 2, 2, rows=rows, dtype=dt, family="inf", init=i % 2 == 1))
    return out


def chain_cases():
    return chain_small_cases() + chain_large_cases()


def _bmm(i, batch, M, N, K, **kw):
    c = {"kind": "bmm", "batch": batch, "M": M, "N": N, "K": K, "trans_a": False, "cin": False, "nan": False, "bias_row": False,
         "tiles": 1, "signed": i % 2 == 1, "seed": i}
    c.update(kw)
    c["kernel"] = bmm_kernel(1 if c["bias_row"] else batch, M, N, K, c["trans_a"], c["tiles"])
    c["id"] = "%s-%dx%dx%dx%d-%d" % (c["kernel"], batch, M, N, K, i)
    return c


def bmm_cases():
    out = []
    shapes = ((1, 1, 1), (5, 7, 3), (31, 33, 32), (64, 64, 33), (65, 95, 17), (96, 96, 32), (100, 130, 47))
    n = 0
    for i, (M, N, K) in enumerate(shapes):
        for j in range(4):
            out.append(_bmm(n, (1, 3, 2, 5)[(i + j) % 4], M, N, K, trans_a=j == 1, cin=j in (2, 3), nan=j == 3))
            n += 1
    out.append(_bmm(n, 256, 65, 95, 17, cin=True))                  # 1024 workgroups of 64 x 64: bmm_f32_kernel<64>
    out.append(_bmm(n + 1, 256, 65, 95, 33, trans_a=True))
    out.append(_bmm(n + 2, 64, 96, 96, 32, cin=True))               # 256 workgroups: the tiles kernel
    out.append(_bmm(n + 3, 43, 100, 130, 47, nan=True))
    out.append(_bmm(n + 4, 43, 100, 130, 47, cin=True, tiles=0))    # option bmm_tiles = 0: the general kernel again
    out.append(_bmm(n + 5, 1, 100, 130, 47, cin=True, bias_row=True))          # mmx_linear_f32
    out.append(_bmm(n + 6, 1, 5, 7, 3, cin=True, bias_row=True))
    return out


def bmm_inputs(c):
    rng = np.random.default_rng(2000 + c["seed"])
    b_, M, N, K = c["batch"], c["M"], c["N"], c["K"]
    if c["bias_row"]:
        b_ = 1
    a = (rng.standard_normal((b_, M, K)) if c["signed"] else rng.random((b_, M, K)) / K).astype(F32)
    b = rng.standard_normal((b_, K, N)).astype(F32)
    if c["nan"]:
        a[0, M // 2, K // 2] = np.nan
    cin = None
    if c["cin"]:
        cin = rng.standard_normal((N,) if c["bias_row"] else (b_, M, N)).astype(F32)
    if c["trans_a"]:
        a = np.ascontiguousarray(np.swapaxes(a, -1, -2))
    return a, b, cin


def _vec(i, op, N, B, **kw):
    c = {"kind": "vec", "op": op, "N": N, "B": B, "H": 1, "dtype": "f32", "base": True, "shared": False, "family": "plain", "seed": i}
    c.update(kw)
    if op == "row":                                 # ops.relevancy_chain_row: N <= 128 picks the row of the default chain (one group)
        c.update(M=0, algo=4, groups=1, pipe=4, rows=0, init=False, causal_flag=False)
        c["kernel"], c["G"], c["cpl"], c["bmm"] = chain_route(c)
    c["id"] = "%s-%dx%dx%d-%s-%d" % (op, B, c["H"], N, c["dtype"], i)
    return c


def vec_cases():
    out = []
    n = 0
    for i, N in enumerate((1, 3, 4, 5, 31, 32, 33, 64, 65, 130, 260)):
        B = (1, 3)[i % 2]
        out.append(_vec(n, "matvec", N, B, base=i % 3 != 0))
        out.append(_vec(n + 1, "vecmat", N, 4 - B, base=i % 3 != 1))
        for j, H in enumerate((1, 3, 12)):
            if (i + j) % 3 == 0 or N in (5, 33, 65):
                out.append(_vec(n + 2 + j, "ahv", N, (3, 1)[(i + j) % 2], H=H, dtype=DTYPES[(i + j) % 3], base=(i + j) % 2 == 0,
                                shared=(i + j) % 4 == 1, family=("plain", "hot", "nan")[(i + j) % 3]))
        n += 5
    for i, (N, dt) in enumerate(((77, "f32"), (130, "f32"), (130, "bf16"), (77, "f16"))):
        out.append(_vec(n + i, "row", N, 3, H=3, dtype=dt, shared=i == 1, L=3))
    return out


def vec_inputs(c, poisoned=True):
    rng = np.random.default_rng(3000 + c["seed"])
    N, B, H = c["N"], c["B"], c["H"]
    x = {"v": rng.standard_normal((B, N)).astype(F32)}
    x["base"] = rng.standard_normal((B, N)).astype(F32) if c["base"] else x["v"]
    if c["op"] in ("matvec", "vecmat"):
        x["A"] = (rng.random((B, N, N)) / N * rng.integers(0, 2, (B, N, N))).astype(F32)
    else:
        L = c.get("L", 1)
        cc = dict(c, L=L, M=0, init=False)
        y = chain_inputs(cc, poisoned=False)
        x["attn"], x["grad"] = y["attn"], y["grad"]
        if c["family"] == "nan" and poisoned:
            x["grad"][0][0, H - 1, N // 2, N // 3] = np.nan
        x["rows"] = (np.arange(B) * 7 + 1) % N
    return x


def _avg(i, B, H, Nq, Nk, dt, shared=False, family="plain"):
    return {"kind": "avg", "B": B, "H": H, "Nq": Nq, "Nk": Nk, "dtype": dt, "shared": shared, "family": family, "seed": i,
            "id": "avg-%dx%dx%dx%d-%s-%d" % (B, H, Nq, Nk, dt, i)}


def avg_cases():
    out = []
    n = 0
    for i, (Nq, Nk) in enumerate(((1, 5), (33, 2), (9, 13), (1, 1), (7, 7), (50, 50), (77, 77), (4, 4), (3, 2), (130, 129))):
        for j, dt in enumerate(DTYPES):
            k = i + j
            out.append(_avg(n, (1, 2, 3)[k % 3], HS[k % 5], Nq, Nk, dt, shared=k % 4 == 1, family=("plain", "hot", "nan", "tiny")[k % 4]))
            n += 1
    return out


def avg_inputs(c, poisoned=True):
    rng = np.random.default_rng(4000 + c["seed"])
    B, H, Nq, Nk = c["B"], c["H"], c["Nq"], c["Nk"]
    a = _softmax32(rng.standard_normal((1 if c["shared"] else B, H, Nq, Nk)))
    g = (rng.standard_normal((B, H, Nq, Nk)) * {"hot": 5.0}.get(c["family"], 0.05)).astype(F32)
    if c["family"] == "tiny" and c["dtype"] != "f16":
        g = np.ldexp(g, -100).astype(F32)
    if c["family"] == "nan" and poisoned:
        g[0, H - 1, Nq // 2, Nk // 2] = np.nan
    return slab_round(a, c["dtype"]), slab_round(g, c["dtype"])
