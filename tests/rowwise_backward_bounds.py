"""Float64 references, counted rounding bounds, input families and mutants for the backward row-wise kernels of
``csrc/elementwise_kernels.hip``: the LayerNorm input gradient fused with the residual add (``layernorm_bwd_add_kernel``, its row-list
form and the bf16 gradient-stream kernels ``layernorm_bwd_add_bf16_row_kernel`` / ``layernorm_bwd_add_bf16_kernel``) and the bf16
QuickGELU backward (``quick_gelu_bwd_bf16_kernel``, ``quick_gelu_bwd_bf16_sweep_kernel``).  CPU only (numpy), on top of
``tests/rowwise_bounds.py`` (imported, not changed): ``tests/test_rowwise_backward_bounds_host.py`` proves the bounds and the input set
here, ``tests/test_gpu_rowwise_backward.py`` holds the kernels to them.

LayerNorm backward.  The reference is float64 of the kernel's DEFINITION on the fp32 operands as given -- ``mean`` / ``rstd`` are
inputs, taken as the fp32 numbers handed in -- with ``m = r % x_rows`` (K-major: row ``r`` of ``dy`` reads row ``r % x_rows`` of ``x``):

    g = dy gamma,  xh = (x[m] - mean[m]) rstd[m],  A = mean(g),  B = mean(g xh),  core = g - A - xh B,  o = core rstd[m] (+ d_res)

The bound counts the kernels' own roundings, to first order in ``u = 2**-24`` (an FMA contraction only removes roundings).  With
``NV = max(1, ceil(E / 256))`` 16-byte groups per lane, ``k = 4 NV + 8``, ``Ga = mean |g|``, ``Gb = mean |g xh|``:

* ``g_i``: one multiply, ``u |g_i|``.  ``xh_i``: the subtraction and the multiply, ``2 u |xh_i|``.
* ``a``: a term carries its own rounding (1), at most ``4 NV`` additions in its lane (three inside the group, one onto the running sum,
  per group), 6 in the xor butterfly and the division (1): ``|a - A| <= k u Ga``.
* ``b``: the same path, and a term ``g_i xh_i`` carries 1 + 2 + 1 (the product) roundings instead of 1: ``|b - B| <= (k + 3) u Gb``.
* ``g_i - a``: the errors of both and the subtraction's own, ``u (|g_i| + k Ga + |g_i - A|) <= u (2 |g_i| + (k + 1) Ga)``.
* ``xh_i b``: ``u |xh_i| ((k + 3) Gb + 2 |B| + |B|)`` (the error of ``b``, that of ``xh_i``, the product).
* the second subtraction and the multiply by ``rstd``: ``2 u |core_i|``; the residual add: ``u |o_i|``.

    |o_i - o64_i| <= u ( rstd ( 2 |g_i| + (k + 1) Ga + |xh_i| ((k + 3) Gb + 3 |B|) + 2 |core_i| ) + |o_i| ) + 2**-140

(``2**-140``: results below the normal range.)  A bf16 ``dy`` converts to fp32 exactly, so the fp32 ``dx`` of the bf16 kernels is held to
the same bound, and their ``dx_h`` must be ``dx`` rounded to nearest even, bit for bit.

True gradient.  With the statistics of the forward kernel (within ``rowwise_bounds.ln_bounds`` of the float64 ones: ``|dmu|`` and
``rho = |d rstd| / rstd``) the result is the gradient of ``layer_norm`` within the bound above plus, to first order,
``rstd ( |dmu| rstd (|B| + |xh_i| |A|) + 2 rho |xh_i B| + rho |core_i| )`` -- ``bwd_stats_slack``.

Exact scaling.  The operation is linear in ``(dy, d_res)`` and every rounding commutes with a power of two while nothing leaves the
normal range: ``f(2**s dy, 2**s d_res) == 2**s f(dy, d_res)`` bit for bit.  No tolerance; this is what shows the small-gradient regime.

bf16 QuickGELU backward.  With the float64 value ``v`` and the fp32 bound ``b = u (2 |z| + 8) |dy| fac + 2**-120`` of
``rowwise_bounds``, a bf16 result is right iff ``rne_bf16(v - b) <= got <= rne_bf16(v + b)`` (rounding is monotone), on ``|z| <= 80``;
outside of it the rules of ``rowwise_bounds`` hold (finite for a finite ``x``, ``dx == dy`` bit for bit at ``z > 80``)."""
import numpy as np

import rowwise_bounds as rb

U, F32 = rb.U, rb.F32
WIDTHS = tuple(sorted(rb.WIDTHS + (1276, 1280, 1284, 1536)))      # + the bf16 dispatch: the widest row kernel and the first generic multiple
BF16_WIDTHS = tuple(sorted(WIDTHS + (508,)))                       # both neighbours of every row-kernel width 512 / 768 / 1024 / 1280
ROW_KERNEL_WIDTHS = (512, 768, 1024, 1280)                         # layernorm_bwd_add_bf16_row_kernel<2..5>
DY_FAMILIES = ("randn", "small", "plus3", "large", "poscode")
DY_SCALE = {"randn": 1.0, "small": 2.0 ** -30, "plus3": 1.0, "large": 2.0 ** 20, "poscode": 1.0}
EPS = 1e-5
# (x_rows, K): rows = K x_rows of dy, row r reading row r % x_rows of x.  Alone, per-row, shared by a batch, grouped (x_rows neither 1
# nor rows), 1 ... 3 rows, counts that are no multiple of the 4 rows of a workgroup; the last: 255 rows, more than one workgroup.
LAYOUTS = ((1, 1), (3, 1), (1, 5), (3, 3), (7, 2), (5, 13), (51, 5))
LAYOUTS_WIDE = ((1, 1), (3, 1), (1, 5), (3, 3), (7, 2), (9, 7))    # at most 64 rows from E = 2048 on (63: 16 workgroups, the last short)


def layouts(E):
    return LAYOUTS if E < 2048 else LAYOUTS_WIDE


# ---------------------------------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------------------------------
def trunc_bf16(a):
    """fp32 -> the bf16 value towards zero (the wrong rounding), as fp32."""
    a = np.ascontiguousarray(a, F32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


def rne_bf16(a):
    """float64 or fp32 -> the nearest bf16 value, ties to even, as fp32; rounded ONCE from the type given.  NaN stays NaN."""
    v = np.asarray(a, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.ascontiguousarray(v.astype(F32))
    bits = f.view(np.uint32)
    lo_b = bits & np.uint32(0xFFFF0000)                             # the two bf16 neighbours, by magnitude
    hi_b = lo_b + np.uint32(0x10000)                                # (past the largest finite bf16: inf)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = lo_b.view(F32).astype(np.float64), hi_b.view(F32).astype(np.float64)
        hi = np.where(np.isinf(hi), np.copysign(2.0 ** 128, lo), hi)   # the overflow threshold lies half way to 2**128
        d_lo, d_hi = np.abs(v - lo), np.abs(hi - v)
        up = (d_hi < d_lo) | ((d_hi == d_lo) & ((lo_b >> np.uint32(16)) & np.uint32(1)).astype(bool))
    out = np.where(up, hi_b, lo_b).view(F32)
    return np.where(np.isfinite(f), out, f).astype(F32)


def bf16_bits(a):
    """fp32 values that are bf16 numbers -> their 16 bits."""
    return (np.ascontiguousarray(a, F32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward
# ---------------------------------------------------------------------------------------------------------------------
def dy_family(name, rows, E, rng):
    """``[rows, E]`` fp32 upstream gradients of one family.  ``poscode`` is a function of the position alone and exact in bf16
    (values in [1, 4) on a grid of 1 / 64), so a swapped pair, a shifted column or another row cannot cancel."""
    n = rng.standard_normal((rows, E))
    if name == "randn":
        d = n
    elif name == "small":
        d = n * 2.0 ** -30
    elif name == "plus3":
        d = n + 3.0                                                  # the mean(g) term dominates
    elif name == "large":
        d = n * 2.0 ** 20
    elif name == "poscode":
        d = 1.0 + (np.arange(E)[None, :] % 7) / 8.0 + (np.arange(rows)[:, None] % 64) / 64.0
    else:
        raise KeyError(name)
    return d.astype(F32)


def bwd_case(xfam, dyfam, x_rows, K, E, with_res, bf16=False, seed=0):
    """One case, a function of its arguments only: dict of ``dy [K x_rows, E]``, ``x [x_rows, E]``, ``mean rstd [x_rows]`` (the fp32
    statistics of ``rowwise_bounds.ln_restatement`` at eps = 1e-5), ``gamma beta [E]``, ``d_res`` (``randn`` at ``dy``'s scale, or
    None).  ``bf16``: ``dy`` rounded to bf16 (still fp32 numbers; ``bf16_bits`` gives the operand)."""
    rng = np.random.default_rng([rb.FAMILIES.index(xfam), DY_FAMILIES.index(dyfam), x_rows, K, E, int(with_res), seed])
    rows = x_rows * K
    x = rb.family(xfam, x_rows, E, rng)
    gamma, beta = rng.standard_normal(E).astype(F32), rng.standard_normal(E).astype(F32)
    dy = dy_family(dyfam, rows, E, rng)
    if bf16:
        dy = rne_bf16(dy)
    d_res = (rng.standard_normal((rows, E)) * DY_SCALE[dyfam]).astype(F32) if with_res else None
    st = rb.ln_restatement(x, None, gamma, beta, EPS)
    return {"dy": dy, "x": x, "mean": st["mean"], "rstd": st["rstd"], "gamma": gamma, "beta": beta, "d_res": d_res}


def operands(case):
    return tuple(case[k] for k in ("dy", "x", "mean", "rstd", "gamma", "d_res"))


def _f64(*arrays):
    return [None if a is None else np.asarray(a, np.float64) for a in arrays]


def _row_of_x(rows, x_rows):
    return np.arange(rows) % x_rows


def bwd_ref(dy, x, mean, rstd, gamma, d_res, m=None, gamma_in_core=True):
    """Float64 of the definition -> dict of ``g xh A B core o rstd Ga Gb`` (``rstd``: per row of ``dy``).  ``m``: which row of ``x`` a
    row of ``dy`` reads (default ``r % x_rows``)."""
    dy, x, mean, rstd, gamma, d_res = _f64(dy, x, mean, rstd, gamma, d_res)
    rows = dy.shape[0]
    m = _row_of_x(rows, x.shape[0]) if m is None else m
    with np.errstate(invalid="ignore", over="ignore"):
        g = dy * gamma
        rs = rstd[m][:, None]
        xh = (x[m] - mean[m][:, None]) * rs
        A, B = g.mean(-1, keepdims=True), (g * xh).mean(-1, keepdims=True)
        core = g - A - xh * B
        o = core * rs
        if d_res is not None:
            o = o + d_res
        Ga, Gb = np.abs(g).mean(-1, keepdims=True), np.abs(g * xh).mean(-1, keepdims=True)
    return {"g": g, "xh": xh, "A": A, "B": B, "core": core, "o": o, "rstd": rs, "Ga": Ga, "Gb": Gb}


def bwd_bound(ref, E):
    """The bound of the module docstring, per element."""
    k = rb.k1(E)
    a = np.abs
    with np.errstate(invalid="ignore", over="ignore"):
        inner = 2 * a(ref["g"]) + (k + 1) * ref["Ga"] + a(ref["xh"]) * ((k + 3) * ref["Gb"] + 3 * a(ref["B"])) + 2 * a(ref["core"])
        return U * (a(ref["rstd"]) * inner + a(ref["o"])) + 2.0 ** -140


def bwd_ratio(got, ref, E, extra=None):
    """Worst error / bound over every element (``rowwise_bounds._ratio``: a one-sided NaN / inf is infinitely wrong)."""
    b = bwd_bound(ref, E)
    return rb._ratio(got, ref["o"], b if extra is None else b + extra)


def bwd_stats_slack(ref, x, gamma, beta, m=None):
    """What the forward statistics' own bounds (``rowwise_bounds.ln_bounds`` of ``x``) can move the result by, first order, per element
    -- added to ``bwd_bound`` when the result is compared with the float64 gradient of ``layer_norm`` (``ref`` built on float64
    statistics)."""
    fwd = rb.ln_ref(x, None, gamma, beta, EPS)
    fb = rb.ln_bounds(fwd, x.shape[1])
    m = _row_of_x(ref["o"].shape[0], x.shape[0]) if m is None else m
    dmu, rho = fb["mean"][m][:, None], (fb["rstd"] / fwd["rstd"])[m][:, None]
    a = np.abs
    return a(ref["rstd"]) * (dmu * a(ref["rstd"]) * (a(ref["B"]) + a(ref["xh"]) * a(ref["A"])) + 2 * rho * a(ref["xh"] * ref["B"])
                             + rho * a(ref["core"]))


def lane_sum(v):
    """``[rows, E]`` fp32 -> ``[rows]`` fp32 in the kernels' order: lane ``l`` of 64 takes the 16-byte groups ``l, l + 64, ...`` (four
    elements left to right, then onto its running sum), then the xor butterfly 32, 16, ..., 1."""
    rows, E = v.shape
    n4, NV = E // 4, rb.nv(E)
    pad = np.zeros((rows, NV * 64, 4), F32)
    pad[:, :n4] = v.reshape(rows, n4, 4)
    g = pad.reshape(rows, NV, 64, 4)
    live = (np.arange(NV * 64) < n4).reshape(NV, 64)
    lane = np.zeros((rows, 64), F32)
    for j in range(NV):
        part = ((g[:, j, :, 0] + g[:, j, :, 1]) + g[:, j, :, 2]) + g[:, j, :, 3]
        lane = np.where(live[j], lane + part, lane).astype(F32)
    for off in (32, 16, 8, 4, 2, 1):
        lane = (lane + lane[:, np.arange(64) ^ off]).astype(F32)
    return lane[:, 0]


def bwd_restatement(dy, x, mean, rstd, gamma, d_res):
    """fp32 numpy restatement of ``layernorm_bwd_add_kernel`` (and of the bf16 kernels' fp32 result) in its own order, every operation
    rounded (the device build contracts multiply-adds; the bound holds either way)."""
    rows, E = dy.shape
    m = _row_of_x(rows, x.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        g = (dy * gamma).astype(F32)
        rs = rstd[m][:, None].astype(F32)
        xh = ((x[m] - mean[m][:, None]).astype(F32) * rs).astype(F32)
        a = (lane_sum(g) / F32(E)).astype(F32)[:, None]
        b = (lane_sum((g * xh).astype(F32)) / F32(E)).astype(F32)[:, None]
        o = (((g - a).astype(F32) - (xh * b).astype(F32)).astype(F32) * rs).astype(F32)
        if d_res is not None:
            o = (o + d_res).astype(F32)
    return o


def scaled(case, s):
    """The case with ``dy`` and ``d_res`` times ``2**s`` (exact)."""
    out = dict(case)
    out["dy"] = np.ldexp(case["dy"], s).astype(F32)
    out["d_res"] = None if case["d_res"] is None else np.ldexp(case["d_res"], s).astype(F32)
    return out


def scales_exactly(f, case, shifts=(-40, 40)):
    """``f(operands) -> fp32 [rows, E]``: is ``f(2**s dy, 2**s d_res)`` the bits of ``2**s f(dy, d_res)`` for every ``s``?"""
    base = np.ascontiguousarray(f(*operands(case)), F32)
    for s in shifts:
        got = np.ascontiguousarray(f(*operands(scaled(case, s))), F32)
        want = np.ldexp(base, s).astype(F32)
        if not np.array_equal(got.view(np.int32), want.view(np.int32)):
            return False
    return True


# wrong float64 references: (dy, x, mean, rstd, gamma, d_res) -> o
def _mut_drop_A(dy, x, mean, rstd, gamma, d_res):
    r = bwd_ref(dy, x, mean, rstd, gamma, None)
    return _finish((r["g"] - r["xh"] * r["B"]) * r["rstd"], d_res)


def _mut_drop_B(dy, x, mean, rstd, gamma, d_res):
    r = bwd_ref(dy, x, mean, rstd, gamma, None)
    return _finish((r["g"] - r["A"]) * r["rstd"], d_res)


def _mut_A_without_last(dy, x, mean, rstd, gamma, d_res):
    r = bwd_ref(dy, x, mean, rstd, gamma, None)
    A = r["g"][:, :-1].sum(-1, keepdims=True) / r["g"].shape[1]
    return _finish((r["g"] - A - r["xh"] * r["B"]) * r["rstd"], d_res)


def _mut_B_unbiased(dy, x, mean, rstd, gamma, d_res):
    r = bwd_ref(dy, x, mean, rstd, gamma, None)
    E = r["g"].shape[1]
    return _finish((r["g"] - r["A"] - r["xh"] * (r["B"] * E / max(E - 1, 1))) * r["rstd"], d_res)


def _mut_gamma_after(dy, x, mean, rstd, gamma, d_res):
    r = bwd_ref(dy, x, mean, rstd, np.ones_like(gamma), None)
    return _finish(r["core"] * np.asarray(gamma, np.float64) * r["rstd"], d_res)


def _mut_gamma_rolled(dy, x, mean, rstd, gamma, d_res):
    return bwd_ref(dy, x, mean, rstd, np.roll(gamma, 4), d_res)["o"]


def _mut_row_by_division(dy, x, mean, rstd, gamma, d_res):
    rows, x_rows = dy.shape[0], x.shape[0]
    return bwd_ref(dy, x, mean, rstd, gamma, d_res, m=np.arange(rows) // (rows // x_rows))["o"]


def _mut_neighbour_stats(dy, x, mean, rstd, gamma, d_res):
    return bwd_ref(dy, x, np.roll(mean, 1), np.roll(rstd, 1), gamma, d_res)["o"]


def _mut_res_ignored(dy, x, mean, rstd, gamma, d_res):
    return bwd_ref(dy, x, mean, rstd, gamma, None)["o"]


def _mut_res_before_rstd(dy, x, mean, rstd, gamma, d_res):
    r = bwd_ref(dy, x, mean, rstd, gamma, None)
    return (r["core"] + np.asarray(d_res, np.float64)) * r["rstd"]


def _finish(o, d_res):
    return o if d_res is None else o + np.asarray(d_res, np.float64)


# name -> (wrong float64 reference, where it can differ from the right one at all: (E, x_rows, K, with_res, xfam) -> bool)
#   const: every row of x is the same row and xh = 0 up to the rounding of the mean, so the B term, the row of x and the row of the
#          statistics do not matter;
#   gamma_rolled_by_4 at E == 4: one 16-byte group, the roll is the identity;
#   row_by_division: r // K == r % x_rows for every row when x_rows == 1 or K == 1;
#   B_over_E_minus_1: can differ wherever B does; where it must break the bound is narrower, see NOT_REQUIRED.
BWD_MUTANTS = {
    "A_dropped": (_mut_drop_A, lambda E, xr, K, res, xf: True),
    "B_dropped": (_mut_drop_B, lambda E, xr, K, res, xf: xf != "const"),
    "last_element_left_out_of_A": (_mut_A_without_last, lambda E, xr, K, res, xf: True),
    "B_over_E_minus_1": (_mut_B_unbiased, lambda E, xr, K, res, xf: xf != "const"),
    "gamma_after_centring": (_mut_gamma_after, lambda E, xr, K, res, xf: True),
    "gamma_rolled_by_4": (_mut_gamma_rolled, lambda E, xr, K, res, xf: E > 4),
    "row_by_division": (_mut_row_by_division, lambda E, xr, K, res, xf: xr > 1 and K > 1 and xf != "const"),
    "neighbour_row_statistics": (_mut_neighbour_stats, lambda E, xr, K, res, xf: xr > 1 and xf != "const"),
    "d_res_ignored": (_mut_res_ignored, lambda E, xr, K, res, xf: res),
    "d_res_before_rstd": (_mut_res_before_rstd, lambda E, xr, K, res, xf: res),
}

# Where a mutant that CAN differ need not break the bound, with the reason.  Everything else must, at every width, for every dy family
# and on every x family its predicate admits (on at least one of the cases of that width / dy family / x family).
#   B_over_E_minus_1 moves the B term by 1 / E of itself, next to a bound that allows (k + 3) u Gb on the same term.  On ``tiny`` the
#     variance is below eps: rstd is 1 / sqrt(eps), xh and with it B are 0.03 of what they are on ``std``, and the difference stays
#     inside the bound on every case from E = 512 on (on single cases from E = 252 on).  Below E = 8 the mutant is required nowhere
#     (B / 3 for B / 4 is far outside the bound there all the same, see the host test's lines).
NOT_REQUIRED = {
    "B_over_E_minus_1": ("tiny",),
}


def required(mutant, E, xfam):
    """Must ``mutant`` break the bound on x family ``xfam`` at width ``E`` (for every dy family, wherever its predicate holds)?"""
    if mutant == "B_over_E_minus_1" and E < 8:
        return False
    return xfam not in NOT_REQUIRED.get(mutant, ())


# ---------------------------------------------------------------------------------------------------------------------
# bf16 QuickGELU backward
# ---------------------------------------------------------------------------------------------------------------------
def gelu_bf16_case(x_n, batch, x_batch=1, seed=0):
    """``x`` fp32 ``[x_batch * x_n]`` (``rowwise_bounds.gelu_inputs``: specials, points outside the domain, the grid, ``3 randn`` at
    the end; ``x_n`` a multiple of the kernels' 8-element groups) and ``dy [batch * x_batch * x_n]``: ``randn`` rounded to bf16, never
    zero, in K-major order (element ``i`` reads ``x[i % x.size]``)."""
    assert x_n % 8 == 0
    few = len(rb.FAR) + len(rb.SPECIALS)                            # a row shorter than the specials: ``3 randn`` alone (seeds from there on)
    x = np.concatenate([rb.gelu_inputs(x_n, seed + 31 * b + (few if x_n <= few else 0))[0] for b in range(x_batch)])
    rng = np.random.default_rng([x_n, batch, x_batch, seed])
    dy = rne_bf16(rng.standard_normal(batch * x.size).astype(F32))
    dy[dy == 0] = 1.0
    return x, dy


def gelu_bf16_check(got, x_full, dy, c=rb.C):
    """``got``: the bf16 result as fp32 numbers, ``x_full``: the ``x`` every element read, ``dy``: bf16 numbers as fp32.  -> (number of
    elements inside ``|z| <= 80`` outside ``[rne(v - b), rne(v + b)]``, the violated rules outside of the domain and on NaNs)."""
    got = np.ascontiguousarray(got, F32)
    r = rb.gelu_ref(x_full, dy, c=c)
    with np.errstate(invalid="ignore", over="ignore"):
        b = U * (2 * np.abs(r["z"]) + 8) * r["fac"] + 2.0 ** -120
        lo, hi = rne_bf16(r["dx"] - b), rne_bf16(r["dx"] + b)
        inside = np.abs(r["z"]) <= 80.0
        fin = inside & np.isfinite(r["dx"])
        bad = int((fin & ~((lo <= got) & (got <= hi))).sum())
    _, why = rb._gelu_check(got, x_full, r["dx"], r["fac"], r["z"], np.asarray(dy, F32))
    if not np.array_equal(trunc_bf16(got).view(np.uint32), got.view(np.uint32)):
        why.append("not a bf16 number")
    return bad, why


def gelu_bf16_restatement(x_full, dy):
    """The kernels' formula in fp32 numpy, rounded once to bf16 (nearest even)."""
    return rne_bf16(rb.gelu_restatement(x_full, dy)[1])


def _gb_truncated(x, dy, x_n):
    return trunc_bf16(rb.gelu_restatement(x[rb.bcast_index(dy.size, x.size)], dy)[1])


def _gb_swapped(x, dy, x_n):
    o = gelu_bf16_restatement(x[rb.bcast_index(dy.size, x.size)], dy)
    return o.reshape(-1, 2)[:, ::-1].reshape(-1).copy()


def _gb_constant(x, dy, x_n):
    return rne_bf16(rb.gelu_ref(x[rb.bcast_index(dy.size, x.size)], dy, c=1.7)["dx"])


def _gb_row_by_division(x, dy, x_n):
    return gelu_bf16_restatement(x[rb.bcast_index(dy.size, x.size, wrong=True)], dy)


# name -> (wrong result: (x, dy, x_n) -> bf16 numbers as fp32, where it can differ: (x_batch, K) -> bool)
GELU_BF16_MUTANTS = {
    "truncated": (_gb_truncated, lambda xb, K: True),
    "halves_swapped": (_gb_swapped, lambda xb, K: True),
    "constant_1.7": (_gb_constant, lambda xb, K: True),
    "row_by_division": (_gb_row_by_division, lambda xb, K: xb > 1 and K > 1),
}
