"""Float64 references, worst-case rounding bounds, input families and mutants for the forward row-wise kernels of
``csrc/elementwise_kernels.hip``: the fused residual add + LayerNorm (``add_layernorm_fwd_kernel``) and QuickGELU forward / backward.
CPU only (numpy): ``tests/test_rowwise_bounds_host.py`` proves the bounds and the input set here, ``tests/test_gpu_rowwise_forward.py``
holds the kernels to them.

The bounds count the kernel's own operations; they are no tuned tolerances.  ``u = 2**-24`` is the unit roundoff of fp32.

LayerNorm of a row of ``E`` elements, ``NV = max(1, ceil(E / 256))`` 16-byte groups per lane: a lane adds 4 NV numbers on the way to the
row sum, the xor butterfly 6 more, and the division plus slack make ``k1 = 4 NV + 8``.  The reference is float64 of ``v = fp32(x + y)``
-- the fp32 sum, because the output ``s`` is defined as that rounding.  With ``m = mean |v|``:

* ``s`` has the bits of ``x + y`` in fp32;
* ``|mean - mu64| <= k1 u m``;
* ``|rstd - rs64| / rs64 <= (k1 + 6) u + (k1 u m rs64)**2`` (an error in the mean enters the two-pass variance only squared);
* ``|h_i - h64_i| <= u (|gamma_i| (k1 m rs64 + (k1 + 10) |xhat64_i|) + 2 |h64_i|)``.

QuickGELU with ``c = float(float32(1.702))``, ``z = c x``, ``sig = 1 / (1 + exp(-z))``, on the domain ``|z| <= 80``:

* ``|y - y64| <= u (2 |z| + 8) |y64| + 2**-120``;
* ``|dx - dx64| <= u (2 |z| + 8) |dy| (sig + |z| sig (1 - sig)) + 2**-120``

(``2 |z|``: the rounding of ``z`` feeding ``exp``; 8: a 1-ulp ``expf``, the add, the divide, the multiplies).  Outside the domain the fp32
formula itself underflows (``1 + exp(-z)`` overflows at ``z < -88.7``); there only: finite results for finite ``x``, ``|y| <= 2**-100`` for
``z < -80``, ``y == x`` and ``dx == dy`` bit for bit for ``z > 80``.  ``z`` must be finite in fp32 (``|x| < 1.9e38``)."""
import math

import numpy as np

U = 2.0 ** -24
WIDTHS = (4, 20, 252, 256, 260, 512, 516, 768, 1024, 1028, 2048, 2052, 4096)     # both sides of every NV switch, and the edges
FAMILIES = ("std", "off1e3", "off1e3s", "tiny", "big", "const", "spike")
EPSES = (1e-5, 1e-6, 1e-12)
C = float(np.float32(1.702))
F32 = np.float32


def nv(E):
    return max(1, -(-E // 256))


def k1(E):
    return 4 * nv(E) + 8


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm forward
# ---------------------------------------------------------------------------------------------------------------------
def family(name, rows, E, rng):
    """``[rows, E]`` fp32 rows of one input family."""
    n = rng.standard_normal((rows, E))
    if name == "std":
        x = n
    elif name == "off1e3":
        x = n + 1000.0
    elif name == "off1e3s":
        x = 1e-2 * n + 1000.0
    elif name == "tiny":
        x = 1e-4 * n
    elif name == "big":
        x = 1e4 * n + 3e4
    elif name == "const":
        x = np.full((rows, E), 0.1)
    elif name == "spike":
        x = n
        x[:, -1] = 1e4
    else:
        raise KeyError(name)
    return x.astype(F32)


def ln_case(name, rows, E, with_y, seed=0):
    """``x, y (or None), gamma, beta`` of one case, fp32, a function of its arguments only."""
    rng = np.random.default_rng([FAMILIES.index(name), rows, E, int(with_y), seed])
    x = family(name, rows, E, rng)
    y = rng.standard_normal((rows, E)).astype(F32) if with_y else None
    gamma, beta = rng.standard_normal(E).astype(F32), rng.standard_normal(E).astype(F32)
    return x, y, gamma, beta


def ln_cases(rows, E, seed=0):
    """Every (family, y given or not, eps) of the issue's input set at one shape."""
    for name in FAMILIES:
        for with_y in (False, True):
            ops = ln_case(name, rows, E, with_y, seed)
            for eps in EPSES:
                yield (name, with_y, eps), ops, eps


def fp32_sum(x, y):
    return x if y is None else (x + y).astype(F32)


def ln_ref(x, y, gamma, beta, eps):
    """Float64 reference of ``v = fp32(x + y)`` -> dict of ``s`` (fp32) and float64 ``mean rstd xhat h m``."""
    v = fp32_sum(x, y)
    with np.errstate(invalid="ignore", over="ignore"):
        v64 = v.astype(np.float64)
        mu = v64.mean(-1)
        var = ((v64 - mu[:, None]) ** 2).mean(-1)
        rs = 1.0 / np.sqrt(var + eps)
        xhat = (v64 - mu[:, None]) * rs[:, None]
        h = xhat * gamma.astype(np.float64) + beta.astype(np.float64)
        m = np.abs(v64).mean(-1)
    return {"s": v, "mean": mu, "rstd": rs, "xhat": xhat, "h": h, "m": m, "gamma": gamma.astype(np.float64)}


def ln_bounds(ref, E):
    """The three error bounds of the module docstring, per element: ``mean [rows]``, ``rstd [rows]`` (absolute), ``h [rows, E]``."""
    k = k1(E)
    m, rs = ref["m"], ref["rstd"]
    b_mean = k * U * m
    b_rstd = ((k + 6) * U + (k * U * m * rs) ** 2) * rs
    b_h = U * (np.abs(ref["gamma"]) * ((k * m * rs)[:, None] + (k + 10) * np.abs(ref["xhat"])) + 2 * np.abs(ref["h"]))
    return {"mean": b_mean, "rstd": b_rstd, "h": b_h}


def _ratio(got, want, bound):
    """Largest error / bound over every element; an element that is NaN / inf on one side only counts as infinitely wrong."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return math.inf
    if got.size == 0:
        return 0.0
    bad = ~(np.isfinite(got) & np.isfinite(want))
    if bad.any():
        same = np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[bad & ~np.isnan(got)], want[bad & ~np.isnan(want)])
        if not same:
            return math.inf
    ok = ~bad
    if not ok.any():
        return 0.0
    err, b = np.abs(got[ok] - want[ok]), np.broadcast_to(bound, got.shape)[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    return float(r.max())


def ln_ratios(got, ref, E):
    """``got``: dict with any of ``mean rstd h`` (any float type) and ``s`` -> worst error / bound per output.  ``s`` is a bit
    comparison: 0.0 when every bit matches (a NaN matches a NaN of any payload), inf otherwise."""
    b = ln_bounds(ref, E)
    out = {k: _ratio(got[k], ref[k], b[k]) for k in ("mean", "rstd", "h") if got.get(k) is not None}
    if got.get("s") is not None:
        gs = np.ascontiguousarray(got["s"], dtype=F32)
        same = gs.shape == ref["s"].shape and ((gs.view(np.int32) == ref["s"].view(np.int32)) | (np.isnan(gs) & np.isnan(ref["s"]))).all()
        out["s"] = 0.0 if same else math.inf
    return out


def ln_restatement(x, y, gamma, beta, eps):
    """fp32 numpy restatement of ``add_layernorm_fwd_kernel`` in its summation order: lane ``l`` of 64 adds the 16-byte groups
    ``l, l + 64, ...`` (four elements left to right, then onto its running sum), the xor butterfly 32, 16, ..., 1 joins the lanes, and
    the variance is a second pass over ``v - mean``.  No FMA contraction and a correctly rounded ``1 / sqrt`` (the device build
    contracts and uses ``rsqrtf``; the bounds' headroom is for that)."""
    v = fp32_sum(x, y)
    rows, E = v.shape
    n4, NV = E // 4, nv(E)
    pad = np.zeros((rows, NV * 64, 4), F32)
    pad[:, :n4] = v.reshape(rows, n4, 4)
    live = (np.arange(NV * 64) < n4).reshape(NV, 64)

    def row_sum(g):                                  # g: [rows, NV * 64, 4] fp32 -> [rows] fp32
        g = g.reshape(rows, NV, 64, 4)
        lane = np.zeros((rows, 64), F32)
        for j in range(NV):
            part = ((g[:, j, :, 0] + g[:, j, :, 1]) + g[:, j, :, 2]) + g[:, j, :, 3]
            lane = np.where(live[j], lane + part, lane).astype(F32)
        for off in (32, 16, 8, 4, 2, 1):
            lane = (lane + lane[:, np.arange(64) ^ off]).astype(F32)
        return lane[:, 0]

    mu = (row_sum(pad) / F32(E)).astype(F32)
    d = (pad - mu[:, None, None]).astype(F32)
    q = row_sum((d * d).astype(F32))
    rs = (F32(1) / np.sqrt((q / F32(E) + F32(eps)).astype(F32))).astype(F32)
    h = (((v - mu[:, None]) * rs[:, None]).astype(F32) * gamma + beta).astype(F32)
    return {"s": v, "mean": mu, "rstd": rs, "h": h}


def _ln_from_stats(v64, mu, rs, gamma, beta):
    return (v64 - mu[:, None]) * rs[:, None] * gamma.astype(np.float64) + beta.astype(np.float64)


def _stats64(v64, eps):
    mu = v64.mean(-1)
    return mu, 1.0 / np.sqrt(((v64 - mu[:, None]) ** 2).mean(-1) + eps)


def _mut_drop_last(x, y, gamma, beta, eps):
    v64 = fp32_sum(x, y).astype(np.float64)
    mu = v64[:, :-1].sum(-1) / v64.shape[1]          # an element dropped at the end of the row
    rs = 1.0 / np.sqrt(((v64 - mu[:, None]) ** 2).mean(-1) + eps)
    return {"mean": mu, "rstd": rs, "h": _ln_from_stats(v64, mu, rs, gamma, beta)}


def _mut_unbiased(x, y, gamma, beta, eps):
    v64 = fp32_sum(x, y).astype(np.float64)
    mu = v64.mean(-1)
    rs = 1.0 / np.sqrt(((v64 - mu[:, None]) ** 2).sum(-1) / max(v64.shape[1] - 1, 1) + eps)
    return {"mean": mu, "rstd": rs, "h": _ln_from_stats(v64, mu, rs, gamma, beta)}


def _mut_one_pass(x, y, gamma, beta, eps):
    v = fp32_sum(x, y)
    E = F32(v.shape[1])
    mu = (v.sum(-1, dtype=F32) / E).astype(F32)
    var = ((v * v).astype(F32).sum(-1, dtype=F32) / E - mu * mu).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = 1.0 / np.sqrt(var.astype(np.float64) + eps)
    mu = mu.astype(np.float64)
    return {"mean": mu, "rstd": rs, "h": _ln_from_stats(v.astype(np.float64), mu, rs, gamma, beta)}


def _mut_eps_outside(x, y, gamma, beta, eps):
    v64 = fp32_sum(x, y).astype(np.float64)
    mu = v64.mean(-1)
    rs = 1.0 / (np.sqrt(((v64 - mu[:, None]) ** 2).mean(-1)) + eps)
    return {"mean": mu, "rstd": rs, "h": _ln_from_stats(v64, mu, rs, gamma, beta)}


def _mut_roll_affine(x, y, gamma, beta, eps):
    v64 = fp32_sum(x, y).astype(np.float64)
    mu, rs = _stats64(v64, eps)
    return {"mean": mu, "rstd": rs, "h": _ln_from_stats(v64, mu, rs, np.roll(gamma, 4), np.roll(beta, 4))}


def _mut_ignore_y(x, y, gamma, beta, eps):
    v64 = x.astype(np.float64)
    mu, rs = _stats64(v64, eps)
    return {"s": x, "mean": mu, "rstd": rs, "h": _ln_from_stats(v64, mu, rs, gamma, beta)}


def _mut_neighbour_stats(x, y, gamma, beta, eps):
    v64 = fp32_sum(x, y).astype(np.float64)
    mu, rs = _stats64(v64, eps)
    mu, rs = np.roll(mu, 1), np.roll(rs, 1)
    return {"mean": mu, "rstd": rs, "h": _ln_from_stats(v64, mu, rs, gamma, beta)}


# name -> (wrong float64 LayerNorm, the cases it can differ on at all: (E, rows, with_y) -> bool)
#   roll4 at E == 4: a row of one 16-byte group has no neighbouring group, the roll by four is the identity there;
#   ignore_y without y and neighbour_stats on a single row are the correct operation as well.
LN_MUTANTS = {
    "drop_last": (_mut_drop_last, lambda E, rows, with_y: True),
    "unbiased_variance": (_mut_unbiased, lambda E, rows, with_y: True),
    "one_pass_fp32_variance": (_mut_one_pass, lambda E, rows, with_y: True),
    "eps_outside_sqrt": (_mut_eps_outside, lambda E, rows, with_y: True),
    "affine_rolled_by_4": (_mut_roll_affine, lambda E, rows, with_y: E > 4),
    "y_ignored": (_mut_ignore_y, lambda E, rows, with_y: with_y),
    "neighbour_row_statistics": (_mut_neighbour_stats, lambda E, rows, with_y: rows > 1),
}


# ---------------------------------------------------------------------------------------------------------------------
# QuickGELU
# ---------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf, np.nan], F32)
FAR = np.array([48.0, -48.0, 60.0, -60.0, 100.0, -100.0, 1e4, -1e4], F32)      # finite, outside |z| <= 80


def gelu_inputs(n, seed=0):
    """``x, dy`` of ``n`` elements: the specials +-0, +-1e-40, +-inf, NaN and a few finite points outside the domain, a grid over
    [-47, 47] (at least 4096 points once ``n`` has the room), then ``3 randn`` -- ordinary values at the END, where the kernels'
    scalar tail is.  ``n`` up to the number of specials (all of it tail, or nearly): the window of them that ``seed`` picks, and
    ``3 randn`` alone from ``seed = len(FAR) + len(SPECIALS)`` on."""
    rng = np.random.default_rng([n, seed])
    head = np.concatenate([FAR, SPECIALS])
    if n <= len(head):
        x = np.roll(head, -seed)[:n] if seed < len(head) else 3.0 * rng.standard_normal(n)
    else:
        body = n - len(head)
        grid = body // 2                                      # >= 4096 points from n = 8207 on: the large shapes carry the full grid
        x = np.concatenate([head, np.linspace(-47.0, 47.0, grid), 3.0 * rng.standard_normal(body - grid)])
    dy = rng.standard_normal(n).astype(F32)
    dy[dy == 0] = 1.0
    return x.astype(F32), dy


def gelu_ref(x, dy=None, c=C):
    """Float64 ``z sig y`` (and ``dx fac`` with ``fac = sig + |z| sig (1 - sig)`` when ``dy`` is given) of fp32 ``x``."""
    x64 = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        z = c * x64
        sig = 1.0 / (1.0 + np.exp(-z))
        out = {"z": z, "sig": sig, "y": x64 * sig}
        if dy is not None:
            dy64 = np.asarray(dy, np.float64)
            out["dx"] = dy64 * (sig + z * sig * (1.0 - sig))
            out["fac"] = np.abs(dy64) * (sig + np.abs(z) * sig * (1.0 - sig))
    return out


def _gelu_check(got, x, want, scale, z, passthrough):
    """Worst error / bound inside ``|z| <= 80`` and the list of violated rules outside of it."""
    got = np.asarray(got)
    got64 = got.astype(np.float64)
    inside = np.abs(z) <= 80.0
    why = []
    if not np.array_equal(np.isnan(got64), np.isnan(want)):
        why.append("NaN positions differ from the reference's")
    with np.errstate(invalid="ignore"):
        bound = U * (2 * np.abs(z) + 8) * scale + 2.0 ** -120
        ratio = _ratio(got64[inside], want[inside], bound[inside])
    finite_x = np.isfinite(np.asarray(x, np.float64))
    if not np.isfinite(got64[finite_x]).all():
        why.append("a finite x gave a non-finite result")
    lo, hi = finite_x & (z < -80.0), finite_x & (z > 80.0)
    if passthrough is None and (np.abs(got64[lo]) > 2.0 ** -100).any():
        why.append("|y| > 2**-100 at z < -80")
    pt = np.asarray(x if passthrough is None else passthrough, F32)
    if got.shape == pt.shape and not np.array_equal(got.astype(F32)[hi].view(np.int32), pt[hi].view(np.int32)):
        why.append("not the identity at z > 80")
    return ratio, why


def gelu_fwd_check(y, x):
    r = gelu_ref(x, None)
    return _gelu_check(y, x, r["y"], np.abs(r["y"]), r["z"], None)


def gelu_bwd_check(dx, x, dy):
    r = gelu_ref(x, dy)
    return _gelu_check(dx, x, r["dx"], r["fac"], r["z"], dy)


def gelu_restatement(x, dy):
    """The kernels' formulas in fp32 numpy: ``y = x * (1 / (1 + exp(-(c x))))``, ``dx = dy * (s + c x s (1 - s))``."""
    x, dy, one, c = np.asarray(x, F32), np.asarray(dy, F32), F32(1), F32(1.702)
    with np.errstate(over="ignore", invalid="ignore"):
        z = c * x
        s = one / (one + np.exp(-z))
        return x * s, dy * (s + z * s * (one - s))


def bcast_index(n, x_n, wrong=False):
    """Which element of ``x`` (``x_n`` of them) element ``i`` of ``dy`` (``n``) reads in the broadcast backward: ``i % x_n`` -- target
    ``t`` of a K-major batch reads sample ``t % M``.  ``wrong``: the mutant ``i // (n / x_n)``."""
    i = np.arange(n)
    return i // (n // x_n) if wrong else i % x_n


def _gmut_constant(x, dy):
    r = gelu_ref(x, dy, c=1.7)
    return r["y"], r["dx"]


def _gmut_scale(x, dy):
    r = gelu_ref(x, dy)
    return r["y"] * (1 + 3e-6), r["dx"] * (1 + 3e-6)


def _gmut_tail(x, dy):
    r = gelu_ref(x, dy)
    y, dx = r["y"].copy(), r["dx"].copy()
    y[-1], dx[-1] = 0.0, 0.0                         # the last element keeps what the buffer held (zeros here)
    return y, dx


GELU_MUTANTS = {"constant_1.7": _gmut_constant, "scaled_by_1+3e-6": _gmut_scale, "tail_unwritten": _gmut_tail}
