"""-m gpu: the backward row-wise kernels of ``csrc/elementwise_kernels.hip`` -- the LayerNorm input gradient fused with the residual
add (``ops.layernorm_bwd_add``, ``ops.layernorm_bwd_add_rows``, ``ops.layernorm_bwd_add_bf16``), the bf16 QuickGELU backward
(``ops.quick_gelu_bwd`` with a bf16 ``dy``) and the one-row scatter / add (``ops.rows_to_dense``, ``ops.rows_add_``) -- against the
float64 references and counted rounding bounds of ``tests/rowwise_backward_bounds.py`` (proved on the CPU by
``tests/test_rowwise_backward_bounds_host.py``, where every mutant of these kernels is shown to break them).

Every element of every output is checked.  The worst error / bound of every kernel and width is recorded (``parity.note``) and printed.
What the wrappers refuse -- a ``d_res`` or an ``x`` of another shape, rows of ``x`` that do not tile ``dy``'s, misaligned views -- is
tested as a refusal: no kernel is launched."""
import ctypes

import numpy as np
import pytest
import torch

import rowwise_backward_bounds as bb
import rowwise_bounds as rb
from test_gpu_rowwise_forward import dev, host, report, same_bits, worst

pytestmark = pytest.mark.gpu

SCALED = ("randn", "poscode")                 # dy families of the exact-scaling identity, on the ``std`` x family
SHIFTS = (-40, 40)


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    return _ops


def bf(a):
    """bf16 numbers held as fp32 -> a bf16 device tensor (exact)."""
    return dev(a).to(torch.bfloat16)


def family_pairs(rows):
    """Every (x family, dy family, d_res given) for a layout of up to 21 rows; for a larger one every pair still, ``d_res`` alternating."""
    i = 0
    for xf in rb.FAMILIES:
        for df in bb.DY_FAMILIES:
            for res in ((False, True) if rows <= 21 else (bool(i % 2),)):
                yield xf, df, res
            i += 1


def shaped(case, x_rows, K, E):
    """Device operands in the shapes of the model code: ``dy`` / ``d_res`` ``[K, x_rows, E]``, ``x`` ``[1 or x_rows, ., E]``."""
    dy, x, mean, rstd, gamma, d_res = (dev(a) for a in bb.operands(case))
    return dy.view(K, x_rows, E), x.view(1, x_rows, E), mean, rstd, gamma, (None if d_res is None else d_res.view(K, x_rows, E))


def scaled_by(t, s):
    return None if t is None else torch.ldexp(t.float(), torch.tensor(s, device=t.device)).to(t.dtype)


@pytest.mark.parametrize("E", bb.WIDTHS)
def test_layernorm_bwd_add_meets_the_float64_bound(ops, E):
    """Every row layout of this width x every family pair, ``d_res`` given and ``None``: every element within the counted bound, the
    same bits on a second call, and -- ``std`` rows, ``randn`` and position-coded ``dy`` -- the bits of ``2**s`` times the result for
    ``2**s`` times ``(dy, d_res)``, s = -40 and +40."""
    top = {}
    for x_rows, K in bb.layouts(E):
        for xf, df, res in family_pairs(x_rows * K):
            case = bb.bwd_case(xf, df, x_rows, K, E, res)
            ref = bb.bwd_ref(*bb.operands(case))
            dy, x, mean, rstd, gamma, d_res = shaped(case, x_rows, K, E)
            got = ops.layernorm_bwd_add(dy, x, mean, rstd, gamma, d_res)
            assert got.shape == dy.shape and got.dtype == torch.float32
            r = bb.bwd_ratio(host(got).reshape(-1, E), ref, E)
            worst({"dx": r}, top)
            assert r <= 1.0, (E, x_rows, K, xf, df, res, r)
            assert same_bits(got, ops.layernorm_bwd_add(dy, x, mean, rstd, gamma, d_res)), (E, x_rows, K, xf, df, res)
            if xf == "std" and df in SCALED:
                for s in SHIFTS:
                    moved = ops.layernorm_bwd_add(scaled_by(dy, s), x, mean, rstd, gamma, scaled_by(d_res, s))
                    assert same_bits(moved, scaled_by(got, s)), ("scaling by 2**%d" % s, E, x_rows, K, df, res)
    report("layernorm_bwd_add E=%d" % E, top)


@pytest.mark.parametrize("E", [20, 260, 1028, 4096])
def test_layernorm_bwd_add_with_the_forward_kernels_statistics_is_the_gradient(ops, E):
    """``add_layernorm``'s ``mean`` / ``rstd`` fed to the backward: the float64 gradient of ``layer_norm`` within the backward bound
    plus what the forward's own bounds on the statistics carry through (``bwd_stats_slack``)."""
    top = {}
    for xf in rb.FAMILIES:
        for df in bb.DY_FAMILIES:
            case = bb.bwd_case(xf, df, 3, 3, E, True)
            dy, x, _, _, gamma, d_res = shaped(case, 3, 3, E)
            _, _, mean, rstd = ops.add_layernorm(x, None, gamma, dev(case["beta"]), bb.EPS)
            got = ops.layernorm_bwd_add(dy, x, mean, rstd, gamma, d_res)
            f64 = rb.ln_ref(case["x"], None, case["gamma"], case["beta"], bb.EPS)
            ref = bb.bwd_ref(case["dy"], case["x"], f64["mean"], f64["rstd"], case["gamma"], case["d_res"])
            r = bb.bwd_ratio(host(got).reshape(-1, E), ref, E, extra=bb.bwd_stats_slack(ref, case["x"], case["gamma"], case["beta"]))
            worst({"dx": r}, top)
            assert r <= 1.0, (E, xf, df, r)
    report("add_layernorm -> layernorm_bwd_add E=%d (bound + carried)" % E, top)


ROW_PAIRS = (("std", "randn"), ("std", "small"), ("off1e3", "poscode"), ("spike", "plus3"), ("big", "large"), ("const", "randn"))


@pytest.mark.parametrize("E", [4, 260, 516, 1028, 1536, 2052, 4096])
def test_layernorm_bwd_add_rows_meets_the_bound_on_the_listed_rows(ops, E):
    """The listed rows against float64 directly (that they have the dense kernel's bits is ``tests/test_gpu_rows_kernels_edges.py``'s
    subject), on that file's lists -- none, one, all, shuffled, ids outside the tensor, counts outside the capacity -- up to E = 1536 and
    on a shuffled list over 23 of 37 rows above; every other row keeps the bits it had."""
    from test_gpu_gemm_rows_pipeline import hand_list, mask
    from test_gpu_rows_kernels_edges import CAP, SENTINEL, hand_lists
    if E < 2048:
        lists = {name: (live, listed, CAP) for name, (live, listed, _) in hand_lists().items()}
    else:
        entries = torch.randperm(37, generator=torch.Generator().manual_seed(E)).tolist()[:23]
        lists = {"shuffled": (hand_list(entries, 37), mask(entries, 37), 37)}
    top = {}
    for name, (live, listed, cap) in lists.items():
        rows_listed = listed.cpu().numpy()
        for i, (xf, df) in enumerate(ROW_PAIRS):
            case = bb.bwd_case(xf, df, cap, 1, E, bool(i % 2))
            ref = bb.bwd_ref(*bb.operands(case))
            dy, x, mean, rstd, gamma, d_res = shaped(case, cap, 1, E)
            out = torch.full((1, cap, E), SENTINEL, device="cuda")
            got = ops.layernorm_bwd_add_rows(dy, x, mean, rstd, gamma, d_res, live, out=out)
            assert got is out
            got = host(got).reshape(cap, E)
            assert (got[~rows_listed] == SENTINEL).all(), ("an unlisted row was written", E, name, xf, df)
            if rows_listed.any():
                part = {k: (v[rows_listed] if v.shape[0] == cap else v) for k, v in ref.items()}
                r = bb.bwd_ratio(got[rows_listed], part, E)
                worst({"dx": r}, top)
                assert r <= 1.0, (E, name, xf, df, r)
    report("layernorm_bwd_add_rows E=%d" % E, top)


def bf16_cases(E):
    for x_rows, K in bb.layouts(E):
        small = x_rows * K <= 21
        for i, xf in enumerate(rb.FAMILIES):
            for j, df in enumerate(bb.DY_FAMILIES):
                if small or xf == "std" or i % len(bb.DY_FAMILIES) == j:     # a large layout: every dy family on std and on one more
                    yield x_rows, K, xf, df, bool((i + j) % 2)


@pytest.mark.parametrize("E", bb.BF16_WIDTHS)
def test_layernorm_bwd_add_bf16_meets_the_bound_and_rounds_once(ops, E):
    """bf16 ``dy`` (the row-resident kernel at 512 / 768 / 1024 / 1280, the generic one everywhere else -- 256, 1536, 2048 and 4096
    included): the fp32 ``dx`` within the fp32 kernel's bound, ``dx_h`` the bits of ``dx`` rounded to nearest even, the bf16-only call
    the same ``dx_h``, the scaling identity, and a ``dy`` that is 8 but not 16 bytes aligned takes the same route to the same bits."""
    top = {}
    for x_rows, K, xf, df, res in bf16_cases(E):
        case = bb.bwd_case(xf, df, x_rows, K, E, res, bf16=True)
        ref = bb.bwd_ref(*bb.operands(case))
        _, x, mean, rstd, gamma, d_res = shaped(case, x_rows, K, E)
        dy = bf(case["dy"]).view(K, x_rows, E)
        assert np.array_equal(host(dy).reshape(-1, E), case["dy"])
        dx, dx_h = ops.layernorm_bwd_add_bf16(dy, x, mean, rstd, gamma, d_res)
        assert dx.dtype == torch.float32 and dx_h.dtype == torch.bfloat16 and dx.shape == dx_h.shape == dy.shape
        r = bb.bwd_ratio(host(dx).reshape(-1, E), ref, E)
        worst({"dx": r}, top)
        assert r <= 1.0, (E, x_rows, K, xf, df, res, r)
        assert same_bits(dx_h, dx.to(torch.bfloat16)), (E, x_rows, K, xf, df, res)
        none, only_h = ops.layernorm_bwd_add_bf16(dy, x, mean, rstd, gamma, d_res, want_f32=False)
        assert none is None and same_bits(only_h, dx_h), (E, x_rows, K, xf, df, res)
        if xf == "std" and df in SCALED:
            for s in SHIFTS:
                moved, moved_h = ops.layernorm_bwd_add_bf16(scaled_by(dy, s), x, mean, rstd, gamma, scaled_by(d_res, s))
                assert same_bits(moved, scaled_by(dx, s)) and same_bits(moved_h, scaled_by(dx_h, s)), ("2**%d" % s, E, x_rows, K, df)
            shifted = torch.empty(dy.numel() + 4, dtype=torch.bfloat16, device="cuda")[4:].view(dy.shape).copy_(dy)
            if shifted.data_ptr() % 16 == 8:
                again, again_h = ops.layernorm_bwd_add_bf16(shifted, x, mean, rstd, gamma, d_res)
                assert same_bits(again, dx) and same_bits(again_h, dx_h), (E, x_rows, K, df)
    report("layernorm_bwd_add_bf16 E=%d" % E, top)


@pytest.mark.parametrize("E", [20, 516, 1024])
def test_layernorm_backward_rows_do_not_touch_each_other(ops, E):
    """Nine rows over three shared rows of ``x``.  A NaN, +inf, -inf in one row of ``dy`` or of ``d_res`` changes that row and no bit
    of another; one in a shared row of ``x`` changes the three rows that read it (``r % 3``) and no bit of another.  fp32 kernel, bf16
    kernel (generic at 20 and 516, row-resident at 1024), and the row-list kernel (there ``x`` is per row)."""
    from test_gpu_gemm_rows_pipeline import hand_list
    x_rows, K, rows = 3, 3, 9
    case = bb.bwd_case("std", "randn", x_rows, K, E, True, bf16=True)
    per_row = bb.bwd_case("std", "randn", rows, 1, E, True)
    live = hand_list([7, 0, 4, 2, 8, 5], rows)
    listed = [0, 2, 4, 5, 7, 8]

    def run(c, p):
        dy, x, mean, rstd, gamma, d_res = (dev(a) for a in bb.operands(c))
        dxb, dxh = ops.layernorm_bwd_add_bf16(dy.to(torch.bfloat16), x, mean, rstd, gamma, d_res)
        dy, x, mean, rstd, gamma, d_res = (dev(a) for a in bb.operands(p))
        out = torch.full((1, rows, E), 7.25, device="cuda")
        ops.layernorm_bwd_add_rows(dy.view(1, rows, E), x.view(1, rows, E), mean, rstd, gamma, d_res.view(1, rows, E), live, out=out)
        dy0, x0, mean0, rstd0, gamma0, d_res0 = (dev(a) for a in bb.operands(c))
        return {"fp32": ops.layernorm_bwd_add(dy0, x0, mean0, rstd0, gamma0, d_res0), "bf16 dx": dxb, "bf16 dx_h": dxh,
                "rows": out.view(rows, E)}

    clean = run(case, per_row)
    for value in (float("nan"), float("inf"), float("-inf")):
        for what, row, col in (("dy", 4, 0), ("d_res", 7, E - 1), ("x", 2, E // 2)):
            c, p = {k: (None if v is None else v.copy()) for k, v in case.items()}, {k: v.copy() for k, v in per_row.items()}
            c[what][row, col] = value
            p[what][row, col] = value
            got = run(c, p)
            for name, t in got.items():
                hit = [row] if what != "x" or name == "rows" else [r for r in range(rows) if r % x_rows == row]
                if name == "rows":
                    hit = [r for r in hit if r in listed]
                    assert bool((t[[r for r in range(rows) if r not in listed]] == 7.25).all()), (E, value, what, name)
                rest = [r for r in range(rows) if r not in hit]
                assert same_bits(t[rest], clean[name][rest]), ("another row changed", E, value, what, name)
                for r in hit:
                    assert not same_bits(t[r], clean[name][r]) and not bool(torch.isfinite(t[r].float()).all()), (E, value, what, name, r)


# ---------------------------------------------------------------------------------------------------------------------
# bf16 QuickGELU backward
# ---------------------------------------------------------------------------------------------------------------------
SHARED_BATCHES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)       # both sides of the sweep kernel's threshold (4), of its unrolled four and
GROUPED = tuple((M, K) for M in (2, 3) for K in (1, 3, 4, 5, 9))   # of its blocks of 8 samples; x of batch M: K = n / x_n picks the kernel


@pytest.mark.parametrize("row", [8, 24, 2040, 2048, 2056])
def test_quick_gelu_bwd_bf16_is_within_one_rounding_of_float64(ops, row):
    """Every element inside ``[rne(v - b), rne(v + b)]`` of its float64 value ``v`` and fp32 bound ``b`` (nearest-even or nothing: a
    truncated result, swapped halves of a pair, another constant or the sample ``i // K`` are outside, see the host file); the rules
    outside ``|z| <= 80``; and the bits of the call with ``x`` expanded to ``dy``'s shape."""
    checked = 0
    for M, K in tuple((1, B) for B in SHARED_BATCHES) + GROUPED:
        x, dy = bb.gelu_bf16_case(row, K, M)
        full = x[rb.bcast_index(dy.size, x.size)]
        xd, dyd = dev(x).view(M, 1, row), bf(dy).view(K * M, 1, row)
        got = ops.quick_gelu_bwd(xd, dyd)
        assert got.dtype == torch.bfloat16 and got.shape == dyd.shape
        bad, why = bb.gelu_bf16_check(host(got).reshape(-1), full, dy)
        assert bad == 0 and not why, (row, M, K, bad, why)
        assert same_bits(got, ops.quick_gelu_bwd(dev(full).view(K * M, 1, row), dyd)), ("the un-shared form differs", row, M, K)
        checked += dy.size
    report("quick_gelu_bwd bf16 row=%d (%d elements)" % (row, checked), {"outside their interval": 0.0})


# ---------------------------------------------------------------------------------------------------------------------
# one row per sample <-> dense
# ---------------------------------------------------------------------------------------------------------------------
GUARD, FILL = 64, -3.5                          # 256 bytes of sentinel on either side: the operand stays 16-byte aligned


def guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), FILL, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def guards_intact(buf):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all())


@pytest.mark.parametrize("B,N,E", [(4, 1, 4), (5, 7, 260), (6, 5, 1028), (4, 3, 2052)])
@pytest.mark.parametrize("ids", [torch.int64, torch.int32])
def test_rows_to_dense_and_rows_add_at_the_edges(ops, B, N, E, ids):
    """Rows 0 and N - 1, and ids -1 and N: ``rows_to_dense`` gives an all-zero sample for an id outside ``[0, N)``, ``rows_add_`` leaves
    that sample as it is.  int32 ids go through the wrappers' conversion.  The outputs live inside sentinel-filled buffers whose guard
    elements keep their bits (``rows_to_dense`` through the C entry point, which takes the output pointer)."""
    from transformer_mm_explainability_amd import _lib
    g = torch.Generator().manual_seed(B * 1000 + E)
    rows = torch.tensor(([0, N - 1, -1, N, N // 2, 0])[:B], dtype=ids).cuda()
    vals = torch.randn(B, E, generator=g).cuda()
    inside = [(b, int(r)) for b, r in enumerate(rows.tolist()) if 0 <= r < N]
    want = torch.zeros(B, N, E, device="cuda")
    for b, r in inside:
        want[b, r] = vals[b]
    assert same_bits(ops.rows_to_dense(vals, rows, N), want)
    buf, out = guarded((B, N, E))
    rows64 = rows.to(torch.long).contiguous()
    _lib.check(_lib.lib().mmx_rows_to_dense(ctypes.c_void_p(vals.data_ptr()), ctypes.c_void_p(rows64.data_ptr()),
                                            ctypes.c_void_p(out.data_ptr()), B, N, E, ops._stream()), "mmx_rows_to_dense")
    assert same_bits(out, want) and guards_intact(buf)
    buf, dense = guarded((B, N, E))
    dense.copy_(torch.randn(B, N, E, generator=g))
    want2 = dense.clone()
    for b, r in inside:
        want2[b, r] += vals[b]
    assert ops.rows_add_(dense, rows, vals) is dense
    assert same_bits(dense, want2) and guards_intact(buf)


# ---------------------------------------------------------------------------------------------------------------------
# what the wrappers refuse (no kernel runs in these tests but the aligned calls)
# ---------------------------------------------------------------------------------------------------------------------
def test_layernorm_backward_wrappers_refuse_operands_of_another_shape(ops):
    from test_gpu_gemm_rows_pipeline import hand_list
    from transformer_mm_explainability_amd._lib import MMXError
    rows, E = 6, 20
    t = lambda *shape: torch.randn(*shape, device="cuda")
    dy, x, gamma, mean, rstd = t(rows, E), t(rows, E), t(E), t(rows), t(rows).abs()
    dyh = dy.to(torch.bfloat16)
    live = hand_list([0, 3], rows)
    for d_res in (t(rows - 1, E), t(rows + 1, E), t(1, E), t(rows, E - 4), t(2 * rows, E // 2), t(E)):       # shorter, longer, reshaped
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add(dy, x, mean, rstd, gamma, d_res)
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add_bf16(dyh, x, mean, rstd, gamma, d_res)
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add_bf16(dyh, x, mean, rstd, gamma, d_res, want_f32=False)
    for bad_x, n in ((t(rows, E + 4), rows), (t(rows, E - 4), rows), (t(2 * rows, E // 2), 2 * rows), (t(rows * E // 4, 4), rows * E // 4)):
        m, r = t(n), t(n).abs()                                               # statistics that match the rows of the wrong x
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add(dy, bad_x, m, r, gamma)
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add_bf16(dyh, bad_x, m, r, gamma)
    with pytest.raises(MMXError):
        ops.layernorm_bwd_add_rows(dy.view(1, rows, E), t(1, rows * 2, E // 2), mean, rstd, gamma, None, live)
    for x_rows in (4, 5, 12):                                                 # 6 rows of dy over 4, 5 or 12 rows of x
        m, r = t(x_rows), t(x_rows).abs()
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add(dy, t(x_rows, E), m, r, gamma)
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add_bf16(dyh, t(x_rows, E), m, r, gamma)
    # and what stays allowed: the same rows under another leading shape (the model code hands [B, N, E] next to [B * N, E])
    a = ops.layernorm_bwd_add(dy, x, mean, rstd, gamma, t(rows, E))
    assert a.shape == dy.shape
    d = t(rows, E)
    assert same_bits(ops.layernorm_bwd_add(dy.view(2, 3, E), x.view(1, rows, E), mean, rstd, gamma, d.view(3, 2, E)).view(rows, E),
                     ops.layernorm_bwd_add(dy, x, mean, rstd, gamma, d))


def off_by_one(like):
    """A contiguous view of ``like``'s shape and dtype that starts one element into its buffer."""
    v = torch.empty(like.numel() + 1, dtype=like.dtype, device="cuda")[1:].view(like.shape)
    v.copy_(like)
    assert v.is_contiguous() and v.data_ptr() % 16 == like.element_size()
    return v


def test_bf16_and_one_row_entries_refuse_misaligned_pointers(ops):
    """One element into its buffer a view is contiguous and 4 (bf16: 2) bytes off the 16- and 8-byte groups of the kernels: each operand
    in turn is refused -- at both widths, so neither the row-resident nor the generic bf16 kernel has a misaligned route -- and the
    aligned call next to it goes through."""
    from transformer_mm_explainability_amd._lib import MMXError
    t = lambda *shape: torch.randn(*shape, device="cuda")
    for E in (20, 512):
        rows = 6
        good = dict(dy=t(rows, E).to(torch.bfloat16), x=t(rows, E), gamma=t(E), d_res=t(rows, E))
        mean, rstd = t(rows), t(rows).abs()
        call = lambda o, **kw: ops.layernorm_bwd_add_bf16(o["dy"], o["x"], mean, rstd, o["gamma"], o["d_res"], **kw)
        call(good)
        for name in good:
            bad = dict(good, **{name: off_by_one(good[name])})
            with pytest.raises(MMXError):
                call(bad)
            with pytest.raises(MMXError):
                call(bad, want_f32=False)
    B, N, E = 3, 5, 20
    vals, dense, rows = t(B, E), t(B, N, E), torch.tensor([0, 4, 2], device="cuda")
    ops.rows_to_dense(vals, rows, N)
    ops.rows_add_(dense, rows, vals)
    with pytest.raises(MMXError):
        ops.rows_to_dense(off_by_one(vals), rows, N)
    with pytest.raises(MMXError):
        ops.rows_add_(dense, rows, off_by_one(vals))
    with pytest.raises(MMXError):
        ops.rows_add_(off_by_one(dense), rows, vals)
    kept = dense.clone()
    odd_rows = off_by_one(rows)                                               # int64 ids one element in: 8-byte aligned, what the kernel needs
    assert same_bits(ops.rows_add_(dense, odd_rows, torch.zeros_like(vals)), kept)
