"""-m gpu: the forward row-wise kernels of ``csrc/elementwise_kernels.hip`` -- the fused residual add + LayerNorm
(``ops.add_layernorm``, ``ops.add_layernorm_rows``) and QuickGELU (``ops.quick_gelu_fwd``, ``ops.quick_gelu``, ``ops.quick_gelu_bwd``
and its fp32 broadcast forms) -- against the float64 references and worst-case rounding bounds of ``tests/rowwise_bounds.py``
(proved on the CPU by ``tests/test_rowwise_bounds_host.py``, where every mutant of these kernels is shown to break them).

Every element of every output is checked.  The worst error / bound of every output is recorded (``parity.note``) and printed, next to
the same figure for ATen's ``native_layer_norm`` on the device, which is recorded only.  What the wrappers refuse -- operands of the
wrong length, misaligned views, a broadcast ``x`` that is no multiple of 16 bytes -- is tested as a refusal: no kernel is launched."""
import numpy as np
import pytest
import torch

import rowwise_bounds as rb
from parity import note

pytestmark = pytest.mark.gpu

# rows per width: 1 ... 5 and 7 are the workgroup's four rows with a remainder, 70 and 257 more than one workgroup; at most 64 rows
# from E = 2048 on.  Every width meets a count that is no multiple of 4.
ROWS = {4: (1, 2, 3, 4, 5, 7, 70, 257), 20: (5, 257), 252: (3, 70), 256: (1, 7, 257), 260: (2, 70), 512: (4, 7), 516: (5, 70),
        768: (7, 257), 1024: (3, 70), 1028: (1, 7), 2048: (5, 7), 2052: (2, 3, 7), 4096: (1, 4, 7)}


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    return _ops


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    """Bit for bit; a NaN matches a NaN whatever its payload."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


def run_ln(ops, x, y, gamma, beta, eps, **kw):
    s, h, mean, rstd = ops.add_layernorm(dev(x), dev(y), dev(gamma), dev(beta), eps, **kw)
    return s, h, mean, rstd


def as_dict(s, h, mean, rstd):
    return {"s": host(s), "h": host(h), "mean": host(mean), "rstd": host(rstd)}


def worst(ratios, into):
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)


def report(what, top):
    line = "  ".join("%s %.3f" % (k, v) for k, v in top.items())
    print("\nrowwise-bounds %s worst error / bound: %s" % (what, line))
    for k, v in top.items():
        note("%s %s error/bound" % (what, k), v, bound=1.0)


@pytest.mark.parametrize("E", rb.WIDTHS)
def test_add_layernorm_meets_the_float64_bounds(ops, E):
    """Every family, ``y`` given and ``None``, the three ``eps``, at every row count of this width: ``s`` has the bits of the fp32 sum
    (``y=None``: it IS ``x``), ``mean`` / ``rstd`` / ``h`` are within their bounds, and a second call gives the same bits."""
    top, aten = {}, {}
    for rows in ROWS[E]:
        for case, (x, y, gamma, beta), eps in rb.ln_cases(rows, E):
            ref = rb.ln_ref(x, y, gamma, beta, eps)
            xd, yd, gd, bd = dev(x), dev(y), dev(gamma), dev(beta)
            s, h, mean, rstd = ops.add_layernorm(xd, yd, gd, bd, eps)
            assert s.shape == h.shape == (rows, E) and mean.shape == rstd.shape == (rows,)
            assert all(t.dtype == torch.float32 for t in (s, h, mean, rstd))
            if y is None:
                assert s is xd
            ratios = rb.ln_ratios(as_dict(s, h, mean, rstd), ref, E)
            worst(ratios, top)
            assert max(ratios.values()) <= 1.0, (E, rows, case, ratios)
            again = ops.add_layernorm(xd, yd, gd, bd, eps)
            assert all(same_bits(a, b) for a, b in zip((s, h, mean, rstd), again)), (E, rows, case)
            # where the library stands on the same v = fp32(x + y): recorded, never asserted
            ah, am, ar = torch.native_layer_norm(dev(ref["s"]), (E,), gd, bd, eps)
            worst(rb.ln_ratios({"h": host(ah), "mean": host(am).reshape(-1), "rstd": host(ar).reshape(-1)}, ref, E), aten)
    report("add_layernorm E=%d" % E, {k: top[k] for k in ("s", "mean", "rstd", "h")})
    report("aten native_layer_norm E=%d" % E, {k: aten[k] for k in ("mean", "rstd", "h")})


@pytest.mark.parametrize("E", [20, 260, 1028, 2052])
def test_add_layernorm_rows_do_not_touch_each_other(ops, E):
    """rows = 7: a NaN, then +inf, then -inf in one row makes that row's ``h`` NaN as in the reference and leaves every bit of every other
    row's ``s``, ``h``, ``mean`` and ``rstd`` what the clean run gave; the same with one constant row among ``off1e3`` rows."""
    rows, bad, eps = 7, 4, 1e-5
    x, y, gamma, beta = rb.ln_case("off1e3", rows, E, True)
    clean = run_ln(ops, x, y, gamma, beta, eps)
    others = [r for r in range(rows) if r != bad]

    def check(xp, yp, what):
        got = run_ln(ops, xp, yp, gamma, beta, eps)
        for name, a, b in zip(("s", "h", "mean", "rstd"), got, clean):
            assert same_bits(a[others], b[others]), (E, what, name)
        return got

    for value in (float("nan"), float("inf"), float("-inf")):
        for col in (0, E - 1):
            xp = x.copy()
            xp[bad, col] = value
            s, h, mean, rstd = check(xp, y, value)
            ref = rb.ln_ref(xp, y, gamma, beta, eps)
            assert np.isnan(ref["h"][bad]).all() and bool(torch.isnan(h[bad]).all()), (E, value, col)
            assert max(rb.ln_ratios(as_dict(s, h, mean, rstd), ref, E).values()) <= 1.0          # NaN / inf where the reference has them
    xp, yp = x.copy(), y.copy()
    xp[bad], yp[bad] = 0.1, 0.0
    got = check(xp, yp, "const")
    ratios = rb.ln_ratios(as_dict(*got), rb.ln_ref(xp, yp, gamma, beta, eps), E)
    assert max(ratios.values()) <= 1.0, (E, ratios)


@pytest.mark.parametrize("E", rb.WIDTHS)
def test_add_layernorm_bf16_h_is_the_fp32_h_rounded_once(ops, E):
    rows = ROWS[E][-1] if E < 2048 else 7
    for name in ("std", "off1e3", "spike"):
        for with_y in (False, True):
            x, y, gamma, beta = rb.ln_case(name, rows, E, with_y)
            s32, h32, m32, r32 = run_ln(ops, x, y, gamma, beta, 1e-5)
            s16, h16, m16, r16 = run_ln(ops, x, y, gamma, beta, 1e-5, h_dtype=torch.bfloat16)
            assert h16.dtype == torch.bfloat16 and same_bits(h16, h32.to(torch.bfloat16)), (E, name, with_y)
            assert same_bits(s16, s32) and same_bits(m16, m32) and same_bits(r16, r32), (E, name, with_y)


@pytest.mark.parametrize("E", [252, 516, 1028, 2052, 4096])
def test_add_layernorm_rows_inherits_the_bounds(ops, E):
    """One case per register-width instantiation of the row-list kernel, on a shuffled list: the listed rows against float64 under the
    dense kernel's bounds (that they have the dense kernel's bits is ``tests/test_gpu_rows_kernels_edges.py``'s subject)."""
    from test_gpu_gemm_rows_pipeline import hand_list
    cap, top = 37, {}
    entries = torch.randperm(cap, generator=torch.Generator().manual_seed(E)).tolist()[:23]
    live = hand_list(entries, cap)
    listed = sorted(entries)
    for name in ("std", "off1e3s", "spike", "const"):
        for with_y in (False, True):
            x, y, gamma, beta = rb.ln_case(name, cap, E, with_y)
            sentinel = lambda *shape: torch.full(shape, 7.25, device="cuda")
            out = (sentinel(1, cap, E), sentinel(1, cap, E), sentinel(cap), sentinel(cap))
            xd, yd = dev(x).view(1, cap, E), (dev(y).view(1, cap, E) if with_y else None)
            s, h, mean, rstd = ops.add_layernorm_rows(xd, yd, dev(gamma), dev(beta), 1e-6, live, out=out)
            got = {k: v.reshape(cap, -1)[listed].reshape((len(listed), E) if k in ("s", "h") else (len(listed),))
                   for k, v in as_dict(s, h, mean, rstd).items()}
            ref = rb.ln_ref(x[listed], None if y is None else y[listed], gamma, beta, 1e-6)
            ratios = rb.ln_ratios(got, ref, E)
            worst(ratios, top)
            assert max(ratios.values()) <= 1.0, (E, name, with_y, ratios)
    report("add_layernorm_rows E=%d" % E, top)


# ---------------------------------------------------------------------------------------------------------------------
# QuickGELU
# ---------------------------------------------------------------------------------------------------------------------
GRID_STRIDE = 4096 * 256 * 4 + 4 * 256 * 3 + 3          # past the 4096 workgroups of 256 lanes x 4 elements, with a scalar tail
COUNTS = (1, 2, 3, 5, 1023, 1024, 1027, GRID_STRIDE)


@pytest.mark.parametrize("n", COUNTS)
def test_quick_gelu_meets_the_float64_bounds(ops, n):
    """``quick_gelu_fwd``, the autograd op and ``quick_gelu_bwd`` on the grid, ``3 randn`` and the specials; the bf16 forward is the
    fp32 result rounded once, at every count (the bf16 kernel takes multiples of 4 only)."""
    top = {}
    for seed in (range(20) if n <= 5 else (0,)):         # tiny counts: every window of the special values, then five of 3 randn
        x, dy = rb.gelu_inputs(n, seed)
        xd, dyd = dev(x), dev(dy)
        y = ops.quick_gelu_fwd(xd)
        r, why = rb.gelu_fwd_check(host(y), x)
        assert y.dtype == torch.float32 and r <= 1.0 and not why, (n, seed, r, why)
        dx = ops.quick_gelu_bwd(xd, dyd)
        rbk, why = rb.gelu_bwd_check(host(dx), x, dy)
        assert rbk <= 1.0 and not why, (n, seed, rbk, why)
        worst({"forward": r, "backward": rbk}, top)
        leaf = xd.clone().requires_grad_(True)
        ya = ops.quick_gelu(leaf)
        ya.backward(dyd)
        assert same_bits(ya.detach(), y) and same_bits(leaf.grad, dx), (n, seed)
        y16 = ops.quick_gelu_fwd(xd, torch.bfloat16)
        assert y16.dtype == torch.bfloat16 and same_bits(y16, y.to(torch.bfloat16)), (n, seed)
    report("quick_gelu n=%d" % n, top)


@pytest.mark.parametrize("xb", [1, 3])
def test_quick_gelu_bwd_fp32_broadcast_forms(ops, xb):
    """``x`` of batch 1 (shared forward) and of batch M = 3 against ``dy`` of batch 6 = K * M in K-major order (target t reads sample
    t % M): the bits of the call with ``x`` expanded to ``dy``'s shape, within the backward bound."""
    top = {}
    for shape in ((5, 12), (7, 4), (3, 1028)):
        rng = np.random.default_rng([xb, shape[1]])
        x = (3.0 * rng.standard_normal((xb,) + shape)).astype(np.float32)
        x.reshape(-1)[:8] = rb.FAR                           # finite points outside |z| <= 80 ride along
        dy = rng.standard_normal((6,) + shape).astype(np.float32)
        got = ops.quick_gelu_bwd(dev(x), dev(dy))
        full = np.tile(x, (6 // xb, 1, 1))
        assert np.array_equal(full.reshape(-1), x.reshape(-1)[rb.bcast_index(dy.size, x.size)])
        assert same_bits(got, ops.quick_gelu_bwd(dev(full), dev(dy))), (xb, shape)
        r, why = rb.gelu_bwd_check(host(got), full, dy)
        assert got.shape == dy.shape and r <= 1.0 and not why, (xb, shape, r, why)
        worst({"broadcast": r}, top)
    report("quick_gelu_bwd broadcast x batch %d" % xb, top)


def test_quick_gelu_bwd_refuses_a_broadcast_x_that_is_no_multiple_of_four(ops):
    from transformer_mm_explainability_amd._lib import MMXError
    x, dy = torch.randn(1, 5, 3, device="cuda"), torch.randn(6, 5, 3, device="cuda")
    with pytest.raises(MMXError):
        ops.quick_gelu_bwd(x, dy)
    with pytest.raises(MMXError):
        ops.quick_gelu_bwd(torch.randn(3, 5, 3, device="cuda"), dy)


# ---------------------------------------------------------------------------------------------------------------------
# what the wrappers refuse (no kernel runs in these tests but the last one's aligned calls)
# ---------------------------------------------------------------------------------------------------------------------
def test_layernorm_wrappers_refuse_operands_of_the_wrong_length(ops):
    from test_gpu_gemm_rows_pipeline import hand_list
    from transformer_mm_explainability_amd._lib import MMXError
    rows, E = 6, 20
    t = lambda *shape: torch.randn(*shape, device="cuda")
    x, y, dy, gamma, beta, mean, rstd = t(rows, E), t(rows, E), t(rows, E), t(E), t(E), t(rows), t(rows).abs()
    live = hand_list([0, 3], rows)
    x3, y3, dy3 = x.view(1, rows, E), y.view(1, rows, E), dy.view(1, rows, E)
    for short in (t(E - 4), t(E + 4), t(1)):
        for g, b in ((short, beta), (gamma, short)):
            with pytest.raises(MMXError):
                ops.add_layernorm(x, y, g, b)
            with pytest.raises(MMXError):
                ops.add_layernorm(x, None, g, b, h_dtype=torch.bfloat16)
            with pytest.raises(MMXError):
                ops.add_layernorm_rows(x3, y3, g, b, 1e-5, live)
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add(dy, x, mean, rstd, short)
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add_bf16(dy.to(torch.bfloat16), x, mean, rstd, short)
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add_rows(dy3, x3, mean, rstd, short, None, live)
    for m, r in ((t(rows - 1), rstd), (mean, t(rows + 1)), (t(1), t(1)), (t(2 * rows), t(2 * rows))):
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add(dy, x, m, r, gamma)
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add(t(2, rows, E), x, m, r, gamma)             # x shared by a batch of 2: still x's row count
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add_bf16(dy.to(torch.bfloat16), x, m, r, gamma)
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add_rows(dy3, x3, m, r, gamma, None, live)


def test_layernorm_entries_refuse_pointers_that_are_not_16_byte_aligned(ops):
    """A contiguous view that starts one element into its buffer is contiguous fp32 -- and 4 bytes off the 16-byte loads of the
    kernels.  Each operand in turn; the aligned call next to it goes through."""
    from test_gpu_gemm_rows_pipeline import hand_list
    from transformer_mm_explainability_amd._lib import MMXError
    rows, E = 6, 20
    live = hand_list([0, 3], rows)

    def off(*shape):
        n = int(np.prod(shape))
        v = torch.randn(n + 1, device="cuda")[1:].view(*shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    t = lambda *shape: torch.randn(*shape, device="cuda")
    fwd = dict(x=t(rows, E), y=t(rows, E), gamma=t(E), beta=t(E))
    ops.add_layernorm(**fwd)
    for name in fwd:
        bad = dict(fwd, **{name: off(*fwd[name].shape)})
        with pytest.raises(MMXError):
            ops.add_layernorm(**bad)
        with pytest.raises(MMXError):
            ops.add_layernorm(**bad, h_dtype=torch.bfloat16)
        bad3 = {k: (v.view(1, rows, E) if v.dim() == 2 else v) for k, v in bad.items()}
        with pytest.raises(MMXError):
            ops.add_layernorm_rows(bad3["x"], bad3["y"], bad3["gamma"], bad3["beta"], 1e-5, live)
    for name in ("s", "h"):                                                   # the outputs a caller hands to the row-list form
        out = dict(s=t(1, rows, E), h=t(1, rows, E), mean=t(rows), rstd=t(rows))
        out[name] = off(1, rows, E)
        with pytest.raises(MMXError):
            ops.add_layernorm_rows(fwd["x"].view(1, rows, E), fwd["y"].view(1, rows, E), fwd["gamma"], fwd["beta"], 1e-5, live,
                                   out=(out["s"], out["h"], out["mean"], out["rstd"]))
    _, _, mean, rstd = ops.add_layernorm(fwd["x"], None, fwd["gamma"], fwd["beta"])
    bwd = dict(dy=t(rows, E), x=fwd["x"], gamma=fwd["gamma"], d_res=t(rows, E))
    ops.layernorm_bwd_add(bwd["dy"], bwd["x"], mean, rstd, bwd["gamma"], bwd["d_res"])
    for name in bwd:
        bad = dict(bwd, **{name: off(*bwd[name].shape)})
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add(bad["dy"], bad["x"], mean, rstd, bad["gamma"], bad["d_res"])
        with pytest.raises(MMXError):
            ops.layernorm_bwd_add_rows(bad["dy"].view(1, rows, E), bad["x"].view(1, rows, E), mean, rstd, bad["gamma"],
                                       bad["d_res"].view(1, rows, E), live)
    with pytest.raises(MMXError):
        ops.layernorm_bwd_add_rows(bwd["dy"].view(1, rows, E), bwd["x"].view(1, rows, E), mean, rstd, bwd["gamma"], None, live,
                                   out=off(1, rows, E))
