"""-m gpu: the LRP relprop kernels -- the attention core of ``csrc/attention_lrp.hip`` and the rule kernels of ``csrc/lrp_kernels.hip``
behind ``ops.lrp_linear`` / ``lrp_add`` / ``lrp_clone`` / ``lrp_mha_rescale`` -- against the float64 references and the counted
per-element bounds of ``tests/lrp_bounds.py`` (proved on the CPU by ``tests/test_lrp_bounds_host.py``, where an fp32 restatement of
every row is shown inside them and every mutant outside by 2x).

Every element of every output is judged: error <= its bound (infinite where the module says an element cannot be judged), NaN exactly
where the reference is NaN.  The attention core runs through ``ops.attn_relprop`` in every layout of the table -- ``[B, N, H, D]``,
``[B, H, N, D]``, slices of one packed ``[B, N, 3, H, D]``, ``o`` / ``cam_o`` with a NaN-filled margin behind every row -- and its
ragged-tile rows once more through ``mmx_attn_relprop_phase`` on a NaN-filled arena with guard bands (``tests/guard_arena.py``): the
guards stay NaN and a phase that does not run writes nothing.  A second call gives the same bits; in SCALE_SCORES mode scale = 0.37
gives the bits of scale = 1; a NaN stays inside its (b, h).  The rules: the three raw entries on an arena over one, two and three
trips of the capped grid, ``ops.lrp_linear`` on both GEMM routes, ``ops.lrp_add`` per sample and whole, ``ops.lrp_clone`` with up
to 8 inputs, ``ops.lrp_mha_rescale`` with its branch taken and not, and the torch fall-backs beyond the kernels' limits.  The worst
error / bound of every output and family is recorded (``parity.note``) and printed."""
import ctypes as C

import numpy as np
import pytest
import torch

import lrp_bounds as lb
from guard_arena import Arena, ptr
from parity import note
from test_gpu_rowwise_forward import dev, host

pytestmark = pytest.mark.gpu

CHUNK = 25
NAME = {"cam_P": 0, "cam_q": 1, "cam_k": 2, "cam_v": 3}


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    return _ops


def same_bits(a, b):
    """Bit for bit; a NaN matches a NaN whatever its payload."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def record(what, top):
    print("\nlrp %s worst error / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(top.items()))))
    for k, v in top.items():
        note("lrp_bounds %s %s" % (what, k), v, bound=1.0)


def bump(top, key, value):
    top[key] = max(top.get(key, 0.0), value)


def chunks(cases, key):
    by = {}
    for c in cases:
        by.setdefault(key(c), []).append(c)
    out = []
    for name, rows in sorted(by.items()):
        for i in range(0, len(rows), CHUNK):
            out.append(pytest.param(rows[i:i + CHUNK], id="%s-%d" % (name, i // CHUNK)))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# attention core
# ---------------------------------------------------------------------------------------------------------------------
def margin_view(a, extra=8):
    """``a [B, N, H, D]`` as a view of a NaN-filled ``[B, N, H D + extra]`` buffer: a row stride above H D."""
    B, N, Hh, D = a.shape
    buf = torch.full((B, N, Hh * D + extra), float("nan"), dtype=torch.float32, device="cuda")
    view = buf[..., :Hh * D].unflatten(-1, (Hh, D))
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.stride(1) == Hh * D + extra
    return view


def core_operands(c, x):
    """The device operands of a row in its layout -> ``(dict, layout)``."""
    lay = c["layout"]
    t = {n: dev(x[n]) for n in ("q", "k", "v", "o", "cam_o", "probs", "cam_scores")}
    if lay == "packed":
        qkv = torch.stack((t["q"], t["k"], t["v"]), dim=2).contiguous()          # [B, N, 3, H, D]
        t["q"], t["k"], t["v"] = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        assert not t["q"].is_contiguous()
    if lay == "padded_o":
        t["o"], t["cam_o"] = margin_view(x["o"]), margin_view(x["cam_o"])
    if lay == "bhnd":
        for n in ("q", "k", "v", "o", "cam_o"):
            t[n] = t[n].permute(0, 2, 1, 3).contiguous()
        return t, "bhnd"
    return t, "bnhd"


def run_core(ops, c, t, layout, scale=None):
    """One ``ops.attn_relprop`` call in the form of the row -> dict of the outputs it stores, q / k / v cams as ``[B, N, H, D]``."""
    values = bool(c["phase"] & lb.VALUES)
    pick = lambda n: t[n] if values else None                       # noqa: E731
    got = ops.attn_relprop(t["q"], t["k"], pick("v"), pick("probs"), pick("o"), pick("cam_o"), lb.scale_of(c) if scale is None else scale,
                           c["mode"], layout, phase=c["phase"], cam_scores=t["cam_scores"] if lb.with_scores(c) else None)
    torch.cuda.synchronize()
    out = {}
    for n in lb.CORE_OUT:
        g = got[NAME[n]]
        assert (g is not None) == (n in lb.stored(c)), (c["id"], n)
        if g is not None:
            out[n] = g.permute(0, 2, 1, 3) if (layout == "bhnd" and n != "cam_P") else g
    return out


def judge_core(c, got, ref, top, bad):
    figs = {}
    for n in lb.stored(c):
        g = host(got[n])
        if not np.array_equal(np.isnan(g), np.isnan(ref[n])):
            bad.append((c["id"], n, "NaN pattern"))
        figs[n] = lb.ratio(g, ref[n], ref["e_" + n])
        bump(top, "%s %s" % (c["family"], n), figs[n])
        if not figs[n] <= 1.0:
            bad.append((c["id"], n, figs[n]))
    print("%s mode %d %s: %s   unjudged %s" % (c["id"], c["mode"], c["layout"], "  ".join("%s %.4g" % kv for kv in figs.items()),
                                               "  ".join("%s %.4f" % (n, lb.unjudged_share(ref["e_" + n])) for n in lb.stored(c))))


def phase_name(c):
    return {lb.FUSED: "fused", lb.VALUES: "values", lb.SCORES_PHASE: "scores"}[c["phase"]]


@pytest.mark.parametrize("rows", chunks(lb.core_cases(), lambda c: "%s-dp%d" % (phase_name(c), 32 if c["D"] <= 32 else 64)))
def test_attention_core_meets_the_float64_bound(ops, rows):
    """Every table row of one (phase, DP): every output within its bound and NaN where the reference is; the same bits on a second
    call; SCALE_SCORES: scale = 0.37 gives the bits of scale = 1; ``nanrow``: every (b, h) but the two poisoned ones keeps the bits of
    the clean run."""
    top, bad = {}, []
    for c in rows:
        x = lb.core_inputs(c)
        ref = lb.core_ref(x, lb.scale_of(c), c["mode"], c["phase"], lb.with_scores(c))
        t, layout = core_operands(c, x)
        got = run_core(ops, c, t, layout)
        judge_core(c, got, ref, top, bad)
        again = run_core(ops, c, t, layout)
        assert all(same_bits(got[n], again[n]) for n in got), ("second call", c["id"])
        if c["mode"] == lb.SCORES:
            one = run_core(ops, c, t, layout, scale=1.0)
            assert all(same_bits(got[n], one[n]) for n in got), ("SCALE_SCORES reads scale", c["id"])
        if c["family"] == "nanrow":
            clean_c = dict(c, family="offset")
            tc, _ = core_operands(clean_c, lb.core_inputs(clean_c))
            clean = run_core(ops, clean_c, tc, layout)
            B, Hh = c["B"], c["H"]
            for n in got:
                a, b = (v if n == "cam_P" else v.permute(0, 2, 1, 3) for v in (got[n], clean[n]))        # [B, H, ...]
                for bi in range(B):
                    for h in range(Hh):
                        if (bi, h) not in ((0, 0), (B - 1, Hh - 1)):
                            assert same_bits(a[bi, h], b[bi, h]), ("a NaN left its (b, h)", c["id"], n, bi, h)
    record("core %s dp%d" % (phase_name(rows[0]), 32 if rows[0]["D"] <= 32 else 64), top)
    assert not bad, bad


def _strides(N, Hh, D):
    return [N * Hh * D, D, Hh * D]                                   # (batch, head, token) of a contiguous [B, N, H, D]


@pytest.mark.parametrize("rows", chunks([c for c in lb.core_cases() if (c["Nq"], c["Nk"]) in lb.RAGGED],
                                        lambda c: "arena-%s" % phase_name(c)))
def test_ragged_rows_on_a_guarded_arena(ops, rows):
    """``mmx_attn_relprop_phase`` itself, outputs inside one NaN-filled arena: every output the phase stores within its bound, the
    guard bands untouched, and the outputs of a phase that does not run still all NaN."""
    from transformer_mm_explainability_amd import _lib
    top, bad = {}, []
    for c in rows:
        x = lb.core_inputs(c)
        ref = lb.core_ref(x, lb.scale_of(c), c["mode"], c["phase"], lb.with_scores(c))
        B, Hh, Nq, Nk, D = c["B"], c["H"], c["Nq"], c["Nk"], c["D"]
        t = {n: dev(x[n]) for n in ("q", "k", "v", "o", "cam_o", "probs", "cam_scores")}
        sizes = [B * Hh * Nq * Nk, B * Nq * Hh * D, B * Nk * Hh * D, B * Nk * Hh * D]                 # cam_P, cam_q, cam_k, cam_v
        arena = Arena(sizes)
        out = [arena.region(i) for i in range(4)]
        sq, sk = _strides(Nq, Hh, D), _strides(Nk, Hh, D)
        rc = _lib.lib().mmx_attn_relprop_phase(
            ptr(t["q"]), ptr(t["k"]), ptr(t["v"]), ptr(t["o"]), ptr(t["cam_o"]), *sq, *sk, *sk, *sq, *sq,
            ptr(t["probs"]), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), *sq, *sk, *sk,
            B, Hh, Nq, Nk, D, float(lb.scale_of(c)), c["mode"], ptr(t["cam_scores"] if lb.with_scores(c) else None), c["phase"],
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "mmx_attn_relprop_phase")
        torch.cuda.synchronize()
        values, scores = bool(c["phase"] & lb.VALUES), bool(c["phase"] & lb.SCORES_PHASE)
        arena.assert_guards_untouched([sizes[0] if values else 0, sizes[1] if scores else 0, sizes[2] if scores else 0,
                                       sizes[3] if values else 0])
        got = {"cam_P": out[0].view(B, Hh, Nq, Nk), "cam_q": out[1].view(B, Nq, Hh, D), "cam_k": out[2].view(B, Nk, Hh, D),
               "cam_v": out[3].view(B, Nk, Hh, D)}
        judge_core(c, {n: got[n] for n in lb.stored(c)}, ref, top, bad)
    record("core arena %s" % phase_name(rows[0]), top)
    assert not bad, bad


def test_head_dim_65_raises(ops):
    from transformer_mm_explainability_amd import _lib
    g = torch.Generator().manual_seed(1)
    q, k, v, o, cam_o = (torch.randn(1, 5, 2, 65, generator=g).cuda() for _ in range(5))
    probs = torch.softmax(torch.randn(1, 2, 5, 5, generator=g), -1).cuda()
    with pytest.raises(_lib.MMXError):
        ops.attn_relprop(q, k, v, probs, o, cam_o, 65 ** -0.5)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# rules
# ---------------------------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lrp_workspace(ops):
    from transformer_mm_explainability_amd import _lib
    return ops._workspace(_lib.lib().mmx_lrp_workspace_bytes(), torch.device("cuda", torch.cuda.current_device()), tag="lrp")


def judge_rule(c, got, ref, top, bad):
    figs = {}
    for n, (val, bound) in ref.items():
        g = host(got[n]).reshape(val.shape)
        if not np.array_equal(np.isnan(g), np.isnan(val)):
            bad.append((c["id"], n, "NaN pattern"))
        figs[n] = lb.ratio(g, val, bound)
        bump(top, "%s %s %s" % (c["kind"], c["family"], n), figs[n])
        if not figs[n] <= 1.0:
            bad.append((c["id"], n, figs[n]))
    print("%s %s: %s   unjudged %s" % (c["id"], {k: v for k, v in c.items() if k not in ("id", "kind", "seed", "family")},
                                       "  ".join("%s %.4g" % kv for kv in figs.items()),
                                       "  ".join("%s %.4f" % (n, lb.unjudged_share(b)) for n, (_v, b) in ref.items())))


@pytest.mark.parametrize("rows_n", lb.COUNTS, ids=lambda p: "%dx%d" % p)
def test_split_signs_and_safe_divide_on_an_arena(ops, rows_n):
    """``mmx_lrp_split_signs`` gives the bits of the two clamps (a NaN in both halves, -0 kept), ``mmx_lrp_safe_divide`` is within
    ``2 u |s| + 2**-126`` of float64 with the reference's NaN pattern -- over one, two and three trips of the capped grid, the guard
    bands untouched."""
    from transformer_mm_explainability_amd import _lib
    rows, n = rows_n
    g = np.random.default_rng(rows * 31 + n)
    X = g.standard_normal((rows, n)).astype(lb.F32)
    X.reshape(-1)[::5] = 0.0
    X.reshape(-1)[1::7] = -0.0
    lb.specials(X, g)
    a, b = (g.standard_normal(rows * n) * 0.05).astype(lb.F32), g.standard_normal(rows * n).astype(lb.F32)
    b[::6] = 0.0
    b[1::6] = -lb.EPS
    lb.specials(b, g)
    lb.specials(a, g)
    arena = Arena([2 * rows * n, rows * n])
    Xd, ad, bd = dev(X), dev(a), dev(b)                              # (held until the kernels have run)
    _lib.check(_lib.lib().mmx_lrp_split_signs(ptr(Xd), ptr(arena.region(0)), rows, n, _stream()), "mmx_lrp_split_signs")
    _lib.check(_lib.lib().mmx_lrp_safe_divide(ptr(ad), ptr(bd), ptr(arena.region(1)), rows * n, _stream()), "mmx_lrp_safe_divide")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([2 * rows * n, rows * n])
    assert same_bits(arena.region(0).view(rows, 2 * n).cpu(), torch.from_numpy(lb.split_signs(X)))
    s, e, unj = lb.sd(a, b)
    got = host(arena.region(1))
    assert not unj.any() and np.array_equal(np.isnan(got), np.isnan(s))
    fig = lb.ratio(got, s, e)
    record("safe_divide %dx%d" % rows_n, {"s": fig})
    assert fig <= 1.0, fig


def run_rule(ops, c, x):
    """One call of the rule a row names -> dict of device outputs."""
    from transformer_mm_explainability_amd import _lib
    kind = c["kind"]
    if kind == "combine":
        rows, n = c["rows"], c["n"]
        arena = Arena([rows * n])
        R, XX, Y = (dev(x["R"]) if c["m"] else None), dev(x["XX"]), dev(x["Y"])          # (held until the kernels have run)
        ws = _lrp_workspace(ops) if c["m"] else None
        _lib.check(_lib.lib().mmx_lrp_linear_combine(ptr(XX), ptr(Y), ptr(arena.region(0)), rows, n, ptr(R), x["R"].size if c["m"] else 0,
                                                     ptr(ws), _stream()), "mmx_lrp_linear_combine")
        torch.cuda.synchronize()
        arena.assert_guards_untouched([rows * n])
        return {"out": arena.region(0).view(rows, n)}
    if kind == "linear":
        return {"out": ops.lrp_linear(dev(x["R"]), dev(x["X"]), dev(x["W"]), c["normalize"])}
    if kind == "add":
        ra, rb = ops.lrp_add(dev(x["R"]), dev(x["a"]), dev(x["b"]), c["per_sample"])
        return {"ra": ra, "rb": rb}
    if kind == "clone":
        return {"out": ops.lrp_clone([dev(r) for r in x["Rs"]], dev(x["X"]))}
    k, q = ops.lrp_mha_rescale(*(dev(x[n]) for n in ("v_pre", "v_post", "cam_k", "cam_q", "cam_o")))
    return {"cam_k": k, "cam_q": q}


@pytest.mark.parametrize("rows", chunks(lb.rule_cases(), lambda c: c["kind"]))
def test_rules_meet_the_float64_bound(ops, rows):
    """Every row of the rules table of one kind: every output within its bound, NaN where the reference is, the same bits on a second
    call; a rescale whose branch is not taken leaves the bits of cam_k / cam_q alone."""
    top, bad = {}, []
    for c in rows:
        x = lb.rule_inputs(c)
        ref = lb.rule_ref(c, x)
        got = run_rule(ops, c, x)
        torch.cuda.synchronize()
        judge_rule(c, got, ref, top, bad)
        again = run_rule(ops, c, x)
        torch.cuda.synchronize()
        assert all(same_bits(got[n], again[n]) for n in got), ("second call", c["id"])
        if c["kind"] == "rescale":
            taken = lb.rescale_taken(x["v_pre"], x["v_post"])
            assert taken == (c["branch"] in ("taken", "pre_nan")), c["id"]
            if not taken:
                assert same_bits(got["cam_k"].cpu(), torch.from_numpy(x["cam_k"])) and same_bits(got["cam_q"].cpu(), torch.from_numpy(x["cam_q"]))
    record("rules %s" % rows[0]["kind"], top)
    assert not bad, bad


def test_sign_split_weight_follows_an_in_place_update(ops):
    """The cached ``[max(W, 0) | min(W, 0)]`` and its transposed copy are rebuilt after ``weight.mul_(-1)``, and ``lrp_linear`` on the
    updated weight is inside the bound of the reference on -W (the 32 x 32-tile GEMM route reads the transposed copy)."""
    c = next(c for c in lb.rule_cases() if c["kind"] == "linear" and (c["rows"], c["n_in"], c["n_out"]) == (15, 12, 7) and c["normalize"])
    x = lb.rule_inputs(c)
    W = dev(x["W"])
    first = ops.lrp_linear(dev(x["R"]), dev(x["X"]), W, True)
    # (values, not bits: torch.clamp turns the -0 of a negated zero weight into +0, the numpy form keeps it)
    assert torch.equal(ops.sign_split_weight(W).cpu(), torch.from_numpy(lb.split_signs(x["W"])))
    W.mul_(-1)
    x2 = dict(x, W=-x["W"])
    assert torch.equal(ops.sign_split_weight(W).cpu(), torch.from_numpy(lb.split_signs(x2["W"])))
    assert torch.equal(ops.sign_split_weight(W, transposed=True).cpu(), torch.from_numpy(np.ascontiguousarray(lb.split_signs(x2["W"]).T)))
    second = ops.lrp_linear(dev(x["R"]), dev(x["X"]), W, True)
    torch.cuda.synchronize()
    top, bad = {}, []
    judge_rule(c, {"out": first}, lb.rule_ref(c, x), top, bad)
    judge_rule(c, {"out": second}, lb.rule_ref(c, x2), top, bad)
    record("rules linear after weight.mul_(-1)", top)
    assert not bad, bad
    assert not same_bits(first, second)


def test_beyond_the_kernels_limits_torch_takes_over_inside_the_bound():
    """``lrp.add_relprop`` with 65 samples and ``lrp.clone_relprop`` with 9 inputs run the torch formulation: still inside the bounds."""
    from transformer_mm_explainability_amd import lrp
    top, bad = {}, []
    c = dict(kind="add", batch=65, per=257, per_sample=True, family="positive", seed=900, id="add-65-samples")
    x = lb.rule_inputs(c)
    ra, rb = lrp.add_relprop(dev(x["R"]), dev(x["a"]), dev(x["b"]), per_sample=True)
    judge_rule(c, {"ra": ra, "rb": rb}, lb.rule_ref(c, x), top, bad)
    c = dict(kind="clone", inputs=9, n=257, family="signed", seed=901, id="clone-9-inputs")
    x = lb.rule_inputs(c)
    out = lrp.clone_relprop([dev(r) for r in x["Rs"]], dev(x["X"]))
    judge_rule(c, {"out": out}, lb.rule_ref(c, x), top, bad)
    record("rules torch fall-back", top)
    assert not bad, bad


def test_safe_divide_special_values(ops):
    """Every pair of the special values through ``mmx_lrp_safe_divide``: the zero, sign, inf and NaN pattern of the fp32 CPU
    ``lrp.safe_divide`` and within ``2 u |s| + 2**-126`` of it.  Whether the bits are equal is recorded, not asserted."""
    from transformer_mm_explainability_amd import _lib, lrp
    a, b = lb.special_pairs()
    want = lrp.safe_divide(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    arena = Arena([a.size])
    ad, bd = dev(a), dev(b)
    _lib.check(_lib.lib().mmx_lrp_safe_divide(ptr(ad), ptr(bd), ptr(arena.region(0)), a.size, _stream()), "mmx_lrp_safe_divide")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([a.size])
    got = host(arena.region(0))
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok] == 0, want[ok] == 0) and np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
    assert np.array_equal(np.isinf(got), np.isinf(want))
    fin = np.isfinite(want)
    w64 = want[fin].astype(np.float64)
    assert (np.abs(got[fin] - w64) <= 2 * lb.U * np.abs(w64) + lb.TINY).all()
    equal = int(np.array_equal(got[ok].view(np.int32), want[ok].view(np.int32)))
    print("\nlrp safe_divide special values: %d pairs, bits equal to the fp32 CPU form: %s" % (a.size, "yes" if equal else "no"))
    note("lrp_bounds safe_divide special values: bits differ from the fp32 CPU form (0 = equal)", 1 - equal)
