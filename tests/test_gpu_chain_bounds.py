"""-m gpu: the kernels of the self-attention relevancy chain -- ``avg_heads_kernel``, ``self_chain_fused_kernel`` (plain and pipelined
stream loop), ``self_chain_groups_kernel``, ``self_chain_cols_kernel``, the one-launch-per-layer kernel of ``relevancy_chain_rows.hip``,
the split path on ``bmm_f32_kernel<32 / 64>`` / ``bmm_f32_tiles_kernel`` and the vector chain -- against the float64 references and the
counted per-element bounds of ``tests/chain_bounds.py`` (proved on the CPU by ``tests/test_chain_bounds_host.py``, where an fp32
restatement of every kernel is shown inside them and every mutant outside by 2x).

Every element of every output is checked: error <= its bound, NaN exactly where the reference has NaN and +inf exactly where it has
+inf.  In the ``nan`` and ``inf`` rows every sample but the poisoned one keeps the bits of the clean run.  A second call gives the same
bits (scratch, tickets and LDS counters are reused cleanly).  Where ``tests/test_gpu_ops.py`` promises equal bits they are asserted on
these rows too: the cols kernel against the fused kernel with one group, the groups kernel against the fused kernel at equal G, the
pipelined against the plain stream loop, the causal flag on and off, ``ChainPlan.launch`` against ``relevancy_self_chain``.  What the
raw C entries write lives in a NaN-filled arena whose guard bands must stay NaN (``tests/guard_arena.py``); every input slab is carved
out of a NaN-filled buffer with NaN margins on both sides, so that an over-read value that reaches a result shows.  The route is set by
the options and checked where the ABI shows it (``mmx_self_chain_workspace_bytes``: the group count, the split path).  The worst
error / bound per output and kernel is recorded (``parity.note``) and printed."""
import ctypes as C

import numpy as np
import pytest
import torch

import chain_bounds as cb
from guard_arena import Arena, ptr
from parity import note
from test_gpu_rowwise_forward import host

pytestmark = pytest.mark.gpu

CHUNK = 10                                   # table rows per test: a few seconds each
MARGIN = 64                                  # NaN elements on either side of every input slab
DEFAULTS = (("self_chain_algo", 0), ("self_chain_groups", 0), ("self_chain_pipe", 4), ("self_chain_nt", 1), ("self_chain_cols_c", 0),
            ("self_chain_cols_nb", 0), ("self_chain_rows", 0), ("debug_flags", 0), ("bmm_tiles", 1))
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture
def ops():
    """Options of the chain kernels are process-global: whatever a row sets is put back, also when the test fails."""
    from transformer_mm_explainability_amd import ops as _ops
    try:
        yield _ops
    finally:
        for key, value in DEFAULTS:
            _ops.set_option(key, value)


def lib():
    from transformer_mm_explainability_amd import _lib
    return _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    """Bit for bit; a NaN matches a NaN whatever its payload."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def carve(a, dt="f32", misaligned=False):
    """``a`` on the device as the slab type ``dt``, inside a NaN-filled buffer with ``MARGIN`` NaN elements before and behind it;
    ``misaligned``: the slab starts 4 bytes past a 16-byte boundary."""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(TORCH_DT[dt])
    shift = (4 // t.element_size()) if misaligned else 0
    buf = torch.full((t.numel() + 2 * MARGIN + shift,), float("nan"), dtype=t.dtype, device="cuda")
    view = buf[MARGIN + shift:MARGIN + shift + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return view


def chunks(cases, key=lambda c: c["kernel"]):
    by = {}
    for c in cases:
        by.setdefault(key(c), []).append(c)
    out = []
    for fam, rows in sorted(by.items()):
        for i in range(0, len(rows), CHUNK):
            out.append(pytest.param(rows[i:i + CHUNK], id="%s-%d" % (fam, i // CHUNK)))
    return out


def record(what, top):
    print("\nchain %s worst error / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(top.items()))))
    for k, v in top.items():
        note("chain_bounds %s %s" % (what, k), v, bound=1.0)


def bump(top, key, value):
    top[key] = max(top.get(key, 0.0), value)


# ---------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------
def on_device(c, x):
    dt, mis = c["dtype"], c["misaligned"]
    return {"attn": [carve(a[0] if c["shared"] else a, dt, mis) for a in x["attn"]], "grad": [carve(g, dt, mis) for g in x["grad"]],
            "R_init": carve(x["R_init"]), "R_sq_init": carve(x["R_sq_init"])}


def set_route(ops, c):
    for key, field in (("self_chain_algo", "algo"), ("self_chain_groups", "groups"), ("self_chain_pipe", "pipe"),
                       ("self_chain_cols_c", "cols_c"), ("self_chain_rows", "rows")):
        ops.set_option(key, c[field])


def run_chain(ops, c, d, plan=False, **over):
    """One call on the route of the case (``over``: options / the causal flag changed for a bit-identity partner) -> ``(R, SQ or None)``."""
    o = dict(c, **over)
    set_route(ops, o)
    if plan:
        out = ops.ChainPlan(d["attn"], d["grad"], c["B"], shared_attn=c["shared"], causal=o["causal_flag"]).launch()
    else:
        out = ops.relevancy_self_chain(d["attn"], d["grad"], c["B"], R_init=d["R_init"], R_sq_init=d["R_sq_init"],
                                       shared_attn=c["shared"], causal=o["causal_flag"])
    torch.cuda.synchronize()
    return (out[0].clone(), out[1].clone()) if isinstance(out, tuple) else (out.clone(), None)


def check_route(c):
    """The ABI's own account of the route: no scratch for one group and the cols kernel, tickets + G partial products for the layer
    groups, two matrices (+ the second right-hand side) on the split path."""
    L = lib()
    dt = {"f32": L.MMX_F32, "f16": L.MMX_F16, "bf16": L.MMX_BF16}[c["dtype"]]
    need = L.lib().mmx_self_chain_workspace_bytes(c["L"], c["B"], c["H"], c["N"], c["M"], dt)
    assert need == cb.workspace_bytes(c), (c["id"], need, cb.workspace_bytes(c))


def partners(c):
    """The runs that must give the bits of the row's own: ``(what, options)``."""
    out = []
    f32 = c["dtype"] == "f32"
    small = c["kernel"] in ("fused", "cols", "groups")
    if small and f32 and c["L"] >= 1 and c["G"] == 1:
        out.append(("cols == fused with one group", {"algo": 1 if c["kernel"] == "cols" else 5}))
    if small and f32 and c["G"] > 1:
        out.append(("groups == fused at equal G", {"algo": 4 if c["algo"] == 1 else 1}))
    if c["kernel"] == "fused" and c["cpl"]:
        out.extend(("stream loop at pipe %d == pipe %d" % (p, c["pipe"]), {"pipe": p}) for p in (0, 1, 2, 4) if p != c["pipe"])
    if small and f32 and c["family"] == "causal":
        out.append(("causal flag on == off", {"causal_flag": not c["causal_flag"]}))
    return out


@pytest.mark.parametrize("rows", chunks(cb.chain_cases(), lambda c: c["kernel"] + ("-grouped" if c["G"] > 1 else "")))
def test_the_chain_meets_the_float64_bound(ops, rows):
    top, bad = {}, []
    for c in rows:
        x = cb.chain_inputs(c)
        ref = cb.chain_ref(c, x)
        d = on_device(c, x)
        set_route(ops, c)
        check_route(c)
        R, SQ = run_chain(ops, c, d, plan=c["plan"])
        figs = {"R": cb.ratio(host(R), ref["R"], ref["e_R"])}
        if c["M"]:
            figs["SQ"] = cb.ratio(host(SQ), ref["SQ"], ref["e_SQ"])
        print("%s cpl %d%s%s%s%s%s: %s" % (c["id"], c["cpl"], " shared" if c["shared"] else "", " init" if c["init"] else "",
                                          " flag" if c["causal_flag"] else "", " +4B" if c["misaligned"] else "", " plan" if c["plan"] else "",
                                          "  ".join("%s %.4g" % kv for kv in figs.items())))
        for n, f in figs.items():
            if not f <= 1.0:
                bad.append((c["id"], n, f))                         # (every row's figures are printed before the chunk is judged)
            bump(top, "%s %s" % (c["family"], n), f)
        if c["family"] in ("nan", "inf"):
            g = host(R)
            if not (np.array_equal(np.isnan(g), np.isnan(ref["R"])) and np.array_equal(np.isposinf(g), np.isposinf(ref["R"]))):
                bad.append((c["id"], "non-finite class: NaN at %d (reference %d), +inf at %d (reference %d) elements"
                            % (np.isnan(g).sum(), np.isnan(ref["R"]).sum(), np.isposinf(g).sum(), np.isposinf(ref["R"]).sum())))
            clean, _ = run_chain(ops, c, on_device(c, cb.chain_inputs(c, poisoned=False)), plan=c["plan"])
            if not same_bits(R[1:], clean[1:]):
                bad.append((c["id"], "the poison left sample 0"))
        R2, SQ2 = run_chain(ops, c, d, plan=c["plan"])
        if not (same_bits(R, R2) and (SQ is None or same_bits(SQ, SQ2))):
            bad.append((c["id"], "second call"))
        for what, over in partners(c):
            if not same_bits(R, run_chain(ops, c, d, plan=c["plan"], **over)[0]):
                bad.append((c["id"], what))
        if c["plan"] and not same_bits(R, run_chain(ops, c, d)[0]):
            bad.append((c["id"], "ChainPlan.launch == relevancy_self_chain"))
    record(rows[0]["kernel"] + (" grouped" if rows[0]["G"] > 1 else ""), top)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the product alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", chunks(cb.bmm_cases()))
def test_the_product_meets_the_float64_bound(ops, rows):
    L = lib().lib()
    top, bad = {}, []
    for c in rows:
        a, b, cin = cb.bmm_inputs(c)
        want, e = cb.bmm_ref(a, b, cin, c["trans_a"], c["nan"], c["bias_row"])
        da, db, dc = carve(a), carve(b), carve(cin)
        batch, M, N, K = (1 if c["bias_row"] else c["batch"]), c["M"], c["N"], c["K"]
        ops.set_option("bmm_tiles", c["tiles"])
        outs = []
        for _ in range(2):
            arena = Arena([batch * M * N])
            out = arena.region(0)
            if c["bias_row"]:
                rc = L.mmx_linear_f32(ptr(da), ptr(db), ptr(dc), ptr(out), M, N, K, stream())
            else:
                rc = L.mmx_bmm_f32(ptr(da), ptr(db), ptr(dc), ptr(out), batch, M, N, K, int(c["trans_a"]), M * K, K * N, M * N,
                                   int(c["nan"]), stream())
            torch.cuda.synchronize()
            assert rc == 0, c["id"]
            arena.assert_guards_untouched([batch * M * N])
            outs.append(out.view(batch, M, N))
        f = cb.ratio(host(outs[0]), want, e)
        print("%s%s%s%s%s: %.4g" % (c["id"], " trans_a" if c["trans_a"] else "", " Cin" if c["cin"] else "", " nan_to_zero" if c["nan"] else "",
                                    " bias row" if c["bias_row"] else "", f))
        if not f <= 1.0:
            bad.append((c["id"], f))
        assert same_bits(outs[0], outs[1]), ("second call", c["id"])
        bump(top, "C", f)
    record("product " + rows[0]["kernel"], top)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# the vector chain and the head mean alone
# ---------------------------------------------------------------------------------------------------------------------
def run_vec(ops, c, x, d):
    """-> ``(out, reference, bound)``; the raw entries write into a guarded arena."""
    Lm = lib()
    L = Lm.lib()
    B, N = c["B"], c["N"]
    if c["op"] == "row":
        rows = torch.from_numpy(x["rows"]).cuda()
        out = ops.relevancy_chain_row(d["attn"], d["grad"], B, rows, shared_attn=c["shared"])
        torch.cuda.synchronize()
        y = dict(x, R_init=None, R_sq_init=None)
        return (out.clone(),) + cb.chain_row_ref(c, y, x["rows"])
    arena = Arena([B * N])
    out = arena.region(0)
    base = d["base"] if c["base"] else d["v"]
    if c["op"] == "matvec":
        rc = L.mmx_chain_matvec(ptr(d["A"]), ptr(d["v"]), ptr(base), ptr(out), B, N, stream())
        pair = cb.matvec_ref(x["A"], x["v"], x["base"])
    elif c["op"] == "vecmat":
        need = L.mmx_chain_vecmat_workspace_bytes(B, N)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        rc = L.mmx_chain_vecmat(ptr(d["A"]), ptr(d["v"]), ptr(base), ptr(out), B, N, ptr(ws), need, stream())
        pair = cb.vecmat_ref(x["v"], x["A"], x["base"])
    else:
        need = L.mmx_avg_heads_vecmat_workspace_bytes(B, N)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        dt = {"f32": Lm.MMX_F32, "f16": Lm.MMX_F16, "bf16": Lm.MMX_BF16}[c["dtype"]]
        rc = L.mmx_avg_heads_vecmat(ptr(d["attn"][0]), ptr(d["grad"][0]), ptr(d["v"]), ptr(base), ptr(out), B, c["H"], N, dt,
                                    0 if c["shared"] else -1, ptr(ws), need, stream())
        pair = cb.ahv_ref(x["v"], x["attn"][0], x["grad"][0], x["base"])
    torch.cuda.synchronize()
    assert rc == 0, c["id"]
    arena.assert_guards_untouched([B * N])
    return (out.view(B, N).clone(),) + pair


def vec_on_device(c, x):
    d = {"v": carve(x["v"]), "base": carve(x["base"]), "A": carve(x.get("A"))}
    if "attn" in x:
        d["attn"] = [carve(a[0] if c["shared"] else a, c["dtype"]) for a in x["attn"]]
        d["grad"] = [carve(g, c["dtype"]) for g in x["grad"]]
    return d


@pytest.mark.parametrize("rows", chunks(cb.vec_cases(), lambda c: c["op"]))
def test_the_vector_chain_meets_the_float64_bound(ops, rows):
    top, bad = {}, []
    for c in rows:
        x = cb.vec_inputs(c)
        d = vec_on_device(c, x)
        got, want, e = run_vec(ops, c, x, d)
        f = cb.ratio(host(got), want, e)
        print("%s%s%s %s: %.4g" % (c["id"], " base" if c["base"] else "", " shared" if c["shared"] else "", c["family"], f))
        if not f <= 1.0:
            bad.append((c["id"], f))
        assert same_bits(got, run_vec(ops, c, x, d)[0]), ("second call", c["id"])
        if c["family"] == "nan":                                    # the NaN gradient of sample 0 stays in sample 0
            xc = cb.vec_inputs(c, poisoned=False)
            assert bool(torch.isnan(got[0]).any()) and same_bits(got[1:], run_vec(ops, c, xc, vec_on_device(c, xc))[0][1:]), ("isolation", c["id"])
        bump(top, c["dtype"], f)
    record("vector " + rows[0]["op"], top)
    assert not bad, bad


@pytest.mark.parametrize("rows", chunks(cb.avg_cases(), lambda c: c["dtype"]))
def test_the_head_mean_meets_the_float64_bound(ops, rows):
    Lm = lib()
    L = Lm.lib()
    top, bad = {}, []
    for c in rows:
        a, g = cb.avg_inputs(c)
        want, e = cb.abar_ref(a, g)
        B, H, Nq, Nk = c["B"], c["H"], c["Nq"], c["Nk"]
        dt = {"f32": Lm.MMX_F32, "f16": Lm.MMX_F16, "bf16": Lm.MMX_BF16}[c["dtype"]]

        def run(a, g):
            da, dg = carve(a[0] if c["shared"] else a, c["dtype"]), carve(g, c["dtype"])
            arena = Arena([B * Nq * Nk])
            rc = L.mmx_avg_heads_ex(ptr(da), ptr(dg), ptr(arena.region(0)), B, H, Nq, Nk, dt, 0 if c["shared"] else -1, stream())
            torch.cuda.synchronize()
            assert rc == 0, c["id"]
            arena.assert_guards_untouched([B * Nq * Nk])
            return arena.region(0).view(B, Nq, Nk)
        outs = [run(a, g), run(a, g)]
        if c["family"] == "nan":                                    # one NaN element in sample 0, every other element as in the clean run
            clean = run(*cb.avg_inputs(c, poisoned=False))
            assert int(torch.isnan(outs[0]).sum()) == 1 and same_bits(outs[0][1:], clean[1:]), ("isolation", c["id"])
        f = cb.ratio(host(outs[0]), want, e)
        print("%s%s %s: %.4g" % (c["id"], " shared" if c["shared"] else "", c["family"], f))
        if not f <= 1.0:
            bad.append((c["id"], f))
        assert same_bits(outs[0], outs[1]), ("second call", c["id"])
        bump(top, c["family"], f)
    record("head mean " + rows[0]["dtype"], top)
    assert not bad, bad
