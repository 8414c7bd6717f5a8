"""-m gpu: the exact-fp32 attention kernels -- the whole-head kernels of ``csrc/attention_head.hip``, the streaming kernels of
``csrc/attention_stream.hip`` (64-row, small-grid and one-sweep forward, query and key side of the backward) and the tiled kernels
of ``csrc/attention_kernels.hip`` -- against the float64 references and the counted per-element bounds of
``tests/attention_f32_bounds.py`` (proved on the CPU by ``tests/test_attention_f32_bounds_host.py``, where an fp32 restatement of
every family is shown inside them and every mutant outside by 2x).

Every element of every output is checked: error <= its bound, NaN exactly where the reference is NaN (a fully masked query row).
The backward is fed the REFERENCE's P and O, so that it is judged on its own; one test per path chains the device forward into the
device backward.  Outputs live in one NaN-filled arena with guard bands (``tests/guard_arena.py``) that must stay NaN (all but
``rel_out``, which ``ops.attn_capture_bwd`` allocates itself); rows of P whose length is no multiple of 4 exercise the unaligned
16-byte store of the whole-head kernels.  The no-slab forward gives the bits of the capture forward wherever the whole-head kernel
serves it; a second call gives the same bits; ``2**s dO`` gives ``2**s`` times dP / dq / dk / dv bit for bit; a NaN row stays in its
row (forward) or its sample (backward).  ``route`` of the table says which kernel family a row must reach -- the options
``attn_head`` / ``attn_stream`` / ``attn_fwd_split`` and the shapes decide -- and the row is judged on THAT family's bounds: the
misaligned view on the tiled kernels', the ``NTK >= 7, Nq > 128`` backward on the streaming kernels'.  The worst error / bound of
every output and kernel family is recorded (``parity.note``) and printed."""
import numpy as np
import pytest
import torch

import attention_f32_bounds as fb
from guard_arena import Arena
from parity import note
from test_gpu_rowwise_forward import dev, host

pytestmark = pytest.mark.gpu

NORMAL = 2.0 ** -100
CHUNK = 24                                   # table rows per test: a few seconds each
DEFAULTS = (("attn_head", 1), ("attn_stream", 1), ("attn_fwd_split", 1))
BOUND = {"dP": "e_dP", "dq": "e_dq", "dk": "e_dk", "dv": "e_dv", "rel_out": "e_rel"}


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    try:
        yield _ops
    finally:
        for key, value in DEFAULTS:
            _ops.set_option(key, value)


def set_route(ops, c):
    for key, field in (("attn_head", "head"), ("attn_stream", "stream"), ("attn_fwd_split", "split")):
        ops.set_option(key, c[field])


def same_bits(a, b):
    """Bit for bit; a NaN matches a NaN whatever its payload."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())


def shifted(a):
    """A copy of ``a`` on the device that starts one float past a 16-byte boundary."""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda")
    view = buf[1:1 + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4
    return view


def qkv_operands(c, x):
    put = shifted if c["misaligned"] else dev
    return put(x["q"]), put(x["k"]), put(x["v"])


def chunks(cases):
    by = {}
    for c in cases:
        by.setdefault(c["kernel"], []).append(c)
    out = []
    for fam, rows in sorted(by.items()):
        for i in range(0, len(rows), CHUNK):
            out.append(pytest.param(rows[i:i + CHUNK], id="%s-%d" % (fam, i // CHUNK)))
    return out


def record(what, top):
    print("\nattention-f32 %s worst error / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(top.items()))))
    for k, v in top.items():
        note("attention_f32 %s %s" % (what, k), v, bound=1.0)


def bump(top, key, value):
    top[key] = max(top.get(key, 0.0), value)


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def run_forward(ops, c, x, q, k, v, noslab=False):
    """One call -> ``(probs or None, out)``, both inside one guarded arena whose margins were checked."""
    set_route(ops, c)
    B, Nq, Nk, Hh, D = c["Bq"], c["Nq"], c["Nk"], c["H"], c["D"]
    sizes = [B * Hh * Nq * Nk, B * Nq * Hh * D]
    arena = Arena(sizes)
    probs, out = arena.region(0).view(B, Hh, Nq, Nk), arena.region(1).view(B, Nq, Hh, D)
    mask = dev(x["mask"])
    if noslab:
        o = ops.attn_fwd(q, k, v, fb.scale_of(c), c["mode"], mask, out=out)
    else:
        o = ops.attn_capture_fwd(q, k, v, probs, fb.scale_of(c), c["mode"], mask, out=out)
    torch.cuda.synchronize()
    assert o is out
    arena.assert_guards_untouched([0 if noslab else sizes[0], sizes[1]])
    return (None if noslab else probs), out


def forward_refs(c, x):
    routes = {c["kernel"], c["kernel_noslab"]}
    return {r: fb.fwd_ref(x["q"], x["k"], x["v"], fb.scale_of(c), c["mode"], x["mask"], r) for r in routes}


@pytest.mark.parametrize("rows", chunks(fb.fwd_cases()))
def test_forward_meets_the_float64_bound(ops, rows):
    """Capture forward: P within ``e_P`` and O within ``e_O`` of the family ``route`` names.  No-slab forward: O within the bound of
    ITS family, and the bits of the capture forward's O where that family is the whole-head one.  Guard bands intact, a second call
    gives the same bits."""
    top, bad = {}, []
    for c in rows:
        x = fb.case_inputs(c)
        refs = forward_refs(c, x)
        q, k, v = qkv_operands(c, x)
        probs, out = run_forward(ops, c, x, q, k, v)
        ref = refs[c["kernel"]]
        gp = host(probs)
        fp, fo = fb.ratio(gp, ref["P"], ref["e_P"]), fb.ratio(host(out), ref["O"], ref["e_O"])
        # recorded beside it: the same figure over the entries well inside the normal range (where a family flushes a result below
        # 2**-126 to zero, the bound's 2**-126 term is what covers it and the figure sits just below 1 whatever the rest does)
        big = ref["P"] >= NORMAL
        fb_ = fb.ratio(gp[big], ref["P"][big], ref["e_P"][big])
        _, out_n = run_forward(ops, c, x, q, k, v, noslab=True)
        ref_n = refs[c["kernel_noslab"]]
        fn = fb.ratio(host(out_n), ref_n["O"], ref_n["e_O"])
        print("%s %s mask %s mode %d: P %.4g (above 2**-100: %.4g) O %.4g  no-slab (%s) O %.4g"
              % (c["id"], c["family"], c["mask"], c["mode"], fp, fb_, fo, c["kernel_noslab"], fn))
        if not (fp <= 1.0 and fo <= 1.0 and fn <= 1.0):
            bad.append((c["id"], fp, fo, fn))                       # (every row's figures are printed before the chunk is judged)
        if c["kernel_noslab"] == "head":
            assert same_bits(out, out_n), ("the no-slab O is not the capture forward's", c["id"])
        probs2, out2 = run_forward(ops, c, x, q, k, v)
        assert same_bits(probs, probs2) and same_bits(out, out2), ("second call", c["id"])
        bump(top, c["kernel"] + " P", fp)
        bump(top, c["kernel"] + " P above 2**-100", fb_)
        bump(top, c["kernel"] + " O", fo)
        bump(top, "no-slab " + c["kernel_noslab"] + " O", fn)
    record("forward " + rows[0]["kernel"], top)
    assert not bad, bad


def one_per_route(cases, key, pred):
    seen, out = set(), []
    for c in cases:
        if pred(c) and key(c) not in seen:
            seen.add(key(c))
            out.append(pytest.param(c, id=c["id"]))
    return out


@pytest.mark.parametrize("c", one_per_route(fb.fwd_cases(), lambda c: (c["kernel"], c["kernel_noslab"]),
                                            lambda c: c["family"] == "randn" and c["Nq"] > 16 and c["mask"] in ("none", "keypad")))
def test_a_nan_query_row_stays_in_its_row(ops, c):
    """A NaN row of q: that row of P and of O is NaN, every other row keeps the bits of the clean run -- capture and no-slab."""
    x = fb.case_inputs(c)
    q, k, v = qkv_operands(c, x)
    probs, out = run_forward(ops, c, x, q, k, v)
    _, out_n = run_forward(ops, c, x, q, k, v, noslab=True)
    row = c["Nq"] // 2
    q[0, row] = float("nan")
    probs_d, out_d = run_forward(ops, c, x, q, k, v)
    _, out_nd = run_forward(ops, c, x, q, k, v, noslab=True)
    keep = torch.ones(c["Nq"], dtype=torch.bool, device="cuda")
    keep[row] = False
    assert bool(torch.isnan(probs_d[0, :, row]).all()) and bool(torch.isnan(out_d[0, row]).all()) and bool(torch.isnan(out_nd[0, row]).all())
    assert same_bits(probs_d[0][:, keep], probs[0][:, keep]) and same_bits(probs_d[1:], probs[1:])
    for dirty, clean in ((out_d, out), (out_nd, out_n)):
        assert same_bits(dirty[0][keep], clean[0][keep]) and same_bits(dirty[1:], clean[1:])


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def run_backward(ops, c, q, k, v, probs, d_o, o, rel):
    """One call in the form of the case -> dict of device tensors (``dP dq dk dv rel_out``, those the case produces); the guard bands
    of the arena they live in were checked."""
    set_route(ops, c)
    B, Nq, Nk, Hh, D = c["B"], c["Nq"], c["Nk"], c["H"], c["D"]
    sizes = ([B * Hh * Nq * Nk] if c["dprobs"] else []) + ([B * Nq * Hh * D, B * Nk * Hh * D, B * Nk * Hh * D] if c["need"] else [])
    arena = Arena(sizes) if sizes else None
    res, at = {}, 0
    dprobs = out = None
    if c["dprobs"]:
        dprobs = res["dP"] = arena.region(0).view(B, Hh, Nq, Nk)
        at = 1
    if c["need"]:
        out = tuple(arena.region(at + j).view(B, n, Hh, D) for j, n in enumerate((Nq, Nk, Nk)))
        res["dq"], res["dk"], res["dv"] = out
    got = ops.attn_capture_bwd(q, k, v, probs, d_o, dprobs, fb.scale_of(c), c["mode"], need_dqkv=c["need"], out=out,
                               batch=B if c["shared"] else None, o=o, rel_row=rel, images=c["images"] or None)
    torch.cuda.synchronize()
    if rel is not None:
        res["rel_out"] = got[3]
    if arena is not None:
        arena.assert_guards_untouched(sizes)
    return res


def check_backward(c, res, ref, top, bad):
    figs = {n: fb.ratio(host(t), ref[n], ref[BOUND[n]]) for n, t in res.items()}
    print("%s %s mode %d%s%s%s: %s" % (c["id"], c["family"], c["mode"], " shared" if c["shared"] else "", " grouped" if c["images"] else "",
                                       " o" if c["o"] else "", "  ".join("%s %.4g" % kv for kv in figs.items())))
    form = "grouped " if c["images"] else ("row " if c["rel"] else "")
    for n, f in figs.items():
        if not f <= 1.0:
            bad.append((c["id"], n, f))
        assert not bool(torch.isnan(res[n]).any()), (c["id"], n)    # no in-range element stays NaN
        bump(top, "%s%s %s" % (form, c["kernel"], n), f)


def reference_backward(c, x, P, o):
    return fb.bwd_ref(x["q"], x["k"], x["v"], P, x["dO"], o, fb.scale_of(c), c["mode"], c["kernel"], x["rel"] if c["rel"] else None,
                      c["need"])


def shifts_of(c):
    """``2**s dO`` stays inside the normal range at every intermediate: not downwards for the ``small`` operands (already x 2**-20)
    and the ``peaked`` slabs (P down to 2**-126)."""
    return (20,) if c["family"] in ("small", "peaked") else (-20, 20)


@pytest.mark.parametrize("rows", chunks(fb.bwd_cases()))
def test_backward_meets_the_float64_bound(ops, rows):
    """Every table row of one kernel family, fed the reference's P and O: every output within its bound; the guard bands NaN; the same
    bits on a second call; ``2**s dO`` -> ``2**s`` times dP / dq / dk / dv bit for bit; a NaN row in the first dO leaves every output of
    the other samples (targets) with the bits of the clean run."""
    top, bad = {}, []
    for c in rows:
        x = fb.case_inputs(c)
        P, o = fb.reference_forward_for(c, x)
        ref = reference_backward(c, x, P, o)
        q, k, v = qkv_operands(c, x)
        probs, d_o, od, rel = dev(P), dev(x["dO"]), dev(o), (dev(x["rel"]) if c["rel"] else None)
        res = run_backward(ops, c, q, k, v, probs, d_o, od, rel)
        check_backward(c, res, ref, top, bad)
        again = run_backward(ops, c, q, k, v, probs, d_o, od, rel)
        assert all(same_bits(res[n], again[n]) for n in res), ("second call", c["id"])
        for s in shifts_of(c):
            moved = run_backward(ops, c, q, k, v, probs, d_o * 2.0 ** s, od, rel)
            for n in ("dP", "dq", "dk", "dv"):
                if n in res:
                    assert same_bits(moved[n], res[n] * 2.0 ** s), ("scaling by 2**%d" % s, c["id"], n)
        poisoned = d_o.clone()
        poisoned[0, c["Nq"] // 2] = float("nan")
        dirty = run_backward(ops, c, q, k, v, probs, poisoned, od, rel)
        for n in res:
            assert same_bits(dirty[n][1:], res[n][1:]), ("isolation", c["id"], n)
            assert bool(torch.isnan(dirty[n][0]).any()), ("the NaN row reached no output of its own sample", c["id"], n)
    record("backward " + rows[0]["kernel"], top)
    assert not bad, bad


@pytest.mark.parametrize("c", one_per_route(fb.bwd_cases(), lambda c: (c["kernel"], c["o"] and c["kernel"] == "stream"),
                                            lambda c: c["family"] == "randn" and c["need"] and c["dprobs"] and c["Nq"] > 16 and not c["images"]))
def test_what_a_nan_row_of_dO_does_to_its_own_sample(ops, c):
    """As the kernels do it today, pinned: with a NaN row r in sample 0's dO (P > 0 everywhere), row r of dP and of dq is NaN and
    every other row of them keeps its bits; dk and dv of that sample -- sums over ALL query rows -- are NaN in every element."""
    x = fb.case_inputs(c)
    P, o = fb.reference_forward_for(c, x)
    assert (P > 0).all()
    q, k, v = qkv_operands(c, x)
    probs, d_o, od, rel = dev(P), dev(x["dO"]), dev(o), (dev(x["rel"]) if c["rel"] else None)
    res = run_backward(ops, c, q, k, v, probs, d_o, od, rel)
    row = c["Nq"] // 2
    d_o[0, row] = float("nan")
    dirty = run_backward(ops, c, q, k, v, probs, d_o, od, rel)
    keep = torch.ones(c["Nq"], dtype=torch.bool, device="cuda")
    keep[row] = False
    assert bool(torch.isnan(dirty["dP"][0, :, row]).all()) and bool(torch.isnan(dirty["dq"][0, row]).all())
    assert same_bits(dirty["dP"][0][:, keep], res["dP"][0][:, keep]) and same_bits(dirty["dq"][0][keep], res["dq"][0][keep])
    assert bool(torch.isnan(dirty["dk"][0]).all()) and bool(torch.isnan(dirty["dv"][0]).all())
    for n in ("dP", "dq", "dk", "dv"):
        assert same_bits(dirty[n][1:], res[n][1:]), n


def chain_rows():
    """One row per path that computes dq / dk / dv: (kernel family, row mode, grouped, delta from O)."""
    return one_per_route(fb.bwd_cases(), lambda c: (c["kernel"], c["rel"], c["images"], c["o"] and c["kernel"] == "stream", c["misaligned"]),
                         lambda c: c["need"] and c["Nk"] > 16 and c["family"] in ("randn", "poscode"))


@pytest.mark.parametrize("c", chain_rows())
def test_device_forward_chained_into_device_backward(ops, c):
    """The device's own P slab and O go into the device backward; the reference backward is the function of THOSE inputs (the forward
    is judged by its own test), so the bound is the same."""
    x = fb.case_inputs(c)
    q, k, v = qkv_operands(c, x)
    probs, out = run_forward(ops, dict(c, B=c["Bq"]), x, q, k, v)
    o = out if c["o"] else None
    ref = reference_backward(c, x, host(probs), host(out) if c["o"] else None)
    res = run_backward(ops, c, q, k, v, probs, dev(x["dO"]), o, dev(x["rel"]) if c["rel"] else None)
    top, bad = {}, []
    check_backward(c, res, ref, top, bad)
    record("chained " + c["id"], top)
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# refusals: argument checks that return before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ops):
    """``rel_row`` on a cross shape, no dP slab outside the row mode, the row mode at a head_dim that is no multiple of 4: ``MMXError``,
    and every output buffer keeps its NaN fill."""
    from transformer_mm_explainability_amd import _lib
    for key, value in DEFAULTS:
        ops.set_option(key, value)
    B, Hh, N = 2, 3, 40
    g = torch.Generator().manual_seed(7)

    def operands(D, Nk=N):
        q = torch.randn(B, N, Hh, D, generator=g).cuda()
        k, v = (torch.randn(B, Nk, Hh, D, generator=g).cuda() for _ in range(2))
        return q, k, v, torch.randn(B, N, Hh, D, generator=g).cuda()

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) for t in ts)

    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
    q, k, v, d_o = operands(8, Nk=50)
    slab, grads = torch.rand(B, Hh, N, 50, device="cuda"), (nan(B, N, Hh, 8), nan(B, 50, Hh, 8), nan(B, 50, Hh, 8))
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_bwd(q, k, v, slab, d_o, None, 8 ** -0.5, out=grads, rel_row=torch.rand(B, N, device="cuda"))
    assert untouched(*grads)
    q, k, v, d_o = operands(8)
    slab, grads = torch.rand(B, Hh, N, N, device="cuda"), tuple(nan(B, N, Hh, 8) for _ in range(3))
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_bwd(q, k, v, slab, d_o, None, 8 ** -0.5, out=grads)
    assert untouched(*grads)
    q, k, v, d_o = operands(6)
    dprobs, grads = nan(B, Hh, N, N), tuple(nan(B, N, Hh, 6) for _ in range(3))
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_bwd(q, k, v, slab, d_o, dprobs, 6 ** -0.5, out=grads, rel_row=torch.rand(B, N, device="cuda"))
    assert untouched(dprobs, *grads)
