"""-m gpu: the bf16 matrix-core attention (``mma_bf16=True``) -- ``attn_fwd_stream_kernel<MM>``, the first-generation backward of
``csrc/attention_stream.hip``, the second generation of ``csrc/attention_bf16.hip``, the third-generation query side with the third- and
fourth-generation key sides of ``csrc/attention_bf16_v3.hip`` and their bf16 gradient I/O -- against the float64 references and the
counted per-element bounds of ``tests/attention_bf16_bounds.py`` (proved on the CPU by ``tests/test_attention_bf16_bounds_host.py``,
where an fp32 restatement is shown inside them and every mutant outside by 2x).

The operands are plain fp32 ``randn`` (and the other families of the table), NOT pre-rounded: the kernels' own rounding is under test.
The backward is fed the REFERENCE's P (rounded to the slab type) and O, so that it is judged on its own; one test per path chains the
device forward into the device backward.  Every element of every output is checked: within its bound (16-bit outputs: inside the
interval of their stored type), NaN where the reference is NaN; outputs live inside NaN-filled guard buffers whose margins must stay
NaN (all but ``rel_out``, which ``ops.attn_capture_bwd`` allocates itself); ``2**s dO`` gives ``2**s`` times dP / dq / dk / dv bit for bit; a NaN row in sample 0's dO leaves the other samples' bits alone;
a second call gives the same bits.  The worst error / bound of every output and kernel family is recorded (``parity.note``) and printed."""
import numpy as np
import pytest
import torch

import attention_bf16_bounds as ab
from parity import note
from test_gpu_rowwise_forward import dev, host

pytestmark = pytest.mark.gpu

GUARD = 64                                   # elements of NaN in front of and behind every output (256 / 128 bytes: keeps 16-byte alignment)
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
CHUNK = 26                                   # table rows per test: a few seconds each
SHIFTS = (-20, 20)


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    yield _ops
    _ops.set_option("attn_bf16_v2", 1)       # the defaults
    _ops.set_option("attn_bf16_v3", 3)


def same_bits(a, b):
    """Bit for bit (fp32 / fp16 / bf16); a NaN matches a NaN whatever its payload."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    as_int = torch.int32 if a.dtype == torch.float32 else torch.int16
    a, b = a.contiguous().reshape(-1), b.contiguous().reshape(-1)
    return bool(((a.view(as_int) == b.view(as_int)) | (torch.isnan(a) & torch.isnan(b))).all())


def guarded(shape, dtype):
    """``(buffer, view)``: a NaN-filled flat buffer with ``GUARD`` elements of margin around a contiguous view of ``shape``."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda", dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def margins_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def qkv_operands(c, x):
    """q, k, v on the device: contiguous, or (``packed``, self-attention) views of ONE ``[B, N, 3, H, D]`` tensor as
    ``clip_model.backward_tape`` hands them in -- both satisfy the 16-byte alignment tests of the ``*_try`` functions."""
    if c["packed"] and c["Nq"] == c["Nk"]:
        qkv = dev(np.stack([x["q"], x["k"], x["v"]], 2))
        return qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    return dev(x["q"]), dev(x["k"]), dev(x["v"])


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
    print("\nattention-bf16 %s worst figure (fp32: error / bound; 16-bit: elements outside their interval): %s"
          % (what, "  ".join("%s %.3f" % kv for kv in sorted(top.items()))))
    for k, v in top.items():
        note("attention_bf16 %s %s" % (what, k), v, bound=1.0)


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def run_forward(ops, c, x, q, k, v):
    B, Nq, Nk = c["Bq"], c["Nq"], c["Nk"]
    pbuf, probs = guarded((B, c["H"], Nq, Nk), TORCH[c["slab"]])
    obuf, out = guarded((B, Nq, c["H"], c["D"]), torch.float32)
    o = ops.attn_capture_fwd(q, k, v, probs, ab.scale_of(c), c["mode"], dev(x["mask"]), mma_bf16=True, out=out)
    torch.cuda.synchronize()
    assert o is out
    return pbuf, probs, obuf, out


@pytest.mark.parametrize("rows", chunks(ab.fwd_cases()))
def test_forward_meets_the_float64_bound(ops, rows):
    """``attn_fwd_stream_kernel<32 | 64, slab, MM>``: P in the slab within ``e_P`` (a 16-bit slab: inside its interval), O within
    ``e_O`` (the near-tie allowance on the fp32 P it rounds), NaN exactly where ``torch.softmax`` gives NaN (a fully masked row)."""
    top = {}
    for c in rows:
        x = ab.case_inputs(c)
        ref = ab.fwd_ref(x["q"], x["k"], x["v"], ab.scale_of(c), c["mode"], x["mask"], c["slab"])
        q, k, v = qkv_operands(c, x)
        pbuf, probs, obuf, out = run_forward(ops, c, x, q, k, v)
        gp, go = host(probs), host(out)
        fp, fo = ab.judge(gp, ref["P"], ref["e_P"], c["slab"]), ab.ratio(go, ref["O"], ref["e_O"])
        print("%s %s mask %s slab %s mode %d: P %.4g O %.4g (near-tie share %.4f)" % (c["id"], c["family"], c["mask"], c["slab"], c["mode"],
                                                                                     fp, fo, ref["flagged"]))
        assert ab.passes(fp, c["slab"]) and ab.passes(fo), (c["id"], fp, fo)
        assert np.array_equal(np.isnan(gp), np.isnan(ref["P"])) and np.array_equal(np.isnan(go), np.isnan(ref["O"])), c["id"]
        assert margins_intact(pbuf) and margins_intact(obuf), c["id"]
        again = run_forward(ops, c, x, q, k, v)
        assert same_bits(probs, again[1]) and same_bits(out, again[3]), c["id"]
        top["P " + c["slab"]] = max(top.get("P " + c["slab"], 0.0), fp)
        top["O"] = max(top.get("O", 0.0), fo)
    record("forward " + rows[0]["kernel"], top)


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def run_backward(ops, c, q, k, v, probs, d_o, o, rel):
    """One call in the form of the case -> dict of device tensors (``dP dq dk dv rel_out``, those the case produces) and the guard
    buffers."""
    ops.set_option("attn_bf16_v2", c["v2"])
    ops.set_option("attn_bf16_v3", c["v3"])
    B, Nq, Nk, H, D = c["B"], c["Nq"], c["Nk"], c["H"], c["D"]
    bufs, res = [], {}
    dprobs = None
    if c["dprobs"]:
        b, dprobs = guarded((B, H, Nq, Nk), TORCH[c["slab"]])
        bufs.append(b)
    out = None
    if c["need"]:
        if Nq == Nk:                                                # views of one packed gradient tensor, as the tape hands them in
            b, packed = guarded((B, Nq, 3, H, D), d_o.dtype)
            bufs.append(b)
            out = (packed[:, :, 0], packed[:, :, 1], packed[:, :, 2])
        else:
            out = []
            for n in (Nq, Nk, Nk):
                b, t = guarded((B, n, H, D), d_o.dtype)
                bufs.append(b)
                out.append(t)
            out = tuple(out)
    got = ops.attn_capture_bwd(q, k, v, probs, d_o, dprobs, ab.scale_of(c), c["mode"], need_dqkv=c["need"], out=out,
                               batch=B if c["shared"] else None, o=o, mma_bf16=True, rel_row=rel)
    torch.cuda.synchronize()
    if dprobs is not None:
        res["dP"] = dprobs
    if c["need"]:
        res["dq"], res["dk"], res["dv"] = out
    if rel is not None:
        res["rel_out"] = got[3]
    return res, bufs


def kinds_of(c):
    io = "bf16" if c["io_bf16"] else "f32"
    return {"dP": c["slab"], "dq": io, "dk": io, "dv": io, "rel_out": "f32"}


BOUND = {"dP": "e_dP", "dq": "e_dq", "dk": "e_dk", "dv": "e_dv", "rel_out": "e_rel"}


def check_backward(c, res, bufs, ref, top):
    kinds = kinds_of(c)
    figs = {n: ab.judge(host(t), ref[n], ref[BOUND[n]], kinds[n]) for n, t in res.items()}
    print("%s %s slab %s mode %d%s%s: %s (near-tie share of dS %.4f)"
          % (c["id"], c["family"], c["slab"], c["mode"], " shared" if c["shared"] else "", " bf16 dO" if c["io_bf16"] else "",
             "  ".join("%s %.4g" % kv for kv in figs.items()), ref["flagged_dS"]))
    for n, f in figs.items():
        assert ab.passes(f, kinds[n]), (c["id"], n, f, figs)
        assert not bool(torch.isnan(res[n].float()).any()), (c["id"], n)        # no in-range element stays NaN
        key = "%s %s" % (n, kinds[n])
        top[key] = max(top.get(key, 0.0), f)
    assert all(margins_intact(b) for b in bufs), c["id"]


def device_operands(c, x, P, o):
    q, k, v = qkv_operands(c, x)
    probs = dev(P).to(TORCH[c["slab"]])                             # exact: P holds numbers of the slab type
    d_o = dev(x["dO"]).to(torch.bfloat16) if c["io_bf16"] else dev(x["dO"])
    return q, k, v, probs, d_o, dev(o), (dev(x["rel"]) if c["rel"] else None)


def scaled(t, s):
    """``2**s t``, exactly (``torch.ldexp`` on the device goes through an inexact ``exp2``: 2**20 comes out as 1048575.9375)."""
    return (t.float() * (2.0 ** s)).to(t.dtype)


@pytest.mark.parametrize("rows", chunks(ab.bwd_cases()))
def test_backward_meets_the_float64_bound(ops, rows):
    """Every table row of one kernel family, fed the reference's P and O: every output within its bound; the margins NaN; the same bits
    on a second call; ``2**s dO`` -> ``2**s`` times dP / dq / dk / dv bit for bit (s = -20, +20; not the dP of an fp16 slab); a NaN
    row in sample 0's dO leaves every output of the other samples with the bits of the clean run."""
    top = {}
    for c in rows:
        x = ab.case_inputs(c)
        P, o = ab.reference_forward_for(c, x)
        ref = ab.bwd_ref(x["q"], x["k"], x["v"], P, x["dO"], o, ab.scale_of(c), c["mode"], x["rel"] if c["rel"] else None)
        q, k, v, probs, d_o, od, rel = device_operands(c, x, P, o)
        res, bufs = run_backward(ops, c, q, k, v, probs, d_o, od, rel)
        check_backward(c, res, bufs, ref, top)
        again, _ = run_backward(ops, c, q, k, v, probs, d_o, od, rel)
        assert all(same_bits(res[n], again[n]) for n in res), ("second call", c["id"])
        for s in SHIFTS:
            moved, _ = run_backward(ops, c, q, k, v, probs, scaled(d_o, s), od, rel)
            for n in ("dP", "dq", "dk", "dv"):
                if n in res and not (n == "dP" and c["slab"] == "f16"):
                    assert same_bits(moved[n], scaled(res[n], s)), ("scaling by 2**%d" % s, c["id"], n)
        poisoned = d_o.clone()
        poisoned[0, c["Nq"] // 2] = float("nan")
        dirty, _ = run_backward(ops, c, q, k, v, probs, poisoned, od, rel)
        for n in res:
            assert same_bits(dirty[n][1:], res[n][1:]), ("isolation", c["id"], n)
            assert bool(torch.isnan(dirty[n][0].float()).any()), ("the NaN row reached no output of its own sample", c["id"], n)
    record("backward " + rows[0]["kernel"], top)


def chain_rows():
    """One row per path: the first of every (kernel family, dO type, row mode) that computes dq / dk / dv."""
    seen, out = set(), []
    for c in ab.bwd_cases():
        key = (c["kernel"], c["io_bf16"], c["rel"], c["o"])
        if c["need"] and c["Nk"] > 64 and key not in seen:
            seen.add(key)
            out.append(pytest.param(c, id=c["id"]))
    return out


@pytest.mark.parametrize("c", chain_rows())
def test_device_forward_chained_into_device_backward(ops, c):
    """The device's own P slab and O go into the device backward; the reference backward is the function of THOSE inputs (the forward
    is judged by its own test), so the bound is the same."""
    x = ab.case_inputs(c)
    q, k, v = qkv_operands(c, x)
    fc = dict(c, Bq=c["Bq"], mask="none")
    x["mask"] = None
    _, probs, _, out = run_forward(ops, fc, x, q, k, v)
    o = out if c["o"] else None
    P, o_np = host(probs), (host(out) if c["o"] else None)
    rel = x["rel"] if c["rel"] else None
    ref = ab.bwd_ref(x["q"], x["k"], x["v"], P, x["dO"], o_np, ab.scale_of(c), c["mode"], rel)
    d_o = dev(x["dO"]).to(torch.bfloat16) if c["io_bf16"] else dev(x["dO"])
    res, bufs = run_backward(ops, c, q, k, v, probs, d_o, o, dev(rel))
    top = {}
    check_backward(c, res, bufs, ref, top)
    record("chained " + c["id"], top)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ops):
    """D % 4 != 0, a dP slab of another type than P's, ``rel_row`` on a cross shape: ``MMXError``, and every output buffer keeps its
    NaN fill."""
    from transformer_mm_explainability_amd import _lib
    B, H, N = 2, 3, 70
    g = torch.Generator().manual_seed(6)

    def operands(D, Nk=N):
        q = torch.randn(B, N, H, D, generator=g).cuda()
        k, v = (torch.randn(B, Nk, H, D, generator=g).cuda() for _ in range(2))
        return q, k, v, torch.randn(B, N, H, D, generator=g).cuda()

    def untouched(*ts):
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t.float()).all()) for t in ts)

    nan = lambda *shape, dtype=torch.float32: torch.full(shape, float("nan"), device="cuda", dtype=dtype)
    # head dim 6
    q, k, v, d_o = operands(6)
    probs, out = nan(B, H, N, N), nan(B, N, H, 6)
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_fwd(q, k, v, probs, 6 ** -0.5, mma_bf16=True, out=out)
    assert untouched(probs, out)
    slab = torch.rand(B, H, N, N, device="cuda")
    dprobs, grads = nan(B, H, N, N), tuple(nan(B, N, H, 6) for _ in range(3))
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_bwd(q, k, v, slab, d_o, dprobs, 6 ** -0.5, out=grads, mma_bf16=True)
    assert untouched(dprobs, *grads)
    # a dP slab whose type is not P's
    q, k, v, d_o = operands(8)
    dprobs, grads = nan(B, H, N, N, dtype=torch.bfloat16), tuple(nan(B, N, H, 8) for _ in range(3))
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_bwd(q, k, v, slab, d_o, dprobs, 8 ** -0.5, out=grads, mma_bf16=True)
    assert untouched(dprobs, *grads)
    # the row mode on a cross shape
    q, k, v, d_o = operands(8, Nk=130)
    slab = torch.rand(B, H, N, 130, device="cuda")
    grads = (nan(B, N, H, 8), nan(B, 130, H, 8), nan(B, 130, H, 8))
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_bwd(q, k, v, slab, d_o, None, 8 ** -0.5, out=grads, mma_bf16=True, rel_row=torch.rand(B, N, device="cuda"))
    assert untouched(*grads)
