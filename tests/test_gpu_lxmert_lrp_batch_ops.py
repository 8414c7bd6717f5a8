"""-m gpu: ``mmx_lxmert_attr`` and ``mmx_head_minmax_live`` at op level, over the case table of ``tests/lxmert_lrp_batch_cases.py``
(signed ``randn * 1e-2`` cams, ``randn`` gradients, 1e3 in BOTH slabs outside the live blocks), against the float64 restatements of
that file, PER ELEMENT with ``u = 2^-24`` (``tests/test_lxmert_lrp_batch_host.py`` proves the bounds: an fp32 emulation stays inside
them in three summation orders, eight mutants are at least twice a bound away):

    R_tt   expm1(n_text (t + H + 3) u) ref        R_ii   expm1(n_img (I + H + 3) u) ref        R_ti   expm1((H + 3) u) ref
    min-max   2 e (1 + |out|) / (max - min) + 3 u |out|,   e = (H + 1) u max_block(mean_h |cam|)

Every operand of the chain is non-negative, so the chain bounds are relative, and a zero of the restatement -- ``R_tt[b, 0, 0]``,
everything outside the live blocks -- has to be an exact zero.  Further: the NaN mask equals the restatement's on the degenerate rows
(a constant block, a one-entry block, a NaN in a live block); the same bits when the garbage outside the live blocks is NaN instead
of 1e3, on a second call, through ``ops``, and for sample b alone at B = 1; guard bands around the outputs and the workspace stay
untouched; the golden trios of ``lxmert_chain_lrp.npz``, embedded in a padded B = 3 batch, reproduce the reference's ``tattr_*`` /
``plrp_*`` at ``atol = 1e-5`` (the bar of ``tests/test_gpu_lrp_route.py``).  ``check_attr`` / ``check_minmax`` return the worst
error / bound per output; ``tools/probe_lxmert_lrp_batch.py`` writes them to ``profiles/lxmert_lrp_batch_probe.txt``."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lxmert_lrp_batch_cases as cases  # noqa: E402
import parity  # noqa: E402
from test_gpu_lxmert_baselines_ops import Arena, _dev, _ptr  # noqa: E402
from test_lxmert_lrp_batch_host import golden_tables  # noqa: E402

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_attr(text, img, cross, t_len):
    """The C entry on its own output regions and workspace between guard bands -> ``(R_tt, R_ti, R_ii)`` (copies)."""
    from transformer_mm_explainability_amd import _lib
    B, H, T, I = cross[0].shape
    need = _lib.lib().mmx_lxmert_attr_workspace_bytes(len(text), len(img), B, T, I)
    assert need > 0 and need % 4 == 0
    sizes = [B * T * T, B * T * I, B * I * I, need // 4]
    arena = Arena(sizes)
    tables = [_lib.ptr_table([p[w].data_ptr() for p in pairs]) for pairs in (text, img) for w in (0, 1)]
    rc = _lib.lib().mmx_lxmert_attr(tables[0][0], tables[1][0], len(text), tables[2][0], tables[3][0], len(img), _ptr(cross[0]),
                                    _ptr(cross[1]), B, H, T, I, _ptr(t_len), _ptr(arena.region(0)), _ptr(arena.region(1)),
                                    _ptr(arena.region(2)), _ptr(arena.region(3)), need, _stream())
    _lib.check(rc, "mmx_lxmert_attr")
    torch.cuda.synchronize()
    # the workspace holds n_text + n_img blocks per sample, each written up to its own extent: only its guard bands are checked
    arena.assert_guards_untouched(sizes)
    return arena.region(0).reshape(B, T, T).clone(), arena.region(1).reshape(B, T, I).clone(), arena.region(2).reshape(B, I, I).clone()


def run_minmax(cam, q_len, k_len, zero_cls):
    from transformer_mm_explainability_amd import _lib
    B, H, Nq, Nk = cam.shape
    arena = Arena([B * Nq * Nk])
    rc = _lib.lib().mmx_head_minmax_live(_ptr(cam), _ptr(arena.region(0)), B, H, Nq, Nk, _ptr(q_len), _ptr(k_len),
                                         _lib.HEAD_MEAN_ZERO_CLS if zero_cls else 0, _stream())
    _lib.check(rc, "mmx_head_minmax_live")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([B * Nq * Nk])
    return arena.region(0).reshape(B, Nq, Nk).clone()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _worst(label, got, want, bound, live=None):
    """Assert ``|got - want| <= bound`` per element (where ``live``), return the worst error / bound of the elements with a bound."""
    err = np.abs(got.double().cpu().numpy() - want)
    if live is None:
        live = np.ones(want.shape, dtype=bool)
    bad = live & ~(err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(live & (bound > 0), err / bound, 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    parity.note(label + " worst error / bound", worst, 1.0)
    print("%s: worst error / bound %.3f" % (label, worst))
    assert not bad.any(), "%s: %d elements outside their bound, worst error / bound %.3g" % (label, int(bad.sum()), worst)
    return worst


def _device_case(c):
    pairs = lambda ps: [(_dev(a), _dev(g)) for a, g in ps]  # noqa: E731
    return pairs(c["text"]), pairs(c["img"]), pairs([c["cross"]])[0], _dev(c["raw"])


def check_attr(case):
    """Everything the module docstring lists for ``mmx_lxmert_attr`` on one case -> ``{output: worst error / bound}``."""
    from transformer_mm_explainability_amd import ops
    T, I, H, B, kind, n_text, n_img = case
    c = cases.make_case(*case, cases.SEEDS[case])
    text, img, cross, raw = _device_case(c)
    got = run_attr(text, img, cross, raw)
    ref = cases.attr64(c["text"], c["img"], c["cross"], c["t"])
    worst = {}
    for name, g, w, bound in zip(("R_tt", "R_ti", "R_ii"), got, ref, cases.attr_bounds(c, ref)):
        worst[name] = _worst("attr " + name, g, w, bound)
        assert not bool(g[torch.from_numpy(w == 0).cuda()].any()), name + ": not an exact zero where the restatement is zero"
    assert not bool(got[0][:, 0, 0].any())
    nan_text, nan_img, nan_cross, _ = _device_case(cases.make_case(*case, cases.SEEDS[case], pad=np.nan))
    for name, a, b in zip(("R_tt", "R_ti", "R_ii"), got, run_attr(nan_text, nan_img, nan_cross, raw)):
        assert _same_bits(a, b), name + ": NaN outside the live blocks changes the result"
    for name, a, b in zip(("R_tt", "R_ti", "R_ii"), got, run_attr(text, img, cross, raw)):
        assert _same_bits(a, b), name + ": two calls differ"
    for name, a, b in zip(("R_tt", "R_ti", "R_ii"), got, ops.lxmert_transformer_attr(text, img, cross, text_len=raw)):
        assert _same_bits(a, b), name + ": ops differs from the C entry"
    if kind == "oob":                                    # an out-of-range length IS its clamped value
        for name, a, b in zip(("R_tt", "R_ti", "R_ii"), got, run_attr(text, img, cross, _dev(c["t"]))):
            assert _same_bits(a, b), name + ": an out-of-range length is not its clamped value"
    if B > 1:
        one = lambda ps, b: [(a[b:b + 1].contiguous(), g[b:b + 1].contiguous()) for a, g in ps]  # noqa: E731
        for b in range(B):
            alone = run_attr(one(text, b), one(img, b), one([cross], b)[0], None if raw is None else raw[b:b + 1].contiguous())
            for name, g, a in zip(("R_tt", "R_ti", "R_ii"), got, alone):
                assert _same_bits(g[b:b + 1], a), "%s: sample %d of the batch differs from the sample alone" % (name, b)
    return worst


def check_minmax(case):
    """The same for ``mmx_head_minmax_live`` on the three maps of the case -> ``{map: worst error / bound}``."""
    from transformer_mm_explainability_amd import ops
    T, I, H, B, kind, n_text, n_img = case
    c = cases.make_case(*case, cases.SEEDS[case])
    nan = cases.make_case(*case, cases.SEEDS[case], pad=np.nan)
    worst = {}
    for (name, cam_np, rq, q, rk, k, cls), (_n, nan_np, *_rest) in zip(cases.minmax_maps(c), cases.minmax_maps(nan)):
        cam, ql, kl = _dev(cam_np), _dev(rq), _dev(rk)
        got = run_minmax(cam, ql, kl, cls)
        want = cases.minmax64(cam_np, q, k, cls)
        assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want)), name + ": NaN mask"      # (one-entry blocks are NaN)
        ok = ~np.isnan(want)
        worst[name] = _worst("minmax " + name, got, want, cases.minmax_bound(cam_np, q, k, want), live=ok)
        for b in range(B):
            assert not bool(got[b, int(q[b]):].any()) and not bool(got[b, :, int(k[b]):].any()), name + ": not zero outside the live block"
        if cls:
            assert not bool(got[:, 0, 0].any())
        assert _same_bits(got, run_minmax(_dev(nan_np), ql, kl, cls)), name + ": NaN outside the live blocks changes the result"
        assert _same_bits(got, run_minmax(cam, ql, kl, cls)), name + ": two calls differ"
        assert _same_bits(got, ops.head_minmax_live(cam, ql, kl, cls)), name + ": ops differs from the C entry"
        if kind == "oob":
            assert _same_bits(got, run_minmax(cam, _dev(q), None if rk is None else _dev(k), cls)), name
        if B > 1:
            for b in range(B):
                alone = run_minmax(cam[b:b + 1].contiguous(), None if ql is None else ql[b:b + 1].contiguous(),
                                   None if kl is None else kl[b:b + 1].contiguous(), cls)
                assert _same_bits(got[b:b + 1], alone), "%s: sample %d of the batch differs from the sample alone" % (name, b)
    return worst


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_transformer_attr_on_the_live_blocks(case):
    check_attr(case)


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_head_minmax_on_the_live_blocks(case):
    check_minmax(case)


@pytest.mark.parametrize("zero_cls", [False, True])
def test_minmax_degenerate_rows_have_the_restatements_nan_mask(zero_cls):
    for name, cam_np, q_len, k_len in cases.degenerate_minmax():
        cam, ql, kl = _dev(cam_np), _dev(q_len), _dev(k_len)
        got = run_minmax(cam, ql, kl, zero_cls)
        want = cases.minmax64(cam_np, q_len, k_len, zero_cls)
        assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(want)), name
        # the row is degenerate (before the [CLS] write, which IS the one-entry block's only entry) and stays inside its sample
        assert np.isnan(cases.minmax64(cam_np, q_len, k_len)[1]).any() and not np.isnan(want[0]).any()
        bound = cases.minmax_bound(cam_np, q_len, k_len, want)
        ok = ~np.isnan(want) & ~np.isnan(bound)          # (the [CLS] zero of a NaN block has no bound: it is an exact zero, below)
        _worst("minmax degenerate " + name, got, want, bound, live=ok)
        if zero_cls:
            assert not bool(got[:, 0, 0].any())
        assert _same_bits(got, run_minmax(cam, ql, kl, zero_cls)), name + ": two calls differ"
        assert _same_bits(got[1:2], run_minmax(cam[1:2].contiguous(), ql[1:2].contiguous(), kl[1:2].contiguous(), zero_cls)), name


def test_attr_keeps_a_nan_of_a_live_entry():
    """The clamp propagates a NaN as ``torch.clamp`` does: a NaN cam entry inside a live block reaches the outputs."""
    case = (12, 20, 3, 1, "ragged", 1, 1)
    c = cases.make_case(*case, 0)
    c["cross"][0][0, 1, 2, 3] = np.nan
    c["text"][0][0][0, 0, 1, 4] = np.nan
    text, img, cross, raw = _device_case(c)
    got = run_attr(text, img, cross, raw)
    with np.errstate(invalid="ignore"):
        ref = cases.attr64(c["text"], c["img"], c["cross"], c["t"])
    for g, w in zip(got, ref):
        assert np.array_equal(np.isnan(g.cpu().numpy()), np.isnan(w))
    assert np.isnan(ref[1][0, 2, 3]) and np.isnan(ref[0][0, 1, 4])


def test_golden_trios_in_a_padded_batch_reproduce_the_reference(golden):
    """The trios of ``lxmert_chain_lrp.npz`` as sample 1 of a padded B = 3 batch (T 8 -> 11, I = 11): ``tattr_*`` / ``plrp_*``."""
    g = golden("lxmert_chain_lrp")
    text, img, cross = golden_tables(g)
    T0, I = cross[0].shape[-2:]
    T, B, at = T0 + 3, 3, 1
    rng = np.random.default_rng(3)
    t_len = np.array([T, T0, 2], dtype=np.int32)

    def embed(slab, q, k):
        out = (rng.standard_normal((B, slab.shape[1], T if q else I, T if k else I)) * 1e-2).astype(np.float32)
        out[at] = cases.PAD
        out[at, :, :slab.shape[2], :slab.shape[3]] = slab[0]
        return _dev(out)

    e_text = [(embed(c, 1, 1), embed(gr, 1, 1)) for c, gr in text]
    e_img = [(embed(c, 0, 0), embed(gr, 0, 0)) for c, gr in img]
    e_cross = (embed(cross[0], 1, 0), embed(cross[1], 1, 0))
    R_tt, R_ti, _ = run_attr(e_text, e_img, e_cross, _dev(t_len))
    parity.close(R_tt[at, :T0, :T0], g["tattr_R_t_t"], atol=1e-5)
    parity.close(R_ti[at, :T0], g["tattr_R_t_i"], atol=1e-5)
    assert not bool(R_tt[at, T0:].any()) and not bool(R_tt[at, :, T0:].any()) and not bool(R_ti[at, T0:].any())
    ql = _dev(t_len)
    p_tt = run_minmax(e_text[-1][0], ql, ql, True)
    p_ti = run_minmax(e_cross[0], ql, None, False)
    parity.close(p_tt[at, :T0, :T0], g["plrp_R_t_t"], atol=1e-5)
    parity.close(p_ti[at, :T0], g["plrp_R_t_i"], atol=1e-5)
