"""-m gpu: ``mmx_head_mean_live`` and ``mmx_lxmert_rollout`` at op level, over the case table of ``tests/lxmert_baselines_cases.py``
(random softmax slabs, ``randn`` gradients with 1e3 in their padding).  Every result is

1. compared with the float64 restatement: its distance may be at most the larger of 1e-6 and TWICE the distance the existing fp32
   per-item composition shows on the same slabs (head mean / ``rules.gradcam`` / ``rules.compute_rollout_attention`` /
   ``ops.matmul`` on the live sub-blocks), and never above the project's absolute 1e-5 (both distances go to ``tests/parity.py``),
2. exactly zero outside the live blocks, with ``R_tt[b, 0, 0] == 0``,
3. for B = 5: bit-equal, sample by sample, to the same sample run alone,
4. bit-equal between two calls,
5. written between NaN-filled guard bands (outputs and workspace) that stay NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lxmert_baselines_cases as cases  # noqa: E402
import parity  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 256                     # floats on either side of every region
CONTRACT = 1e-5                 # the project's absolute bound on a relevancy map


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Arena:
    """One NaN-filled device buffer, regions carved out of it with guard bands between them (offsets are multiples of 64 floats, so
    every region is 256-byte aligned like a fresh allocation)."""

    def __init__(self, sizes):
        self.spans, at = [], GUARD
        for n in sizes:
            self.spans.append((at, n))
            at += ((n + 63) // 64) * 64 + GUARD
        self.buf = torch.full((at,), float("nan"), dtype=torch.float32, device="cuda")

    def region(self, i):
        at, n = self.spans[i]
        return self.buf[at:at + n]

    def assert_guards_untouched(self, written):
        """Everything outside the regions is still NaN; region i is NaN beyond its first ``written[i]`` floats."""
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        for (at, _n), w in zip(self.spans, written):
            keep[at:at + w] = False
        assert bool(torch.isnan(self.buf[keep]).all()), "a guard band was written"


def run_head_mean(attn, grad, q_len, k_len, zero_cls):
    """The C entry on its own output region between guard bands -> ``[B, Nq, Nk]`` (a copy)."""
    from transformer_mm_explainability_amd import _lib
    B, H, Nq, Nk = attn.shape
    arena = Arena([B * Nq * Nk])
    rc = _lib.lib().mmx_head_mean_live(_ptr(attn), _ptr(grad), _ptr(arena.region(0)), B, H, Nq, Nk, _ptr(q_len), _ptr(k_len),
                                       _lib.HEAD_MEAN_ZERO_CLS if zero_cls else 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "mmx_head_mean_live")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([B * Nq * Nk])
    return arena.region(0).reshape(B, Nq, Nk).clone()


def run_rollout(text, img, cross, t_len, want_ii=True):
    from transformer_mm_explainability_amd import _lib
    B, H, T, I = cross.shape
    need = _lib.lib().mmx_lxmert_rollout_workspace_bytes(len(text), len(img), B, T, I)
    assert need > 0 and need % 4 == 0
    sizes = [B * T * T, B * T * I, B * I * I, need // 4]
    arena = Arena(sizes)
    tt, _k0 = _lib.ptr_table([t.data_ptr() for t in text])
    ti, _k1 = _lib.ptr_table([t.data_ptr() for t in img])
    rc = _lib.lib().mmx_lxmert_rollout(tt, len(text), ti, len(img), _ptr(cross), B, H, T, I, _ptr(t_len), _ptr(arena.region(0)),
                                       _ptr(arena.region(1)), _ptr(arena.region(2)) if want_ii else C.c_void_p(0),
                                       _ptr(arena.region(3)), need, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "mmx_lxmert_rollout")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([sizes[0], sizes[1], sizes[2] if want_ii else 0, sizes[3]])
    return (arena.region(0).reshape(B, T, T).clone(), arena.region(1).reshape(B, T, I).clone(),
            arena.region(2).reshape(B, I, I).clone() if want_ii else None)


def _err(got, want64):
    return float(np.abs(got.double().cpu().numpy() - want64).max())


def _judge(label, got, want64, composed):
    """Rule 1 of the module docstring; ``composed``: what the existing fp32 per-item composition gives for the same map."""
    err, base = _err(got, want64), _err(composed, want64)
    bound = min(max(1e-6, 2.0 * base), CONTRACT)
    scale = float(np.abs(want64).max())
    parity.note(label + " kernel vs float64", err, bound, scale)
    parity.note(label + " per-item fp32 composition vs float64", base, None, scale)
    print("%s: kernel %.3e  per-item fp32 composition %.3e  bound %.3e" % (label, err, base, bound))
    assert err <= bound, "%s: |kernel - float64| = %.3e > %.3e (fp32 composition: %.3e)" % (label, err, bound, base)


def _assert_zero_outside(out, q_len, k_len):
    for b in range(out.shape[0]):
        q, k = int(q_len[b]), int(k_len[b])
        assert not bool(out[b, q:].any()) and not bool(out[b, :, k:].any())


def _composed_head_mean(P, G, q_len, k_len, zero_cls):
    """The parent's route, item by item on the live sub-block: ``GeneratorBaselines._head_mean`` / ``rules.gradcam``."""
    from transformer_mm_explainability_amd import rules
    out = torch.zeros(P.shape[0], P.shape[2], P.shape[3], device="cuda")
    for b in range(P.shape[0]):
        q, k = int(q_len[b]), int(k_len[b])
        cam = P[b:b + 1, :, :q, :k].contiguous()
        if G is None:
            out[b, :q, :k] = cam.reshape(-1, q, k).mean(dim=0)
        else:
            out[b, :q, :k] = rules.gradcam(cam, G[b:b + 1, :, :q, :k].contiguous())
        if zero_cls:
            out[b, 0, 0] = 0
    return out


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_head_mean_and_gradcam_on_the_live_blocks(case):
    from transformer_mm_explainability_amd import ops
    T, I, H, B, kind = case
    c = cases.make_case(*case, cases.SEEDS[case])
    raw, t, k_len = _dev(c["raw"]), c["t"], c["k_len"]
    full_i = np.full(B, I, dtype=np.int32)
    # (probabilities, gradients, query lengths as given / as meant, key lengths as given / as meant, [CLS] flag)
    slabs = [("self", c["text"][-1], c["g_tt"], raw, t, raw, t, True),
             ("cross", c["cross"], c["g_ti"], raw, t, None, full_i, False),
             ("cross ragged keys", c["cross_k"], c["g_ti_k"], raw, t, _dev(k_len), k_len, False)]
    for name, P_np, G_np, ql, q_live, kl, k_live, cls in slabs:
        P, G = _dev(P_np), _dev(G_np)
        for method, grad in (("head mean", None), ("gradcam", G)):
            label = "%s %s" % (method, name)
            got = run_head_mean(P, grad, ql, kl, cls)
            want = cases.head_mean64(P_np, q_live, k_live, cls) if grad is None else cases.gradcam64(P_np, G_np, q_live, k_live, cls)
            _judge(label, got, want, _composed_head_mean(P, grad, q_live, k_live, cls))
            _assert_zero_outside(got, q_live, k_live)
            if cls:
                assert not bool(got[:, 0, 0].any())
            assert torch.equal(got, run_head_mean(P, grad, ql, kl, cls)), label + ": two calls differ"
            via_ops = ops.head_mean_live(P, ql, kl, cls) if grad is None else ops.attn_gradcam_live(P, grad, ql, kl, cls)
            assert torch.equal(got, via_ops), label + ": ops differs from the C entry"
            if kind == "oob":                            # an out-of-range length IS its clamped value
                assert torch.equal(got, run_head_mean(P, grad, _dev(q_live), None if kl is None else _dev(k_live), cls)), label
            if B > 1:
                for b in range(B):
                    alone = run_head_mean(P[b:b + 1].contiguous(), None if grad is None else grad[b:b + 1].contiguous(),
                                          None if ql is None else ql[b:b + 1].contiguous(),
                                          None if kl is None else kl[b:b + 1].contiguous(), cls)
                    assert torch.equal(got[b:b + 1], alone), "%s: sample %d of the batch differs from the sample alone" % (label, b)


def _composed_rollout(text, img, cross, t_len):
    """The parent's ``generate_rollout`` arithmetic, item by item on the live sub-blocks."""
    from transformer_mm_explainability_amd import ops, rules
    B, H, T, I = cross.shape
    R_tt, R_ti, R_ii = torch.zeros(B, T, T, device="cuda"), torch.zeros(B, T, I, device="cuda"), torch.zeros(B, I, I, device="cuda")
    for b in range(B):
        t = int(t_len[b])
        cams_t = [m[b, :, :t, :t].mean(dim=0).contiguous() for m in text]
        cams_i = [m[b].mean(dim=0).contiguous() for m in img]
        cam_ti = cross[b, :, :t, :].mean(dim=0).contiguous()
        r_prime = rules.compute_rollout_attention(cams_t[:-1])
        R_ii[b] = rules.compute_rollout_attention(cams_i)
        R_ti[b, :t] = ops.matmul(r_prime, ops.matmul(cam_ti, R_ii[b].contiguous()), trans_a=True)
        R_tt[b, :t, :t] = rules.compute_rollout_attention(cams_t)
        R_tt[b, 0, 0] = 0
    return R_tt, R_ti, R_ii


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_rollout_on_the_live_blocks(case):
    from transformer_mm_explainability_amd import ops
    T, I, H, B, kind = case
    full_i = np.full(B, I, dtype=np.int32)
    for n_text in cases.N_TEXT:
        for n_img in cases.N_IMG:
            c = cases.make_case(*case, cases.SEEDS[case], n_text=n_text, n_img=n_img)
            raw, t = _dev(c["raw"]), c["t"]
            text, img, cross = [_dev(m) for m in c["text"]], [_dev(m) for m in c["img"]], _dev(c["cross"])
            got = run_rollout(text, img, cross, raw)
            want = cases.rollout64(c["text"], c["img"], c["cross"], t)
            composed = _composed_rollout(text, img, cross, t)
            tag = "rollout n_text=%d n_img=%d " % (n_text, n_img)
            for name, g, w, comp in zip(("R_tt", "R_ti", "R_ii"), got, want, composed):
                _judge(tag + name, g, w, comp)
            _assert_zero_outside(got[0], t, t)
            _assert_zero_outside(got[1], t, full_i)
            assert not bool(got[0][:, 0, 0].any())
            again = run_rollout(text, img, cross, raw, want_ii=False)
            assert again[2] is None and torch.equal(got[0], again[0]) and torch.equal(got[1], again[1]), tag + "two calls differ"
            via_ops = ops.lxmert_rollout(text, img, cross, text_len=raw)
            assert all(torch.equal(a, b) for a, b in zip(got, via_ops)), tag + "ops differs from the C entry"
            if kind == "oob":
                clamped = run_rollout(text, img, cross, _dev(t))
                assert all(torch.equal(a, b) for a, b in zip(got, clamped)), tag + "an out-of-range length is not its clamped value"
            if B > 1:
                for b in range(B):
                    alone = run_rollout([m[b:b + 1].contiguous() for m in text], [m[b:b + 1].contiguous() for m in img],
                                        cross[b:b + 1].contiguous(), None if raw is None else raw[b:b + 1].contiguous())
                    for name, g, a in zip(("R_tt", "R_ti", "R_ii"), got, alone):
                        assert torch.equal(g[b:b + 1], a), "%s%s: sample %d of the batch differs from the sample alone" % (tag, name, b)
