"""-m gpu: ``mmx_selfattn_row_live`` and ``mmx_selfattn_rollout_row`` at op level, over the case table of
``tests/visualbert_baselines_cases.py`` (softmax slabs with exact zeros at padded keys, ``randn + c_h`` gradients with 1e3 in their
padding).  Every result is

1. compared with the float64 restatement on the compacted live set: inside the COUNTED bound of its method (see the helper) and
   inside the project's ``1e-4 x max|ref|`` per sample; both distances go to ``tests/parity.py`` together with the distance of the
   existing fp32 per-item composition on the compacted slabs (``.mean`` / ``rules.gradcam`` + min-max /
   ``compute_rollout_attention_batched``), which is recorded, not judged,
2. exactly zero outside the live set and at column ``c_b``,
3. bit-equal between the C entry and ``ops``, between two calls, between "oob" lengths and their clamped form, between "null" and
   "full", and -- for B = 5 -- sample by sample to the same sample run alone,
4. written between NaN-filled guard bands (output and workspace) that stay NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402
import visualbert_baselines_cases as cases  # noqa: E402
from guard_arena import Arena, ptr as _ptr, to_device as _dev  # noqa: E402

pytestmark = pytest.mark.gpu
RELMAX = parity.RELMAX


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_row(attn, grad, T, raw_t, raw_v):
    """``mmx_selfattn_row_live`` on its own output and workspace regions between guard bands -> ``[B, N]`` (a copy)."""
    from transformer_mm_explainability_amd import _lib
    B, H, N, _ = attn.shape
    need = _lib.lib().mmx_selfattn_row_live_workspace_bytes(B, H, T, N - T) if grad is not None else 0
    assert need % 4 == 0 and (grad is None or need > 0)
    arena = Arena([B * N, max(need // 4, 4)])
    rc = _lib.lib().mmx_selfattn_row_live(_ptr(attn), _ptr(grad), _ptr(arena.region(0)), B, H, T, N - T, _ptr(raw_t), _ptr(raw_v),
                                          _ptr(arena.region(1)) if grad is not None else C.c_void_p(0), need, _stream())
    _lib.check(rc, "mmx_selfattn_row_live")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([B * N, need // 4])
    return arena.region(0).reshape(B, N).clone()


def run_rollout(layers, T, raw_t, raw_v):
    from transformer_mm_explainability_amd import _lib
    B, H, N, _ = layers[0].shape
    need = _lib.lib().mmx_selfattn_rollout_row_workspace_bytes(len(layers), B, T, N - T)
    assert need > 0 and need % 4 == 0
    arena = Arena([B * N, need // 4])
    tbl, _k = _lib.ptr_table([t.data_ptr() for t in layers])
    rc = _lib.lib().mmx_selfattn_rollout_row(tbl, len(layers), B, H, T, N - T, _ptr(raw_t), _ptr(raw_v), _ptr(arena.region(0)),
                                             _ptr(arena.region(1)), need, _stream())
    _lib.check(rc, "mmx_selfattn_rollout_row")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([B * N, need // 4])
    return arena.region(0).reshape(B, N).clone()


def _judge(label, got, ref, bound, composed=None):
    """Rule 1 of the module docstring.  ``bound``: ``[B, N]`` elementwise or ``[B]`` per sample."""
    got64 = got.double().cpu().numpy()
    assert np.array_equal(np.isnan(got64), np.isnan(ref)), label + ": NaN pattern"
    err = np.abs(got64 - ref)
    bound = np.asarray(bound)
    full = bound if bound.ndim == 2 else np.broadcast_to(bound[:, None], ref.shape)
    scale = float(np.abs(ref).max())
    parity.note(label + " kernel vs float64", float(err.max()), float(full.max()), scale, RELMAX)
    if composed is not None:
        parity.note(label + " per-item fp32 composition vs float64", float(np.abs(composed.double().cpu().numpy() - ref).max()), None, scale)
    worst = err - full
    print("%s: kernel %.3e  largest bound %.3e  max|ref| %.3e" % (label, float(err.max()), float(full.max()), scale))
    assert (err <= full).all(), "%s: |kernel - float64| exceeds the counted bound by %.3e" % (label, float(worst.max()))
    for b in range(ref.shape[0]):
        assert err[b].max() <= RELMAX * np.abs(ref[b]).max(), \
            "%s: sample %d: %.3e > 1e-4 x %.3e" % (label, b, float(err[b].max()), float(np.abs(ref[b]).max()))


def _assert_zero_pattern(out, T, t, v):
    N = out.shape[1]
    for b in range(out.shape[0]):
        dead = np.ones(N, dtype=bool)
        dead[cases.live_index(T, t[b], v[b])] = False
        dead[int(t[b]) - 2] = True
        assert not bool(out[b][torch.from_numpy(dead).cuda()].any()), "sample %d: not exact zero outside the live set / at c_b" % b


def _composed(method, layers, grad, T, t, v):
    """The parent's per-item arithmetic on each sample's compacted slabs, scattered back to the padded layout."""
    from transformer_mm_explainability_amd import rules
    B, H, N, _ = layers[0].shape
    out = torch.zeros(B, N, device="cuda")
    for b in range(B):
        idx = torch.from_numpy(cases.live_index(T, t[b], v[b])).cuda()
        c = int(t[b]) - 2
        cut = lambda m: m[b][:, idx][:, :, idx].contiguous()
        if method == "raw":
            row = cut(layers[-1]).mean(dim=0)[c]
        elif method == "rollout":
            cams = [(cut(m).sum(dim=0) / H).unsqueeze(0) for m in layers]
            row = rules.compute_rollout_attention_batched(cams)[0, c]
        else:
            cam = rules.gradcam(cut(layers[-1]), cut(grad))
            row = ((cam - cam.min()) / (cam.max() - cam.min()))[c]
        row = row.clone()
        row[c] = 0
        out[b, idx] = row
    return out


def _sub(x, b):
    return None if x is None else x[b:b + 1].contiguous()


def _check_method(label, run, run_ops, ref, bound, composed, c, raw_t, raw_v):
    """Everything of the module docstring for one method; ``run(lengths..., sample=None)`` calls the C entry."""
    T, t, v, B, kind = c["T"], c["t"], c["v"], c["B"], c["kind"]
    got = run(raw_t, raw_v)
    _judge(label, got, ref, bound, composed)
    _assert_zero_pattern(got, T, t, v)
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
    assert same(got, run(raw_t, raw_v)), label + ": two calls differ"
    assert same(got, run_ops(raw_t, raw_v)), label + ": ops differs from the C entry"
    if kind == "oob":                                    # an out-of-range length IS its clamped value
        assert same(got, run(_dev(t), _dev(v))), label + ": oob differs from its clamped form"
    if kind == "null":
        assert same(got, run(_dev(t), _dev(v))), label + ": null differs from full"
    if B > 1:
        for b in range(B):
            assert same(got[b:b + 1], run(_sub(raw_t, b), _sub(raw_v, b), sample=b)), \
                "%s: sample %d of the batch differs from the sample alone" % (label, b)
    return got


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_three_methods_on_the_live_sets(case):
    from transformer_mm_explainability_amd import ops
    T, V, H, B, kind = case
    c = cases.make_case(*case, cases.SEEDS[case], n_layers=max(cases.N_LAYERS))
    t, v = c["t"], c["v"]
    raw_t, raw_v = _dev(c["raw_t"]), _dev(c["raw_v"])
    layers, G = [_dev(m) for m in c["attn"]], _dev(c["grad"])
    P = layers[-1]

    def pick(x, sample):
        return x if sample is None else x[sample:sample + 1].contiguous()

    ref, bound = cases.raw64(c["attn"][-1], T, t, v)
    _check_method("raw attention", lambda a, b, sample=None: run_row(pick(P, sample), None, T, a, b),
                  lambda a, b: ops.selfattn_raw_row(P, a, b, n_text=T), ref, bound, _composed("raw", [P], None, T, t, v), c, raw_t, raw_v)

    ref, bound = cases.gradcam64(c["attn"][-1], c["grad"], T, t, v)
    _check_method("gradcam", lambda a, b, sample=None: run_row(pick(P, sample), pick(G, sample), T, a, b),
                  lambda a, b: ops.selfattn_gradcam_row(P, G, a, b, n_text=T), ref, bound, _composed("gradcam", [P], G, T, t, v),
                  c, raw_t, raw_v)

    for L in cases.N_LAYERS:
        tab = layers[-L:]
        ref, bound = cases.rollout64(c["attn"][-L:], T, t, v)
        _check_method("rollout L=%d" % L, lambda a, b, sample=None: run_rollout([pick(m, sample) for m in tab], T, a, b),
                      lambda a, b: ops.selfattn_rollout_row(tab, a, b, n_text=T), ref, bound, _composed("rollout", tab, None, T, t, v),
                      c, raw_t, raw_v)


SPIKE = 1e6
SPIKES = ("first", "last_text", "first_region", "last_region", "c_row_first_region")


def _spike_at(which, T, t, v):
    t, v = int(t), int(v)
    return {"first": (0, 0), "last_text": (t - 1, t - 1), "first_region": (T, T), "last_region": (T + v - 1, T + v - 1),
            "c_row_first_region": (t - 2, T)}[which]


@pytest.mark.parametrize("which", SPIKES)
def test_gradcam_with_one_huge_live_gradient_entry(which):
    """(128, 100), H = 3, ragged B = 5: one live gradient entry of every sample set to 1e6 -- at the corners of the two live runs and
    in row c_b -- still meets the counted bound against float64 (a sum that loses the spike, or takes it twice, does not)."""
    case = (128, 100, 3, 5, "ragged")
    T = case[0]
    c = cases.make_case(*case, cases.SEEDS[case])
    G = c["grad"].copy()
    for b in range(5):
        i, j = _spike_at(which, T, c["t"][b], c["v"][b])
        G[b, 0, i, j] = SPIKE
    ref, bound = cases.gradcam64(c["attn"][-1], G, T, c["t"], c["v"])
    assert np.isfinite(bound).all()
    got = run_row(_dev(c["attn"][-1]), _dev(G), T, _dev(c["raw_t"]), _dev(c["raw_v"]))
    _judge("gradcam spike " + which, got, ref, bound)
    _assert_zero_pattern(got, T, c["t"], c["v"])


def test_gradcam_ignores_a_huge_gradient_entry_at_a_padded_position():
    case = (128, 100, 3, 5, "ragged")
    T, V = case[:2]
    c = cases.make_case(*case, cases.SEEDS[case])
    P, rt, rv = _dev(c["attn"][-1]), _dev(c["raw_t"]), _dev(c["raw_v"])
    G = c["grad"].copy()
    touched = 0
    for b in range(5):
        t, v = int(c["t"][b]), int(c["v"][b])
        if t < T:
            G[b, :, t, 0] = G[b, :, 0, t] = G[b, :, t, t] = SPIKE
            touched += 1
        if v < V:
            G[b, :, T + v, 1] = G[b, :, 1, T + v] = G[b, :, T + V - 1, T + V - 1] = SPIKE
            touched += 1
    assert touched >= 6
    assert torch.equal(run_row(P, _dev(G), T, rt, rv), run_row(P, _dev(c["grad"]), T, rt, rv))


def test_an_all_clamped_sample_is_nan_and_leaves_its_neighbours_alone():
    """H = 1 and a negative head weight in ONE sample of the batch: its whole cam is clamped, ``mx == mn`` and its live entries off
    c_b are NaN (as in the per-item route); the other samples are bit-equal to themselves run alone."""
    case = (8, 10, 1, 5, "ragged")
    T = case[0]
    c = cases.make_case(*case, cases.SEEDS[case])
    G = c["grad"].copy()
    idx = cases.live_index(T, c["t"][2], c["v"][2])
    G[2][:, idx[:, None], idx[None, :]] *= -1.0
    ref, _bound = cases.gradcam64(c["attn"][-1], G, T, c["t"], c["v"])
    P, Gd, rt, rv = _dev(c["attn"][-1]), _dev(G), _dev(c["raw_t"]), _dev(c["raw_v"])
    got = run_row(P, Gd, T, rt, rv)
    off_c = np.delete(idx, int(c["t"][2]) - 2)
    assert np.isnan(ref[2, off_c]).all() and bool(torch.isnan(got[2, torch.from_numpy(off_c).cuda()]).all())
    assert np.array_equal(np.isnan(got.cpu().numpy()), np.isnan(ref))
    _assert_zero_pattern(torch.nan_to_num(got, nan=1.0) * torch.isfinite(got), T, c["t"], c["v"])
    for b in (0, 1, 3, 4):
        alone = run_row(P[b:b + 1].contiguous(), Gd[b:b + 1].contiguous(), T, rt[b:b + 1].contiguous(), rv[b:b + 1].contiguous())
        assert torch.equal(got[b:b + 1], alone) and bool(torch.isfinite(alone).all())
    composed = _composed("gradcam", [P], Gd, T, c["t"], c["v"])
    assert bool(torch.isnan(composed[2, torch.from_numpy(off_c).cuda()]).all())


def test_ops_refuse_shapes_outside_the_limits():
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    x = torch.zeros(1, 1, 12, 12, device="cuda")
    for bad in (None, 1, 12, 13):
        with pytest.raises(MMXError):
            ops.selfattn_raw_row(x, n_text=bad)
    with pytest.raises(MMXError):
        ops.selfattn_rollout_row([x] * 33, n_text=4)
    with pytest.raises(MMXError):
        ops.selfattn_gradcam_row(x, torch.zeros(1, 1, 12, 11, device="cuda"), n_text=4)
    with pytest.raises(MMXError):
        ops.selfattn_raw_row(torch.zeros(1, 1, 257, 257, device="cuda"), n_text=100)
