"""-m gpu: ``mmx_selfattn_ours_row`` at op level, over the case table of ``tests/visualbert_ours_cases.py`` (per layer a softmax slab
with exact zeros at padded keys and a ``randn + c_h`` gradient slab with 1e3 in its padding).  Every result is

1. compared with the float64 restatement of the reference's :83-97 on the compacted live set, elementwise inside the counted bound
   ``expm1(L (N + H + 3) u) ref`` (the worst error / bound is printed),
2. exactly zero outside the live set and at column ``c_b``,
3. bit-equal between the C entry and ``ops``, between two calls, between "oob" lengths and their clamped form, between "null" and
   "full", to the same call with NaN written to the gradients everywhere outside ``L_b x L_b``, and -- for B = 5 -- sample by sample
   to the same sample run alone,
4. written between NaN-filled guard bands, with a workspace that is NaN before the call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visualbert_ours_cases as cases  # noqa: E402
from guard_arena import Arena, ptr as _ptr, to_device as _dev  # noqa: E402

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_ours(attn, grad, T, raw_t, raw_v):
    """``mmx_selfattn_ours_row`` on its own output and (NaN-filled) workspace regions between guard bands -> ``[B, N]`` (a copy)."""
    from transformer_mm_explainability_amd import _lib
    B, H, N, _ = attn[0].shape
    need = _lib.lib().mmx_selfattn_ours_row_workspace_bytes(len(attn), B, T, N - T)
    assert need > 0 and need % 4 == 0
    arena = Arena([B * N, need // 4])
    assert bool(torch.isnan(arena.region(1)).all())
    at, _k0 = _lib.ptr_table([t.data_ptr() for t in attn])
    gt, _k1 = _lib.ptr_table([t.data_ptr() for t in grad])
    rc = _lib.lib().mmx_selfattn_ours_row(at, gt, len(attn), B, H, T, N - T, _ptr(raw_t), _ptr(raw_v), _ptr(arena.region(0)),
                                          _ptr(arena.region(1)), need, _stream())
    _lib.check(rc, "mmx_selfattn_ours_row")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([B * N, need // 4])
    return arena.region(0).reshape(B, N).clone()


def _assert_zero_pattern(out, T, t, v):
    N = out.shape[1]
    for b in range(out.shape[0]):
        dead = np.ones(N, dtype=bool)
        dead[cases.live_index(T, t[b], v[b])] = False
        dead[int(t[b]) - 2] = True
        assert not bool(out[b][torch.from_numpy(dead).cuda()].any()), "sample %d: not exact zero outside the live set / at c_b" % b


def _nan_outside_live(grad, T, t, v):
    """The gradient slabs with NaN at every entry outside ``L_b x L_b``."""
    out = []
    for g in grad:
        g = g.copy()
        for b in range(g.shape[0]):
            dead = np.ones(g.shape[-1], dtype=bool)
            dead[cases.live_index(T, t[b], v[b])] = False
            g[b][:, dead, :] = np.nan
            g[b][:, :, dead] = np.nan
        out.append(g)
    return out


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_ours_row_on_the_live_sets(case):
    from transformer_mm_explainability_amd import ops
    T, V, H, B, kind, L = case
    c = cases.make_case(*case, cases.SEEDS[case])
    t, v = c["t"], c["v"]
    raw_t, raw_v = _dev(c["raw_t"]), _dev(c["raw_v"])
    P, G = [_dev(m) for m in c["attn"]], [_dev(m) for m in c["grad"]]
    ref, bound = cases.ours64(c["attn"], c["grad"], T, t, v)

    got = run_ours(P, G, T, raw_t, raw_v)
    got64 = got.double().cpu().numpy()
    assert np.isfinite(got64).all()
    err = np.abs(got64 - ref)
    print("%s: worst error / bound %.3f  (max error %.3e, largest bound %.3e, max|ref| %.3e)"
          % (cases.case_id(case), float(cases.distance_in_bounds(got64, ref, bound).max()), float(err.max()), float(bound.max()),
             float(ref.max())))
    assert (err <= bound).all(), "|kernel - float64| exceeds the counted bound by %.3e" % float((err - bound).max())
    _assert_zero_pattern(got, T, t, v)

    assert torch.equal(got, run_ours(P, G, T, raw_t, raw_v)), "two calls differ"
    assert torch.equal(got, ops.selfattn_ours_row(P, G, raw_t, raw_v, n_text=T)), "ops differs from the C entry"
    Gn = [_dev(g) for g in _nan_outside_live(c["grad"], T, t, v)]
    if kind in ("ragged", "oob") and B > 1:
        assert all(bool(torch.isnan(g).any()) for g in Gn)
    assert torch.equal(got, run_ours(P, Gn, T, raw_t, raw_v)), "NaN in the gradients outside L_b x L_b reaches the output"
    del Gn
    if kind in ("oob", "null"):                          # an out-of-range length IS its clamped value; no array IS the full extent
        assert torch.equal(got, run_ours(P, G, T, _dev(t), _dev(v))), kind + " differs from its explicit form"
    if B > 1:
        for b in range(B):
            alone = run_ours([m[b:b + 1].contiguous() for m in P], [m[b:b + 1].contiguous() for m in G], T,
                             None if raw_t is None else raw_t[b:b + 1].contiguous(),
                             None if raw_v is None else raw_v[b:b + 1].contiguous())
            assert torch.equal(got[b:b + 1], alone), "sample %d of the batch differs from the sample alone" % b


def test_a_nan_in_a_live_gradient_entry_is_propagated_not_clamped():
    """The clamp is the project's NaN-propagating one: a NaN at a LIVE entry of row c_b of the top layer reaches that sample's
    output (as ``torch.clamp(min=0)`` does in the reference) and no other sample's."""
    case = (8, 10, 3, 5, "ragged", 2)
    T = case[0]
    c = cases.make_case(*case, 1)
    G = [g.copy() for g in c["grad"]]
    b, cb = 2, int(c["t"][2]) - 2
    G[-1][b, 1, cb, 0] = np.nan
    P, Gd, rt, rv = [_dev(m) for m in c["attn"]], [_dev(m) for m in G], _dev(c["raw_t"]), _dev(c["raw_v"])
    got = run_ours(P, Gd, T, rt, rv)
    clean = run_ours(P, [_dev(m) for m in c["grad"]], T, rt, rv)
    assert bool(torch.isnan(got[b]).any())
    for other in (0, 1, 3, 4):
        assert torch.equal(got[other], clean[other])


def test_ops_refuse_shapes_outside_the_limits():
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    x = torch.zeros(1, 1, 12, 12, device="cuda")
    for bad in (None, 1, 12, 13):
        with pytest.raises(MMXError):
            ops.selfattn_ours_row([x], [x], n_text=bad)
    with pytest.raises(MMXError):
        ops.selfattn_ours_row([x] * 33, [x] * 33, n_text=4)
    with pytest.raises(MMXError):
        ops.selfattn_ours_row([x, x], [x], n_text=4)
    with pytest.raises(MMXError):
        ops.selfattn_ours_row([], [], n_text=4)
    with pytest.raises(MMXError):
        ops.selfattn_ours_row([x], [torch.zeros(1, 1, 12, 11, device="cuda")], n_text=4)
    with pytest.raises(MMXError):
        ops.selfattn_ours_row([x], [x.double()], n_text=4)
    big = torch.zeros(1, 1, 257, 257, device="cuda")
    with pytest.raises(MMXError):
        ops.selfattn_ours_row([big], [big], n_text=100)
    out = ops.selfattn_ours_row([x], [x], n_text=4)
    assert out.shape == (1, 12) and not bool(out.any())
