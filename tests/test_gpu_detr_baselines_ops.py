"""-m gpu: ``mmx_detr_cross_rows`` and ``mmx_detr_rollout_rows`` at op level.

1. On the slabs of the ``detr_chain`` fixture against what the reference's generator recorded (the project's contract: 1e-5 absolute
   and 1e-4 x max|ref|).
2. Over the case table of ``tests/detr_baselines_cases.py`` and at the real size (950 tokens, 100 queries, 8 heads, 6 + 6 layers,
   K = 16) against the float64 restatement in matrix form: inside the COUNTED bound of the method AND inside the contract.  The largest
   error-to-bound ratio and the largest absolute error per method are printed.
3. Bit-equal between the C entry and ``ops``, between two calls, between equal targets in different slots, between K = 1 and the same
   target inside a longer list, and between an out-of-range target and its clamped value.
4. Written between NaN-filled guard bands (output and workspace) that stay NaN."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detr_baselines_cases as cases  # noqa: E402
import parity  # noqa: E402
from guard_arena import Arena, ptr as _ptr, to_device as _dev  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WORST = {}                       # method -> [largest err / bound, largest |err|]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_cross(P, G, targets):
    """``mmx_detr_cross_rows`` on its own output and workspace regions between guard bands -> ``[K, Ni]`` (a copy).  ``G``: ``None``,
    ``[K, H, Q, Ni]`` or the shared ``[H, Q, Ni]``."""
    from transformer_mm_explainability_amd import _lib
    H, Q, Ni = P.shape
    K = targets.numel()
    need = _lib.lib().mmx_detr_cross_rows_workspace_bytes(K, H, Q, Ni) if G is not None else 0
    assert need % 4 == 0 and (G is None or need > 0)
    arena = Arena([K * Ni, max(need // 4, 4)])
    bstride = H * Q * Ni if (G is not None and G.dim() == 4) else 0
    rc = _lib.lib().mmx_detr_cross_rows(_ptr(P), _ptr(G), bstride, _ptr(targets), _ptr(arena.region(0)), K, H, Q, Ni,
                                        _ptr(arena.region(1)) if G is not None else C.c_void_p(0), need, _stream())
    _lib.check(rc, "mmx_detr_cross_rows")
    torch.cuda.synchronize()
    strips = (Q * Ni + cases.GRAD_STRIP - 1) // cases.GRAD_STRIP
    arena.assert_guards_untouched([K * Ni, 0 if G is None else (K if bstride else 1) * H * strips])
    return arena.region(0).reshape(K, Ni).clone()


def run_rollout(enc, dec, P, targets):
    from transformer_mm_explainability_amd import _lib
    H, Q, Ni = P.shape
    K = targets.numel()
    need = _lib.lib().mmx_detr_rollout_rows_workspace_bytes(len(enc), len(dec), K, Q, Ni)
    assert need > 0 and need % 4 == 0
    arena = Arena([K * Ni, need // 4])
    et, _k0 = _lib.ptr_table([t.data_ptr() for t in enc])
    dt, _k1 = _lib.ptr_table([t.data_ptr() for t in dec])
    rc = _lib.lib().mmx_detr_rollout_rows(et, len(enc), dt, len(dec), _ptr(P), _ptr(targets), _ptr(arena.region(0)), K, H, Q, Ni,
                                          _ptr(arena.region(1)), need, _stream())
    _lib.check(rc, "mmx_detr_rollout_rows")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([K * Ni, need // 4])
    return arena.region(0).reshape(K, Ni).clone()


def _judge(method, label, got, ref, bound):
    """Rule 2 of the module docstring: the counted bound elementwise, the contract per call."""
    got64 = got.double().cpu().numpy()
    assert got64.shape == ref.shape and np.isfinite(got64).all(), label
    err = np.abs(got64 - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0
    w = WORST.setdefault(method, [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], float(err.max()))
    print("%s %s: max|err| %.3e  largest bound %.3e  err/bound %.3f  max|ref| %.3e   (worst so far: ratio %.3f, |err| %.3e)"
          % (method, label, float(err.max()), float(bound.max()), ratio, float(np.abs(ref).max()), w[0], w[1]))
    parity.note("detr baselines %s %s kernel vs float64" % (method, label), float(err.max()), float(bound.max()),
                float(np.abs(ref).max()), parity.RELMAX)
    assert (err <= bound).all(), "%s %s: |kernel - float64| exceeds the counted bound by %.3e (ratio %.3f)" % (
        method, label, float((err - bound).max()), ratio)
    parity.close(got, ref, what="detr baselines %s %s" % (method, label))


def _device_case(case):
    c = cases.make_case(case)
    d = dict(c)
    d["P"], d["G"], d["Gs"] = _dev(c["cross"]), _dev(c["grad"]), _dev(c["grad_shared"])
    d["enc_d"], d["dec_d"] = [_dev(a) for a in c["enc"]], [_dev(b) for b in c["dec"]]
    d["t"] = _dev(c["targets"])
    return d


def test_the_three_ops_on_the_reference_generators_fixture():
    from transformer_mm_explainability_amd import ops
    g = np.load(os.path.join(GOLDEN, "detr_chain.npz"))
    t = _dev(g["target_index"].astype(np.int64))
    enc, dec = [_dev(a) for a in g["enc_attn"]], [_dev(a) for a in g["dself_attn"]]
    P, G = _dev(g["dcross_attn"][-1]), _dev(g["dcross_grad"][-1])
    parity.close(ops.detr_rollout_rows(enc, dec, P, t), g["rollout_out"][0, 0], what="detr_rollout_rows vs the reference's rollout_out")
    parity.close(ops.detr_raw_rows(P, t), g["raw_attn_out"][0, 0], what="detr_raw_rows vs the reference's raw_attn_out")
    parity.close(ops.detr_gradcam_rows(P, G, t), g["gradcam_out"][0, 0], what="detr_gradcam_rows vs the reference's gradcam_out")
    # the same gradient slab handed in once per target is the same map
    assert torch.equal(ops.detr_gradcam_rows(P, torch.cat([G, G]), t), ops.detr_gradcam_rows(P, G, t))


@pytest.mark.parametrize("case", cases.CASES, ids=cases.case_id)
def test_the_three_methods_over_the_case_table(case):
    from transformer_mm_explainability_amd import ops
    c = _device_case(case)
    K, H, Q, Ni = c["K"], c["H"], c["Q"], c["Ni"]
    t, P = c["t"], c["P"]
    label = cases.case_id(case)

    got = run_cross(P, None, t)
    _judge("raw_attn", label, got, *cases.raw64(c["cross"], c["targets"]))
    assert torch.equal(got, run_cross(P, None, t)) and torch.equal(got, ops.detr_raw_rows(P, t))

    got = run_cross(P, c["G"], t)
    _judge("attn_gradcam", label + " per-target slabs", got, *cases.gradcam64(c["cross"], c["grad"], c["targets"]))
    assert torch.equal(got, run_cross(P, c["G"], t)) and torch.equal(got, ops.detr_gradcam_rows(P, c["G"].reshape(K * H, Q, Ni), t))
    shared = run_cross(P, c["Gs"], t)
    _judge("attn_gradcam", label + " shared slab", shared, *cases.gradcam64(c["cross"], c["grad_shared"], c["targets"]))
    assert torch.equal(shared, run_cross(P, c["Gs"], t))
    if K > 1:
        assert torch.equal(shared, ops.detr_gradcam_rows(P, c["Gs"], t))
    # a shared slab is the same as K copies of it
    assert torch.equal(shared, run_cross(P, c["Gs"].unsqueeze(0).repeat(K, 1, 1, 1).contiguous(), t))

    got = run_rollout(c["enc_d"], c["dec_d"], P, t)
    _judge("rollout", label, got, *cases.rollout64(c["enc"], c["dec"], c["cross"], c["targets"]))
    assert torch.equal(got, run_rollout(c["enc_d"], c["dec_d"], P, t))
    assert torch.equal(got, ops.detr_rollout_rows(c["enc_d"], c["dec_d"], P, t))

    # row k alone (K = 1) has the bits of row k inside the K-target call, whatever its slot
    for k in sorted({0, K // 2, K - 1}):
        one = t[k:k + 1].contiguous()
        assert torch.equal(run_cross(P, None, one), run_cross(P, None, t)[k:k + 1])
        assert torch.equal(run_cross(P, c["G"][k:k + 1].contiguous(), one), run_cross(P, c["G"], t)[k:k + 1])
        assert torch.equal(run_rollout(c["enc_d"], c["dec_d"], P, one), got[k:k + 1])


@pytest.fixture(scope="module")
def full_case():
    return _device_case(cases.FULL)


@pytest.mark.parametrize("method", ["raw_attn", "attn_gradcam", "rollout"])
def test_the_real_size(full_case, method):
    """950 tokens, 100 queries, 8 heads, 6 + 6 layers, K = 16."""
    c = full_case
    if method == "raw_attn":
        _judge(method, "full size", run_cross(c["P"], None, c["t"]), *cases.raw64(c["cross"], c["targets"]))
    elif method == "attn_gradcam":
        _judge(method, "full size", run_cross(c["P"], c["G"], c["t"]), *cases.gradcam64(c["cross"], c["grad"], c["targets"]))
    else:
        _judge(method, "full size", run_rollout(c["enc_d"], c["dec_d"], c["P"], c["t"]),
               *cases.rollout64(c["enc"], c["dec"], c["cross"], c["targets"]))


def test_equal_targets_and_slots():
    """Equal targets in different slots give equal bits; K = 1 and the same target inside K = 17 give equal bits."""
    c = _device_case((63, 100, 3, 17, 6, 2))
    K, Q = 17, 100
    t = torch.tensor([5, 99, 5, 0, 42, 5, 99] + [7] * 10, device="cuda")
    G = c["G"][:1].repeat(K, 1, 1, 1).contiguous()                       # the same gradient slab in every slot
    outs = {"raw_attn": run_cross(c["P"], None, t), "attn_gradcam": run_cross(c["P"], G, t),
            "rollout": run_rollout(c["enc_d"], c["dec_d"], c["P"], t)}
    for method, out in outs.items():
        for a, b in ((0, 2), (0, 5), (1, 6), (7, 16), (8, 12)):
            assert torch.equal(out[a], out[b]), "%s: slots %d and %d hold target %d but differ" % (method, a, b, int(t[a]))
        assert not torch.equal(out[0], out[1]), method
    one = torch.tensor([5], device="cuda")
    assert torch.equal(run_cross(c["P"], None, one)[0], outs["raw_attn"][5])
    assert torch.equal(run_cross(c["P"], G[:1].contiguous(), one)[0], outs["attn_gradcam"][5])
    assert torch.equal(run_rollout(c["enc_d"], c["dec_d"], c["P"], one)[0], outs["rollout"][5])


def test_an_out_of_range_target_behaves_as_its_clamped_value():
    c = _device_case((65, 7, 8, 5, 6, 6))
    raw = torch.tensor([-1, 7, 3, 1 << 40, -(1 << 40)], device="cuda")
    clamped = torch.tensor([0, 6, 3, 6, 0], device="cuda")
    assert torch.equal(run_cross(c["P"], None, raw), run_cross(c["P"], None, clamped))
    assert torch.equal(run_cross(c["P"], c["G"], raw), run_cross(c["P"], c["G"], clamped))
    assert torch.equal(run_rollout(c["enc_d"], c["dec_d"], c["P"], raw), run_rollout(c["enc_d"], c["dec_d"], c["P"], clamped))


def test_gradcam_sums_the_whole_block_not_only_the_target_row():
    """A gradient that is zero outside row t_k and one that is not give different maps: the sum runs over [Q, Ni]."""
    c = _device_case((65, 7, 8, 5, 6, 6))
    G = c["G"].clone()
    only_row = torch.zeros_like(G)
    for k, t in enumerate(c["targets"]):
        only_row[k, :, t] = G[k, :, t]
    a, b = run_cross(c["P"], G, c["t"]), run_cross(c["P"], only_row, c["t"])
    assert not torch.equal(a, b)
    ref, bound = cases.gradcam64(c["cross"], only_row.cpu().numpy(), c["targets"])
    _judge("attn_gradcam", "rows-only gradient", b, ref, bound)


def test_ops_refuse_shapes_outside_the_limits():
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    z = lambda *s: torch.zeros(*s, device="cuda")
    t = torch.tensor([0], device="cuda")
    with pytest.raises(MMXError):
        ops.detr_raw_rows(z(1, 129, 8), t)
    with pytest.raises(MMXError):
        ops.detr_raw_rows(z(33, 4, 8), t)
    with pytest.raises(MMXError):
        ops.detr_raw_rows(z(1, 4, 2049), t)
    with pytest.raises(MMXError):
        ops.detr_raw_rows(z(1, 1, 4, 8), t)
    with pytest.raises(MMXError):
        ops.detr_raw_rows(z(2, 4, 8), torch.zeros(0, dtype=torch.long, device="cuda"))
    with pytest.raises(MMXError):
        ops.detr_gradcam_rows(z(2, 4, 8), z(3, 4, 8), t)
    with pytest.raises(MMXError):
        ops.detr_gradcam_rows(z(2, 4, 8), z(2, 4, 9), t)
    with pytest.raises(MMXError):
        ops.detr_rollout_rows([z(2, 8, 8)] * 33, [z(2, 4, 4)], z(2, 4, 8), t)
    with pytest.raises(MMXError):
        ops.detr_rollout_rows([], [z(2, 4, 4)], z(2, 4, 8), t)
    with pytest.raises(MMXError):
        ops.detr_rollout_rows([z(2, 8, 7)], [z(2, 4, 4)], z(2, 4, 8), t)
    with pytest.raises(MMXError):
        ops.detr_rollout_rows([z(3, 8, 8)], [z(2, 4, 4)], z(2, 4, 8), t)
    with pytest.raises(MMXError):
        ops.detr_raw_rows(z(2, 4, 8).half(), t)
