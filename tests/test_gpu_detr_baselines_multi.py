"""-m gpu: ``Generator.generate_{rollout, raw_attn, attn_gradcam}_multi``, ``GraphedBaselinesMulti`` and
``MaskGenerator(batch_baselines=True)`` on the ``detr_transformer`` fixture body, on a small random ``DETRFromFeatures`` and -- one case
per method -- on ``detr_resnet50_head`` with 25 x 38 features.

The multi call is compared with the ``torch.cat`` of the per-query calls.  Tolerance: each route's own distance to ONE float64 map -- the
restatement of ``tests/detr_baselines_cases.py`` (matrix form) evaluated on the slabs the multi call captured -- the two distances
summed, which bounds the difference by the triangle inequality, and never looser than the project's contract (1e-5 absolute,
1e-4 x max|ref|); each distance has to meet the contract by itself as well.  Raw attention and rollout run the per-query route's own
forward, so both routes see the same slabs.  GradCAM does not: its multi route takes the slabs of the shared forward and the hand-written
backward, the per-query route those of autograd, and the two sets differ in their last bits.  Measured on the ``detr_transformer``
fixture body: |multi - cat| 1.7e-9 at max|map| 2.6e-3, with 2.9e-10 / 1.6e-10 from each route to the restatement on ITS OWN slabs -- a
tolerance built from those two would ignore the distance between the slab sets, so the per-query distance is taken to the common map
(its distance on its own slabs is printed beside it).  Every figure is printed before it is judged."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detr_baselines_cases as cases  # noqa: E402
import parity  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METHODS = ("rollout", "raw_attn", "attn_gradcam")


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _golden():
    return dict(np.load(os.path.join(GOLDEN, "detr_transformer.npz")))


def _detr_from_golden(g):
    """The recipe of ``tests/test_gpu_generators.py``: the fixture's weights in ``detr_model``, its random position tensor in place of
    the sine embedding."""
    from transformer_mm_explainability_amd import detr_model
    d, heads, Le, Ld, ff, Q, n_cls, Cb, h, w = (int(x) for x in g["dims"])
    model = detr_model.DETRFromFeatures(
        detr_model.Transformer(d_model=d, nhead=heads, num_encoder_layers=Le, num_decoder_layers=Ld, dim_feedforward=ff, dropout=0.0,
                               return_intermediate_dec=True), num_classes=n_cls, num_queries=Q, backbone_channels=Cb)
    weights = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w__")}
    missing, unexpected = model.load_state_dict(weights, strict=False)
    assert not unexpected and all(m.startswith("bbox_embed.") for m in missing), (missing, unexpected)
    model = model.cuda().eval()
    pos_dev = cu(g["pos"])

    class FixedPos(nn.Module):
        def forward(self, mask):
            return pos_dev

    model.position = FixedPos()
    return model


def _body(name):
    """``(model, features, targets)``"""
    from transformer_mm_explainability_amd import detr_model
    if name == "golden":
        g = _golden()
        return _detr_from_golden(g), cu(g["features"]), torch.tensor([4, 0, 6, 4, 2], device="cuda")
    torch.manual_seed(3)
    if name == "small":
        model = detr_model.DETRFromFeatures(
            detr_model.Transformer(d_model=32, nhead=4, num_encoder_layers=2, num_decoder_layers=3, dim_feedforward=64, dropout=0.0,
                                   return_intermediate_dec=True), num_classes=5, num_queries=9, backbone_channels=16).cuda().eval()
        return model, torch.randn(1, 16, 4, 7, device="cuda"), torch.tensor([8, 0, 3, 8], device="cuda")
    model = detr_model.detr_resnet50_head().cuda().eval()
    return model, torch.randn(1, 2048, 25, 38, device="cuda") * 0.5, torch.tensor([3, 57, 99, 0, 57], device="cuda")


def _slabs(model):
    """The slabs the last pass left behind, as numpy: encoder / decoder self-attention lists, the top cross-attention ``[H, Q, Ni]`` and
    its gradient ``[n, H, Q, Ni]`` (n = 1 after a per-query pass; a replicated-batch forward's K equal probability slabs are cut to one)."""
    tr = model.transformer
    H = tr.nhead

    def probs(mod):
        a = mod.get_attn().detach()
        return a.reshape(-1, a.shape[-2], a.shape[-1])[:H].cpu().numpy()

    last = tr.decoder.layers[-1].multihead_attn
    g = last.get_attn_gradients().detach()
    g = g.reshape(-1, H, g.shape[-2], g.shape[-1]).cpu().numpy()
    return [probs(b.self_attn) for b in tr.encoder.layers], [probs(b.self_attn) for b in tr.decoder.layers], probs(last), g


def _ref(method, slabs, targets, k=None):
    """The float64 restatement on ``slabs``; ``k``: the slot whose gradient slab serves (``None``: slab k for target k)."""
    enc, dec, cross, grad = slabs
    if method == "raw_attn":
        return cases.raw64(cross, targets)[0]
    if method == "rollout":
        return cases.rollout64(enc, dec, cross, targets)[0]
    return cases.gradcam64(cross, grad if k is None else grad[k], targets)[0]


def _multi(gen, method, feats, targets):
    return getattr(gen, "generate_%s_multi" % method)(feats, targets)


def _single(gen, method, feats, t):
    return getattr(gen, "generate_" + method)(feats, t)


def _compare_routes(model, feats, targets, method, label):
    from transformer_mm_explainability_amd.detr_explainability import Generator
    gen = Generator(model)
    tl = targets.cpu().numpy()
    multi = _multi(gen, method, feats, targets)
    K, Ni = targets.numel(), multi.shape[-1]
    assert multi.shape == (1, 1, K, Ni)
    ref_m = _ref(method, _slabs(model), tl)
    rows, d_pq, d_own = [], 0.0, 0.0
    for k in range(K):
        one = _single(gen, method, feats, targets[k:k + 1])
        assert one.shape == (1, 1, 1, Ni)
        rows.append(one.detach().clone())
        got = one[0, 0, 0].double().cpu().numpy()
        d_pq = max(d_pq, float(np.abs(got - ref_m[k]).max()))
        if method == "attn_gradcam":                        # (the other two run the same forward: the same slabs)
            d_own = max(d_own, float(np.abs(got - _ref(method, _slabs(model), tl[k:k + 1], k=0)[0]).max()))
    cat = torch.cat(rows, dim=2)
    d_multi = float(np.abs(multi[0, 0].double().cpu().numpy() - ref_m).max())
    diff = float((multi - cat).abs().max())
    scale = float(np.abs(ref_m).max())
    contract = min(1e-5, 1e-4 * scale)
    tol = min(d_multi + d_pq, contract)
    print("%s %s: |multi - cat| %.3e   multi to float64 %.3e + per-query to the same float64 map %.3e (to float64 on its own slabs: %.3e)"
          "   contract %.3e   max|ref| %.3e" % (label, method, diff, d_multi, d_pq, d_own if method == "attn_gradcam" else d_pq, contract, scale))
    parity.note("detr baselines multi vs per-query %s %s" % (label, method), diff, tol, scale, parity.RELMAX)
    assert diff <= tol, "%s %s: |multi - cat(per query)| = %.3e > %.3e (= min(%.3e + %.3e, contract %.3e))" % (
        label, method, diff, tol, d_multi, d_pq, contract)
    assert d_multi <= contract and d_pq <= contract, "%s %s: a route is %.3e / %.3e from float64, contract %.3e" % (
        label, method, d_multi, d_pq, contract)
    parity.close(multi, ref_m.reshape(1, 1, K, Ni), what="detr baselines multi %s %s vs float64 on its own slabs" % (label, method))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("body", ["golden", "small"])
def test_multi_equals_the_cat_of_the_per_query_calls(body, method):
    model, feats, targets = _body(body)
    _compare_routes(model, feats, targets, method, body)


@pytest.mark.parametrize("method", METHODS)
def test_the_real_size(method):
    """``detr_resnet50_head``, 25 x 38 features, 5 targets."""
    model, feats, targets = _body("r50")
    _compare_routes(model, feats, targets, method, "r50")


def test_the_goldens_from_inside_a_three_target_call():
    from transformer_mm_explainability_amd.detr_explainability import Generator
    g = _golden()
    model, feats = _detr_from_golden(g), cu(g["features"])
    t = [int(x) for x in g["target_index"]]
    other = next(q for q in range(int(g["dims"][5])) if q not in t)
    targets = torch.tensor([t[0], other, t[1]], device="cuda")
    for method, key in (("rollout", "rollout_out"), ("raw_attn", "raw_attn_out")):
        out = _multi(Generator(model), method, feats, targets)
        assert out.shape[:3] == (1, 1, 3)
        parity.close(out[:, :, [0, 2]], g[key], what="%s of the fixture from inside a K = 3 call" % key)


def test_the_truncated_backward_leaves_the_same_bits_in_the_top_cross_slab():
    model, feats, targets = _body("small")
    K = targets.numel()
    last = model.transformer.decoder.layers[-1].multihead_attn
    first_enc = model.transformer.encoder.layers[0].self_attn
    with torch.no_grad():
        logits, state = model.forward_shared(feats, K)
        n_cls = logits.shape[-1]
        one_hot = torch.zeros(K, logits.shape[1] * n_cls, device="cuda")
        one_hot.scatter_(1, (targets * n_cls + torch.arange(K, device="cuda") % (n_cls - 1)).reshape(K, 1), 1.0)
        one_hot = one_hot.view(K, logits.shape[1], n_cls)
        last.get_attn_gradients().fill_(float("nan"))
        first_enc.get_attn_gradients().fill_(float("nan"))
        model.backward_shared(state, one_hot, stop_after_top_cross=True)
        short = last.get_attn_gradients().clone()
        assert bool(torch.isfinite(short).all())
        assert bool(torch.isnan(first_enc.get_attn_gradients()).all()), "the truncated backward went on below the top cross-attention"
        last.get_attn_gradients().fill_(float("nan"))
        model.backward_shared(state, one_hot)
        full = last.get_attn_gradients().clone()
        assert bool(torch.isfinite(first_enc.get_attn_gradients()).all())
    assert torch.equal(short, full)


@pytest.mark.parametrize("method", METHODS)
def test_replays_are_bit_equal_to_the_eager_multi_call(method):
    """K = 4 slots: a full set of targets, new targets copied in, fewer targets than slots, and more (chunks).  The eager call is
    given what the slots hold -- a short list filled up with repeats of its last target, a long one cut into chunks of 4 -- so that
    both sides run the same launches at the same batch size."""
    from transformer_mm_explainability_amd.detr_explainability import Generator, GraphedBaselinesMulti
    g = _golden()
    model, feats = _detr_from_golden(g), cu(g["features"])
    run = GraphedBaselinesMulti(model, feats, method, K=4)
    gen = Generator(model)

    def eager(ts):
        out = []
        for i in range(0, len(ts), 4):
            part = ts[i:i + 4]
            filled = part + [part[-1]] * (4 - len(part))
            out.append(_multi(gen, method, feats, torch.tensor(filled, device="cuda"))[:, :, :len(part)])
        return torch.cat(out, dim=2)

    for ts in ([4, 0, 6, 2], [1, 5, 3, 1], [6, 2], [1, 2, 3, 4, 5, 6, 0], [3]):
        got = run(feats, torch.tensor(ts, device="cuda")).clone()
        want = eager(ts)
        assert got.shape == want.shape == (1, 1, len(ts), feats.shape[-1] * feats.shape[-2])
        diff = float((got - want).abs().max())
        print("%s replay, targets %s: |replay - eager| = %.3e" % (method, ts, diff))
        assert torch.equal(got, want), "%s targets %s: replay differs from the eager call by %.3e" % (method, ts, diff)
        if method != "attn_gradcam":                          # no batch size in these two: the plain list gives the same bits
            assert torch.equal(got, _multi(gen, method, feats, torch.tensor(ts, device="cuda")))
    feats2 = feats.flip(-1).contiguous()
    ts = [4, 0, 6]
    assert torch.equal(run(feats2, torch.tensor(ts, device="cuda")),
                       _multi(gen, method, feats2, torch.tensor(ts + [6], device="cuda"))[:, :, :3])


def test_graphed_slot_rules():
    from transformer_mm_explainability_amd.detr_explainability import GraphedBaselinesMulti
    g = _golden()
    model, feats = _detr_from_golden(g), cu(g["features"])
    with pytest.raises(ValueError):
        GraphedBaselinesMulti(model, feats, "attn_gradcam", K=1)
    with pytest.raises(ValueError):
        GraphedBaselinesMulti(model, feats, "ours_no_lrp", K=4)
    one = GraphedBaselinesMulti(model, feats, "raw_attn", K=1)          # a single slot is fine without a backward
    out = one(feats, torch.tensor([2, 5], device="cuda"))
    assert out.shape == (1, 1, 2, 15)


@pytest.mark.parametrize("graph_slots", [None, 4])
def test_mask_generator_with_batched_baselines(graph_slots):
    """``MaskGenerator(batch_baselines=True).get_masks`` against the default (per-query) route: masks differ in fewer than 1 % of the
    pixels per kept query (rounding at the Otsu edge, the allowance of ``test_detr_mask_generator_r50_shape``)."""
    from transformer_mm_explainability_amd.detr_explainability import MaskGenerator
    g = _golden()
    model, feats = _detr_from_golden(g), cu(g["features"])
    with torch.no_grad():
        conf = model(feats)["pred_logits"].softmax(-1)[0, :, :-1].max(-1).values.sort().values
    th = float((conf[-6] + conf[-5]) / 2)                               # five kept queries: more than the four slots
    ref = MaskGenerator(model, threshold=th)
    new = MaskGenerator(model, threshold=th, graph_slots=graph_slots, batch_baselines=True)
    for method in METHODS:
        want, keep_w = ref.get_masks(feats, method)
        got, keep_g = new.get_masks(feats, method)
        assert torch.equal(keep_w, keep_g) and int(keep_w.sum()) == 5 and got.shape == want.shape
        assert bool((got[0, ~keep_g] == -1).all())
        for q in torch.nonzero(keep_w).reshape(-1).tolist():
            share = float((got[0, q] != want[0, q]).float().mean())
            print("%s query %d: %.4f of the pixels differ" % (method, q, share))
            assert share < 0.01, "%s query %d: %.3f of the mask pixels differ" % (method, q, share)
    if graph_slots:
        assert sorted(k[0] for k in new._graphs) == sorted(METHODS)
    # an LRP baseline stays on the per-query route
    want, _ = ref.get_masks(feats, "partial_lrp")
    got, _ = new.get_masks(feats, "partial_lrp")
    assert got.shape == want.shape and float((got != want).float().mean()) < 0.01
