"""-m gpu: the batched baselines of ``GeneratorBaselines`` (``generate_rollout_batch`` / ``generate_raw_attn_batch`` /
``generate_attn_gradcam_batch``) and ``GraphedBaselinesBatch`` on real bodies: a padded batch of ragged questions == every item
explained alone and unpadded by the per-item methods (the way the reference's evaluator calls them, lxmert/lxmert/perturbation.py:216-245),
the reference's own goldens, a body with one x-layer, the hook route, and graph replays."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402
import test_gpu_perturbation as tp  # noqa: E402  (the tiny body and its ragged batches)

pytestmark = pytest.mark.gpu
METHODS = ("rollout", "raw_attn", "attn_gradcam")
TEXT_KEYS = ("input_ids", "attention_mask", "token_type_ids")


def _batch_call(gen, method, batch, index=None):
    if method == "attn_gradcam":
        return gen.generate_attn_gradcam_batch(batch, index)
    return getattr(gen, "generate_%s_batch" % method)(batch)


def _item_call(gen, method, index=None):
    if method == "attn_gradcam":
        return gen.generate_attn_gradcam(None, index=index)
    return getattr(gen, "generate_" + method)(None)


def _one(batch, b, n):
    return {k: v[b:b + 1, :n] if k in TEXT_KEYS else v[b:b + 1] for k, v in batch.items()}


def _assert_equals_per_item(model, batch, lens, method, got, R_ii=None, I=20):
    from transformer_mm_explainability_amd import lxmert_explainability as le
    R_t_t, R_t_i = got
    T = batch["input_ids"].shape[1]
    assert R_t_t.shape == (len(lens), T, T) and R_t_i.shape == (len(lens), T, I)
    for b, n in enumerate(lens):
        one = _one(batch, b, n)
        usage = types.SimpleNamespace(model=model, text_len=n, image_boxes_len=I, forward=lambda item: model(**one))
        base = le.GeneratorBaselines(usage)
        want_tt, want_ti = _item_call(base, method)
        torch.testing.assert_close(R_t_t[b, :n, :n], want_tt, rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(R_t_i[b, :n], want_ti, rtol=1e-4, atol=1e-5)
        if R_ii is not None:
            torch.testing.assert_close(R_ii[b], base.R_i_i, rtol=1e-4, atol=1e-5)
        assert (R_t_t[b, n:] == 0).all() and (R_t_t[b, :, n:] == 0).all() and (R_t_i[b, n:] == 0).all()
        assert R_t_t[b, 0, 0] == 0
    assert R_t_t.abs().max() > 0 and R_t_i.abs().max() > 0                      # (GradCAM may clamp one sample's map away, not all)


@pytest.mark.parametrize("method", METHODS)
def test_padded_batch_equals_every_item_explained_alone(method):
    """A batch padded to T = 12 with questions of 5 / 12 / 8 / 9 tokens == each item explained alone, unpadded, by the existing
    per-item method; zeros beyond each length."""
    from transformer_mm_explainability_amd import lxmert_explainability as le
    model, _, g = tp._model_and_inputs()
    lens = [5, 12, 8, 9]
    batch = tp._ragged_batch(g, lens)
    gen = le.GeneratorBaselines(types.SimpleNamespace(model=model))
    got = tuple(t.clone() for t in _batch_call(gen, method, batch))
    _assert_equals_per_item(model, batch, lens, method, got, R_ii=gen.R_i_i.clone() if method == "rollout" else None)


def _golden_body(g):
    from transformer_mm_explainability_amd import lxmert_model as lm
    hidden, heads, inter, ll, xl, rl, feat, vocab, labels, max_pos, T, I = (int(x) for x in g["dims"])
    cfg = lm.LxmertConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter, l_layers=ll, x_layers=xl,
                          r_layers=rl, visual_feat_dim=feat, vocab_size=vocab, num_qa_labels=labels,
                          max_position_embeddings=max_pos)
    model = lm.LxmertForQuestionAnswering(cfg)
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w__")}, strict=True)
    return model.cuda().eval(), (T, I, feat, vocab)


def test_reference_goldens_inside_a_padded_batch(golden):
    """The item of ``tests/golden/lxmert_model.npz`` (maps made by the reference's own ``GeneratorBaselines``), padded by three tokens
    and batched with two random items, reproduces ``rollout_*`` / ``raw_*`` / ``gradcam_*`` (GradCAM with the golden's answer)."""
    from transformer_mm_explainability_amd import lxmert_explainability as le
    g = golden("lxmert_model")
    model, (T, I, feat, vocab) = _golden_body(g)
    rng = torch.Generator().manual_seed(11)
    P, lens = T + 3, [T, T + 3, T - 2]
    ids, mask = torch.zeros(3, P, dtype=torch.long), torch.zeros(3, P)
    ids[0, :T] = torch.from_numpy(g["in__input_ids"][0])
    for b in (1, 2):
        ids[b, :lens[b]] = torch.randint(1, vocab, (lens[b],), generator=rng)
    for b in range(3):
        mask[b, :lens[b]] = 1
    feats, pos = torch.randn(3, I, feat, generator=rng), torch.rand(3, I, 4, generator=rng)
    feats[0], pos[0] = torch.from_numpy(g["in__visual_feats"][0]), torch.from_numpy(g["in__visual_pos"][0])
    batch = dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), token_type_ids=torch.zeros(3, P, dtype=torch.long).cuda(),
                 visual_feats=feats.cuda(), visual_pos=pos.cuda())
    answer = int(np.argmax(g["score"][0]))
    gen = le.GeneratorBaselines(types.SimpleNamespace(model=model))
    for method, tag in (("rollout", "rollout"), ("raw_attn", "raw"), ("attn_gradcam", "gradcam")):
        R_t_t, R_t_i = _batch_call(gen, method, batch, index=[answer, 0, 1])
        parity.close(R_t_t[0, :T, :T], g[tag + "_R_t_t"], atol=1e-5, rtol=0, what=tag + " R_t_t")
        parity.close(R_t_i[0, :T], g[tag + "_R_t_i"], atol=1e-5, rtol=0, what=tag + " R_t_i")
        assert (R_t_t[0, T:] == 0).all() and (R_t_t[0, :, T:] == 0).all() and (R_t_i[0, T:] == 0).all()


def _one_x_layer_body():
    from transformer_mm_explainability_amd import lxmert_model as lm
    torch.manual_seed(7)
    cfg = lm.LxmertConfig(hidden_size=96, num_attention_heads=4, intermediate_size=192, l_layers=2, x_layers=1, r_layers=2,
                          visual_feat_dim=40, vocab_size=200, num_qa_labels=31, max_position_embeddings=64)
    model = lm.LxmertForQuestionAnswering(cfg).cuda().eval()
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(3.0)
    return model


@pytest.mark.parametrize("method", METHODS)
def test_a_body_with_one_x_layer(method):
    """``x_layers = 1``: the image table is ``r_layers`` alone and the text table ends right after the language layers."""
    from transformer_mm_explainability_amd import lxmert_explainability as le
    model = _one_x_layer_body()
    lens = [7, 12, 3]
    batch = tp._ragged_batch(torch.Generator().manual_seed(8), lens)
    gen = le.GeneratorBaselines(types.SimpleNamespace(model=model))
    got = tuple(t.clone() for t in _batch_call(gen, method, batch))
    _assert_equals_per_item(model, batch, lens, method, got)


@pytest.mark.parametrize("method", METHODS)
def test_hook_route_equals_tape_route(method):
    from transformer_mm_explainability_amd import lxmert_explainability as le
    model, _, g = tp._model_and_inputs()
    assert hasattr(model, "forward_tape")
    batch = tp._ragged_batch(g, [5, 12, 8, 9])
    gen = le.GeneratorBaselines(types.SimpleNamespace(model=model))
    tape = tuple(t.clone() for t in _batch_call(gen, method, batch))
    gen.use_tape = False
    hook = _batch_call(gen, method, batch)
    for a, b in zip(hook, tape):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
    assert all(p.grad is None for p in model.parameters())          # the hook route's backward forms no weight gradients


def test_sizes_above_the_kernel_limit_are_refused():
    from transformer_mm_explainability_amd import lxmert_explainability as le
    model, _, g = tp._model_and_inputs()
    gen = le.GeneratorBaselines(types.SimpleNamespace(model=model))
    batch = tp._ragged_batch(g, [49, 20], T=49)
    for method in METHODS:
        with pytest.raises(NotImplementedError):
            _batch_call(gen, method, batch)


@pytest.mark.parametrize("method", METHODS)
def test_graphed_baselines_replay_any_lengths(method):
    """ONE captured graph (padded length 12) serves batches of different question lengths, bit-equal to eager calls on the same
    inputs; its outputs feed the evaluator's next steps."""
    from transformer_mm_explainability_amd import lxmert_explainability as le
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    model, _, g = tp._model_and_inputs()
    run = le.GraphedBaselinesBatch(model, tp._ragged_batch(g, [12, 12, 12, 12]), method)
    gen = le.GeneratorBaselines(types.SimpleNamespace(model=model))
    pert = lp.LxmertPerturbation(model)
    for lens in ([12, 12, 12, 12], [6, 11, 9, 7]):
        batch = tp._ragged_batch(g, lens)
        want = tuple(t.clone() for t in _batch_call(gen, method, batch))
        got = run(batch)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        if method == "rollout":
            assert torch.equal(run.R_i_i, gen.R_i_i)
        cam_image, cam_text = lp.normalize_cams_batch(got[0], got[1], batch["attention_mask"])
        assert cam_image.shape == (4, 20) and cam_text.shape == (4, 12)
        img = pert.perturbation_image(batch, cam_image)
        txt = pert.perturbation_text(batch, cam_text)
        assert img.shape == txt.shape == (4, 9, 31)
        assert torch.isfinite(img).all() and torch.isfinite(txt).all()
    with pytest.raises(ValueError, match="captured"):
        run(tp._ragged_batch(g, [5, 5, 5], T=12))
    with pytest.raises(ValueError, match="method"):
        le.GraphedBaselinesBatch(model, batch, "ours")
