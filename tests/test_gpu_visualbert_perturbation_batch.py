"""-m gpu: ``VisualBertPerturbation.perturbation_image_batch`` / ``perturbation_text_batch`` (B padded items, all steps, one packed pass)
== the per-item ``perturbation_image`` / ``perturbation_text`` on every item trimmed through ``unpad_row``, to the tolerance
``tests/test_gpu_perturbation.py`` uses for batched-vs-sequential scores (``rtol = 1e-4, atol = 1e-5``); the reference evaluator's own
scores (``tests/golden/visualbert_perturbation.npz``) from ONE batch; the hipGraph replay; and that a batched call leaves the capture
slabs of an earlier explain pass alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-5)


def _tiny_visualbert():
    """The tiny model of ``tests/test_gpu_perturbation.py::_visualbert_and_sample``: hidden 96, 4 heads, 3 layers, weights x 3."""
    from transformer_mm_explainability_amd import visualbert_model as vm
    torch.manual_seed(9)
    cfg = vm.VisualBertConfig(hidden_size=96, num_attention_heads=4, intermediate_size=192, num_hidden_layers=3,
                              vocab_size=300, max_position_embeddings=64, visual_embedding_dim=40, num_labels=23)
    model = vm.VisualBERT(cfg).cuda().eval()
    with torch.no_grad():                                     # default init leaves the scores nearly flat
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(3.0)
    return model


def _ragged_batch(g, lens, T, V, vocab=300, dim=40):
    B = len(lens)
    ids = torch.zeros(B, T, dtype=torch.long)
    mask = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, vocab, (n,), generator=g)
        mask[b, :n] = 1
    return {"input_ids": ids.cuda(), "input_mask": mask.cuda(), "segment_ids": torch.zeros(B, T, dtype=torch.long).cuda(),
            "image_feature_0": torch.randn(B, V, dim, generator=g).cuda()}


def _item(batch, b):
    """Item b of a padded batch as the per-item methods take it (``[1, T]``, padding allowed: they trim by the mask sum)."""
    return {k: v[b:b + 1].clone() for k, v in batch.items()}


def _generated_cams(model, batch, lens):
    """Every item's own ``generate_ours`` row, in the padded layout."""
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    gen = vb.SelfAttentionGenerator(model)
    rows = [gen.generate_ours(_item(batch, b)).detach() for b in range(len(lens))]
    return vb.pad_rows(rows, lens, batch["input_mask"].shape[1])


def _per_item(pert, batch, cams, lens, modality, positive):
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    T = batch["input_mask"].shape[1]
    run = pert.perturbation_image if modality == "image" else pert.perturbation_text
    return torch.stack([run(_item(batch, b), vb.unpad_row(cams, b, n, padded_text=T), positive) for b, n in enumerate(lens)])


@pytest.fixture(scope="module")
def ragged():
    """B = 5 items of 3, 5, 9, 12, 16 tokens at T = 16, V = 14, their cams, and the per-item scores of both tests and signs (computed
    once; the tests only read them)."""
    from transformer_mm_explainability_amd import visualbert_perturbation as vp
    model = _tiny_visualbert()
    lens, T, V = [3, 5, 9, 12, 16], 16, 14
    batch = _ragged_batch(torch.Generator().manual_seed(10), lens, T, V)
    cams = _generated_cams(model, batch, lens)
    pert = vp.VisualBertPerturbation(model)
    want = {(m, p): _per_item(pert, batch, cams, lens, m, p) for m in ("image", "text") for p in (False, True)}
    return model, pert, batch, cams, lens, want


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("modality", ["image", "text"])
def test_batch_equals_per_item(ragged, modality, positive):
    model, pert, batch, cams, lens, want = ragged
    run = pert.perturbation_image_batch if modality == "image" else pert.perturbation_text_batch
    got = run(batch, cams, positive)
    assert got.shape == (5, 9, 23)
    ref = want[(modality, positive)]
    print("%s positive=%s: max |batch - per item| = %.3e, max |per item| = %.3e"
          % (modality, positive, float((got - ref).abs().max()), float(ref.abs().max())))
    torch.testing.assert_close(got, ref, **TOL)
    assert torch.equal(got.argmax(dim=-1), ref.argmax(dim=-1))
    assert not torch.allclose(got[:, 0], got[:, -1], atol=1e-3)           # the perturbation does change the answer scores


def test_steps_with_one_keep_count_come_back_bit_equal(ragged):
    """V = 14: steps 3 .. 8 of the image test keep no region, one group computes them."""
    _model, pert, batch, cams, _lens, _want = ragged
    got = pert.perturbation_image_batch(batch, cams)
    for s in range(4, 9):
        assert torch.equal(got[:, s], got[:, 3])
    assert not torch.equal(got[:, 2], got[:, 3])


def test_batched_accuracy_and_refusals(ragged):
    _model, pert, batch, cams, _lens, _want = ragged
    got = pert.perturbation_text_batch(batch, cams)
    targets = torch.rand(5, 23, device="cuda")
    acc = pert.accuracy(got, targets)
    assert acc.shape == (5, 9)
    for b in range(5):
        assert torch.equal(acc[b], pert.accuracy(got[b], targets[b]))
    with pytest.raises(NotImplementedError, match="image_dim"):
        pert.perturbation_image_batch(dict(batch, image_dim=torch.full((5,), 14, device="cuda")), cams)
    with pytest.raises(ValueError, match="padded layout"):
        pert.perturbation_text_batch(batch, cams[:, :-1])


def test_wide_batch_takes_the_one_sweep_attention_with_a_padded_text_mask():
    """T = 24, V = 110: N = 134 > 128 keys, so ``attn_fwd`` runs its one-sweep kernel, with -10000 at the padded text keys."""
    from transformer_mm_explainability_amd import visualbert_perturbation as vp
    model = _tiny_visualbert()
    lens, T, V = [24, 7, 3], 24, 110
    g = torch.Generator().manual_seed(12)
    batch = _ragged_batch(g, lens, T, V)
    cams = torch.rand(3, T + V, generator=g).cuda()
    for b, n in enumerate(lens):
        cams[b, n:T] = 0
    pert = vp.VisualBertPerturbation(model)
    for modality, run in (("image", pert.perturbation_image_batch), ("text", pert.perturbation_text_batch)):
        for positive in (False, True):
            got, ref = run(batch, cams, positive), _per_item(pert, batch, cams, lens, modality, positive)
            print("wide %s positive=%s: max |batch - per item| = %.3e" % (modality, positive, float((got - ref).abs().max())))
            torch.testing.assert_close(got, ref, **TOL)


def _cu(x):
    return torch.from_numpy(np.asarray(x)).cuda()


@pytest.fixture(scope="module")
def golden_batch(golden):
    """The three golden items plus one shorter made-up item in ONE batch whose text width is 3 wider than theirs, with every item's
    ``generate_ours`` cam."""
    from transformer_mm_explainability_amd import visualbert_model as vm
    gm, g = golden("visualbert_model"), golden("visualbert_perturbation")
    hidden, heads, inter, layers, vocab, max_pos, vdim, labels = (int(x) for x in gm["dims"])
    model = vm.VisualBERT(vm.VisualBertConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter,
                                              num_hidden_layers=layers, vocab_size=vocab, max_position_embeddings=max_pos,
                                              visual_embedding_dim=vdim, num_labels=labels))
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in gm.items() if k.startswith("w__")}, strict=False)
    model = model.cuda().eval()
    wide = gm["input_ids"].shape[1] + 3
    n_golden, V = int(gm["input_mask"].sum()), gm["image_feature_0"].shape[1]
    lens = [n_golden] * 3 + [5]
    gen = torch.Generator().manual_seed(13)
    ids = torch.zeros(4, wide, dtype=torch.long)
    ids[:3, :gm["input_ids"].shape[1]] = torch.from_numpy(gm["input_ids"]).long()
    ids[3, :5] = torch.randint(1, vocab, (5,), generator=gen)
    mask = torch.zeros(4, wide, dtype=torch.long)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    feats = torch.cat((torch.from_numpy(gm["image_feature_0"]), torch.from_numpy(g["image_features_1_2"]),
                       torch.randn(1, V, vdim, generator=gen)), dim=0)
    batch = {"input_ids": ids.cuda(), "input_mask": mask.cuda(), "segment_ids": torch.zeros(4, wide, dtype=torch.long).cuda(),
             "image_feature_0": feats.float().cuda()}
    return model, batch, _generated_cams(model, batch, lens), g


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("modality", ["image", "text"])
def test_one_batch_reproduces_the_reference_evaluator(golden_batch, modality, positive):
    """``scores_<tag>[i]`` of all 3 x 9 re-runs of the reference loop, and the step accuracies it PRINTS (three items evaluated,
    divided by ``num_samples = 2``: its ``i > num_samples`` accounting, ``evaluation_loop(reference_exact=True)``)."""
    from transformer_mm_explainability_amd import visualbert_perturbation as vp
    model, batch, cams, g = golden_batch
    pert = vp.VisualBertPerturbation(model)
    tag = "%s_%s" % (modality, "pos" if positive else "neg")
    run = pert.perturbation_image_batch if modality == "image" else pert.perturbation_text_batch
    scores = run(batch, cams, positive)
    assert scores.shape == (4, 9, g["targets"].shape[1])
    torch.testing.assert_close(scores[:3].cpu(), torch.from_numpy(g["scores_" + tag]), **TOL)
    acc = pert.accuracy(scores[:3], _cu(g["targets"]).expand(3, -1))
    printed = acc.double().sum(dim=0).cpu() / 2 * 100
    torch.testing.assert_close(printed, torch.from_numpy(g["printed_step_acc_" + tag]).double(), rtol=0, atol=1e-4)


@pytest.mark.parametrize("modality", ["image", "text"])
def test_graph_replays_any_ragged_batch_of_the_captured_shape(modality):
    """The capture succeeds (no host read is left in the pass); a replay is bit-equal to the eager call, also on a second batch with
    other lengths, ids, features and cams copied in (no recapture) and back on the first."""
    from transformer_mm_explainability_amd import visualbert_perturbation as vp
    model = _tiny_visualbert()
    T, V = 16, 14
    g = torch.Generator().manual_seed(14)
    pert = vp.VisualBertPerturbation(model)
    eager = pert.perturbation_image_batch if modality == "image" else pert.perturbation_text_batch
    first = _ragged_batch(g, [16, 4, 9, 12], T, V)
    cams = torch.rand(4, T + V, generator=g).cuda()
    run = vp.GraphedVisualBertPerturbation(pert, first, cams, modality, is_positive_pert=True)
    want = eager(first, cams, True).clone()
    assert torch.equal(run(first, cams), want)
    second = _ragged_batch(g, [3, 16, 7, 5], T, V)
    cams2 = torch.rand(4, T + V, generator=g).cuda()
    want2 = eager(second, cams2, True).clone()
    assert not torch.allclose(want2, want, atol=1e-3)
    assert torch.equal(run(second, cams2), want2)                         # nothing of the captured batch is left in the replay
    assert torch.equal(run(first, cams), want)                            # ... in either direction
    with pytest.raises(ValueError, match="captured"):
        run(_ragged_batch(g, [5, 5, 5], T, V), cams2[:3])
    with pytest.raises(ValueError, match="modality"):
        vp.GraphedVisualBertPerturbation(pert, first, cams, "audio")


def test_batched_calls_leave_the_capture_slabs_alone(ragged):
    """``scores_packed`` writes no probability slab: after an explain pass, the slabs ``get_attn()`` hands out keep their address and
    their contents through both batch methods (the per-item route rewrites them nine sequences at a time)."""
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    model, pert, batch, cams, _lens, _want = ragged
    vb.SelfAttentionGenerator(model).generate_ours(_item(batch, 3))
    blocks = [blk.attention.self for blk in model.model.bert.encoder.layer]
    before = [(sa.get_attn().data_ptr(), sa.get_attn().clone(), sa.get_attn_gradients().data_ptr()) for sa in blocks]
    pert.perturbation_image_batch(batch, cams)
    pert.perturbation_text_batch(batch, cams, True)
    torch.cuda.synchronize()
    for sa, (where, probs, grads_where) in zip(blocks, before):
        assert sa.get_attn().data_ptr() == where and sa.get_attn_gradients().data_ptr() == grads_where
        assert torch.equal(sa.get_attn(), probs)
