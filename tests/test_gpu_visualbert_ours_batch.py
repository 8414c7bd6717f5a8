"""-m gpu: ``SelfAttentionGenerator.generate_ours_padded_batch``, ``unpad_row`` and ``GraphedGenerateOursPadded`` on real bodies: the
reference's own golden row inside a padded batch, a padded batch of ragged questions == every item explained alone by
``generate_ours`` (tape and hook routes, arg-max and named answers), ``image_dim``, the size limit, graph replays of ragged batches,
and the evaluator's ``--explain-batch`` for ``ours_no_lrp``."""
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(batch, b):
    return {k: v[b:b + 1].clone() for k, v in batch.items()}


def _golden_body(g):
    from transformer_mm_explainability_amd import visualbert_model as vm
    hidden, heads, inter, layers, vocab, max_pos, vdim, labels = (int(x) for x in g["dims"])
    model = vm.VisualBERT(vm.VisualBertConfig(hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter,
                                              num_hidden_layers=layers, vocab_size=vocab, max_position_embeddings=max_pos,
                                              visual_embedding_dim=vdim, num_labels=labels))
    weights = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w__")}
    missing, unexpected = model.load_state_dict(weights, strict=False)
    assert not unexpected and all(m.startswith("model.bert.pooler.") for m in missing), (missing, unexpected)
    return model.cuda().eval(), vocab


@pytest.mark.parametrize("position", [0, 2])
def test_reference_golden_inside_a_padded_batch(golden, position):
    """The item of ``tests/golden/visualbert_model.npz`` (8 live of 12 text positions; ``out`` made by the reference's own
    ``SelfAttentionGenerator.generate_ours``) batched with two random questions of 12 and 5 tokens: ``unpad_row`` of its sample
    reproduces ``out`` on the tolerance ``tests/test_gpu_generators.py`` applies to the per-item call (``parity.close`` defaults),
    wherever it sits in the batch."""
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    g = golden("visualbert_model")
    model, vocab = _golden_body(g)
    T, V = g["input_ids"].shape[1], g["image_feature_0"].shape[1]
    n = int(g["input_mask"].sum())
    assert (T, n) == (12, 8)
    rng = torch.Generator().manual_seed(11)
    where = [position] + [b for b in range(3) if b != position]            # batch slots of: the golden item, the 12-, the 5-token one
    lens = [0, 0, 0]
    ids, mask = torch.zeros(3, T, dtype=torch.long), torch.zeros(3, T, dtype=torch.long)
    feats = torch.randn(3, V, g["image_feature_0"].shape[2], generator=rng)
    for slot, length in zip(where, (n, 12, 5)):
        lens[slot] = length
        ids[slot, :length] = torch.randint(1, vocab, (length,), generator=rng)
        mask[slot, :length] = 1
    ids[position], feats[position] = torch.from_numpy(g["input_ids"][0]), torch.from_numpy(g["image_feature_0"][0])
    assert torch.equal(mask[position], torch.from_numpy(g["input_mask"][0]))
    batch = {"input_ids": ids.cuda(), "input_mask": mask.cuda(), "segment_ids": torch.zeros_like(ids).cuda(),
             "image_feature_0": feats.cuda()}
    scores = vb.SelfAttentionGenerator(model).generate_ours_padded_batch(batch)
    assert scores.shape == (3, T + V) and bool(torch.isfinite(scores).all())
    parity.close(vb.unpad_row(scores, position, n, padded_text=T), g["out"], what="generate_ours_padded_batch")
    for b in range(3):
        assert not bool(scores[b, lens[b]:T].any()) and float(scores[b, lens[b] - 2]) == 0.0
        assert float(scores[b].abs().max()) > 0


def _small_body():
    from transformer_mm_explainability_amd import visualbert_model as vm
    torch.manual_seed(5)
    model = vm.VisualBERT(vm.VisualBertConfig(hidden_size=64, num_attention_heads=4, intermediate_size=128, num_hidden_layers=2,
                                              vocab_size=120, max_position_embeddings=32, visual_embedding_dim=24, num_labels=13))
    with torch.no_grad():
        for p in model.parameters():
            if p.dim() > 1:
                p.mul_(3.0)
    return model.cuda().eval()


T_SMALL, V_SMALL = 16, 52                       # N = 68 crosses 64


def _small_batch(lens, seed=3):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    ids, mask = torch.zeros(B, T_SMALL, dtype=torch.long), torch.zeros(B, T_SMALL, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, 120, (n,), generator=g)
        mask[b, :n] = 1
    return {"input_ids": ids.cuda(), "input_mask": mask.cuda(), "segment_ids": torch.zeros_like(ids).cuda(),
            "image_feature_0": torch.randn(B, V_SMALL, 24, generator=g).cuda()}


def _assert_rows_equal_per_item(model, batch, lens, scores, index=None):
    """Row b == ``generate_ours`` of item b alone, on ``parity.close``'s defaults scaled by ``max|per-item row|`` (the tolerance
    ``tests/test_gpu_visualbert_baselines_batch.py`` applies to the baselines)."""
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    assert scores.shape == (len(lens), T_SMALL + V_SMALL)
    for b, n in enumerate(lens):
        want = vb.SelfAttentionGenerator(model).generate_ours(_one(batch, b), index=None if index is None else [int(index[b])]).detach()
        assert want.shape == (1, n + V_SMALL)
        scale = float(want.abs().max())
        assert scale > 0 and bool(torch.isfinite(want).all())
        got = vb.unpad_row(scores, b, n, padded_text=T_SMALL)
        parity.close(got / scale, (want / scale).cpu().numpy(), what="ours sample %d (rows divided by max|per-item row| = %.3e)"
                     % (b, scale))
        assert not bool(scores[b, n:T_SMALL].any()) and float(scores[b, n - 2]) == 0.0


def _argmax_answers(model, batch):
    B = batch["input_ids"].shape[0]
    with torch.no_grad():
        ones = torch.ones(B, V_SMALL, dtype=torch.long, device="cuda")
        return model.model(batch["input_ids"], batch["input_mask"], torch.cat((batch["input_mask"], ones), dim=-1),
                           batch["segment_ids"], batch["image_feature_0"], torch.zeros_like(ones))["scores"].argmax(dim=-1)


@pytest.mark.parametrize("route", ["tape", "hook"])
def test_padded_batch_equals_every_item_explained_alone(route):
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    model = _small_body()
    assert hasattr(model.model, "forward_tape")
    lens = [3, 16, 9, 12]
    batch = _small_batch(lens)
    gen = vb.SelfAttentionGenerator(model)
    gen.use_tape = route == "tape"
    scores = gen.generate_ours_padded_batch(batch).clone()
    _assert_rows_equal_per_item(model, batch, lens, scores)
    best = _argmax_answers(model, batch)
    assert torch.equal(gen.generate_ours_padded_batch(batch, index=best), scores)
    other = (best + 1) % 13
    named = gen.generate_ours_padded_batch(batch, index=other).clone()
    assert not torch.equal(named, scores)
    _assert_rows_equal_per_item(model, batch, lens, named, index=other)
    if route == "hook":
        assert all(p.grad is None for p in model.parameters())      # the hook route's backward forms no weight gradients


def test_equal_length_and_ragged_routes_are_both_there():
    """``generate_ours_batch`` keeps refusing ragged input; on items of EQUAL length both batched routes give the per-item rows."""
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    model = _small_body()
    gen = vb.SelfAttentionGenerator(model)
    with pytest.raises(ValueError, match="bucket them"):
        gen.generate_ours_batch(_small_batch([3, 16, 9, 12]))
    lens = [9, 9, 9]
    batch = _small_batch(lens, seed=8)
    _assert_rows_equal_per_item(model, batch, lens, gen.generate_ours_padded_batch(batch).clone())
    trimmed = gen.generate_ours_batch(batch)                        # [B, 9 + V]: the text padding trimmed away
    padded = gen.generate_ours_padded_batch(batch)
    for b in range(3):
        scale = float(trimmed[b].abs().max())
        parity.close(vb.unpad_row(padded, b, 9, padded_text=T_SMALL) / scale, (trimmed[b:b + 1] / scale).cpu().numpy(),
                     what="padded vs trimmed route, sample %d" % b)


def test_image_dim_masks_the_trailing_regions():
    """``image_dim``: sample b sees its first ``image_dim[b]`` regions only -- the rows equal those of a batch whose other regions
    hold other features, and are zero there."""
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    model = _small_body()
    lens, dims = [3, 16, 9, 12], torch.tensor([52, 7, 30, 1], device="cuda")
    batch = dict(_small_batch(lens), image_dim=dims)
    other = dict(batch)
    other["image_feature_0"] = batch["image_feature_0"].clone()
    for b in range(4):
        other["image_feature_0"][b, int(dims[b]):] = 9.0
    gen = vb.SelfAttentionGenerator(model)
    a = gen.generate_ours_padded_batch(batch).clone()
    assert torch.equal(a, gen.generate_ours_padded_batch(other))
    plain = gen.generate_ours_padded_batch(_small_batch(lens))
    assert not torch.equal(a[1], plain[1])                          # sample 1 sees 7 of its 52 regions
    for b in range(4):
        assert not bool(a[b, T_SMALL + int(dims[b]):].any()) and float(a[b].abs().max()) > 0


def test_sizes_above_the_kernel_limit_are_refused():
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    gen = vb.SelfAttentionGenerator(_small_body())
    batch = _small_batch([5, 9])
    batch["image_feature_0"] = torch.zeros(2, 241, 24, device="cuda")
    with pytest.raises(NotImplementedError):
        gen.generate_ours_padded_batch(batch)


def test_graphed_ours_padded_replays_any_lengths():
    """ONE captured graph serves batches of other lengths (and other answers) copied into it, bit-equal to the eager batched call."""
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    model = _small_body()
    run = vb.GraphedGenerateOursPadded(model, _small_batch([16, 16, 16, 16]))
    gen = vb.SelfAttentionGenerator(model)
    for lens, seed in (([16, 16, 16, 16], 3), ([6, 11, 3, 14], 4), ([16, 2, 9, 5], 6)):
        batch = _small_batch(lens, seed=seed)
        want = gen.generate_ours_padded_batch(batch).clone()
        got = run(batch)
        assert torch.equal(got, want), lens
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
    with pytest.raises(ValueError, match="captured"):
        run({k: v[:3] for k, v in batch.items()})
    with pytest.raises(ValueError, match="index=None"):
        run(batch, index=[1, 2, 3, 4])
    with pytest.raises(ValueError, match="method"):
        vb.GraphedBaselinesBatch(model, batch, "ours")              # the baselines' wrapper keeps its three methods
    dims = torch.tensor([52, 7, 30, 1], device="cuda")
    named = vb.GraphedGenerateOursPadded(model, dict(_small_batch([16, 16, 16, 16]), image_dim=torch.full_like(dims, 52)),
                                         index=[0, 0, 0, 0])
    batch = dict(_small_batch([6, 11, 3, 14], seed=4), image_dim=dims)
    answers = torch.tensor([1, 5, 12, 0], device="cuda")
    assert torch.equal(named(batch, index=answers), gen.generate_ours_padded_batch(batch, index=answers))
    with pytest.raises(KeyError):
        named(_small_batch([6, 11, 3, 14], seed=4))                 # captured with image_dim: the replay needs one


def test_evaluator_explain_batch_prints_the_same_accuracies():
    """``examples/visualbert_pert_eval.py --method ours_no_lrp``: ``--explain-batch 4`` and ``--explain-batch 1`` print the same
    samples, keys and ``step_accuracy_percent`` (each run a fresh child process under its own time limit)."""
    printed = []
    for explain in ("4", "1"):
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "visualbert_pert_eval.py"), "--method",
               "ours_no_lrp", "--explain-batch", explain, "--num-samples", "8"]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        printed.append(json.loads(res.stdout.strip().splitlines()[-1]))
    assert printed[0]["samples"] == printed[1]["samples"] == 8
    assert printed[0]["step_accuracy_percent"] == printed[1]["step_accuracy_percent"]
    assert set(printed[0]) == set(printed[1])
