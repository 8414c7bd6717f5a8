"""-m gpu: the batched baselines of ``SelfAttentionGenerator`` (``generate_rollout_batch`` / ``generate_raw_attn_batch`` /
``generate_attn_gradcam_batch``), ``unpad_row`` and ``GraphedBaselinesBatch`` on real bodies: the reference's own goldens inside a
padded batch, a padded batch of ragged questions == every item explained alone by the per-item methods (tape and hook routes),
graph replays, and the evaluator's ``--explain-batch``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("rollout", "raw_attn", "attn_gradcam")
GOLDEN_KEY = {"rollout": "rollout_out", "raw_attn": "raw_attn_out", "attn_gradcam": "gradcam_out"}


def _batch_call(gen, method, batch, index=None, start_layer=0):
    if method == "attn_gradcam":
        return gen.generate_attn_gradcam_batch(batch, index)
    if method == "rollout":
        return gen.generate_rollout_batch(batch, start_layer=start_layer)
    return gen.generate_raw_attn_batch(batch)


def _item_call(gen, method, item, index=None, start_layer=0):
    if method == "attn_gradcam":
        return gen.generate_attn_gradcam(item, index=index)
    if method == "rollout":
        return gen.generate_rollout(item, start_layer=start_layer)
    return gen.generate_raw_attn(item)


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
def test_reference_goldens_inside_a_padded_batch(golden, position):
    """The item of ``tests/golden/visualbert_model.npz`` (8 live of 12 text positions; maps made by the reference's own
    ``SelfAttentionGenerator``) batched with two random questions of 12 and 5 tokens: ``unpad_row`` of its sample reproduces
    ``rollout_out`` / ``raw_attn_out`` / ``gradcam_out`` on the tolerance ``tests/test_gpu_generators.py`` applies to the per-item
    calls (``parity.close`` defaults), wherever it sits in the batch.  For GradCAM the golden pins the NaN pattern only: the item's
    whole cam is clamped, so ``gradcam_out`` is NaN everywhere off ``c_b`` (``mx == mn``); GradCAM VALUES at generator level are
    pinned by ``test_padded_batch_equals_every_item_explained_alone``."""
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
    gen = vb.SelfAttentionGenerator(model)
    for method in METHODS:
        scores = _batch_call(gen, method, batch)
        assert scores.shape == (3, T + V)
        parity.close(vb.unpad_row(scores, position, n, padded_text=T), g[GOLDEN_KEY[method]], what=method)
        for b in range(3):
            assert not bool(torch.nan_to_num(scores[b, lens[b]:T], nan=1.0).any()) and float(scores[b, lens[b] - 2]) == 0.0


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


def _assert_rows_equal_per_item(model, batch, lens, method, scores, index=None, start_layer=0):
    """Row b == the per-item method on item b alone, on ``parity.close``'s defaults scaled by ``max|per-item row|``."""
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    assert scores.shape == (len(lens), T_SMALL + V_SMALL)
    for b, n in enumerate(lens):
        want = _item_call(vb.SelfAttentionGenerator(model), method, _one(batch, b), None if index is None else [int(index[b])],
                          start_layer).detach()
        assert want.shape == (1, n + V_SMALL)
        fin = torch.isfinite(want)
        scale = float(want[fin].abs().max()) if bool(fin.any()) else 0.0
        scale = scale if scale > 0 else 1.0              # (an all-clamped GradCAM item: NaN off its own column, nothing to scale by)
        got = vb.unpad_row(scores, b, n, padded_text=T_SMALL)
        parity.close(got / scale, (want / scale).cpu().numpy(), what="%s sample %d (rows divided by max|per-item row| = %.3e)"
                     % (method, b, scale))
        assert not bool(scores[b, n:T_SMALL].any()) and float(scores[b, n - 2]) == 0.0
    assert bool(torch.isfinite(scores).any()) and float(torch.nan_to_num(scores).abs().max()) > 0


@pytest.mark.parametrize("route", ["tape", "hook"])
@pytest.mark.parametrize("method", METHODS)
def test_padded_batch_equals_every_item_explained_alone(method, route):
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    model = _small_body()
    assert hasattr(model.model, "forward_tape")
    lens = [3, 16, 9, 12]
    batch = _small_batch(lens)
    gen = vb.SelfAttentionGenerator(model)
    gen.use_tape = route == "tape"
    for start_layer in ((0, 1) if method == "rollout" else (0,)):
        scores = _batch_call(gen, method, batch, start_layer=start_layer).clone()
        _assert_rows_equal_per_item(model, batch, lens, method, scores, start_layer=start_layer)
    if method == "attn_gradcam":
        with torch.no_grad():
            best = model.model(batch["input_ids"], batch["input_mask"],
                               torch.cat((batch["input_mask"], torch.ones(4, V_SMALL, dtype=torch.long, device="cuda")), dim=-1),
                               batch["segment_ids"], batch["image_feature_0"],
                               torch.zeros(4, V_SMALL, dtype=torch.long, device="cuda"))["scores"].argmax(dim=-1)
        named = gen.generate_attn_gradcam_batch(batch, index=best)
        assert torch.equal(torch.nan_to_num(named, nan=-7.0), torch.nan_to_num(scores, nan=-7.0))
        other = (best + 1) % 13
        _assert_rows_equal_per_item(model, batch, lens, method, gen.generate_attn_gradcam_batch(batch, index=other).clone(), index=other)
    if route == "hook":
        assert all(p.grad is None for p in model.parameters())      # the hook route's backward forms no weight gradients


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
    for method in METHODS:
        a, o = _batch_call(gen, method, batch).clone(), _batch_call(gen, method, other)
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(o, nan=-7.0)), method
        for b in range(4):
            assert not bool(a[b, T_SMALL + int(dims[b]):].any()), method


def test_sizes_above_the_kernel_limit_are_refused():
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    model = _small_body()
    gen = vb.SelfAttentionGenerator(model)
    batch = _small_batch([5, 9])
    batch["image_feature_0"] = torch.zeros(2, 241, 24, device="cuda")
    for method in METHODS:
        with pytest.raises(NotImplementedError):
            _batch_call(gen, method, batch)


@pytest.mark.parametrize("method", METHODS)
def test_graphed_baselines_replay_any_lengths(method):
    """ONE captured graph serves batches of other lengths copied into it, bit-equal to the eager batched call."""
    from transformer_mm_explainability_amd import visualbert_explainability as vb
    model = _small_body()
    run = vb.GraphedBaselinesBatch(model, _small_batch([16, 16, 16, 16]), method)
    gen = vb.SelfAttentionGenerator(model)
    for lens, seed in (([16, 16, 16, 16], 3), ([6, 11, 3, 14], 4), ([16, 2, 9, 5], 6)):
        batch = _small_batch(lens, seed=seed)
        want = _batch_call(gen, method, batch).clone()
        got = run(batch)
        assert torch.equal(torch.nan_to_num(got, nan=-7.0), torch.nan_to_num(want, nan=-7.0)), (method, lens)
        assert bool(torch.isfinite(got).any())
    with pytest.raises(ValueError, match="captured"):
        run({k: v[:3] for k, v in batch.items()})
    with pytest.raises(ValueError, match="method"):
        vb.GraphedBaselinesBatch(model, batch, "ours")
    if method == "rollout":
        late = vb.GraphedBaselinesBatch(model, _small_batch([16, 16, 16, 16]), method, start_layer=1)
        assert torch.equal(late(batch), gen.generate_rollout_batch(batch, start_layer=1))


def test_evaluator_explain_batch_prints_the_same_accuracies():
    """``examples/visualbert_pert_eval.py --method rollout``: ``--explain-batch 4`` and ``--explain-batch 1`` print the same
    ``step_accuracy_percent`` (each run a fresh child process under its own time limit)."""
    printed = []
    for explain in ("4", "1"):
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "visualbert_pert_eval.py"), "--method",
               "rollout", "--explain-batch", explain, "--num-samples", "8"]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stderr[-2000:]
        printed.append(json.loads(res.stdout.strip().splitlines()[-1]))
    assert printed[0]["samples"] == printed[1]["samples"] == 8
    assert printed[0]["step_accuracy_percent"] == printed[1]["step_accuracy_percent"]
    assert set(printed[0]) == set(printed[1])
