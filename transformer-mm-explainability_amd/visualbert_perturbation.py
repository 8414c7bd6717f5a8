"""Perturbation evaluator inner loop for VisualBERT --
``VisualBERT/mmf/trainers/core/evaluation_loop.py:100-166``, same scheme as ``lxmert_perturbation``:

the reference re-runs the model 9 times per sample, each time after a host ``topk`` and a physical gather of the kept
image regions / question tokens.  Here the 9 perturbed inputs are ONE batch through ``VisualBERTForClassification``:

  * image test: the visual tokens' position / type embeddings do not depend on their index
    (``embeddings.py:399-417``: all visual position ids are 0), so a region masked as an attention key is
    indistinguishable from a removed one; the step that keeps no region needs no special case here because the text
    keys stay unmasked in the same softmax;
  * text test: kept token ids are gathered and left-aligned (positions re-index exactly as after the reference's
    gather), the tail is masked; [CLS] (0), the token at ``cls_index = len - 2`` (the '?' the 'vqa' pooler reads) and
    [SEP] always stay (``evaluation_loop.py:139-143``).

``perturbation_image_batch`` / ``perturbation_text_batch`` run B padded items and all steps as ONE packed pass with nothing read
back (``GraphedVisualBertPerturbation`` replays it): two HIP builders (``ops.selfattn_perturb_regions`` gathers the kept regions
physically, once per distinct keep count; ``ops.selfattn_perturb_text``) feed ``VisualBERTForClassification.scores_packed``, the
grad-free forward on packed rows that writes no capture slab.
"""
from __future__ import annotations

import torch

from . import graphed, ops
from .lxmert_perturbation import PERT_STEPS, image_keep_masks, ranking

# evaluation_loop.py:93-96: the image test removes regions on a finer scale near "all removed" than the text test
IMAGE_STEPS = (0, 0.5, 0.75, 0.95, 0.96, 0.97, 0.98, 0.99, 1)
TEXT_STEPS = PERT_STEPS


def text_keep_batch(input_ids, segment_ids, text_scores, n_text, steps=PERT_STEPS):
    """``input_ids``, ``segment_ids``: ``[1, T]`` (first ``n_text`` positions real); ``text_scores [n_text - 3]``: the
    scores of tokens ``1 .. cls_index - 1``.  Returns left-aligned ``(ids [S, T], segments [S, T], input_mask [S, T])``."""
    T = input_ids.shape[1]
    cls_index = n_text - 2
    n_inner = text_scores.shape[-1]
    order = ranking(text_scores) + 1
    S = len(steps)
    keep = torch.zeros(S, T, dtype=torch.bool, device=input_ids.device)
    keep[:, 0] = keep[:, cls_index] = keep[:, cls_index + 1] = True
    for s, step in enumerate(steps):
        keep[s, order[: int((1 - step) * n_inner)]] = True
    pos = torch.arange(T, device=input_ids.device).expand(S, T)
    perm = torch.argsort(torch.where(keep, pos, pos + T), dim=1)
    mask = torch.gather(keep, 1, perm)
    ids = torch.gather(input_ids.expand(S, T), 1, perm) * mask
    seg = torch.gather(segment_ids.expand(S, T), 1, perm) * mask
    return ids, seg, mask.long()


def image_step_groups(steps, V):
    """The image test's steps by DISTINCT keep count ``int((1 - step) * V)`` (evaluation_loop.py:111): steps with equal counts are the
    same input and are computed once -- ``IMAGE_STEPS`` at V = 36 keeps (36, 18, 9, 1, 1, 1, 0, 0, 0) regions, five groups; at V = 14 six of
    the nine steps keep none.  -> ``(group_counts, step_group)``: the distinct counts in descending order and, per step, the index of
    its group."""
    counts = [int((1 - step) * V) for step in steps]
    group_counts = sorted(set(counts), reverse=True)
    return group_counts, [group_counts.index(c) for c in counts]


def group_offsets(group_counts, T, B):
    """Where the groups start in the packed rows of ``ops.selfattn_perturb_regions``: group g is B sequences of ``T + c_g`` rows.
    -> ``(offsets, rows)`` with ``rows = B * sum_g (T + c_g)``."""
    offsets, rows = [], 0
    for c in group_counts:
        offsets.append(rows)
        rows += B * (T + c)
    return offsets, rows


def text_step_counts(steps, T):
    """``counts[s][w] = int((1 - step_s) * w)`` for every word count ``w < T`` (evaluation_loop.py:140), the ``[S, T]`` table
    ``ops.selfattn_perturb_text`` indexes with a question's own word count: host float arithmetic, as in the reference."""
    return [[int((1 - step) * w) for w in range(T)] for step in steps]


class VisualBertPerturbation:
    """``model``: a ``visualbert_model.VisualBERT``.  ``sample``: ``input_ids``, ``input_mask``, ``segment_ids``
    (``[1, T]``, padding allowed), ``image_feature_0`` (``[1, V, dim]``).  ``method_cam``: the generator's ``[1, N]`` row
    (``N = n_text + V``).  Both methods return the 9 steps' ``scores [S, num_labels]``.  ``steps=None`` (default): the
    reference's step lists, which differ per modality (``IMAGE_STEPS`` / ``TEXT_STEPS``, evaluation_loop.py:93-96).
    ``perturbation_image_batch`` / ``perturbation_text_batch``: B padded items in one pass -> ``[B, S, num_labels]``."""

    def __init__(self, model, steps=None):
        self.model = model
        self.image_steps = tuple(IMAGE_STEPS if steps is None else steps)
        self.text_steps = tuple(TEXT_STEPS if steps is None else steps)
        self._const = {}

    def _run(self, ids, seg, input_mask, feats, visual_mask):
        S = ids.shape[0]
        attention_mask = torch.cat((input_mask, visual_mask), dim=-1)
        return self.model.model(ids, input_mask, attention_mask, seg, feats.expand(S, -1, -1),
                                torch.zeros_like(visual_mask))["scores"]

    @torch.no_grad()
    def perturbation_image(self, sample, method_cam, is_positive_pert=False):
        n_text = int(sample["input_mask"].sum())                      # one host read per sample, as in the reference
        S = len(self.image_steps)
        keep = image_keep_masks(method_cam[0, n_text:], self.image_steps, is_positive_pert).long()    # [S, V]
        ids = sample["input_ids"][:, :n_text].expand(S, -1)
        seg = sample["segment_ids"][:, :n_text].expand(S, -1)
        return self._run(ids, seg, torch.ones_like(ids), sample["image_feature_0"], keep)

    @torch.no_grad()
    def perturbation_text(self, sample, method_cam, is_positive_pert=False):
        n_text = int(sample["input_mask"].sum())
        cam = -method_cam if is_positive_pert else method_cam
        ids, seg, mask = text_keep_batch(sample["input_ids"][:, :n_text], sample["segment_ids"][:, :n_text],
                                         cam[0, 1:n_text - 2], n_text, self.text_steps)
        feats = sample["image_feature_0"]
        visual_mask = torch.ones(len(self.text_steps), feats.shape[1], dtype=torch.long, device=feats.device)
        return self._run(ids, seg, mask, feats, visual_mask)

    # ---- B padded items and all steps in ONE pass (the per-item forms above: unchanged)
    def _batch_constants(self, T, V, B, device):
        """Per ``(T, V, B, device)``: the device constants of the two batch methods, built ONCE from host arithmetic so that a call
        creates no tensor from a host list and reads nothing back (hipGraph-capturable), as ``LxmertPerturbation._image_constants``."""
        key = (T, V, B, str(device))
        if key not in self._const:
            group_counts, step_group = image_step_groups(self.image_steps, V)
            offsets, rows = group_offsets(group_counts, T, B)
            S = len(self.text_steps)
            self._const[key] = dict(
                counts=torch.tensor(group_counts, dtype=torch.int32, device=device), rows=rows,
                segments=[(off, B, T + c) for off, c in zip(offsets, group_counts)],
                step_group=torch.tensor(step_group, dtype=torch.long, device=device),
                text_counts=torch.tensor(text_step_counts(self.text_steps, T), dtype=torch.int32, device=device),
                text_segments=[(0, S * B, T + V)],
                sequence_start=torch.arange(S * B, device=device) * (T + V),
                visual_type=torch.zeros(B, V, dtype=torch.long, device=device),
                visual_keys=torch.zeros(S * B, V, dtype=torch.float32, device=device))
        return self._const[key]

    def _batch_operands(self, batch, cams):
        if batch.get("image_dim") is not None:
            raise NotImplementedError("the batched perturbation test takes every region of an item (no image_dim), as the per-item one")
        mask, feats = batch["input_mask"], batch["image_feature_0"]
        B, T = mask.shape
        V = feats.shape[1]
        if T + V > ops.SELFATTN_MAX_TOKENS:
            raise NotImplementedError("the batched perturbation test carries rows of at most %d tokens (T + V = %d)"
                                      % (ops.SELFATTN_MAX_TOKENS, T + V))
        if tuple(cams.shape) != (B, T + V):
            raise ValueError("cams must be [B, T + V] = %s in the padded layout (visualbert_explainability.pad_rows), got %s"
                             % ((B, T + V), tuple(cams.shape)))
        return (self._batch_constants(T, V, B, feats.device), mask.sum(dim=1).to(torch.int32), cams.detach().float().contiguous(),
                B, T, V)

    @torch.no_grad()
    def perturbation_image_batch(self, batch, cams, is_positive_pert=False):
        """``perturbation_image`` for the padded ``sample_list`` of B ragged items (``input_ids`` / ``input_mask`` / ``segment_ids``
        ``[B, T]``, masks left-aligned; ``image_feature_0 [B, V, dim]``) and their relevancy rows ``cams [B, T + V]`` in the padded layout
        (what ``generate_*_batch`` returns; ``pad_rows`` for per-item rows) -> ``scores [B, S, num_labels]``.

        Where the per-item form masks the removed regions as keys and keeps all V as rows, this one gathers the kept regions as the
        reference does (evaluation_loop.py:113-120; a visual token has no index-dependent term, embeddings.py:399-417): the rows are
        embedded once per item, ``ops.selfattn_perturb_regions`` packs one sequence per (item, distinct keep count) and
        ``scores_packed`` runs them in one pass; steps with equal counts are the same input and read the one group that computed it."""
        k, text_len, cams, B, T, V = self._batch_operands(batch, cams)
        body = self.model.model
        emb = body.bert.embeddings(batch["input_ids"], batch["segment_ids"], batch["image_feature_0"], k["visual_type"])
        x, key_mask, pooled = ops.selfattn_perturb_regions(emb, cams, text_len, k["counts"], k["rows"], T, is_positive_pert)
        out = body.scores_packed(x, k["segments"], key_mask, pooled)                              # [G * B, num_labels]
        return out.view(len(k["segments"]), B, -1).index_select(0, k["step_group"]).transpose(0, 1)

    @torch.no_grad()
    def perturbation_text_batch(self, batch, cams, is_positive_pert=False):
        """``perturbation_text`` for a padded batch (arguments and result as ``perturbation_image_batch``): ``ops.selfattn_perturb_text``
        builds the S left-aligned copies of every question, their text rows are embedded from those ids (positions re-index as after
        the reference's gather, evaluation_loop.py:156-159), the region rows once per item, and all ``S * B`` sequences of
        ``T + V`` rows run as one segment of ``scores_packed``."""
        k, text_len, cams, B, T, V = self._batch_operands(batch, cams)
        body = self.model.model
        embeddings = body.bert.embeddings
        ids, seg, keep, new_len = ops.selfattn_perturb_text(batch["input_ids"], batch["segment_ids"], cams, text_len, k["text_counts"],
                                                            is_positive_pert)                     # [S, B, T], [S, B]
        S = ids.shape[0]
        regions = embeddings.LayerNorm(embeddings.encode_image(batch["image_feature_0"], k["visual_type"]))       # [B, V, E]
        text = embeddings.LayerNorm(embeddings.encode_text(ids.view(S * B, T), seg.view(S * B, T)))               # [S * B, T, E]
        E = text.shape[-1]
        x = torch.cat((text.view(S, B, T, E), regions.unsqueeze(0).expand(S, -1, -1, -1)), dim=2).reshape(S * B * (T + V), E)
        key_mask = torch.cat(((1.0 - keep.view(S * B, T).to(torch.float32)) * -10000.0, k["visual_keys"]), dim=1).reshape(-1)
        pooled = k["sequence_start"] + new_len.view(-1) - 2
        out = body.scores_packed(x, k["text_segments"], key_mask, pooled)                         # [S * B, num_labels]
        return out.view(S, B, -1).transpose(0, 1)

    @staticmethod
    def accuracy(scores, targets):
        """``targets [num_labels]``: the item's soft scores per answer (``report['targets'][0]``) -> ``[S]``; ``targets [B, num_labels]``
        for batched ``scores [B, S, num_labels]`` -> ``[B, S]``."""
        best = scores.argmax(dim=-1)
        return targets[best] if targets.dim() == 1 else torch.gather(targets, 1, best)


class GraphedVisualBertPerturbation:
    """``VisualBertPerturbation.perturbation_image_batch`` / ``perturbation_text_batch`` of a fixed-shape batch captured ONCE into a
    hipGraph and replayed, the way ``visualbert_explainability.GraphedBaselinesBatch`` replays the batched baselines.  The builders take
    the question lengths from the device (``input_mask.sum(1)`` is part of the graph), so ONE graph serves every ragged batch of the
    captured shape: a new batch and new cams are copied into the captured buffers.

        run = GraphedVisualBertPerturbation(pert, example_batch, example_cams, "image")      # "image" | "text"
        scores = run(batch, cams)                                                              # [B, S, num_labels], the graph's own buffer
    """

    MODALITIES = ("image", "text")
    KEYS = ("input_ids", "input_mask", "segment_ids", "image_feature_0")

    def __init__(self, pert, example_batch, example_cams, modality, is_positive_pert=False, warmup=2):
        if modality not in self.MODALITIES:
            raise ValueError("modality must be one of %s, got %r" % (self.MODALITIES, modality))
        if example_batch.get("image_dim") is not None:
            raise NotImplementedError("the batched perturbation test takes every region of an item (no image_dim)")
        self.pert, self.modality, self.positive = pert, modality, bool(is_positive_pert)
        self.static = {k: example_batch[k].clone() for k in self.KEYS}
        self.cams = example_cams.detach().clone()
        run = pert.perturbation_image_batch if modality == "image" else pert.perturbation_text_batch
        self._call = lambda: run(self.static, self.cams, self.positive)
        self.graph, self.output, self._pinned = graphed.capture(self._call, warmup, pert.model)

    def __call__(self, batch=None, cams=None):
        if batch is not None:
            graphed.copy_inputs(self.static, batch, self.KEYS, hint=graphed.PAD_HINT)
        if cams is not None:
            graphed.copy_inputs({"cams": self.cams}, {"cams": cams})
        self.graph.replay()
        return self.output


def evaluation_loop(generate, pert, loader, num_samples, modality="image", is_positive_pert=False, reference_exact=False):
    """``TrainerEvaluationLoopMixinPert.evaluation_loop`` (evaluation_loop.py:73-169) on the batched evaluator: for every
    item ``method_cam = generate(item)``, the 9 perturbed re-runs in ONE forward, ``step_acc[s] += targets[argmax]``.
    Returns the per-step accuracies in percent (what the reference prints) as a ``[9]`` fp64 tensor.

    ``reference_exact=True`` reproduces the reference's sample accounting: its ``i > num_samples`` test stops only AFTER
    item ``num_samples + 1`` and it still divides by ``num_samples``.  The default evaluates exactly ``num_samples`` items.
    ``loader`` yields ``sample_list`` dicts carrying ``targets [1, num_labels]``."""
    steps = pert.image_steps if modality == "image" else pert.text_steps
    step_acc = torch.zeros(len(steps), dtype=torch.float64)
    limit = num_samples + 1 if reference_exact else num_samples
    for i, item in enumerate(loader):
        if i >= limit:
            break
        cam = generate(item).detach()
        run = pert.perturbation_image if modality == "image" else pert.perturbation_text
        scores = run(item, cam, is_positive_pert)
        step_acc += pert.accuracy(scores, item["targets"][0]).double().cpu()
    return step_acc / num_samples * 100
