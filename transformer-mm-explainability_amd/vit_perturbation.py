"""Perturbation test for image models -- ViT classification and CLIP zero-shot classification -- for a batch of images, on
the device.

The paper scores a vision explanation with the positive / negative perturbation test: patches are removed in order of
relevance, most relevant first (positive test) or least relevant first (negative test), the model is re-run after each
removal, and the class probability and accuracy are followed over the steps.  (The paper's own ViT perturbation script lives in
another repository, the one the ViT notebook clones its model class from, and is not part of the reference tree; the removal
order, the steps and the step counts here are those of the reference's bi-modal evaluator, ``lxmert/lxmert/perturbation.py:112``
and ``lxmert_perturbation.py`` next to this file.)  The unit of removal is the patch: that is the unit the relevancy maps of
``vit_model.generate_relevance_batch`` / ``clip_explainability.interpret_batch`` are computed in.

Two ways of removing a patch:

  * ``mode="zero"`` (the paper's test): the pixels of a removed patch are replaced by ``fill`` (per channel, in the model's
    input space).  One ``ops.patch_ranks`` and one ``ops.perturb_patches`` launch build the ``S`` perturbed copies of every
    image; the ``S * B`` images then run through the scorer in chunks of ``max_batch``.
  * ``mode="drop"`` (what the reference's LXMERT image test does with regions: the removed ones are not there): step ``s``
    runs the model on the class token plus the ``counts[s]`` kept patch tokens, gathered after the position embedding (and
    after ``ln_pre`` for CLIP: it is row-wise).  Every image keeps the same number of patches in a step, so a step is ONE
    batch at ``1 + counts[s]`` tokens with no mask and no padding; the kept tokens stay in their original order.

Every model run is an inference forward (``forward_nocapture`` / ``encode_nocapture``: attention on ``ops.attn_fwd``, no
capture slab written or allocated, no tape).  Nothing is read back to the host inside a call.

Tie policy: the reference calls ``topk(k)`` once per step; which of several EQUAL scores it keeps is whatever the
backend's ``topk`` does for that ``k`` (not specified, and different between CPU and GPU builds of torch).  Here the
ranking is ONE stable descending sort -- among equal scores the lower index ranks first -- so every step keeps a prefix
of the same order.  With distinct scores (any real relevancy map) this equals the reference's per-step ``topk`` exactly.
"""
from __future__ import annotations

import torch

from . import ops
from .lxmert_perturbation import PERT_STEPS


def step_counts(steps, n_patches):
    """Patches kept per step: ``int((1 - step) * n_patches)`` in host float arithmetic, exactly as the reference computes its
    region counts (``lxmert/lxmert/perturbation.py:112``)."""
    return [int((1 - step) * n_patches) for step in steps]


def _check_steps(steps):
    steps = tuple(float(s) if not isinstance(s, int) else s for s in steps)
    if len(steps) < 1 or any(not (0 <= s <= 1) for s in steps) or any(b <= a for a, b in zip(steps, steps[1:])):
        raise ValueError("steps must be an increasing sequence in [0, 1], got %r" % (steps,))
    return steps


def auc(values, steps):
    """Area under ``values [S, ...]`` over ``steps`` (trapezoid rule), divided by ``steps[-1] - steps[0]``: the mean height of
    the curve.  Returns ``values``' trailing shape."""
    x = torch.as_tensor([float(s) for s in steps], dtype=values.dtype if values.is_floating_point() else torch.float32,
                        device=values.device)
    v = values.to(x.dtype)
    if v.shape[0] != x.numel() or x.numel() < 2:
        raise ValueError("auc: %d values over %d steps (at least two steps)" % (v.shape[0], x.numel()))
    w = (x[1:] - x[:-1]).reshape(-1, *([1] * (v.dim() - 1)))
    return ((v[1:] + v[:-1]) * 0.5 * w).sum(dim=0) / (x[-1] - x[0])


class VitScorer:
    """Class logits of a ``vit_model.VisionTransformer`` (inference forward)."""

    def __init__(self, model):
        self.model = model
        self.patch_size = model.patch_embed.patch_size
        self.n_patches = model.patch_embed.num_patches

    def logits(self, images=None, tokens=None):
        return self.model.forward_nocapture(images=images, tokens=tokens)

    @torch.no_grad()
    def embed(self, images):
        """``[B, 1 + P, E]``: class token first, position embedding added (the block input)."""
        return self.model._embed(images)


class ClipZeroShotScorer:
    """``logits_per_image [B, C]`` of a ``clip_model.CLIP`` against C prompts.  The prompts are encoded ONCE, forward only, at
    construction (normalised text features, times ``exp(logit_scale)``)."""

    def __init__(self, model, texts):
        from . import clip_explainability
        clip_explainability._fp32_clip(model, "ClipZeroShotScorer")
        self.model = model
        self.patch_size = model.visual.conv1.kernel_size[0]
        self.n_patches = model.visual.positional_embedding.shape[0] - 1
        with torch.no_grad():
            t = model.encode_text_nocapture(texts)
            self.text_features = (t / t.norm(dim=-1, keepdim=True)).contiguous()          # [C, embed_dim]
            self.logit_scale = model.logit_scale.detach().exp()

    @torch.no_grad()
    def logits(self, images=None, tokens=None):
        f = self.model.visual.encode_nocapture(images=images, tokens=tokens)
        f = f / f.norm(dim=-1, keepdim=True)
        return self.logit_scale * f @ self.text_features.t()                              # CLIP/clip/model.py:369-378

    @torch.no_grad()
    def embed(self, images):
        return self.model.visual._embed(images)


class PerturbationResult:
    """``logits [S, B, C]``, ``target_prob [S, B]`` (softmax probability of the target class), ``pred [S, B]`` (arg-max class),
    ``targets [B]``; with labels also ``correct [S, B]`` (bool) and ``accuracy [S]``.  All on the device."""

    def __init__(self, steps, counts, logits, targets, labels=None):
        self.steps, self.counts = steps, counts
        self.logits, self.targets = logits, targets
        prob = torch.softmax(logits, dim=-1)
        S, B, _ = logits.shape
        self.target_prob = prob.gather(2, targets.reshape(1, B, 1).expand(S, B, 1)).squeeze(2)
        self.pred = logits.argmax(dim=-1)
        self.correct = self.accuracy = None
        if labels is not None:
            self.correct = self.pred == labels.reshape(1, B)
            self.accuracy = self.correct.to(torch.float32).mean(dim=1)

    def auc(self):
        """Mean height of the target-probability curve per image, ``[B]`` (``auc``)."""
        return auc(self.target_prob, self.steps)


class PatchPerturbation:
    """The perturbation test of ``scorer`` (``VitScorer`` / ``ClipZeroShotScorer``) over ``steps`` (fractions of the patches
    removed; default: the reference's ``lxmert/lxmert/perturbation.py:42``).  ``mode`` / ``fill``: module docstring."""

    def __init__(self, scorer, steps=PERT_STEPS, mode="zero", fill=0.0, max_batch=None):
        if mode not in ("zero", "drop"):
            raise ValueError("mode must be 'zero' or 'drop', got %r" % (mode,))
        self.steps = _check_steps(steps)
        self.scorer, self.mode, self.fill, self.max_batch = scorer, mode, fill, max_batch
        self.counts = step_counts(self.steps, scorer.n_patches)
        self._dev = {}

    def _device_state(self, device, channels):
        """(counts [S] int32, fill [C] fp32) on ``device``, built once: a later call makes no tensor from host lists."""
        key = (str(device), channels)
        if key not in self._dev:
            fill = torch.as_tensor(self.fill, dtype=torch.float32).reshape(-1)
            if fill.numel() == 1:
                fill = fill.expand(channels)
            if fill.numel() != channels:
                raise ValueError("fill needs one value or one per channel (%d), got %d" % (channels, fill.numel()))
            self._dev[key] = (torch.tensor(self.counts, dtype=torch.int32, device=device), fill.contiguous().to(device))
        return self._dev[key]

    @torch.no_grad()
    def __call__(self, images, cam, targets=None, labels=None, is_positive_pert=False, max_batch=None):
        """``images [B, 3, R, R]``, ``cam [B, P]`` patch relevancies.  ``targets [B]``: the class whose probability is followed
        (default: the arg-max class of the unperturbed image, picked on the device).  ``labels [B]``: also report accuracy.
        ``is_positive_pert``: remove the MOST relevant patches first.  ``max_batch``: run the scorer on at most that many
        images at a time (zero mode: over the ``S * B`` perturbed images; drop mode: over the B images of a step)."""
        sc = self.scorer
        B, P = images.shape[0], sc.n_patches
        if cam.dim() != 2 or cam.shape[0] != B or cam.shape[1] != P:
            raise ValueError("cam must be [%d, %d] (one relevancy per patch of the model), got %s" % (B, P, tuple(cam.shape)))
        max_batch = max_batch if max_batch is not None else self.max_batch
        counts, fill = self._device_state(images.device, images.shape[1])
        ranks = ops.patch_ranks(-cam.float() if is_positive_pert else cam.float())
        S = len(self.counts)
        if self.mode == "zero":
            pert = ops.perturb_patches(images.float(), ranks, counts, fill)            # [S, B, C, R, R]
            flat = pert.view(S * B, *pert.shape[2:])
            step = max_batch or S * B
            logits = torch.cat([sc.logits(images=flat[i:i + step]) for i in range(0, S * B, step)], dim=0)
            logits = logits.view(S, B, -1)
        else:
            tokens = sc.embed(images.float())                                          # [B, 1 + P, E]
            # kept patches in their original order: a stable sort of the keep flags (kept first) over the patch index
            order = torch.sort(ranks, dim=1, stable=True).indices                      # order[b, r] = patch with rank r
            step = max_batch or B
            rows = []
            for n in self.counts:
                keep = torch.sort(order[:, :n], dim=1).values + 1                      # token rows, ascending
                idx = torch.cat([torch.zeros(B, 1, dtype=keep.dtype, device=keep.device), keep], dim=1)
                sub = torch.gather(tokens, 1, idx.unsqueeze(-1).expand(B, n + 1, tokens.shape[-1]))
                rows.append(torch.cat([sc.logits(tokens=sub[i:i + step]) for i in range(0, B, step)], dim=0))
            logits = torch.stack(rows, dim=0)
        if targets is None:
            targets = sc.logits(images=images.float()).argmax(dim=-1)
        else:
            targets = torch.as_tensor(targets, device=images.device).reshape(B).long()
        if labels is not None:
            labels = torch.as_tensor(labels, device=images.device).reshape(B).long()
        return PerturbationResult(self.steps, self.counts, logits, targets, labels)
