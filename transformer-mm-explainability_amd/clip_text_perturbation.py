"""Perturbation test for the TEXT maps of CLIP -- ``R_text`` of ``clip_explainability.interpret`` -- for a batch of captions, on the
device.

The reference scores a text explanation by removing words in order of relevance and re-running the model
(``lxmert/lxmert/perturbation.py:158-176``, for LXMERT and VisualBERT: [CLS] and [SEP] always stay, the ``int((1 - step) * W)``
top-scoring of the W words in between stay in their original order, the rest is dropped; ``lxmert_perturbation.text_keep_batches`` is
that rule here).  CLIP captions have the same frame -- SOT first, EOT at ``text.argmax(dim=-1)`` (``CLIP/clip/model.py:360``), zeros
behind -- and ``CLIP/example.py:27`` reads a caption's word relevancies as ``R_text[i, CLS_idx, 1:CLS_idx]``: the EOT row, between SOT
and EOT.  This module is that test for CLIP:

  * ``text_cams``: the EOT rows of a batch of ``R_text``, picked on the device.
  * ``ops.perturb_tokens`` (``mmx_perturb_tokens``) builds the S perturbed copies of all B captions in ONE launch, from a count table
    ``token_step_counts`` that is uploaded once per evaluator.
  * ``ClipCaptionScorer`` scores captions against a fixed set of images (encoded once): ``logits_per_text``, the mirror of
    ``vit_perturbation.ClipZeroShotScorer``.
  * ``TokenPerturbation`` runs the S x B captions through the scorer in chunks and returns a ``vit_perturbation.PerturbationResult``
    whose classes are the images.

Every model run is an inference forward (``CLIP.encode_text_nocapture``: no capture slab written or allocated, no tape); nothing is
read back to the host inside a call.  ``live=True`` runs the text tower on the rows up to each perturbed caption's EOT only
(``Transformer.forward_nocapture(live=...)``): step ``1.0`` leaves ``[SOT, EOT]``, 2 live rows of 77.

Tie policy: as in ``vit_perturbation`` -- ONE stable descending order per caption, the lower position first among equal scores, so
every step keeps a prefix of the same order.
"""
from __future__ import annotations

import torch

from . import ops
from .lxmert_perturbation import PERT_STEPS
from .vit_perturbation import PerturbationResult, _check_steps


def token_step_counts(steps, n_positions):
    """``[S][n_positions - 1]`` word counts: entry ``[s][w]`` = ``int((1 - step_s) * w)`` words kept of a caption with ``w`` words,
    ``w = 0 ... n_positions - 2``, in host float arithmetic exactly as the reference computes its counts
    (``lxmert/lxmert/perturbation.py:112``; ``lxmert_perturbation.text_keep_batches``)."""
    if n_positions < 2:
        raise ValueError("token_step_counts: a caption has at least 2 positions, got %d" % n_positions)
    return [[int((1 - step) * w) for w in range(n_positions - 1)] for step in steps]


def text_cams(texts, R_text):
    """``texts [B, N]`` token ids, ``R_text [B, N, N]`` (``clip_explainability.interpret``) -> ``[B, N]``: row ``eot_b`` of every
    caption's relevancy matrix, ``CLIP/example.py:27``'s ``R_text[i, CLS_idx, 1:CLS_idx]`` for a batch (the positions outside the
    words come along; ``TokenPerturbation`` does not read them).  Picked on the device."""
    if texts.dim() != 2 or R_text.dim() != 3 or R_text.shape[0] != texts.shape[0] or R_text.shape[1] != texts.shape[1] \
            or R_text.shape[2] != texts.shape[1]:
        raise ValueError("text_cams: texts [B, N] and R_text [B, N, N] expected, got %s / %s" % (tuple(texts.shape), tuple(R_text.shape)))
    eot = texts.argmax(dim=-1)                                                         # model.py:360
    return R_text[torch.arange(texts.shape[0], device=R_text.device), eot.to(R_text.device)]


class ClipCaptionScorer:
    """``logits_per_text [n, n_images]`` of a ``clip_model.CLIP`` for n captions against a fixed set of images.  The images are
    encoded ONCE, forward only, at construction (normalised image features).  fp32 bodies only."""

    def __init__(self, model, images):
        from . import clip_explainability
        clip_explainability._fp32_clip(model, "ClipCaptionScorer")
        self.model = model
        self.n_positions = model.context_length
        with torch.no_grad():
            f = model.visual.encode_nocapture(images=images.float())
            self.image_features = (f / f.norm(dim=-1, keepdim=True)).contiguous()         # [n_images, embed_dim]
            self.logit_scale = model.logit_scale.detach().exp()

    @torch.no_grad()
    def logits(self, texts, live=False, eot=None):
        """``eot [n]``: the captions' EOT positions where the caller has them already (``ops.perturb_tokens``)."""
        t = self.model.encode_text_nocapture(texts, live=live, eot=eot)
        t = t / t.norm(dim=-1, keepdim=True)
        return self.logit_scale * t @ self.image_features.t()                             # CLIP/clip/model.py:369-378


class TokenPerturbation:
    """The caption perturbation test of ``scorer`` (a ``ClipCaptionScorer``) over ``steps`` (fractions of the words removed; default:
    the reference's ``lxmert/lxmert/perturbation.py:42``).  ``max_batch``: run the scorer on at most that many captions at a time.
    ``live``: run the re-runs' text tower on the rows up to each perturbed caption's EOT token (``encode_text_nocapture(live=True)``)
    instead of all positions; same features to fp32 rounding.  Default ``False`` (the dense forward): the route has not been timed
    against it yet -- ``tools/probe_text_perturbation.py`` measures both, and the default follows its figures."""

    def __init__(self, scorer, steps=PERT_STEPS, max_batch=None, live=False):
        self.steps = _check_steps(steps)
        if len(self.steps) > 64:
            raise ValueError("at most 64 steps, got %d" % len(self.steps))
        self.scorer, self.max_batch, self.live = scorer, max_batch, bool(live)
        self._dev = {}

    def _counts(self, device, n_positions):
        """``[S, n_positions - 1]`` int32 on ``device``, built once: a later call makes no tensor from host lists."""
        key = (str(device), n_positions)
        if key not in self._dev:
            table = token_step_counts(self.steps, n_positions)
            self._dev[key] = (torch.tensor(table, dtype=torch.int32, device=device), table)
        return self._dev[key]

    @torch.no_grad()
    def __call__(self, texts, cam, targets=None, labels=None, is_positive_pert=False):
        """``texts [B, N]`` token ids, ``cam [B, N]`` one relevancy per position (``text_cams``; only the words' are read).
        ``targets [B]``: the image whose probability is followed (default: the arg-max image of the unperturbed caption, picked
        on the device).  ``labels [B]``: also report accuracy.  ``is_positive_pert``: remove the MOST relevant words first."""
        sc = self.scorer
        if texts.dim() != 2 or tuple(cam.shape) != tuple(texts.shape):
            raise ValueError("cam must have the captions' shape %s (one relevancy per position), got %s"
                             % (tuple(texts.shape), tuple(cam.shape)))
        B, N = texts.shape
        S = len(self.steps)
        cam = cam.float()
        counts, table = self._counts(texts.device, N)
        ids, eot = ops.perturb_tokens(texts.long(), -cam if is_positive_pert else cam, counts)
        flat, flat_eot = ids.view(S * B, N), eot.view(S * B)
        step = self.max_batch or S * B
        # (every chunk builds its own row list from its slice of the EOT positions)
        logits = torch.cat([sc.logits(flat[i:i + step], live=self.live, eot=flat_eot[i:i + step]) for i in range(0, S * B, step)],
                           dim=0).view(S, B, -1)
        if targets is None:
            targets = sc.logits(texts.long(), live=self.live).argmax(dim=-1)
        else:
            targets = torch.as_tensor(targets, device=texts.device).reshape(B).long()
        if labels is not None:
            labels = torch.as_tensor(labels, device=texts.device).reshape(B).long()
        res = PerturbationResult(self.steps, table, logits, targets, labels)      # (counts: the [S][W] table, see token_step_counts)
        res.texts, res.eot = ids, eot                                              # the perturbed captions and their EOT positions
        return res
