"""Perturbation evaluator inner loop for LXMERT -- ``lxmert/lxmert/perturbation.py:85-194``.

The reference scores an explanation by removing the least (negative test) or most (positive test) relevant image
regions / question tokens in 9 steps and re-running the model after each removal: 9 sequential batch-1 forwards per
sample, each preceded by a host ``topk`` -> numpy round trip (and a Faster R-CNN re-run, which is outside this path).
Here the 9 perturbed inputs of one sample are ONE batch:

  * image test: a region that is masked as an attention key everywhere (-10000 additive mask -> exp underflows to an
    exact 0) is indistinguishable from a removed region for every other token -- LXMERT's visual stream has no
    index-dependent position term, and the answer is read from the [CLS] text token.  Every step keeps a PREFIX of one ranking of
    the regions, so the live steps run as (at most) two GROUPS: a group is one batch over the gathered ``kmax`` top-ranked regions
    of every sample (what the reference's ``topk`` + index does per step) with a ``visual_attention_mask`` row per step for the
    steps that keep fewer -- (36, 27, 18 | 9, 7, 5, 3, 1) at 36 regions: 153 region rows per sample where one masked batch over
    all regions (rounds 1-5) ran 288; the questions' own 9 layers run once for both groups.  The step that keeps ZERO regions is
    the one exception (a uniform -10000 shift is no mask at all): it runs as a region-free forward.
  * text test: removing tokens re-indexes the position embeddings (``perturbation.py:170``: "text tokens must be
    sorted for positional embedding to work"), so the kept ids are gathered, left-aligned and padded; padding is masked.

Everything (``topk``, mask / gather construction, arg-max, accuracy lookup) stays on the device; one host read per
sample at most.  Results equal the sequential loop up to fp32 summation order; pinned against the 9 score vectors the
reference's own ``perturbation_image`` / ``perturbation_text`` produce on the reference LXMERT body
(``tests/golden/lxmert_perturbation.npz``, ``tests/test_gpu_perturbation.py``).

Tie policy: the reference calls ``topk(k)`` once per step; which of several EQUAL scores it keeps is whatever the
backend's ``topk`` does for that ``k`` (not specified, and different between CPU and GPU builds of torch).  Here the
ranking is ONE stable descending sort -- among equal scores the lower index ranks first -- so every step keeps a prefix
of the same order.  With distinct scores (any real relevancy map) this equals the reference's per-step ``topk`` exactly.
"""
from __future__ import annotations

import contextlib
import types

import torch

from . import graphed, ops, tuned_gemms

PERT_STEPS = (0, 0.25, 0.5, 0.75, 0.8, 0.85, 0.9, 0.95, 1)


def normalize_cams(R_t_t, R_t_i):
    """``perturbation.py:242-245``: first rows of the text / image relevancies, min-max normalised."""
    cam_image, cam_text = R_t_i[0], R_t_t[0]
    cam_image = (cam_image - cam_image.min()) / (cam_image.max() - cam_image.min())
    cam_text = (cam_text - cam_text.min()) / (cam_text.max() - cam_text.min())
    return cam_image, cam_text


def normalize_cams_batch(R_t_t, R_t_i, attention_mask=None):
    """``normalize_cams`` for ``[B, T, T]`` / ``[B, T, I]`` relevancies -> ``(cam_image [B, I], cam_text [B, T])``.
    ``attention_mask [B, T]`` (padded batch): the text min / max run over each sample's real tokens only and the padded
    positions of ``cam_text`` come back as 0."""
    def minmax(x, valid=None):
        if valid is None:
            lo, hi = x.min(dim=-1, keepdim=True).values, x.max(dim=-1, keepdim=True).values
            return (x - lo) / (hi - lo)
        inf = torch.full_like(x, float("inf"))
        lo = torch.where(valid, x, inf).min(dim=-1, keepdim=True).values
        hi = torch.where(valid, x, -inf).max(dim=-1, keepdim=True).values
        return torch.where(valid, (x - lo) / (hi - lo), torch.zeros_like(x))
    valid = attention_mask.bool() if attention_mask is not None else None
    return minmax(R_t_i[:, 0]), minmax(R_t_t[:, 0], valid)


def ranking(scores):
    """Indices by descending score, ties by ascending index (module docstring: tie policy)."""
    return torch.sort(scores, dim=-1, descending=True, stable=True).indices


def _ranks(order):
    """Inverse of a ranking: ``rank[..., i]`` = position of element ``i`` in ``order`` (``[..., n]`` index rows)."""
    pos = torch.arange(order.shape[-1], device=order.device).expand_as(order)
    return torch.empty_like(order).scatter_(-1, order, pos)


def image_keep_masks(cam_image, steps=PERT_STEPS, is_positive_pert=False, counts=None):
    """``[S, I]`` float 0/1 (``[B, S, I]`` for ``cam_image [B, I]``): row s keeps the ``int((1 - step_s) * I)`` top-scoring
    regions (``perturbation.py:114-117``).  Every step keeps a prefix of ONE ranking, so region i stays in step s iff its rank
    is below that step's count: a handful of launches for the whole batch.  ``counts``: the per-step counts already on the device
    (a captured pass must not build tensors from host lists)."""
    cam = -cam_image if is_positive_pert else cam_image
    n = cam.shape[-1]
    if counts is None:
        counts = torch.tensor([int((1 - step) * n) for step in steps], device=cam.device)      # host arithmetic, as the reference
    rank = _ranks(ranking(cam))                                                                 # [..., I]
    return (rank.unsqueeze(-2) < counts.unsqueeze(-1)).to(torch.float32)                        # [..., S, I]


def text_keep_batches(input_ids, token_type_ids, cam_text, steps=PERT_STEPS, is_positive_pert=False, n_tokens=None):
    """``text_keep_batch`` for B questions at once: ``input_ids`` / ``token_type_ids`` / ``cam_text [B, P]``, ``n_tokens`` a
    list of the B real lengths (``None``: all ``P``).  Returns ``(ids, token_types, attention_mask)`` ``[B * S, P]``, the S
    perturbed copies of a question adjacent."""
    cam = -cam_text if is_positive_pert else cam_text
    B, P = cam.shape
    S = len(steps)
    lens = [P if n is None else int(n) for n in (n_tokens if n_tokens is not None else [None] * B)]
    dev = cam.device
    T = torch.tensor(lens, device=dev).unsqueeze(1)                                             # [B, 1]
    counts = torch.tensor([[int((1 - step) * (t - 2)) for step in steps] for t in lens], device=dev)   # [B, S] host arithmetic
    pos = torch.arange(P, device=dev).expand(B, P)
    inner = (pos >= 1) & (pos < T - 1)
    # one stable ranking per question: inner tokens by descending score (ties: lower index first), everything else behind them
    rank = _ranks(ranking(torch.where(inner, cam, torch.full_like(cam, float("-inf")))))
    keep = (inner.unsqueeze(1) & (rank.unsqueeze(1) < counts.unsqueeze(2))) | (pos == 0).unsqueeze(1) | (pos == T - 1).unsqueeze(1)
    keep = keep.reshape(B * S, P)
    # stable left-alignment: kept positions sorted by index first, dropped ones after
    posr = torch.arange(P, device=dev).expand(B * S, P)
    perm = torch.argsort(torch.where(keep, posr, posr + P), dim=1)
    mask = torch.gather(keep, 1, perm)
    ids = torch.gather(input_ids.repeat_interleave(S, dim=0), 1, perm) * mask
    types = torch.gather(token_type_ids.repeat_interleave(S, dim=0), 1, perm) * mask
    return ids, types, mask.to(torch.float32)


def text_keep_batch(input_ids, token_type_ids, cam_text, steps=PERT_STEPS, is_positive_pert=False, n_tokens=None):
    """Perturbed question batch (``perturbation.py:158-176``): [CLS] and [SEP] always stay, the
    ``int((1 - step) * (T - 2))`` top-scoring inner tokens stay in their original order, the rest is dropped.
    Returns ``(ids [S, T], token_types [S, T], attention_mask [S, T])`` with the kept tokens left-aligned.
    ``n_tokens``: the question's real length when ``input_ids`` is padded to a longer ``T`` ([SEP] sits at ``n_tokens - 1``)."""
    return text_keep_batches(input_ids.reshape(1, -1), token_type_ids.reshape(1, -1), cam_text.reshape(1, -1), steps,
                             is_positive_pert, None if n_tokens is None else [n_tokens])


class LxmertPerturbation:
    """``ModelPert.perturbation_image`` / ``perturbation_text``, the 9 steps (and optionally B samples) in one batch.

    ``model``: an ``lxmert_model.LxmertForQuestionAnswering``.  ``inputs``: the tensors the reference's ``forward``
    hands to the model -- ``input_ids``, ``attention_mask``, ``token_type_ids`` (``[B, T]``), ``visual_feats``
    (``[B, I, F]``), ``visual_pos`` (``[B, I, 4]``); B = 1 for the reference's one-item call, B > 1 for items of equal
    question length.  ``cam_image [I]`` / ``cam_text [T]`` (or ``[B, I]`` / ``[B, T]``).  Both methods return the answer
    scores ``[S, num_answers]`` (``[B, S, num_answers]`` for 2-D cams); ``accuracy`` turns them into the per-step VQA
    soft accuracies (``label_scores[argmax]``, ``perturbation.py:134-136``).
    """

    def __init__(self, model, steps=PERT_STEPS, tuned=False, grouped=True):
        """``tuned`` (default OFF since round 6): run the re-runs' library GEMMs with a TunableOp selection ``tuned_gemms`` holds
        under "lxmert_pert" (on for the duration of a call only; a no-op without such a file -- the one of rounds 3-5 was removed: one
        of its solutions hung the GPU at the text test's 5760-row shapes)."""
        self.model = model
        self.steps = tuple(steps)
        self.tuned = tuned
        self.grouped = grouped      # False: all live steps as ONE masked batch over the largest keep count (rounds 1-5; A / B runs)
        self._const = {}

    def _image_constants(self, I, device):
        """Per (region count, device): the steps' keep counts, the live / region-free step indices -- built ONCE from host
        arithmetic (as the reference does per call), so that a call creates no tensor from a host list (hipGraph-capturable)."""
        key = (I, str(device), self.steps, self.grouped)
        if key not in self._const:
            counts = [int((1 - step) * I) for step in self.steps]
            live = [s for s, c in enumerate(counts) if c > 0]
            dead = [s for s in range(len(self.steps)) if s not in live]
            self._const[key] = (torch.tensor(counts, device=device), live, torch.tensor(live, device=device, dtype=torch.long),
                                torch.tensor(dead, device=device, dtype=torch.long), self._step_groups(counts, live, device, self.grouped))
        return self._const[key]

    @staticmethod
    def _step_groups(counts, live, device, split=True):
        """The live steps in at most two GROUPS, each scored as one batch over the ``kmax`` top-ranked regions of every sample (the
        reference gathers the kept regions, ``perturbation.py:114-121``; a group's steps that keep fewer mask the tail): the split that
        needs the fewest region rows -- (36, 27, 18 | 9, 7, 5, 3, 1) for 36 regions: 153 rows against 288 for one masked batch.
        -> ``[(step index tensor, kmax, keep mask [n, kmax])]``, device constants built once (nothing from host lists under a capture)."""
        by_count = sorted(live, key=lambda s: -counts[s])
        n = len(by_count)
        if n == 0:
            return []
        best, cut = n * counts[by_count[0]], n
        for p in range(1, n if split else 1):
            rows = p * counts[by_count[0]] + (n - p) * counts[by_count[p]]
            if rows < best:
                best, cut = rows, p
        groups = []
        for part in (by_count[:cut], by_count[cut:]):
            if part:
                kmax = counts[part[0]]
                keep = (torch.arange(kmax, device=device)[None, :] < torch.tensor([counts[s] for s in part], device=device)[:, None])
                groups.append((torch.tensor(part, device=device, dtype=torch.long), kmax, keep.to(torch.float32)))
        return groups

    def _scores(self, **kw):
        """Answer scores of one batched re-run: the body's grad-free fast forward when it has one."""
        fast = getattr(self.model, "scores_no_grad", None)
        return fast(**kw) if fast is not None else self.model(**kw).question_answering_score

    @staticmethod
    def _rep(x, S):
        return x.repeat_interleave(S, dim=0)

    def perturbation_image(self, inputs, cam_image, is_positive_pert=False):
        with tuned_gemms.scope("lxmert_pert") if self.tuned else contextlib.nullcontext():
            return self._perturbation_image(inputs, cam_image, is_positive_pert)

    def perturbation_text(self, inputs, cam_text, is_positive_pert=False):
        with tuned_gemms.scope("lxmert_pert") if self.tuned else contextlib.nullcontext():
            return self._perturbation_text(inputs, cam_text, is_positive_pert)

    @torch.no_grad()
    def _perturbation_image(self, inputs, cam_image, is_positive_pert=False):
        single = cam_image.dim() == 1
        cams = cam_image.reshape(-1, cam_image.shape[-1])
        B, I = cams.shape
        S = len(self.steps)
        _, live, _, dead, groups = self._image_constants(I, cams.device)                            # host arithmetic only, cached
        scores = None
        if live:
            # ONE stable ranking per sample (module docstring: tie policy); every step keeps a prefix of it, so a group of steps is the
            # gather of the group's kmax top-ranked regions (in rank order, as the reference's ``topk`` hands them over -- the visual
            # stream has no index-dependent term) plus a mask for the steps that keep fewer.  Round 6: before, all live steps ran as
            # ONE batch over all I regions with masks -- 288 region rows per sample instead of 153 for the same answers.
            order = ranking(-cams if is_positive_pert else cams)                                    # [B, I]
            fast = hasattr(self.model, "scores_no_grad")
            lang = self.model.encode_language(inputs["input_ids"], inputs["attention_mask"], inputs["token_type_ids"]) \
                if fast and hasattr(self.model, "encode_language") and len(groups) > 1 else None
            for steps_g, kmax, keep_g in groups:
                n = steps_g.numel()
                top = order[:, :kmax]
                feats = torch.gather(inputs["visual_feats"], 1, top.unsqueeze(-1).expand(-1, -1, inputs["visual_feats"].shape[-1]))
                pos = torch.gather(inputs["visual_pos"], 1, top.unsqueeze(-1).expand(-1, -1, inputs["visual_pos"].shape[-1]))
                vis = dict(visual_feats=self._rep(feats, n), visual_pos=self._rep(pos, n), visual_attention_mask=keep_g.repeat(B, 1))
                if fast:
                    # the text is the same in all n re-runs of a sample: its own 9 layers run once per sample (lang_repeat), and
                    # once for all groups (lang_encoded)
                    out = self.model.scores_no_grad(input_ids=inputs["input_ids"], attention_mask=inputs["attention_mask"],
                                                    token_type_ids=inputs["token_type_ids"], lang_repeat=n, lang_encoded=lang, **vis)
                else:
                    out = self._scores(input_ids=self._rep(inputs["input_ids"], n),
                                       attention_mask=self._rep(inputs["attention_mask"], n),
                                       token_type_ids=self._rep(inputs["token_type_ids"], n), **vis)
                if scores is None:
                    scores = out.new_empty(B, S, out.shape[-1])
                scores[:, steps_g] = out.reshape(B, n, -1)
        if len(live) < S:                                    # steps that keep no region at all: region-free forward
            out = self._scores(input_ids=inputs["input_ids"], attention_mask=inputs["attention_mask"],
                               token_type_ids=inputs["token_type_ids"], visual_feats=inputs["visual_feats"][:, :0],
                               visual_pos=inputs["visual_pos"][:, :0])
            if scores is None:
                scores = out.new_empty(B, S, out.shape[-1])
            scores[:, dead] = out[:, None, :]
        return scores[0] if single else scores

    @torch.no_grad()
    def _perturbation_text(self, inputs, cam_text, is_positive_pert=False):
        single = cam_text.dim() == 1
        cams = cam_text.reshape(-1, cam_text.shape[-1])
        B, S = cams.shape[0], len(self.steps)
        # per-sample question lengths (a padded batch): one device->host read for the whole batch
        mask = inputs.get("attention_mask")
        lens = mask.sum(dim=1).tolist() if mask is not None and mask.shape[1] == cams.shape[1] else [None] * B
        ids, types, mask = text_keep_batches(inputs["input_ids"], inputs["token_type_ids"], cams, self.steps, is_positive_pert,
                                             n_tokens=lens)                                         # [B*S, T]
        if hasattr(self.model, "scores_no_grad") and inputs["visual_feats"].shape[1] > 0:
            # the regions are the same in all S re-runs of a sample: their own 5 layers run once per sample (visn_repeat)
            out = self.model.scores_no_grad(input_ids=ids, attention_mask=mask, token_type_ids=types,
                                            visual_feats=inputs["visual_feats"], visual_pos=inputs["visual_pos"], visn_repeat=S)
        else:
            out = self._scores(input_ids=ids, attention_mask=mask, token_type_ids=types,
                               visual_feats=self._rep(inputs["visual_feats"], S), visual_pos=self._rep(inputs["visual_pos"], S))
        out = out.reshape(B, S, -1)
        return out[0] if single else out

    def text_step_groups(self, T, max_groups=2, device=None):
        """Host only: the steps of the text test on questions padded to ``T`` tokens, in at most ``max_groups`` GROUPS that each run
        at their own width.  Step s keeps ``2 + int((1 - step_s) * (n - 2))`` tokens of a question of n tokens, left-aligned, and
        ``int((1 - step) * w)`` does not decrease with w: ``P_s = 2 + int((1 - step_s) * (T - 2))`` bounds the new length of EVERY
        question of the padded batch, from ``T`` alone.  The steps, sorted by descending ``P_s``, are cut into contiguous groups of
        width ``Q_g = max P_s``; of all cuts the one with the fewest rows ``sum n_g * Q_g`` per sample is taken -- (20, 15, 11 | 6, 5,
        4, 3, 2, 2) at T = 20: 96 text rows per sample against 180 at full width, 86 with three groups.

        -> a namespace, cached per ``(T, device, steps, max_groups)``: ``rows`` (per sample); ``counts [S, T - 1]`` int32 on the device
        (``counts[s][w] = int((1 - step_s) * w)``, host arithmetic as ``perturbation.py:168``); ``groups``: a list of ``(step index
        tensor, n_g, Q_g)``; ``layout(B)`` (host, kept per B): ``table``, the placement table of ``ops.lxmert_perturb_text`` for a
        batch of B, ``offsets``, the element at which every group's block starts, and ``elems``, the length of the buffers.  Group g
        is a contiguous ``[B * n_g, Q_g]`` block with the n_g steps of a sample adjacent (sample-major, so that ``visn_repeat = n_g``
        lines up): its steps share the stride ``n_g * Q_g`` and sit in the windows ``j * Q_g`` of a period, which is why a block
        starts at a multiple of its stride (the entry's rule for interleaved steps; the few elements skipped are never touched)."""
        T, max_groups = int(T), int(max_groups)
        if T < 2 or max_groups < 1:
            raise ValueError("text_step_groups: needs T >= 2 and max_groups >= 1 (got T=%d, max_groups=%d)" % (T, max_groups))
        key = ("text", T, str(device), self.steps, max_groups)
        if key in self._const:
            return self._const[key]
        S = len(self.steps)
        bound = [2 + int((1 - step) * (T - 2)) for step in self.steps]
        order = sorted(range(S), key=lambda s: -bound[s])                     # stable: equal bounds keep their step order
        # cheapest cut of the sorted steps into at most max_groups contiguous groups: cost[g][i] = fewest rows for the first i steps in
        # g groups (a group a .. i - 1 costs (i - a) * its first, i.e. largest, bound); S^2 * groups steps of host arithmetic
        G, inf = min(max_groups, S), float("inf")
        cost = [[inf] * (S + 1) for _ in range(G + 1)]
        back = [[0] * (S + 1) for _ in range(G + 1)]
        cost[0][0] = 0
        for g in range(1, G + 1):
            for i in range(1, S + 1):
                for a in range(g - 1, i):
                    rows = cost[g - 1][a] + (i - a) * bound[order[a]]
                    if rows < cost[g][i]:
                        cost[g][i], back[g][i] = rows, a
        g = min(range(1, G + 1), key=lambda n: (cost[n][S], n))                # the fewest groups among equally cheap cuts
        rows, edges, i = cost[g][S], [S], S
        while g > 0:
            i = back[g][i]
            edges.append(i)
            g -= 1
        edges = edges[::-1]
        parts = [(order[a:b], b - a, bound[order[a]]) for a, b in zip(edges, edges[1:])]
        layouts = {}

        def layout(B):
            if B not in layouts:
                table, offsets, at = [None] * S, [], 0
                for steps_g, n, width in parts:
                    at = -(-at // (n * width)) * (n * width)
                    offsets.append(at)
                    for j, s in enumerate(steps_g):
                        table[s] = (at + j * width, n * width, width)
                    at += B * n * width
                layouts[B] = types.SimpleNamespace(table=ops.text_placement(table), offsets=offsets, elems=at)
            return layouts[B]

        counts = torch.tensor([[int((1 - step) * w) for w in range(T - 1)] for step in self.steps], dtype=torch.int32, device=device)
        groups = [(torch.tensor(steps_g, dtype=torch.long, device=device), n, width) for steps_g, n, width in parts]
        self._const[key] = types.SimpleNamespace(rows=rows, counts=counts, groups=groups, layout=layout, bounds=bound,
                                                 steps=[list(p[0]) for p in parts])
        return self._const[key]

    def perturbation_text_grouped(self, inputs, cam_text, is_positive_pert=False, max_groups=2):
        """The text test of a padded batch on device-built step groups: ``cam_text [B, T]`` -> answer scores ``[B, S, answers]``, the
        ones ``perturbation_text`` gives.  The question lengths stay on the device (``attention_mask.sum``; ``T`` without a mask), ONE
        ``ops.lxmert_perturb_text`` launch writes every step's questions into its group's block at the group's width
        (``text_step_groups``), the regions' own layers run once (``encode_vision``) and every group is one ``scores_no_grad``.  No
        host read, and after the first call of a shape no tensor built from a host list: capturable (``GraphedTextPerturbation``)."""
        with tuned_gemms.scope("lxmert_pert") if self.tuned else contextlib.nullcontext():
            return self._perturbation_text_grouped(inputs, cam_text, is_positive_pert, max_groups)

    @torch.no_grad()
    def _perturbation_text_grouped(self, inputs, cam_text, is_positive_pert=False, max_groups=2):
        if cam_text.dim() != 2 or cam_text.shape != inputs["input_ids"].shape:
            raise ValueError("perturbation_text_grouped: cam_text must be [B, T] like input_ids, got %s / %s"
                             % (tuple(cam_text.shape), tuple(inputs["input_ids"].shape)))
        if inputs["visual_feats"].shape[1] == 0:
            raise ValueError("perturbation_text_grouped: needs a non-empty region set")
        B, T = cam_text.shape
        S = len(self.steps)
        plan = self.text_step_groups(T, max_groups, cam_text.device)
        mask = inputs.get("attention_mask")
        text_len = mask.sum(dim=1).to(torch.int32) if mask is not None else \
            torch.full((B,), T, dtype=torch.int32, device=cam_text.device)
        where = plan.layout(B)
        ids, types_, keep, _ = ops.lxmert_perturb_text(inputs["input_ids"], inputs["token_type_ids"], cam_text.to(torch.float32), text_len,
                                                       plan.counts, where.table, where.elems, is_positive_pert)
        visn = self.model.encode_vision(inputs["visual_feats"], inputs["visual_pos"])
        scores = None
        for (steps_g, n, width), offset in zip(plan.groups, where.offsets):
            block = slice(offset, offset + B * n * width)
            out = self.model.scores_no_grad(input_ids=ids[block].view(B * n, width), attention_mask=keep[block].view(B * n, width),
                                            token_type_ids=types_[block].view(B * n, width), visn_encoded=visn, visn_repeat=n)
            if scores is None:
                scores = out.new_empty(B, S, out.shape[-1])
            scores[:, steps_g] = out.reshape(B, n, -1)
        return scores

    @staticmethod
    def accuracy(scores, label_scores):
        """``label_scores [num_answers]`` (or ``[B, num_answers]`` for batched scores): the item's soft VQA scores per
        answer id (0 where absent) -> ``[S]`` (``[B, S]``)."""
        best = scores.argmax(dim=-1)
        return label_scores[best] if label_scores.dim() == 1 else torch.gather(label_scores, 1, best)



class GraphedImagePerturbation:
    """``normalize_cams_batch`` + ``LxmertPerturbation.perturbation_image`` + ``accuracy`` of a fixed-shape batch captured ONCE into
    a hipGraph and replayed: the 9-step test of a batch is ~700 launches of eager PyTorch (two grad-free forwards at 8x and 1x the
    batch), i.e. ~20 ms of HOST time per batch on the thread that also has to replay the explain graph -- with one process per GPU
    that, not the device work, bounded the evaluator (round 5: 465-507 samples / s end to end against 1170 for the device legs).

        run = GraphedImagePerturbation(pert, batch, R_t_t, R_t_i, labels)       # example tensors of the shapes to come
        acc = run(batch, R_t_t, R_t_i, labels)                                    # [B, S] per-step soft accuracies (graph output)

    The library GEMMs inside run with the DEFAULT selection (a tuned selection is not switched under a capture, ``tuned_gemms.scope``).
    Image test only: ``perturbation_text`` reads the question lengths on the host; the text test that is captured is
    ``perturbation_text_grouped`` (``GraphedTextPerturbation``)."""

    def __init__(self, pert, batch, R_t_t, R_t_i, labels, is_positive_pert=False, warmup=2):
        self.pert, self.positive = pert, bool(is_positive_pert)
        self.static = {k: v.clone() for k, v in batch.items()}
        self.R_t_t, self.R_t_i, self.labels = R_t_t.clone(), R_t_i.clone(), labels.clone()
        self.graph, self.out, self._pinned = graphed.capture(self._call, warmup, pert.model)

    def _call(self):
        cam_image, _ = normalize_cams_batch(self.R_t_t, self.R_t_i, self.static["attention_mask"])
        scores = self.pert._perturbation_image(self.static, cam_image, self.positive)
        return LxmertPerturbation.accuracy(scores, self.labels)

    def __call__(self, batch, R_t_t, R_t_i, labels):
        graphed.copy_inputs(self.static, batch)
        self.R_t_t.copy_(R_t_t)
        self.R_t_i.copy_(R_t_i)
        self.labels.copy_(labels)
        self.graph.replay()
        return self.out


class GraphedTextPerturbation:
    """``normalize_cams_batch`` + ``LxmertPerturbation.perturbation_text_grouped`` + ``accuracy`` of a fixed-shape batch captured ONCE
    into a hipGraph and replayed for any ragged batch of that shape -- ``GraphedImagePerturbation`` for the text test:

        run = GraphedTextPerturbation(pert, batch, R_t_t, R_t_i, labels)        # example tensors of the shapes to come
        acc = run(batch, R_t_t, R_t_i, labels)                                    # [B, S] per-step soft accuracies (graph output)

    The question lengths are read from ``attention_mask`` on the device inside the graph; the step groups' widths depend on the padded
    length alone.  The library GEMMs inside run with the DEFAULT selection.  ``max_groups``: see ``text_step_groups``."""

    def __init__(self, pert, batch, R_t_t, R_t_i, labels, is_positive_pert=False, warmup=2, max_groups=2):
        self.pert, self.positive, self.max_groups = pert, bool(is_positive_pert), int(max_groups)
        self.static = {k: v.clone() for k, v in batch.items()}
        self.R_t_t, self.R_t_i, self.labels = R_t_t.clone(), R_t_i.clone(), labels.clone()
        self.graph, (self.out, self.scores), self._pinned = graphed.capture(self._call, warmup, pert.model)

    def _call(self):
        _, cam_text = normalize_cams_batch(self.R_t_t, self.R_t_i, self.static["attention_mask"])
        scores = self.pert._perturbation_text_grouped(self.static, cam_text, self.positive, self.max_groups)
        return LxmertPerturbation.accuracy(scores, self.labels), scores      # (``scores [B, S, answers]``: a graph output too)

    def __call__(self, batch, R_t_t, R_t_i, labels):
        graphed.copy_inputs(self.static, batch)
        self.R_t_t.copy_(R_t_t)
        self.R_t_i.copy_(R_t_i)
        self.labels.copy_(labels)
        self.graph.replay()
        return self.out
