"""Drop-in ``interpret`` for CLIP -- same signatures as the reference, relevancy chain on the fused HIP kernel.

Reference entry points mirrored here:
  * ``interpret(image, texts, model, device, start_layer=-1, start_layer_text=-1)``
    -- CLIP_explainability.ipynb cell 6 (batched: one image, B texts) -> ``(text_relevance [B,Nt,Nt], image_relevance [B,Ni-1])``
  * ``interpret_single(image, text, model, device, index=None)``
    -- CLIP/example.py:8-32 (one image, K texts, explains ``logits_per_image[0, index]``) -> ``image_relevance [Ni-1]``
    (``clip_example.interpret`` under the reference's name); ``interpret_batch`` runs it over B distinct images in one pass,
    ``interpret_batch_multi`` with the top-K prompts of every image
  * ``interpret_grouped(images, texts, model, device)`` -- cell 6 with K captions per image (caption i against image i // K)
  * ``text_scores(text_encoding, R_text)`` -- notebook cell 8:5-7 post-processing (on device)

What is different under the hood (results agree to fp32 rounding, see tests/test_gpu_clip.py):
  * the reference issues one ``torch.autograd.grad`` per layer (24 partial backward passes); here ONE hand-written
    backward per tower (``clip_model.Transformer.forward_tape`` / ``backward_tape``: no autograd graph through the bodies,
    no weight gradients, fused LayerNorm / QuickGELU / attention-capture kernels) fills every layer's gradient slab;
  * the per-layer reshape/mul/clamp/mean/bmm/add launches are one ``relevancy_self_chain`` launch per tower.
"""
from __future__ import annotations

import numpy as np
import torch

from . import graphed, ops
from .rules import frozen_parameters as _Frozen

def _plan(buffers, first, last, batch_size, shared, half_chain=False, causal=False):
    """Prepared chain launch, cached on the slab object (the slabs keep their addresses from call to call).  ``half_chain``:
    the reference's fp16 chain (a model after ``set_body_dtype(torch.float16)``; ``ops.ChainPlan``).  ``causal``: the tower's
    attention carries CLIP's causal mask (the text tower, CLIP/clip/model.py:334-340): its probabilities are exact zeros above the
    diagonal and the chain kernel does not read that half of either slab (``MMX_CHAIN_CAUSAL``)."""
    cache = buffers.__dict__.setdefault("_chain_plans", {})
    key = (first, last, batch_size, shared, bool(half_chain), bool(causal))
    if key not in cache:
        cache[key] = ops.ChainPlan([buffers.probs[l] for l in range(first, last)],
                                   [buffers.grads[l] for l in range(first, last)], batch_size, shared_attn=shared,
                                   half_chain=half_chain, causal=causal)
    return cache[key]


def _is_causal_tower(tower):
    """True iff every block of ``tower`` runs under an additive mask that is -inf strictly above the diagonal (CLIP's
    ``build_attention_mask``, CLIP/clip/model.py:334-340): its probabilities are then exact zeros there and the chain may skip that
    half (``_plan(causal=True)``).  Checked on the mask tensors themselves, once per mask object (one device -> host read, made during
    the warm-up call that precedes any hipGraph capture); anything else -- no mask, another mask -- is not causal."""
    return tower.is_causal()


def _side_stream(device):
    """The side stream of the image tower (``ops.side_stream``: shared by eager calls, private to a capture inside one)."""
    return ops.side_stream(device)


def _head_grads(model, img_feat, txt_feat, batch_size, img_group=1):
    """``(d image_features, d text_features)`` of ``sum_i logits_per_image[i, i]`` (cell 6:6-10), one row per caption; caption i is
    paired with image row 0 when ``img_feat`` holds one image, else with row ``i // img_group``.  fp32 features: ONE launch of the
    closed form (``ops.clip_head_grads``; ``ops.set_option("clip_head_fused", 0)`` restores autograd, another rounding of the same
    numbers).  Anything else: autograd over ``CLIP.logits`` on per-caption leaves, as the notebook does it."""
    if (img_feat.dtype == torch.float32 and txt_feat.dtype == torch.float32 and img_feat.is_cuda and txt_feat.is_cuda
            and model.logit_scale.dtype == torch.float32 and ops.clip_head_fused_enabled()):
        d_img, d_txt, _ = ops.clip_head_grads(img_feat.detach().contiguous(), txt_feat.detach().contiguous(),
                                              model.logit_scale.detach(), img_group)
        return d_img, d_txt
    with torch.enable_grad():
        if img_feat.shape[0] == 1:
            image_features = img_feat.detach().expand(batch_size, -1).contiguous().requires_grad_(True)   # per-sample leaves
        elif img_group > 1:
            image_features = img_feat.detach().repeat_interleave(img_group, 0).requires_grad_(True)       # cell 6:3
        else:
            image_features = img_feat.detach().contiguous().requires_grad_(True)
        text_features = txt_feat.detach().requires_grad_(True)
        logits_per_image, _ = model.logits(image_features, text_features)
        # one_hot = sum_i logits_per_image[i, i]  (cell 6:6-10)  ->  d one_hot / d logits = I
        eye = torch.eye(batch_size, dtype=torch.float32, device=txt_feat.device)
        torch.autograd.backward(logits_per_image, grad_tensors=eye, inputs=[image_features, text_features])
    return image_features.grad, text_features.grad


def interpret(image, texts, model, device, start_layer=-1, start_layer_text=-1, share_image_forward=True,
              trim_text_padding=False, _n_text=None, overlap_towers=True, image_chain_on_main=False):
    """CLIP_explainability.ipynb cell 6.  ``image``: ``[1,3,R,R]``, ``texts``: ``[B, context]`` token ids.

    ``share_image_forward`` (extra keyword, default on): the reference repeats the ONE image B times (cell 6:3) and
    runs the image tower on B identical copies.  Here its forward runs once and only the backward -- whose upstream
    gradients do differ per text -- runs at batch B (``clip_model.Transformer.forward_shared``); results are the
    same to fp32 rounding (``tests/test_gpu_clip.py``).  ``False`` runs the B copies like the reference.

    ``trim_text_padding`` (extra keyword, default OFF): CLIP pads every caption to 77 tokens and the reference runs the
    text tower over all of them.  The mask is causal and the feature is read at the EOT token, so positions after the
    last EOT of the batch influence nothing: their gradient rows are exactly zero and the returned ``R_text`` is the
    identity there.  With the flag the text tower runs only on the first ``max(EOT)+1`` positions and the ``[B,77,77]``
    result is assembled around that block -- identical output, 5-6x less text-tower work for caption-length inputs.

    The text tower's backward runs on the rows up to each caption's EOT token only (on by default; ``clip_model.Transformer.
    _live_rows_route``): the mask is causal and the feature is read at the EOT token, so every gradient row past it is an exact zero.
    Unlike ``trim_text_padding`` this is decided on the device per call -- no read of the ids, shapes / slabs / accessors unchanged, a
    captured graph follows whatever captions it is replayed with.  The text tower's FORWARD runs on the same rows (``clip_model.
    Transformer.forward_tape(live=...)``; ``ops.set_option("text_live_rows_fwd", 0)`` keeps it dense): the rows past EOT feed neither
    the feature nor any gradient.  Inside that route the attention takes the caption lengths too, forward and backward, where the
    whole-head kernels have a live-length instantiation (65 ... 80 tokens: every CLIP text tower has 77): no dead row of ``qkv`` is
    read, so ``qkv`` is not zero-filled either; ``ops.set_option("text_live_attn", 0)`` restores the dense attention over a zero-filled
    ``qkv`` (same bits; figures: ``profiles/text_attention_live_rows_probe.txt``).  The slabs then hold what the maps need (a filler in the probabilities' padded rows, zeros in the
    gradients' masked entries past EOT) until ``blk.attn_probs`` / ``blk.attn_grad`` is read, which completes them with one dense pass
    (``Transformer.complete_attn_probs``; figures: ``profiles/text_forward_live_rows_probe.txt``).  Cost of that first read: the
    whole dense text forward and the text backward once more (about the text tower's share of a step of the dense path); later reads
    are free until the next call, and a caller that only wants the maps never pays it.
    ``ops.set_option("text_live_rows", 0)`` switches both off process-wide.  Price: captions at the
    truncation limit (77 tokens) have no dead rows and the row-list GEMM then does the library GEMM's work (figures, once measured:
    ``profiles/text_backward_live_rows_probe.txt``); the switch is the answer for such inputs.
    An fp16 body (``model.set_body_dtype(torch.float16)``, the reference's ``convert_weights`` mode) keeps its dense text tower unless
    ``ops.set_option("text_live_rows_half", 1)`` (default 0): the same route then, with its GEMMs on the fp16 matrix cores
    (``mmx_gemm_rows_f16``: activations rounded to fp16 inside the kernel, fp32 accumulation -- the dense fp16 path's roundings, another
    order of the fp32 sums; figures: ``profiles/text_live_rows_half_probe.txt``).  bf16 bodies stay dense.

    ``overlap_towers`` (extra keyword, default on): image tower on a side stream, text tower on the current one (they
    only meet in the similarity head); ``False`` runs them back to back on the current stream.  Same results bit for bit.

    ``image_chain_on_main`` (extra keyword, default off): launch the image tower's chain kernel on the CURRENT stream after
    the text tower's work instead of on the side stream next to the text tower's GEMMs (where it measured 118 us instead of
    its stand-alone 44 us); ``bench.py`` reports the step rate of both orders.  Same results.
    """
    batch_size = texts.shape[0]
    sl = model.visual.transformer.layers - 1 if start_layer == -1 else start_layer
    slt = model.transformer.layers - 1 if start_layer_text == -1 else start_layer_text
    n_text = _n_text
    if trim_text_padding and n_text is None:
        n_text = int(texts.argmax(dim=-1).max()) + 1                                      # one D2H read of the ids
    shared = share_image_forward and image.shape[0] == 1 and batch_size > 1
    # Both towers on the tape path (clip_model.Transformer.forward_tape / backward_tape): no autograd graph through the
    # bodies, no weight gradients; the cosine-similarity head (B x embed_dim features) is one closed-form kernel (_head_grads).
    images = image.type(model.dtype) if shared or image.shape[0] == batch_size else \
        image.type(model.dtype).repeat(batch_size, 1, 1, 1)                                # cell 6:3
    # The two towers are independent up to the similarity head.  The image tower runs on a side stream: its shared
    # forward is ~120 batch-1 launches of a few microseconds (latency-bound) that hide completely behind the text
    # tower's GEMMs, and in the backward the kernel-boundary gaps of one tower are filled by the other's kernels.
    # Fork / join with stream waits only, so the whole thing still captures into one hipGraph (parallel branches).
    main = torch.cuda.current_stream()
    side = _side_stream(texts.device) if overlap_towers else main
    side.wait_stream(main)
    # bf16-body image tower (cfg 5): only R[:, 0, 1:] is returned, so the relevancy ROW is carried through the backward
    # (clip_model.Transformer.backward_tape, rel_row) -- no gradient slabs, no A-bar / R matrices for the image side
    row_mode = shared and model.visual.row_relevancy_ok()
    with torch.cuda.stream(side):
        img_feat, img_state = model.visual.forward_tape(images, batch_size, sl, grads=not row_mode)
    txt_feat, txt_state = model.encode_text_tape(texts, n_text, slt)
    main.wait_stream(side)
    d_image_features, d_text_features = _head_grads(model, img_feat, txt_feat, batch_size)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        vis = model.visual.transformer
        if row_mode:
            image_relevance = model.visual.backward_tape(img_state, d_image_features, sl, cls_row=True)[:, 1:]
        else:
            model.visual.backward_tape(img_state, d_image_features, sl)
            if not image_chain_on_main:
                R = _plan(vis.buffers, sl, vis.layers, batch_size, vis.buffers.shared_probs and batch_size > 1,
                          getattr(vis, "half_chain", False)).launch()
                image_relevance = R[:, 0, 1:]
    model.backward_text_tape(txt_state, d_text_features, slt)
    txt = model.transformer
    R_text = _plan(txt.buffers, slt, txt.layers, batch_size, False, getattr(txt, "half_chain", False),
                   causal=_is_causal_tower(txt)).launch()
    main.wait_stream(side)
    if image_chain_on_main and not row_mode:
        R = _plan(vis.buffers, sl, vis.layers, batch_size, vis.buffers.shared_probs and batch_size > 1,
                  getattr(vis, "half_chain", False)).launch()
        image_relevance = R[:, 0, 1:]
    if R_text.shape[-1] != texts.shape[1]:       # trimmed run: the rest of the [B, 77, 77] matrix is the identity
        n = R_text.shape[-1]
        full = torch.eye(texts.shape[1], dtype=R_text.dtype, device=R_text.device).repeat(batch_size, 1, 1)
        full[:, :n, :n] = R_text
        R_text = full
    return R_text, image_relevance


class GraphedInterpret:
    """``interpret`` captured once into a hipGraph and replayed: the step is ~600 short launches (PyTorch body ops, our
    attention / chain kernels) and an eager step is bound by the Python + launch path on the host (~16 ms) rather than by
    the GPU; a replay costs one ``hipGraphLaunch``.  Shapes, ``start_layer``s and flags are fixed at construction;
    new ``image`` / ``texts`` values are copied into the captured input buffers.

        run = GraphedInterpret(model, image, texts, start_layer=0, start_layer_text=0)
        R_text, image_relevance = run(image2, texts2)      # same results as interpret(image2, texts2, model, device, 0, 0)

    The returned tensors are the graph's output buffers (overwritten by the next call; ``.clone()`` to keep them).
    """

    def __init__(self, model, image, texts, start_layer=-1, start_layer_text=-1, share_image_forward=True,
                 trim_text_padding=False, warmup=3, image_chain_on_main=False):
        self.model = model
        self.image = image.clone()
        self.texts = texts.clone()
        kw = dict(start_layer=start_layer, start_layer_text=start_layer_text, share_image_forward=share_image_forward,
                  image_chain_on_main=image_chain_on_main)
        # a trimmed run fixes the number of text positions at capture time: it must cover every later caption
        self.n_text = int(texts.argmax(dim=-1).max()) + 1 if trim_text_padding else None
        self._call = lambda: interpret(self.image, self.texts, model, self.image.device, _n_text=self.n_text, **kw)
        self.graph, self.outputs, self._pinned_scratch = graphed.capture(self._call, warmup, model)
        # The graph bakes in the raw addresses of the towers' capture slabs and of the cached chain plans' scratch.  Pin
        # them: a later interpret() / GraphedInterpret on the same model with another batch, sharing mode or text length
        # makes ``Transformer._ensure_buffers`` install NEW slabs, and without this reference the old ones would be
        # freed under the graph.  ``__call__`` re-installs the pinned slabs so that ``blk.attn_probs`` / ``attn_grad``
        # and a following eager call see what the replay wrote.
        vis, txt = model.visual.transformer, model.transformer
        self._pinned = (vis.buffers, txt.buffers)
        # a captured row-list text forward leaves the slabs pending after every replay (clip_model.Transformer.complete_attn_probs):
        # the captured block input, rows and upstream gradient rows -- they hold the last replay's values --, re-armed by __call__
        self._txt_pending = txt.__dict__.get("_probs_pending")
        txt._probs_pending = None              # (nothing has run yet: the capture recorded the kernels, the warm-up slabs are gone)
        if self._txt_pending is not None:
            # the row-list forward reads the cached TRANSPOSED copies of the text tower's weights, and the graph has their addresses:
            # keep them alive (an in-place weight update makes a later eager call replace the cache entries).  The replays go on
            # reading these copies -- weights changed after the capture need a new GraphedInterpret to be seen
            # (an fp16 body on the route, option text_live_rows_half: the two cached fp16 copies instead)
            half = getattr(txt, "forward_gemm_dtype", torch.float32) == torch.float16
            self._pinned_weights = [
                copy for blk in txt.resblocks
                for w in (blk.attn.in_proj_weight, blk.attn.out_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight)
                for copy in ((ops._converted(w, torch.float16), ops.transposed_half_weight(w)) if half else (ops.transposed_weight(w),))]

    def _reinstall(self):
        for tr, buf in zip((self.model.visual.transformer, self.model.transformer), self._pinned):
            if tr.buffers is not buf:
                tr.buffers = buf
                for l, blk in enumerate(tr.resblocks):
                    blk.attn_probs, blk.attn_grad = buf.layer_probs(l), buf.layer_grads(l)

    def __call__(self, image=None, texts=None):
        self._reinstall()
        if image is not None:
            self.image.copy_(image)
        if texts is not None:
            if self.n_text is not None and int(texts.argmax(dim=-1).max()) + 1 > self.n_text:
                raise ValueError("caption longer than the %d positions this graph was captured for" % self.n_text)
            self.texts.copy_(texts)
        self.graph.replay()
        if self._txt_pending is not None:
            self.model.transformer._probs_pending = self._txt_pending
        return self.outputs


def interpret_single(image, text, model, device, index=None):
    """CLIP/example.py:8-32 without the plotting: returns ``image_relevance [Ni-1]`` (``R[0,0]`` zeroed first)."""
    prev = (model.capture_only, model.first_grad_layers)
    model.capture_only, model.first_grad_layers = True, (0, model.transformer.layers)   # text tower: no gradient work
    try:
        with _Frozen(model), torch.enable_grad():
            logits_per_image, _ = model(image, text)
            if index is None:
                index = int(np.argmax(logits_per_image.detach().cpu().numpy(), axis=-1).reshape(-1)[0])
            one_hot = torch.zeros_like(logits_per_image)
            one_hot[0, index] = 1
            torch.autograd.backward(logits_per_image, grad_tensors=one_hot)
    finally:
        model.capture_only, model.first_grad_layers = prev
    vis = model.visual.transformer
    vb = vis.buffers
    # example.py flattens batch*heads into one head axis (cam.reshape(-1, N, N).mean(0)): batch_size = 1 here
    R = ops.relevancy_self_chain([vb.probs[l] for l in range(vis.layers)],
                                 [vb.grads[l] for l in range(vis.layers)], 1)[0]
    R[0, 0] = 0
    return R[0, 1:]


def interpret_batch(images, texts, model, device, index=None):
    """Zero-shot explanation of B DISTINCT images against C class prompts in one pass -> ``image_relevance [B, Ni-1]``.

    Row b equals ``interpret_single(images[b:b+1], texts, model, device, index=index[b])`` (CLIP/example.py:8-32, one image
    per call).  ``index``: int tensor ``[B]`` of prompt indices, or ``None`` for each image's arg-max prompt (picked on the
    device).  The C prompts are encoded ONCE, forward only: the gradient of ``logits_per_image[b, c]`` with respect to image
    b depends on text feature c only, so the text tower runs no backward.  The image tower runs at batch B and carries row 0
    of its relevancy matrix through its backward (``Transformer.backward_tape(rel_row=...)``: the exact-fp32 row mode of the
    capture op on an fp32 body -- whole-head kernel at N <= 128, streaming kernels beyond; no gradient slabs are written)."""
    B = images.shape[0]
    with torch.no_grad():
        txt_feat, _ = model.encode_text_tape(texts, first_grad_layer=model.transformer.layers)   # no tape kept: no backward
        img_feat, img_state = model.visual.forward_tape(images.type(model.dtype), first_grad_layer=0, grads=False)
    with torch.enable_grad():
        image_features = img_feat.detach().requires_grad_(True)
        logits_per_image, _ = model.logits(image_features, txt_feat.detach())
        if index is None:
            idx = logits_per_image.detach().argmax(-1)
        else:
            idx = torch.as_tensor(index, device=logits_per_image.device).reshape(-1)
            if idx.numel() != B:
                raise ValueError("interpret_batch: %d indices for %d images" % (idx.numel(), B))
        one_hot = torch.zeros_like(logits_per_image).scatter_(1, idx.reshape(B, 1).long(), 1.0)
        torch.autograd.backward(logits_per_image, grad_tensors=one_hot, inputs=[image_features])
    row = model.visual.backward_tape(img_state, image_features.grad, 0, cls_row=True)
    return row[:, 1:]


def _fp32_clip(model, who):
    """The grouped row mode runs the exact-fp32 kernels only: refuse a bf16 / fp16 body by name."""
    for name, tower in (("image", model.visual.transformer), ("text", model.transformer)):
        for what in ("forward_gemm_dtype", "backward_gemm_dtype", "capture_dtype"):
            dt = getattr(tower, what, torch.float32)
            if dt != torch.float32:
                raise ops.MMXError("%s: fp32 bodies only (the exact-fp32 grouped row mode); the %s tower's %s is %s"
                                   % (who, name, what, str(dt).replace("torch.", "")))
    if model.dtype != torch.float32:
        raise ops.MMXError("%s: fp32 bodies only; the parameters are %s" % (who, str(model.dtype).replace("torch.", "")))


def _k_major_rows(rows, K, M):
    """``[K*M, ...]`` target rows in K-major order -> ``[M, K, ...]`` (image-major, what the caller passed)."""
    return rows.view(K, M, *rows.shape[1:]).transpose(0, 1)


def interpret_batch_multi(images, texts, model, device, index=None, top_k=None):
    """Zero-shot explanation of B DISTINCT images against C class prompts, K prompts per image, in one pass ->
    ``image_relevance [B, K, Ni-1]``.

    Entry ``[b, k]`` equals ``interpret_batch(images, texts, model, device, index=index[:, k])[b]`` (CLIP/example.py:8-32 per
    image and prompt).  ``index``: ``[B, K]`` prompt indices; ``None``: each image's ``top_k`` best prompts (default 1), picked
    on the device with ``topk``.  The C prompts are encoded once, forward only, and the image tower runs ONE forward at batch B;
    its backward carries the B*K class-token rows through the capture op's grouped row mode (an image's K targets share its
    forward operands).  fp32 bodies only."""
    _fp32_clip(model, "interpret_batch_multi")
    B = images.shape[0]
    if index is not None:
        idx = torch.as_tensor(index, device=images.device)
        if idx.dim() != 2 or idx.shape[0] != B or idx.shape[1] < 1:
            raise ValueError("interpret_batch_multi: index must be [B, K] = [%d, K], got %s" % (B, tuple(idx.shape)))
        K = idx.shape[1]
    else:
        K = 1 if top_k is None else int(top_k)
        if K < 1:
            raise ValueError("interpret_batch_multi: top_k must be >= 1")
    if K == 1:
        return interpret_batch(images, texts, model, device, None if index is None else idx.reshape(B)).unsqueeze(1)
    with torch.no_grad():
        txt_feat, _ = model.encode_text_tape(texts, first_grad_layer=model.transformer.layers)   # no tape kept: no backward
        img_feat, img_state = model.visual.forward_tape(images.type(model.dtype), first_grad_layer=0, grads=False)
    T = K * B
    with torch.enable_grad():
        # one leaf row per TARGET, K-major (t = k * B + b): each gets the gradient of its own logit only
        image_features = img_feat.detach().repeat(K, 1).requires_grad_(True)
        logits_per_image, _ = model.logits(image_features, txt_feat.detach())
        if index is None:
            idx = logits_per_image.detach()[:B].topk(K, dim=-1).indices
        one_hot = torch.zeros_like(logits_per_image).scatter_(1, idx.t().reshape(T, 1).long(), 1.0)
        torch.autograd.backward(logits_per_image, grad_tensors=one_hot, inputs=[image_features])
    row = model.visual.backward_tape(img_state, image_features.grad, 0, cls_row=True, targets_per_image=K)
    return _k_major_rows(row, K, B)[:, :, 1:].contiguous()


def interpret_grouped(images, texts, model, device, start_layer=-1, start_layer_text=-1):
    """CLIP_explainability.ipynb cell 6 with K captions per image: ``images [M, 3, R, R]``, ``texts [M*K, context]``; caption i
    is explained against image ``i // K`` -> ``(R_text [M*K, context, context], R_image [M*K, Ni-1])``.

    The same as ``interpret(images.repeat_interleave(K, 0), texts, model, device, start_layer, start_layer_text,
    share_image_forward=False)``: the text tower runs per caption (its backward and its causal relevancy chain, as there); the
    image tower runs ONE forward at batch M and the grouped row-mode backward over the M*K captions (row 0 of R only, the only
    row returned).  ``start_layer`` / ``start_layer_text`` keep their ``interpret`` meaning.  fp32 bodies only."""
    _fp32_clip(model, "interpret_grouped")
    M, T = images.shape[0], texts.shape[0]
    if M < 1 or T % M:
        raise ValueError("interpret_grouped: %d captions are not a whole number per image over %d images" % (T, M))
    K = T // M
    sl = model.visual.transformer.layers - 1 if start_layer == -1 else start_layer
    slt = model.transformer.layers - 1 if start_layer_text == -1 else start_layer_text
    img_feat, img_state = model.visual.forward_tape(images.type(model.dtype), None, sl, grads=False)
    txt_feat, txt_state = model.encode_text_tape(texts, None, slt)
    # caption order: row i of both gradients belongs to caption i, paired with image i // K (the reference's repeated images, cell 6:3)
    d_image_features, d_text_features = _head_grads(model, img_feat, txt_feat, T, img_group=K)
    # caption m*K + k -> target k*M + m (K-major, what the grouped backward addresses)
    d_img = _k_major_rows(d_image_features, M, K).reshape(T, -1)
    row = model.visual.backward_tape(img_state, d_img, sl, cls_row=True, targets_per_image=K)
    image_relevance = _k_major_rows(row, K, M).reshape(T, -1)[:, 1:]
    model.backward_text_tape(txt_state, d_text_features, slt)
    txt = model.transformer
    R_text = _plan(txt.buffers, slt, txt.layers, T, False, getattr(txt, "half_chain", False),
                   causal=_is_causal_tower(txt)).launch()
    return R_text, image_relevance


def text_scores(text_encoding, R_text):
    """Notebook cell 8:5-7 for one sample: row of the EOT token, columns ``1:EOT``, normalised by their sum."""
    cls_idx = int(text_encoding.argmax(dim=-1))
    row = R_text[cls_idx, 1:cls_idx]
    return (row / row.sum()).flatten()


def image_heatmap(image_relevance, size=224):
    """Notebook cell 7:14-18: reshape to the patch grid, bilinear upsample, min-max normalise -> ``[size, size]``
    (``postprocess.image_heatmaps`` does a whole batch in one launch)."""
    from .postprocess import image_heatmaps
    return image_heatmaps(image_relevance.reshape(-1), size)
