"""CLIP (ViT image tower + causal text tower) whose attention runs on the HIP capture op.

Role in this repo: the transformer body that FEEDS the relevancy engine.  Per BASELINE.json's north_star the
body's GEMMs / LayerNorms stay on PyTorch-ROCm; only the attention core is ours, writing P and dP into
preallocated slabs (``capture.CaptureBuffers``).  Parameter names and shapes are those of the reference's
``CLIP/clip/model.py`` (``visual.transformer.resblocks.{i}.attn.in_proj_weight`` ...), so a reference /
OpenAI ViT state dict loads with ``load_state_dict`` unchanged; the surface the explainability code touches
is kept too (reference file:line in the docstrings):

  * ``model.visual.transformer.resblocks`` / ``model.transformer.resblocks`` iterable of blocks
  * ``blk.attn_probs`` / ``blk.attn_grad`` -> ``[B*H, N, N]`` (CLIP/clip/model.py:181-193), here views of the slabs
  * ``model(image, text) -> (logits_per_image, logits_per_text)`` (model.py:364-378)

Design differences (MI355X-first, not a port): activations are batch-first ``[B, N, E]`` end to end (the
reference permutes to LND and back), q/k/v are strided views of the packed in-projection output consumed
in place by the kernel, the head-concatenated output is written by the kernel in the layout ``out_proj`` reads,
and ``capture_only`` mode cuts the autograd graph below the first block so ONE backward yields every layer's
dP without weight or input gradients.  ModifiedResNet towers (RN50 etc.) have no attention stack to explain
(reference notebooks use ViT-B/32) and are not built.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .capture import CaptureBuffers, attention_capture_packed


class QuickGELU(nn.Module):
    def forward(self, x):
        if x.is_cuda and x.dtype == torch.float32:
            return ops.quick_gelu(x)            # one fused HBM pass forward, one backward
        return x * torch.sigmoid(1.702 * x)     # parameter-only / CPU use of the module (no attention can run there)


class _OutProj(nn.Linear):
    """``attn.out_proj`` (name kept for state-dict compatibility)."""


class CapturedSelfAttention(nn.Module):
    """Packed-projection multi-head self-attention.  Parameters: ``in_proj_weight [3E, E]``, ``in_proj_bias``,
    ``out_proj`` -- the ``nn.MultiheadAttention`` naming the reference's ``MultiheadAttention`` uses
    (CLIP/clip/auxilary.py:265-356)."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        if embed_dim % num_heads:
            raise ValueError("embed_dim must be divisible by num_heads")
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = _OutProj(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)

    def forward(self, x, probs_slab, grads_slab, mask=None, need_dqkv=True, grad_hook=None):
        B, N, E = x.shape
        qkv = F.linear(x, self.in_proj_weight, self.in_proj_bias).view(B, N, 3, self.num_heads, self.head_dim)
        o = attention_capture_packed(qkv, probs_slab, grads_slab, self.head_dim ** -0.5, mask=mask,
                                     scale_mode=_lib.SCALE_Q_FIRST, need_dqkv=need_dqkv, grad_hook=grad_hook)
        return self.out_proj(o.view(B, N, E))


class ResidualAttentionBlock(nn.Module):
    """Pre-LN block (CLIP/clip/model.py:167-198).  ``attn_probs`` / ``attn_grad`` are slab views.

    Both are properties: after a row-list forward of the tower (``Transformer.forward_tape(live=...)``) the slabs hold what the maps
    need -- the probabilities of the live rows, the gradients of the entries at and below the diagonal -- and the first read of any
    block's ``attn_probs`` / ``attn_grad`` completes them (``Transformer.complete_attn_probs``).  Assigning to them
    (``set_attn_probs`` / ``set_attn_grad``, a forward) works as before."""

    def __init__(self, d_model, n_head, attn_mask=None):
        super().__init__()
        self.attn = CapturedSelfAttention(d_model, n_head)
        self.ln_1 = nn.LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([
            ("c_fc", nn.Linear(d_model, d_model * 4)),
            ("gelu", QuickGELU()),
            ("c_proj", nn.Linear(d_model * 4, d_model)),
        ]))
        self.ln_2 = nn.LayerNorm(d_model)
        self.attn_mask = attn_mask
        self.attn_probs = None
        self.attn_grad = None

    def _slab_view(self, name):
        owner = self.__dict__.get("_probs_owner")
        if owner is not None:
            owner[0].complete_attn_probs()             # (returns at once unless a row-list forward left the slabs pending)
        return self.__dict__.get(name)

    @property
    def attn_probs(self):
        return self._slab_view("_attn_probs")

    @attn_probs.setter
    def attn_probs(self, value):
        self.__dict__["_attn_probs"] = value

    @property
    def attn_grad(self):
        return self._slab_view("_attn_grad")

    @attn_grad.setter
    def attn_grad(self, value):
        self.__dict__["_attn_grad"] = value

    # kept for API parity with the reference block (model.py:184-188)
    def set_attn_probs(self, attn_probs):
        self.attn_probs = attn_probs

    def set_attn_grad(self, attn_grad):
        self.attn_grad = attn_grad

    def forward(self, x, buffers, layer, need_dqkv=True):
        if self.attn_mask is not None and (self.attn_mask.device != x.device):
            self.attn_mask = self.attn_mask.to(device=x.device, dtype=torch.float32)
        probs, grads = buffers.probs[layer], buffers.grads[layer]
        self.attn_probs = buffers.layer_probs(layer)
        self.attn_grad = buffers.layer_grads(layer)  # valid once backward has run
        mask = self.attn_mask
        if mask is not None and mask.shape[-1] != x.shape[1]:
            mask = mask[: x.shape[1], : x.shape[1]].contiguous()   # trimmed (padding-free) text batch
        x = x + self.attn(self.ln_1(x), probs, grads, mask=mask, need_dqkv=need_dqkv)
        x = x + self.mlp(self.ln_2(x))
        return x


class Transformer(nn.Module):
    def __init__(self, width, layers, heads, attn_mask=None):
        super().__init__()
        self.width, self.layers, self.heads = width, layers, heads
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, attn_mask) for _ in range(layers)])
        self.buffers = None
        # element type of the capture slabs: torch.float16 / torch.bfloat16 halve the resident bytes of a long-sequence
        # tower (ViT-L/14@336: 577 tokens); only the streaming attention kernels write them (capture op, ABI note)
        self.capture_dtype = torch.float32
        # dtype of the input-gradient GEMMs of ``backward_shared`` (the bulk of a long-sequence step: ViT-L/14@336 at
        # batch 128 is ~45 TFLOP of them).  torch.bfloat16 runs them on the bf16 MFMA with fp32 accumulation and fp32
        # results; everything else (forward, LayerNorm, attention, the relevancy rules) stays fp32.
        self.backward_gemm_dtype = torch.float32
        # A bf16 BODY (BASELINE config 5; the reference converts the weights, CLIP/clip/model.py:381-402, and runs the
        # whole tower in half precision): ``forward_gemm_dtype`` rounds the operands of the tape forward's GEMMs to bf16
        # (fp32 accumulate, fp32 activations between the GEMMs), ``attention_mma_bf16`` runs the attention products of
        # the long-sequence streaming kernels on the bf16 matrix cores (fp32 softmax).  R / A-bar stay fp32 always.
        self.forward_gemm_dtype = torch.float32
        self.attention_mma_bf16 = False
        # capture slabs follow ``set_body_dtype`` (image towers: the slabs are the resident bytes of a long sequence);
        # the 77-token text tower keeps fp32 slabs and its register-resident exact-fp32 attention kernels
        self._long_sequence_slabs_follow_body = attn_mask is None
        # what a row-list forward (and the backward on its tape) leave behind for complete_attn_probs: the block input, the slabs, the
        # rows and the upstream gradient rows -- until the slabs have been completed or another forward has rewritten them
        self._probs_pending = None

    def set_body_dtype(self, dtype):
        """``torch.bfloat16``: everything the reference's half-precision body would run in half precision (all GEMMs, the
        attention products where the streaming kernels apply, the capture slabs); ``torch.float32``: the exact path.
        ``torch.float16``: the reference's OWN half-precision mode (``convert_weights``, CLIP/clip/model.py:381-402): every GEMM
        on the fp16 matrix cores with the weights rounded to fp16 exactly as ``convert_weights`` rounds them (fp32 accumulate;
        LayerNorm, softmax and the residual stream stay fp32 -- the reference computes LayerNorm in fp32 too, model.py:157-164),
        long-sequence capture slabs in fp16, and the relevancy chain with the reference's fp16 roundings (``half_chain``: R is
        created in the dtype of the probabilities, notebook cell 6:20,43).  Pinned on the reference's fp16 model in
        ``tests/test_gpu_clip.py`` (fixture clip_tiny_fp16.npz)."""
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("body dtype must be torch.float32, torch.bfloat16 or torch.float16")
        half = dtype == torch.bfloat16
        self.backward_gemm_dtype = self.forward_gemm_dtype = dtype
        self.attention_mma_bf16 = half
        self.half_chain = dtype == torch.float16
        if self._long_sequence_slabs_follow_body:
            self.capture_dtype = dtype
            self.buffers = None

    def _linear(self, x, lin_weight, lin_bias):
        return ops.linear(x, lin_weight, lin_bias, getattr(self, "forward_gemm_dtype", torch.float32))

    def _gemm(self, x, weight):
        """``x @ weight`` for the hand-written backward, in ``backward_gemm_dtype`` (cached converted weights)."""
        return ops.backward_gemm(x, weight, getattr(self, "backward_gemm_dtype", torch.float32))

    def _ensure_buffers(self, batch, n_tokens, device, shared_probs=False, grads=True):
        if self.buffers is None or not self.buffers.matches(self.layers, batch, self.heads, n_tokens, n_tokens, device,
                                                            shared_probs, self.capture_dtype, grads):
            self.buffers = CaptureBuffers(self.layers, batch, self.heads, n_tokens, n_tokens, device=device,
                                          shared_probs=shared_probs, dtype=self.capture_dtype, grads=grads)
        return self.buffers

    # ------------------------------------------------------------------------------------------------------------
    # Tape forward / hand-written backward -- the path ``interpret`` runs for BOTH towers.
    #
    # The explainability pass needs d(logit)/d(attention probabilities) only.  Autograd would rebuild a graph per call
    # (and the reference even runs one partial backward per layer); here the forward keeps a small tape and the backward
    # is the same chain of vector-Jacobian products written out: input-gradient GEMMs, the fused LayerNorm-backward +
    # residual kernel, the fused QuickGELU backward, our attention backward.  Weight gradients are never formed.
    #
    # Shared-forward mode (``x`` has batch 1, ``batch`` > 1): CLIP ``interpret`` repeats ONE image B times (notebook
    # cell 6:3); the B copies have identical activations and differ only in their upstream gradients.  The forward runs
    # ONCE, the backward runs at batch B with batch-stride-0 q / k / v / P and LayerNorm statistics shared by the batch.
    # ------------------------------------------------------------------------------------------------------------
    def _mask_for(self, blk, n_tokens, device):
        mask = blk.attn_mask
        if mask is None:
            return None
        if mask.device != device:
            blk.attn_mask = mask = mask.to(device=device, dtype=torch.float32)
        if mask.shape[-1] != n_tokens:
            mask = mask[:n_tokens, :n_tokens].contiguous()               # trimmed (padding-free) text batch
        return mask

    def is_causal(self):
        """True iff every block runs under an additive mask that is -inf strictly above the diagonal (CLIP's ``build_attention_mask``,
        CLIP/clip/model.py:334-340).  Checked on the mask tensors themselves, once per mask object (one device -> host read, made
        during the warm-up call that precedes any hipGraph capture); anything else -- no mask, another mask -- is not causal."""
        masks = [getattr(blk, "attn_mask", None) for blk in self.resblocks]
        if not masks or any(m is None for m in masks):
            return False
        key = tuple(id(m) for m in masks)
        cached = self.__dict__.get("_causal_mask_check")
        if cached is None or cached[0] != key:
            ok = True
            for m in {id(m): m for m in masks}.values():
                n = m.shape[-1]
                upper = torch.ones(n, n, dtype=torch.bool, device=m.device).triu_(1)
                ok = ok and m.dim() == 2 and m.shape[0] == n and bool(torch.isneginf(m[upper]).all())
            self.__dict__["_causal_mask_check"] = cached = (key, ok)
        return cached[1]

    def _row_gemm_weights_ok(self, dtype=torch.float32):
        for blk in self.resblocks:
            if not ops.gemm_rows_eligible(blk.mlp.c_proj.weight, blk.mlp.c_fc.weight, blk.attn.out_proj.weight, blk.attn.in_proj_weight,
                                          dtype=dtype):
                return False
        return True

    def _row_gemm_dtype(self, which):
        """The GEMM dtype of the row-list route for ``which`` = ``"forward_gemm_dtype"`` / ``"backward_gemm_dtype"``: fp32, or fp16 for
        the reference's half-precision body (``set_body_dtype(torch.float16)``: fp32 slabs, LayerNorms and attention around fp16 GEMMs,
        which ``mmx_gemm_rows_f16`` runs on the list) when option ``text_live_rows_half`` is on; ``None``: the route is not offered
        (bf16 bodies have a bf16 gradient stream and elementwise kernels of their own and stay dense)."""
        dtype = getattr(self, which, torch.float32)
        if dtype == torch.float32:
            return dtype
        if dtype == torch.float16 and self.capture_dtype == torch.float32 and ops.live_rows_half_enabled():
            return dtype
        return None

    def live_rows_for_forward(self, x, out_rows):
        """The row-list FORWARD (``forward_tape(live=...)``): under a causal mask row p of a sample depends on rows ``<= p`` of that
        sample only, and the caller reads row ``out_rows[b]``, so the rows past it feed nothing -- not the feature, and (the backward
        being confined to the same rows, ``_live_rows_route``) no gradient either.  Same conditions as the backward's route: fp32
        tape, causal tower, eligible weights, ``E % 4 == 0``; plus biases on every Linear and options ``text_live_rows`` /
        ``text_live_rows_fwd``.  Returns the ``ops.LiveRows`` of ``out_rows`` or ``None`` (dense forward)."""
        if out_rows is None or x.dim() != 3 or x.dtype != torch.float32 or x.shape[-1] % 4 or not x.is_cuda:
            return None
        dtype = self._row_gemm_dtype("forward_gemm_dtype")       # fp32, or fp16 with option text_live_rows_half
        if dtype is None or self._row_gemm_dtype("backward_gemm_dtype") != dtype or self.capture_dtype != torch.float32:
            return None
        if self.layers < 1 or not ops.live_rows_forward_enabled() or not self.is_causal() or not self._row_gemm_weights_ok(dtype):
            return None
        if x.shape[1] < self.resblocks[0].attn_mask.shape[-1]:
            # a trimmed text batch (``trim_text_padding``: the first max(eot) + 1 positions only) keeps the dense forward: most of its
            # rows are live, and on them the library GEMM beats the row-list kernel (measured, ViT-B/32, 64 captions: 7.65 ms per
            # step against 8.96 with the route; profiles/text_forward_live_rows_probe.txt).  Its backward takes the route as before
            return None
        for blk in self.resblocks:
            for bias in (blk.attn.in_proj_bias, blk.attn.out_proj.bias, blk.mlp.c_fc.bias, blk.mlp.c_proj.bias):
                if bias is None or bias.dtype != torch.float32:
                    return None
        return ops.live_rows(out_rows, x.shape[1])

    @torch.no_grad()
    def complete_attn_probs(self):
        """After a row-list forward the capture slabs hold what the maps need and no more: the probabilities of the live rows (a filler
        in the others: the softmax of zero scores), and gradients that are right at and below the diagonal only -- ``dP[i, j] = dO[i] .
        V[j]`` of a masked entry ``j > eot >= i`` wants the value row of a padded position, which that forward never formed (the chain
        multiplies it with ``P[i, j] = 0``).  This runs the dense forward of the whole stack from the kept block input into the SAME
        slabs and, if the backward has run, the backward again on that tape -- no new slabs, current stream -- so that ``blk.attn_probs``
        and ``blk.attn_grad`` show every entry as a dense forward gives it (the live entries then carry the dense path's roundings).
        Called by the first read of any block's ``attn_probs`` / ``attn_grad``; a no-op when nothing is pending.  Raw ``buffers.probs[l]``
        / ``buffers.grads[l]`` are not accessors and stay as the route left them until then."""
        pending = self.__dict__.get("_probs_pending")
        if pending is None:
            return
        if torch.cuda.is_current_stream_capturing():
            raise _lib.MMXError("attn_probs / attn_grad: the slabs of a row-list forward cannot be completed inside a stream capture "
                                "(read them outside it, or set option text_live_rows_fwd to 0)")
        self._probs_pending = None
        keep, self.buffers = self.buffers, pending["buffers"]
        try:
            _, tape = self.forward_tape(pending["x"], first_grad_layer=pending["first_grad_layer"],
                                        grads=pending["buffers"].grads is not None, out_rows=pending["out_rows"])
            if pending["dy_row_values"] is not None:
                self.backward_tape(tape, None, pending["backward_first_grad_layer"], dy_rows=pending["out_rows"],
                                   dy_row_values=pending["dy_row_values"])
        finally:
            self.buffers = keep

    def _live_rows_route(self, tape, B, N, E, first_grad_layer, dy_rows, dy_row_values, rel_row, grouped):
        """The row-list backward (``ops.live_rows``): an fp32 tape of a causally masked tower whose upstream gradient is one row per
        sample.  Gradient enters at row ``dy_rows[b]`` and causal attention hands it to keys ``j <= i`` only, so every gradient row
        past it is an exact zero in every layer: the row-wise steps (input-gradient GEMMs, QuickGELU', LayerNorm') then run on the
        rows up to it, picked on the device.  Returns the ``ops.LiveRows`` or ``None`` (dense path: any other caller, the
        process-wide switch ``ops.set_option("text_live_rows", 0)``, or a weight outside ``ops.gemm_rows_eligible``)."""
        top = self.layers - 1
        if dy_rows is None or dy_row_values is None or rel_row is not None or grouped or top <= first_grad_layer:
            return None
        dtype = self._row_gemm_dtype("backward_gemm_dtype")      # fp32, or fp16 with option text_live_rows_half
        if dtype is None or dy_row_values.dtype != torch.float32:
            return None
        if tape[top][0].shape[0] != B or E % 4 or not self.is_causal() or not self._row_gemm_weights_ok(dtype):
            return None
        return ops.live_rows(dy_rows, N)

    @torch.no_grad()
    def forward_tape(self, x, batch=None, first_grad_layer=0, grads=True, out_rows=None, live=None):
        """``x``: ``[Bx, N, E]`` block input (embedded, through ``ln_pre`` for the image tower).  ``batch``: how many
        upstream gradients ``backward_tape`` will carry (default ``Bx``; ``Bx == 1 < batch`` = shared-forward mode).
        Returns ``(y [Bx, N, E], tape)``; the probabilities of every block are in the capture slabs afterwards.
        ``grads=False``: no gradient slab is allocated (``backward_tape(..., rel_row=...)`` does not store dP).

        ``out_rows`` (``[Bx]`` long): the caller reads ONE token per sample from the tower output (class token / EOT token:
        CLIP/clip/model.py:235, 360).  Everything after the attention of the top block is row-wise, so ``out_proj``, ``ln_2``
        and the MLP of that block run on those Bx rows only (3 of its 4 GEMMs); ``y`` is then ``[Bx, E]`` -- those rows -- and
        ``backward_tape`` must be given the same rows as ``dy_rows``.

        ``live`` (``live_rows_for_forward(x, out_rows)``, a causally masked fp32 tower): the row-list forward.  Every row-wise step
        (LayerNorms, the four GEMMs with their bias, QuickGELU) runs on the rows up to ``out_rows[b]`` only; the other rows of the
        intermediates and of the tape are NOT written.  The attention takes the caption lengths too where the whole-head kernels have
        a live-length instantiation (``ops.attn_live_shape``: CLIP's 77 tokens; ``ops.attn_capture_fwd(live=...)``): it
        reads the live rows of an uninitialised ``qkv`` and writes ``O`` for them only.  Elsewhere, and with
        ``ops.set_option("text_live_attn", 0)``, it stays dense on a ``qkv`` whose unlisted rows are zeros.  Either way live queries see
        live keys only (causal mask), so their rows of ``P`` and ``O`` are exact and the same bits; the dead rows of ``P`` hold the
        softmax of zero scores, finite, which is all the backward and the chain need (their gradient rows are exact zeros).  The
        gradient slab is then right where ``P`` is not masked (what the chain reads); its masked entries ``dO[i] . V[j]``, ``j`` past
        the last live row, come out as zeros.  ``backward_tape`` must be given the same ``live``; ``blk.attn_probs`` /
        ``blk.attn_grad`` complete both slabs on their first read (``complete_attn_probs``)."""
        if not x.is_cuda:
            raise _lib.MMXError("the CLIP body runs its attention on the HIP capture op: move the model and "
                                "inputs to the MI355X (there is no CPU attention path)")
        Bx, N, E = x.shape
        batch = Bx if batch is None else batch
        shared = Bx == 1 and batch > 1
        if not shared and Bx != batch:
            raise ValueError("forward_tape: %d inputs for %d upstream gradients (only a single input can be shared)" % (Bx, batch))
        buffers = self._ensure_buffers(batch, N, x.device, shared_probs=shared, grads=grads)
        blocks = list(self.resblocks)
        mask = self._mask_for(blocks[0], N, x.device) if blocks else None
        tape = []
        self._probs_pending = None
        if live is not None:
            if out_rows is None or shared or live.cap != Bx * N:
                raise ValueError("forward_tape: the row-list forward needs out_rows, one input per gradient and a list over %d rows"
                                 % (Bx * N))
            self._probs_pending = {"x": x, "buffers": buffers, "live": live, "out_rows": out_rows, "first_grad_layer": first_grad_layer,
                                   "dy_row_values": None, "backward_first_grad_layer": None}
            for blk in blocks:
                blk.__dict__["_probs_owner"] = (self,)
            # the attention on the live rows too (kept on the list: the backward of this tape must then do the same)
            live.attn = ops.attn_live_shape(N, blocks[0].attn.head_dim)

        def ln(res, y, norm):                 # s = res + y, LayerNorm(s) and its statistics: dense, or on the listed rows
            if live is not None:
                return ops.add_layernorm_rows(res, y, norm.weight, norm.bias, norm.eps, live)
            return ops.add_layernorm(res, y, norm.weight, norm.bias, norm.eps, h_dtype=hd)
        # bf16 matrix cores for the attention products: the long-sequence streaming kernels only (the register-resident
        # head kernels of a short tower such as CLIP's 77-token text side stay exact fp32)
        mma = bool(getattr(self, "attention_mma_bf16", False)) and N > 128
        # every LayerNorm but the first is fused with the residual add that produces its input
        first = blocks[0].ln_1
        # bf16 body: what only feeds a GEMM (LayerNorm outputs, the MLP activation) leaves its kernel as bf16 -- no conversion passes
        hd = torch.bfloat16 if getattr(self, "forward_gemm_dtype", torch.float32) == torch.bfloat16 else torch.float32
        gd = getattr(self, "forward_gemm_dtype", torch.float32)      # row-list route: the GEMM dtype of linear_rows (fp32 | fp16)
        _, h1, mean1, rstd1 = ln(x, None, first)
        for l, blk in enumerate(blocks):
            at = blk.attn
            if live is not None:
                # (without live lengths in the attention: zeros, not LiveRows._out -- the dense attention reads every row of qkv)
                qkv = ops.linear_rows(h1, at.in_proj_weight, at.in_proj_bias, live, out=None if live.attn else
                                      torch.zeros(Bx, N, 3 * E, dtype=torch.float32, device=x.device), dtype=gd)
            else:
                qkv = self._linear(h1, at.in_proj_weight, at.in_proj_bias)
            qkv = qkv.view(Bx, N, 3, at.num_heads, at.head_dim)
            o = ops.attn_capture_fwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], buffers.probs[l], at.head_dim ** -0.5,
                                     _lib.SCALE_Q_FIRST, mask, layout="bnhd", mma_bf16=mma,
                                     live=live if live is not None and live.attn else None)
            if out_rows is not None and l + 1 == len(blocks):
                ar = torch.arange(Bx, device=x.device)
                x1, h2, mean2, rstd2 = ops.add_layernorm(
                    x[ar, out_rows], self._linear(o.view(Bx, N, E)[ar, out_rows], at.out_proj.weight, at.out_proj.bias),
                    blk.ln_2.weight, blk.ln_2.bias, blk.ln_2.eps, h_dtype=hd)
                m = self._linear(h2, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias)
                mlp_out = self._linear(ops.quick_gelu_fwd(m, hd), blk.mlp.c_proj.weight, blk.mlp.c_proj.bias)
                # (x1, mean2, rstd2, m hold the Bx selected rows only: what _top_block_rows reads)
                tape.append((x, mean1, rstd1, qkv, x1, mean2, rstd2, m, o, out_rows) if l >= first_grad_layer else None)
                blk.attn_probs, blk.attn_grad = buffers.layer_probs(l), buffers.layer_grads(l)
                return x1 + mlp_out, tape
            if live is not None:
                x1, h2, mean2, rstd2 = ln(x, ops.linear_rows(o.view(Bx, N, E), at.out_proj.weight, at.out_proj.bias, live, dtype=gd),
                                          blk.ln_2)
                m, act = ops.linear_rows(h2, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, live, gelu=True, dtype=gd)
                mlp_out = ops.linear_rows(act, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias, live, dtype=gd)
            else:
                x1, h2, mean2, rstd2 = ln(x, self._linear(o.view(Bx, N, E), at.out_proj.weight, at.out_proj.bias), blk.ln_2)
                m = self._linear(h2, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias)
                mlp_out = self._linear(ops.quick_gelu_fwd(m, hd), blk.mlp.c_proj.weight, blk.mlp.c_proj.bias)
            tape.append((x, mean1, rstd1, qkv, x1, mean2, rstd2, m, o) if l >= first_grad_layer else None)
            blk.attn_probs, blk.attn_grad = buffers.layer_probs(l), buffers.layer_grads(l)
            if l + 1 < len(blocks):
                x, h1, mean1, rstd1 = ln(x1, mlp_out, blocks[l + 1].ln_1)
            else:
                x = x1 + mlp_out
        return x, tape

    @torch.no_grad()
    def forward_nocapture(self, x, out_rows=None, live=None):
        """Inference forward of the stack: ``x [B, N, E]`` -> ``y [B, N, E]``, attention on ``ops.attn_fwd``.  No capture slab is
        touched or allocated (``self.buffers`` stays as it is) and no tape is kept.  ``out_rows``: as in ``forward_tape`` (a
        ``[B]`` long tensor), or a Python int when every sample reads the same row (the class token); the top block then runs on
        those rows only -- with an int also its attention queries -- and ``y`` is ``[B, E]``.  fp32 bodies only.
        ``live`` (``live_rows_for_forward(x, out_rows)``, a causally masked tower, ``out_rows`` a tensor): the row-list route of
        ``forward_tape(live=...)`` without the tape -- LayerNorms and the four GEMMs (QuickGELU from ``c_fc``'s epilogue) on the rows
        up to ``out_rows[b]`` only, the attention on ``ops.attn_fwd(live=...)`` where ``ops.attn_live_shape`` allows it and dense over a
        ``qkv`` whose unlisted rows are zeros elsewhere; the top block gathers row ``out_rows[b]`` as before."""
        for what in ("forward_gemm_dtype", "capture_dtype"):
            dt = getattr(self, what, torch.float32)
            if dt != torch.float32:
                raise _lib.MMXError("forward_nocapture: fp32 bodies only (the no-capture attention is exact fp32); this tower's "
                                    "%s is %s" % (what, str(dt).replace("torch.", "")))
        if x.dtype != torch.float32:
            raise _lib.MMXError("forward_nocapture: fp32 bodies only; the input is %s" % str(x.dtype).replace("torch.", ""))
        if not x.is_cuda:
            raise _lib.MMXError("the CLIP body runs its attention on the HIP kernels: move the model and inputs to the GPU")
        B, N, E = x.shape
        blocks = list(self.resblocks)
        mask = self._mask_for(blocks[0], N, x.device) if blocks else None
        if live is not None:
            if out_rows is None or isinstance(out_rows, int) or live.cap != B * N:
                raise ValueError("forward_nocapture: the row-list forward needs out_rows [B] and a list over %d rows" % (B * N))
            return self._forward_nocapture_rows(x, out_rows, live, blocks, mask)
        first = blocks[0].ln_1
        _, h1, _, _ = ops.add_layernorm(x, None, first.weight, first.bias, first.eps)
        for l, blk in enumerate(blocks):
            at = blk.attn
            top = out_rows is not None and l + 1 == len(blocks)
            one = top and isinstance(out_rows, int)
            qkv = self._linear(h1, at.in_proj_weight, at.in_proj_bias).view(B, N, 3, at.num_heads, at.head_dim)
            q = qkv[:, out_rows:out_rows + 1, 0] if one else qkv[:, :, 0]
            m_l = mask[out_rows:out_rows + 1] if (one and mask is not None) else mask
            o = ops.attn_fwd(q, qkv[:, :, 1], qkv[:, :, 2], at.head_dim ** -0.5, _lib.SCALE_Q_FIRST, m_l, layout="bnhd")
            if one:
                xr, orows = x[:, out_rows], o.view(B, E)
            elif top:
                ar = torch.arange(B, device=x.device)
                xr, orows = x[ar, out_rows], o.view(B, N, E)[ar, out_rows]
            else:
                xr, orows = x, o.view(B, N, E)
            x1, h2, _, _ = ops.add_layernorm(xr, self._linear(orows, at.out_proj.weight, at.out_proj.bias), blk.ln_2.weight,
                                             blk.ln_2.bias, blk.ln_2.eps)
            mlp_out = self._linear(ops.quick_gelu_fwd(self._linear(h2, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias)),
                                   blk.mlp.c_proj.weight, blk.mlp.c_proj.bias)
            if l + 1 < len(blocks):
                nxt = blocks[l + 1].ln_1
                x, h1, _, _ = ops.add_layernorm(x1, mlp_out, nxt.weight, nxt.bias, nxt.eps)
            else:
                x = x1 + mlp_out
        return x

    def _forward_nocapture_rows(self, x, out_rows, live, blocks, mask):
        """``forward_nocapture(live=...)``: the steps of ``forward_tape(live=...)``, nothing kept."""
        B, N, E = x.shape
        live_attn = ops.attn_live_shape(N, blocks[0].attn.head_dim)
        first = blocks[0].ln_1
        _, h1, _, _ = ops.add_layernorm_rows(x, None, first.weight, first.bias, first.eps, live)
        for l, blk in enumerate(blocks):
            at = blk.attn
            # (without live lengths in the attention: zeros, not LiveRows._out -- the dense attention reads every row of qkv)
            qkv = ops.linear_rows(h1, at.in_proj_weight, at.in_proj_bias, live, out=None if live_attn else
                                  torch.zeros(B, N, 3 * E, dtype=torch.float32, device=x.device))
            qkv = qkv.view(B, N, 3, at.num_heads, at.head_dim)
            o = ops.attn_fwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], at.head_dim ** -0.5, _lib.SCALE_Q_FIRST, mask, layout="bnhd",
                             live=live if live_attn else None)
            if l + 1 == len(blocks):
                ar = torch.arange(B, device=x.device)
                x1, h2, _, _ = ops.add_layernorm(x[ar, out_rows],
                                                 self._linear(o.view(B, N, E)[ar, out_rows], at.out_proj.weight, at.out_proj.bias),
                                                 blk.ln_2.weight, blk.ln_2.bias, blk.ln_2.eps)
                mlp_out = self._linear(ops.quick_gelu_fwd(self._linear(h2, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias)),
                                       blk.mlp.c_proj.weight, blk.mlp.c_proj.bias)
                return x1 + mlp_out
            x1, h2, _, _ = ops.add_layernorm_rows(x, ops.linear_rows(o.view(B, N, E), at.out_proj.weight, at.out_proj.bias, live),
                                                  blk.ln_2.weight, blk.ln_2.bias, blk.ln_2.eps, live)
            _, act = ops.linear_rows(h2, blk.mlp.c_fc.weight, blk.mlp.c_fc.bias, live, gelu=True)
            mlp_out = ops.linear_rows(act, blk.mlp.c_proj.weight, blk.mlp.c_proj.bias, live)
            nxt = blocks[l + 1].ln_1
            x, h1, _, _ = ops.add_layernorm_rows(x1, mlp_out, nxt.weight, nxt.bias, nxt.eps, live)

    def forward_shared(self, x, batch):
        """Shared-forward mode of ``forward_tape`` (kept under its round-1 name)."""
        if x.shape[0] != 1:
            raise ValueError("forward_shared takes the single shared sample")
        return self.forward_tape(x, batch)

    @torch.no_grad()
    def backward_tape(self, tape, dy, first_grad_layer=0, dy_rows=None, rel_row=None, dy_row_values=None, targets_per_image=1,
                      live=None):
        """``dy``: ``[B, N, E]`` upstream gradients w.r.t. the tower output; fills ``buffers.grads`` of every block
        ``>= first_grad_layer``.

        ``rel_row`` (``[B, N]`` fp32, bf16-body towers on the streaming kernels only): row-relevancy mode.  The caller
        wants ONE row of ``R = (I + A_top) ... (I + A_first)`` (CLIP ``interpret`` returns ``R[:, 0, 1:]``): that row is
        ``rel_row`` carried through the layers top-down -- the order this backward runs in -- as
        ``row <- row + row . mean_h clamp(dP * P, 0)``, reduced inside the attention backward kernel.  No gradient slab is
        written, no A-bar / R matrix is formed; the final row is returned.

        ``dy_rows`` (``[B]`` long, or an int for the same row of every sample; optional): promise that ``dy`` is zero outside row
        ``dy_rows[b]`` of sample ``b`` -- both CLIP towers read their feature from ONE token (class token / EOT token).  The top block's MLP and ``out_proj``
        vector-Jacobian products are row-wise, so they then run on those B rows instead of B*N (3 of the 4 GEMMs of
        that block); below the top block's attention the gradient is dense and everything runs in full.
        ``dy_row_values`` (``[B, E]``, with ``dy_rows``): those rows themselves -- ``dy`` may then be ``None`` (no dense zero
        tensor is built just to be gathered from again).

        With ``dy_rows`` / ``dy_row_values`` on the fp32 tape of a CAUSALLY masked tower (CLIP's text tower) everything below the top
        block runs on the rows up to ``dy_rows[b]`` only (``_live_rows_route``): the rest of every gradient tensor is exact zeros.
        The attention backward still sees a dense ``d_o`` (zeros in the dead rows) and writes the whole gradient slab.
        ``live``: the list a row-list forward ran on (``forward_tape(live=...)``); it is used again instead of building a second one,
        and it is required then -- such a tape holds the listed rows only.  Where that forward's attention took the caption lengths
        (``live.attn``), the attention backward takes them as well (``ops.attn_capture_bwd(live=...)``): ``qkv`` holds the live rows
        only, the dead rows of ``dqkv`` are not written (nothing reads them), the gradient slab still is written whole, zeros in the
        dead rows as before.  After a dense forward the attention backward stays dense, whatever the row-wise steps do: its masked
        entries ``dO[i] . V[j]`` are what ``blk.attn_grad`` shows.

        ``targets_per_image=K`` (fp32 body, row mode only): the tape holds M distinct samples and the B = K*M upstream gradients
        are K per sample in K-major order (target t explains sample t % M).  The elementwise steps broadcast the per-sample
        activations (modulo kernels); the capture op runs its grouped row mode (``ops.attn_capture_bwd(images=M)``)."""
        if isinstance(dy_rows, int):          # the same row of every sample (a ViT's class token): a kept constant, no fill launch
            ref = dy_row_values if dy_row_values is not None else dy
            dy_rows = ops.const_rows(ref.shape[0], dy_rows, ref.device)
        if dy is None:
            if dy_rows is None or dy_row_values is None:
                raise ValueError("backward_tape: dy=None needs dy_rows and dy_row_values")
            if self.layers - 1 < first_grad_layer:         # nothing to explain (the tape holds None for every layer)
                return rel_row
            B, N, E = dy_row_values.shape[0], tape[-1][0].shape[1], dy_row_values.shape[1]
        else:
            B, N, E = dy.shape
        buffers = self.buffers
        top = self.layers - 1
        dx = dy
        top_rows = None                      # (rows, d_x1 of those rows): the top block's residual gradient, added after LN1'
        mma = bool(getattr(self, "attention_mma_bf16", False)) and N > 128
        grouped = int(targets_per_image) > 1
        # bf16 body on the streaming kernels: the gradients BETWEEN the GEMMs are bf16 (what the bf16 GEMMs produce and
        # consume; the elementwise kernels and the attention backward read / write bf16 directly -- no conversion
        # passes), the residual gradient stream (dx, d_x1) stays fp32
        # A short tower of a bf16 body (CLIP's 77-token text side: register-resident fp32 head kernels) runs the same bf16 stream: the
        # whole-head backward reads a bf16 d_o and writes bf16 dq | dk | dv around its exact-fp32 arithmetic (attention_head.hip, IOH;
        # round 4 -- before that two conversion passes per layer sat around it).
        stream16 = getattr(self, "backward_gemm_dtype", torch.float32) == torch.bfloat16
        gd = getattr(self, "backward_gemm_dtype", torch.float32)     # row-list route: the GEMM dtype of gemm_rows (fp32 | fp16)
        head = self.resblocks[0].attn
        att16 = stream16 and (mma or (self.capture_dtype == torch.float32 and
                                      ops.head_kernel_shape(N, N, head.head_dim) and head.head_dim % 8 == 0))
        if grouped and (rel_row is None or stream16 or mma or B % int(targets_per_image)):
            raise ValueError("backward_tape: targets_per_image=%d needs an fp32 body in the row mode and a multiple of it "
                             "upstream gradients (got %d)" % (int(targets_per_image), B))
        dx_h = None
        handed_in = live is not None
        if live is None:
            live = self._live_rows_route(tape, B, N, E, first_grad_layer, dy_rows, dy_row_values, rel_row, grouped)
        elif dy_rows is None or dy_row_values is None or rel_row is not None or grouped or live.cap != B * N:
            raise ValueError("backward_tape: the tape of a row-list forward needs the row-list backward (dy_rows and dy_row_values, "
                             "no rel_row, one target per sample)")
        else:
            pending = self.__dict__.get("_probs_pending")
            if pending is not None and pending["live"] is live:           # what complete_attn_probs needs to run this backward again
                pending["dy_row_values"], pending["backward_first_grad_layer"] = dy_row_values, first_grad_layer
        live_attn = live if handed_in and live.attn else None      # the forward's attention took the lengths: so does this one
        d_o_dense = None      # live-row route: the top block's dense d_o (zeros outside the EOT rows); every block below rewrites its
                              # live rows only, so the dead rows the attention backward reads stay zero without another pass
        for l in range(top, first_grad_layer - 1, -1):
            blk = self.resblocks[l]
            at = blk.attn
            x, mean1, rstd1, qkv, x1, mean2, rstd2, m, o_fwd = tape[l][:9]
            shared = x.shape[0] != B and not grouped
            if grouped and x.shape[0] * int(targets_per_image) != B:
                raise ValueError("backward_tape: %d upstream gradients for %d samples x %d targets"
                                 % (B, x.shape[0], int(targets_per_image)))
            if len(tape[l]) > 9 and (l != top or dy_rows is None):
                raise ValueError("backward_tape: the forward kept only the output rows of the top block (out_rows): "
                                 "pass the same rows as dy_rows")
            if l == top and dy_rows is not None:
                g = dy_row_values if dy_row_values is not None else dy[torch.arange(B, device=dy_rows.device), dy_rows]
                d_x1_r, d_o = self._top_block_rows(blk, tape[l], g, dy_rows, shared, N, x.shape[0] if grouped else None)
                d_x1, top_rows = None, (dy_rows, d_x1_r)
                d_o_dense = d_o
                if att16:
                    d_o = d_o.to(torch.bfloat16)
            elif live is not None:
                d_a = ops.gemm_rows(dx, blk.mlp.c_proj.weight, live, dtype=gd)
                d_m = ops.quick_gelu_bwd_rows(m, d_a, live)
                d_h2 = ops.gemm_rows(d_m, blk.mlp.c_fc.weight, live, dtype=gd)
                d_x1 = ops.layernorm_bwd_add_rows(d_h2, x1, mean2, rstd2, blk.ln_2.weight, dx, live)
                d_o = ops.gemm_rows(d_x1, at.out_proj.weight, live, out=d_o_dense, dtype=gd)
            elif stream16:
                if dx_h is None:
                    dx_h = dx.to(torch.bfloat16)
                d_a = ops.backward_gemm_bf16(dx_h, blk.mlp.c_proj.weight)
                d_m = ops.quick_gelu_bwd(m, d_a)
                d_h2 = ops.backward_gemm_bf16(d_m, blk.mlp.c_fc.weight)
                d_x1, d_x1_h = ops.layernorm_bwd_add_bf16(d_h2, x1, mean2, rstd2, blk.ln_2.weight, dx)
                d_o = ops.backward_gemm_bf16(d_x1_h, at.out_proj.weight)
            else:
                # MLP branch: x2 = x1 + c_proj(m * sigmoid(1.702 m)),  m = c_fc(ln_2(x1))
                d_a = self._gemm(dx, blk.mlp.c_proj.weight)
                d_m = ops.quick_gelu_bwd(m, d_a)          # shared mode: m [1, N, 4E] is broadcast inside the kernel
                d_h2 = self._gemm(d_m, blk.mlp.c_fc.weight)
                d_x1 = ops.layernorm_bwd_add(d_h2, x1, mean2, rstd2, blk.ln_2.weight, dx)   # dx + LN2'(d_h2), one pass
                # attention branch: x1 = x + out_proj(attn(ln_1(x)))
                d_o = self._gemm(d_x1, at.out_proj.weight)
            if stream16 and not att16 and d_o.dtype != torch.float32:
                d_o = d_o.float()
            d_o = d_o.view(B, N, at.num_heads, at.head_dim)
            need = l > first_grad_layer                                       # nothing below needs gradients
            if need and live_attn is not None:        # (its dead rows are not written: NaN there under LiveRows.poison)
                dqkv = live_attn._out(d_o.view(B, N, E), 3 * E).view(B, N, 3, at.num_heads, at.head_dim)
            else:
                dqkv = torch.empty(B, N, 3, at.num_heads, at.head_dim, dtype=d_o.dtype, device=d_o.device) if need else None
            out = (dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]) if need else None
            res = ops.attn_capture_bwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], buffers.probs[l], d_o,
                                       buffers.grads[l] if buffers.grads is not None else None,
                                       at.head_dim ** -0.5, _lib.SCALE_Q_FIRST, need_dqkv=need, layout="bnhd", out=out,
                                       batch=B if shared else None, o=o_fwd, mma_bf16=mma, rel_row=rel_row,
                                       images=x.shape[0] if grouped else None, live=live_attn)
            if rel_row is not None:
                rel_row = res[3]
            if not need:
                break
            if stream16:
                dq_in = dqkv.view(B, N, 3 * E)
                d_h1 = ops.backward_gemm_bf16(dq_in if att16 else dq_in.to(torch.bfloat16), at.in_proj_weight)
                dx, dx_h = ops.layernorm_bwd_add_bf16(d_h1, x, mean1, rstd1, blk.ln_1.weight, d_x1)
            elif live is not None:
                d_h1 = ops.gemm_rows(dqkv.view(B, N, 3 * E), at.in_proj_weight, live, dtype=gd)
                dx = ops.layernorm_bwd_add_rows(d_h1, x, mean1, rstd1, blk.ln_1.weight, d_x1, live)
            else:
                d_h1 = self._gemm(dqkv.view(B, N, 3 * E), at.in_proj_weight)
                dx = ops.layernorm_bwd_add(d_h1, x, mean1, rstd1, blk.ln_1.weight, d_x1)
            if l == top and top_rows is not None:
                # the top block's residual gradient lives on one row per sample: added to LN1'(.) there (no dense zero tensor)
                ops.rows_add_(dx, *top_rows)
                if stream16:
                    dx_h = dx.to(torch.bfloat16)
        return rel_row

    def _top_block_rows(self, blk, entry, g, rows, shared, N, images=None):
        """MLP / ``out_proj`` backward of the top block on the one row per sample that carries a gradient (``g [B, E]``).
        Returns ``(d_x1 rows [B, E], d_o dense [B, N, E])`` -- the attention backward wants every row of ``d_o``, zero elsewhere.
        ``images``: grouped mode, target b reads sample b % images of the tape."""
        x, mean1, rstd1, qkv, x1, mean2, rstd2, m, o_fwd = entry[:9]
        B = g.shape[0]
        if len(entry) > 9:                                                   # forward_tape(out_rows=...): rows only on the tape
            # [Bx, .] rows, Bx = B (one input per gradient), 1 (shared forward) or ``images`` (grouped, target t reads sample t % Bx):
            # quick_gelu_bwd and layernorm_bwd_add broadcast a batch-1 / batch-M operand themselves -- no index, no copy
            m_r, x1_r, mean2_r, rstd2_r = m, x1, mean2.reshape(-1), rstd2.reshape(-1)
        else:                                                                # full [Bx, N, .] tensors: the row differs per sample
            ar = torch.arange(B, device=g.device)
            src = torch.zeros_like(rows) if shared else ar                   # sample index into the (shared) tape
            if images is not None:
                src = ar % images
            flat = src * N + rows                                            # row of the [Bx*N] statistics
            m_r, x1_r, mean2_r, rstd2_r = m[src, rows], x1[src, rows], mean2.reshape(-1)[flat], rstd2.reshape(-1)[flat]
        d_a = self._gemm(g, blk.mlp.c_proj.weight)
        d_m = ops.quick_gelu_bwd(m_r, d_a) if d_a.dtype == torch.float32 and m_r.numel() % 4 == 0 else \
            d_a * (torch.sigmoid(1.702 * m_r) * (1 + 1.702 * m_r * (1 - torch.sigmoid(1.702 * m_r))))
        d_h2 = self._gemm(d_m, blk.mlp.c_fc.weight)
        d_x1_r = ops.layernorm_bwd_add(d_h2, x1_r, mean2_r, rstd2_r, blk.ln_2.weight, g)
        return d_x1_r, ops.rows_to_dense(self._gemm(d_x1_r, blk.attn.out_proj.weight), rows, N)

    def backward_shared(self, tape, dy, first_grad_layer=0):
        """Round-1 name of ``backward_tape``."""
        return self.backward_tape(tape, dy, first_grad_layer)

    def forward(self, x, capture_only=False, first_grad_layer=0):
        """``x``: ``[B, N, E]``.  ``capture_only``: only d(loss)/d(probs) of blocks ``>= first_grad_layer`` is wanted
        (``start_layer`` of the explainability pass): blocks below run without an autograd graph, the graph is cut at
        the input of block ``first_grad_layer`` and that block skips its dq/dk/dv."""
        if not x.is_cuda:
            raise _lib.MMXError("the CLIP body runs its attention on the HIP capture op: move the model and "
                                "inputs to the MI355X (there is no CPU attention path)")
        buffers = self._ensure_buffers(x.shape[0], x.shape[1], x.device)
        self._probs_pending = None            # this (dense) forward writes every row of the slabs
        if not capture_only:
            for l, blk in enumerate(self.resblocks):
                x = blk(x, buffers, l)
            return x
        with torch.no_grad():
            for l in range(first_grad_layer):
                x = self.resblocks[l](x, buffers, l)
        x = x.detach().requires_grad_(True)
        for l in range(first_grad_layer, self.layers):
            x = self.resblocks[l](x, buffers, l, need_dqkv=(l != first_grad_layer))
        return x


class VisualTransformer(nn.Module):
    """ViT image tower (CLIP/clip/model.py:211-246)."""

    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim):
        super().__init__()
        self.input_resolution, self.output_dim = input_resolution, output_dim
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))

    def _patchify(self, x):
        """``conv1`` has kernel == stride == patch, i.e. it is a GEMM over flattened patches.  Doing it as one keeps
        MIOpen (solver search, and its naive fp32 fallback kernel: 24 ms per call here) off the path."""
        B, C, Hh, Ww = x.shape
        p = self.conv1.kernel_size[0]
        gh, gw = Hh // p, Ww // p
        patches = x.reshape(B, C, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B, gh * gw, C * p * p)
        return F.linear(patches, self.conv1.weight.reshape(self.conv1.out_channels, -1))

    def _embed(self, x):
        x = self._patchify(x)                                               # [B, grid^2, width]
        cls = self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1)
        return self.ln_pre(torch.cat([cls, x], dim=1) + self.positional_embedding.to(x.dtype))

    def forward(self, x, capture_only=False, first_grad_layer=0):
        x = self.transformer(self._embed(x), capture_only=capture_only, first_grad_layer=first_grad_layer)
        x = self.ln_post(x[:, 0, :])
        return x @ self.proj if self.proj is not None else x

    def row_relevancy_ok(self):
        """Can ``backward_tape(..., cls_row=True)`` run?  (bf16-body tower on the long-sequence streaming kernels.)"""
        t = self.transformer
        n_tokens = self.positional_embedding.shape[0]
        return bool(getattr(t, "attention_mma_bf16", False)) and n_tokens > 128

    @torch.no_grad()
    def forward_tape(self, image, batch=None, first_grad_layer=0, grads=True):
        """``image [Bx, 3, R, R]`` -> ``(features [Bx, output_dim], state)``; ``Bx == 1 < batch``: shared-forward mode
        (see ``Transformer.forward_tape``)."""
        x = self._embed(image)
        y, tape = self.transformer.forward_tape(x, batch, first_grad_layer, grads=grads,
                                                out_rows=torch.zeros(x.shape[0], dtype=torch.long, device=x.device))
        cls = y                                                              # [Bx, width]: the class-token rows
        _, f, mean, rstd = ops.add_layernorm(cls, None, self.ln_post.weight, self.ln_post.bias, self.ln_post.eps)
        return f @ self.proj, (tape, x.shape, cls, mean, rstd)

    def forward_shared(self, image, batch):
        return self.forward_tape(image, batch)

    @torch.no_grad()
    def encode_nocapture(self, images=None, tokens=None):
        """Inference forward -> image features ``[B, output_dim]`` (``Transformer.forward_nocapture``: no capture slab, no
        tape; the top block on the class-token row only).  ``tokens [B, n, width]``: rows of the block input (``_embed``: class token first, position
        embedding added, through ``ln_pre``, which is row-wise; any ``n``) instead of ``images``."""
        if (images is None) == (tokens is None):
            raise ValueError("encode_nocapture takes images or tokens (exactly one of them)")
        if self.conv1.weight.dtype != torch.float32:
            raise _lib.MMXError("encode_nocapture: fp32 bodies only; the parameters are %s"
                                % str(self.conv1.weight.dtype).replace("torch.", ""))
        x = self._embed(images) if tokens is None else tokens
        cls = self.transformer.forward_nocapture(x, out_rows=0)
        _, f, _, _ = ops.add_layernorm(cls, None, self.ln_post.weight, self.ln_post.bias, self.ln_post.eps)
        return f @ self.proj

    @torch.no_grad()
    def backward_tape(self, state, d_features, first_grad_layer=0, cls_row=False, targets_per_image=1):
        """``d_features [B, output_dim]``: per-sample upstream gradients of the image features.
        ``cls_row=True``: row-relevancy mode (``Transformer.backward_tape``): returns row 0 (the class token's) of the
        tower's relevancy matrix, ``[B, N]``, instead of filling gradient slabs.
        ``targets_per_image=K`` (with ``cls_row``, fp32 body): ``d_features`` is ``[K*M, output_dim]`` over the M images of the
        forward, K-major (target t explains image t % M); returns ``[K*M, N]`` in the same order."""
        tape, y_shape, cls, mean, rstd = state
        B = d_features.shape[0]
        if int(targets_per_image) > 1 and not cls_row:
            raise ValueError("backward_tape: targets_per_image needs cls_row=True (the grouped mode is a row mode)")
        d_f = torch.matmul(d_features, self.proj.t())
        # LayerNorm' against the (shared) class-token rows' statistics; only the class token feeds the features
        d_cls = ops.layernorm_bwd_add(d_f, cls, mean, rstd, self.ln_post.weight)
        rel_row = None
        if cls_row:
            rel_row = torch.zeros(B, y_shape[1], dtype=torch.float32, device=d_f.device)
            rel_row[:, 0] = 1.0                                              # e_0: row 0 of the identity R starts from
        return self.transformer.backward_tape(tape, None, first_grad_layer,
                                              dy_rows=0, rel_row=rel_row,
                                              dy_row_values=d_cls, targets_per_image=targets_per_image)

    def backward_shared(self, state, d_features, first_grad_layer=0):
        return self.backward_tape(state, d_features, first_grad_layer)


class CLIP(nn.Module):
    """Same constructor signature as the reference ``CLIP`` (CLIP/clip/model.py:249-262); ViT towers only."""

    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size,
                 context_length, vocab_size, transformer_width, transformer_heads, transformer_layers):
        super().__init__()
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError("ModifiedResNet towers have no attention stack; use a ViT config")
        self.context_length = context_length
        self.visual = VisualTransformer(image_resolution, vision_patch_size, vision_width, vision_layers,
                                        vision_width // 64, embed_dim)
        self.transformer = Transformer(transformer_width, transformer_layers, transformer_heads,
                                       attn_mask=self.build_attention_mask())
        self.vocab_size = vocab_size
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = nn.LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.capture_only = False
        self.first_grad_layers = (0, 0)     # (image tower, text tower) start layers of a capture-only pass
        self.initialize_parameters()

    def initialize_parameters(self):
        """Same distributions as the reference (model.py:305-332)."""
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        w, n = self.transformer.width, self.transformer.layers
        proj_std, attn_std, fc_std = (w ** -0.5) * ((2 * n) ** -0.5), w ** -0.5, (2 * w) ** -0.5
        for blk in self.transformer.resblocks:
            nn.init.normal_(blk.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(blk.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(blk.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(blk.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=w ** -0.5)

    def set_body_dtype(self, dtype):
        """``torch.bfloat16``: BASELINE config 5's bf16 body -- both towers' GEMMs on the bf16 matrix cores (fp32
        accumulate), the image tower's attention products too, its capture slabs in bf16; relevancy (A-bar, R) stays fp32.
        ``torch.float16``: the reference's own half-precision mode (``convert_weights``, CLIP/clip/model.py:381-402): fp16 GEMMs
        and the fp16 relevancy chain of notebook cell 6:20,43 -- ``interpret`` then returns fp16 like the reference does.
        ``torch.float32``: back to the exact path."""
        self.visual.transformer.set_body_dtype(dtype)
        self.transformer.set_body_dtype(dtype)

    def build_attention_mask(self):
        """Additive causal mask, -inf above the diagonal (model.py:334-340)."""
        return torch.full((self.context_length, self.context_length), float("-inf")).triu_(1)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def encode_image(self, image):
        return self.visual(image.type(self.dtype), capture_only=self.capture_only,
                           first_grad_layer=self.first_grad_layers[0])

    def encode_text(self, text, n_tokens=None):
        """``n_tokens``: run only the first ``n_tokens`` positions (must cover every sequence's EOT token).  With the
        causal mask nothing after a sequence's EOT can influence its feature, so this is exact, not an approximation."""
        if n_tokens is not None and n_tokens < text.shape[1]:
            text = text[:, :n_tokens]
        n = text.shape[1]
        x = self.token_embedding(text).type(self.dtype) + self.positional_embedding[:n].type(self.dtype)
        x = self.transformer(x, capture_only=self.capture_only, first_grad_layer=self.first_grad_layers[1])
        x = self.ln_final(x)
        # features at the EOT token = highest token id in each sequence (model.py:360)
        return x[torch.arange(x.shape[0], device=x.device), text.argmax(dim=-1)] @ self.text_projection

    @torch.no_grad()
    def encode_text_tape(self, text, n_tokens=None, first_grad_layer=0):
        """``encode_text`` on the tape path -> ``(features [B, embed_dim], state)`` for ``backward_text_tape``."""
        if n_tokens is not None and n_tokens < text.shape[1]:
            text = text[:, :n_tokens]
        n = text.shape[1]
        x = self.token_embedding(text).type(self.dtype) + self.positional_embedding[:n].type(self.dtype)
        eot = text.argmax(dim=-1)                                            # model.py:360
        # the rows up to each EOT token, picked on the device: the forward runs on them where the tower is eligible, and the state
        # hands the same list to the backward (None: dense forward; the backward then decides for itself, _live_rows_route)
        live = self.transformer.live_rows_for_forward(x, eot)
        rows, tape = self.transformer.forward_tape(x, first_grad_layer=first_grad_layer, out_rows=eot, live=live)
        _, f, mean, rstd = ops.add_layernorm(rows, None, self.ln_final.weight, self.ln_final.bias, self.ln_final.eps)
        return f @ self.text_projection, (tape, x.shape, rows, mean, rstd, eot, live)

    @torch.no_grad()
    def encode_text_nocapture(self, text, live=False, eot=None):
        """``encode_text`` as an inference forward (``Transformer.forward_nocapture``) -> ``features [B, embed_dim]``.
        ``live=True``: on the rows up to each caption's EOT token where the tower is eligible (``Transformer.live_rows_for_forward``;
        the dense forward where it is not) -- the re-runs of the caption perturbation test (``clip_text_perturbation``), whose
        captions get shorter with every step.  Default: the dense forward.  ``eot [B]`` long: ``text.argmax(dim=-1)`` where the
        caller holds it already."""
        x = self.token_embedding(text).type(self.dtype) + self.positional_embedding[:text.shape[1]].type(self.dtype)
        if eot is None:
            eot = text.argmax(dim=-1)                                                      # model.py:360
        rows = self.transformer.forward_nocapture(x, out_rows=eot,
                                                  live=self.transformer.live_rows_for_forward(x, eot) if live else None)
        _, f, _, _ = ops.add_layernorm(rows, None, self.ln_final.weight, self.ln_final.bias, self.ln_final.eps)
        return f @ self.text_projection

    @torch.no_grad()
    def backward_text_tape(self, state, d_features, first_grad_layer=0):
        """``d_features [B, embed_dim]`` -> fills the text tower's gradient slabs (``ln_final`` is row-wise, so only the
        EOT rows carry a gradient into the stack)."""
        tape, y_shape, rows, mean, rstd, eot, live = state
        d_f = torch.matmul(d_features, self.text_projection.t())
        d_rows = ops.layernorm_bwd_add(d_f, rows, mean, rstd, self.ln_final.weight)
        self.transformer.backward_tape(tape, None, first_grad_layer, dy_rows=eot, dy_row_values=d_rows,
                                       live=live)

    def forward(self, image, text):
        return self.logits(self.encode_image(image), self.encode_text(text))

    def logits(self, image_features, text_features):
        """Cosine-similarity logits (model.py:369-378) from un-normalised features."""
        image_features = image_features / image_features.norm(dim=-1, keepdim=True)
        text_features = text_features / text_features.norm(dim=-1, keepdim=True)
        logit_scale = self.logit_scale.exp()
        logits_per_image = logit_scale * image_features @ text_features.t()
        logits_per_text = logit_scale * text_features @ image_features.t()
        return logits_per_image, logits_per_text


def build_model(state_dict):
    """Infer the ViT config from a state dict like the reference's ``build_model`` (model.py:405-442), fp32."""
    if "visual.proj" not in state_dict:
        raise NotImplementedError("only ViT CLIP checkpoints carry an attention stack to explain")
    vision_width = state_dict["visual.conv1.weight"].shape[0]
    vision_layers = len([k for k in state_dict if k.startswith("visual.") and k.endswith(".attn.in_proj_weight")])
    vision_patch_size = state_dict["visual.conv1.weight"].shape[-1]
    grid_size = round((state_dict["visual.positional_embedding"].shape[0] - 1) ** 0.5)
    embed_dim = state_dict["text_projection"].shape[1]
    context_length = state_dict["positional_embedding"].shape[0]
    vocab_size = state_dict["token_embedding.weight"].shape[0]
    transformer_width = state_dict["ln_final.weight"].shape[0]
    transformer_layers = len({k.split(".")[2] for k in state_dict if k.startswith("transformer.resblocks")})
    model = CLIP(embed_dim, vision_patch_size * grid_size, vision_layers, vision_width, vision_patch_size,
                 context_length, vocab_size, transformer_width, transformer_width // 64, transformer_layers)
    sd = {k: v.float() for k, v in state_dict.items() if k not in ("input_resolution", "context_length", "vocab_size")}
    model.load_state_dict(sd)
    return model.eval()


CONFIGS = {
    # (embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size,
    #  context_length, vocab_size, transformer_width, transformer_heads, transformer_layers)
    "ViT-B/32": (512, 224, 12, 768, 32, 77, 49408, 512, 8, 12),
    "ViT-B/16": (512, 224, 12, 768, 16, 77, 49408, 512, 8, 12),
    "ViT-L/14@336": (768, 336, 24, 1024, 14, 77, 49408, 768, 12, 12),
}


def random_init(name="ViT-B/32", seed=0):
    """Random-init model of a named architecture (no pretrained weights are available offline)."""
    torch.manual_seed(seed)
    return CLIP(*CONFIGS[name]).float().eval()
