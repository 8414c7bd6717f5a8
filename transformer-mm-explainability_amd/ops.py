"""Thin torch-tensor front end over the C-ABI (``_lib``): pointer/stride plumbing only.

Every function requires HIP-device tensors and launches on torch's current stream.  There is no CPU
path and no PyTorch-op fallback: a CPU tensor or a missing ``libmmx_hip.so`` raises.
"""
from __future__ import annotations

import contextlib
import threading
import ctypes as C
import gc
import os
import weakref

import torch

from . import _lib
from ._lib import MMXError, check, lib

_DTYPES = {torch.float32: _lib.MMX_F32, torch.float16: _lib.MMX_F16, torch.bfloat16: _lib.MMX_BF16}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise MMXError("mmx ops need HIP-device tensors (got %s); there is no CPU path" % t.device)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _f32c(t):
    """fp32 + contiguous (no copy when already so)."""
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _capture(t):
    if t.dtype not in _DTYPES:
        raise MMXError("captured buffers must be fp32/fp16/bf16, got %s" % t.dtype)
    return t.contiguous()


_ws_cache = {}


def set_option(key, value):
    """Process-wide tuning knob of the C library (see ``mmx_set_option`` in include/mmx_relevancy.h)."""
    check(lib().mmx_set_option(key.encode(), int(value)), "mmx_set_option")


def _workspace(nbytes, device, tag="default"):
    """Grow-only scratch per (device, stream, tag): reuse is stream-ordered, so every stream owns its own."""
    if nbytes == 0:
        return None
    key = (device, torch.cuda.current_stream(device).cuda_stream, tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


_SIDE_STREAMS = {}
_CAPTURE = threading.local()     # .side: the private side stream of the capture in progress on this thread (graph_capture)


def side_stream(device, slot=0):
    """The side stream independent chains of an explainability pass run on beside the current stream (LXMERT's two modalities,
    DETR's / ViT's rule kernels beside the backward, CLIP's second tower).  Eager calls share one stream per (device, slot),
    created once; INSIDE ``graph_capture`` every capture gets a PRIVATE side stream (and a private capture stream) that lives
    and dies with its graph.  Why: graphs captured across streams that earlier, since destroyed, graphs had also been captured
    across segfaulted inside ``hipGraphLaunch`` (round 3: the DETR pass after CLIP / ViT graphs in one process, ``bench.py``'s
    config legs and the GPU test suite) -- with no stream shared between two captures the same sequences are clean.
    Use ONE side stream per pass."""
    if os.environ.get("MMX_DEBUG_NO_SIDE"):          # debugging aid (MMX_DEBUG_NO_SIDE=1): every chain on the current stream
        return torch.cuda.current_stream(device)
    private = getattr(_CAPTURE, "side", None)
    if private is not None:
        return private
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), slot)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=key[0])
    return _SIDE_STREAMS[key]


@contextlib.contextmanager
def graph_capture(graph):
    """``torch.cuda.graph(graph, ...)`` the way every ``Graphed*`` wrapper of this package captures:

    * Python's cyclic garbage collector is held off for the duration of the capture.  A collection that happens to run INSIDE a
      capture may destroy objects whose destructors issue HIP calls that are illegal while a stream is capturing -- a
      ``torch.cuda.CUDAGraph`` of an earlier, already dropped wrapper releases its private memory pool (``hipFree``) -- and an
      exception in a C++ destructor aborts the process (seen as "Fatal Python error: Aborted ... Garbage-collecting" in the GPU
      test suite).  ``torch.cuda.graph`` collects once BEFORE the capture begins; this keeps the collector from firing again.
    * the capture runs on its OWN capture stream and ``side_stream()`` hands out a side stream private to this capture (see
      there); both, and the scratch buffers first allocated on them, are kept on the graph object and released with it.
    * ``capture_error_mode="thread_local"``: a collective backend's watchdog thread (RCCL, one rank per GPU) may poll events
      while this thread captures; only calls made by the capturing thread must be capture-safe."""
    was_enabled = gc.isenabled()
    gc.collect()
    gc.disable()
    capture_stream, private_side = torch.cuda.Stream(), torch.cuda.Stream()
    known = set(_ws_cache)
    _CAPTURE.side = private_side
    try:
        with torch.cuda.graph(graph, stream=capture_stream, capture_error_mode="thread_local"):
            yield
    finally:
        _CAPTURE.side = None
        # scratch first allocated on the private streams belongs to this graph alone: off the shared cache, onto the graph
        graph._mmx_private = ([_ws_cache.pop(k) for k in list(_ws_cache) if k not in known], capture_stream, private_side)
        if was_enabled:
            gc.enable()


def pinned_state(model=None):
    """Everything a captured hipGraph may have baked raw addresses of, besides its own pool: the grow-only scratch
    buffers of this module and (``model`` given) the capture slabs of every hooked attention module.  A ``Graphed*``
    wrapper keeps the returned list alive: a later EAGER call that needs a bigger scratch buffer or other slab shapes
    replaces those tensors, and without this reference the old ones would be freed under the graph."""
    keep = list(_ws_cache.values())
    if model is not None:
        for mod in model.modules():
            for name in ("_probs", "_grads"):
                t = getattr(mod, name, None)
                if torch.is_tensor(t):
                    keep.append(t)
            buf = getattr(mod, "buffers", None)
            if buf is not None and hasattr(buf, "probs") and hasattr(buf, "grads"):
                keep.extend([buf.probs, buf.grads, buf])
    return keep


# ------------------------------------------------------------------------------------------- rule 5
def avg_heads(cam, grad, batch_size=1, shared_attn=False):
    """``mean_h(clamp(grad*cam, 0))`` -> ``[batch_size, Nq, Nk]`` fp32 (leading dims flattened into B*H).
    ``shared_attn=True``: ``cam`` holds ONE sample's heads, shared by the ``batch_size`` samples of ``grad``."""
    _dev(cam, grad)
    cam, grad = _capture(cam), _capture(grad)
    nq, nk = grad.shape[-2], grad.shape[-1]
    bh = grad.numel() // (nq * nk)
    ok = cam.numel() * batch_size == grad.numel() if shared_attn else cam.shape == grad.shape
    if not ok or cam.shape[-2:] != grad.shape[-2:] or cam.dtype != grad.dtype:
        raise MMXError("avg_heads: cam %s/%s vs grad %s/%s" % (tuple(cam.shape), cam.dtype, tuple(grad.shape), grad.dtype))
    if bh % batch_size:
        raise MMXError("avg_heads: %d matrices not divisible by batch %d" % (bh, batch_size))
    out = torch.empty(batch_size, nq, nk, dtype=torch.float32, device=cam.device)
    check(lib().mmx_avg_heads_ex(_p(cam), _p(grad), _p(out), batch_size, bh // batch_size, nq, nk, _DTYPES[cam.dtype],
                                 0 if shared_attn else -1, _stream()), "mmx_avg_heads_ex")
    return out


# ------------------------------------------------------------------------------------------- fused chain
def relevancy_self_chain(attn_layers, grad_layers, batch_size, R_init=None, R_sq_init=None, shared_attn=False, causal=False):
    """All-layer chain ``R <- R + A_bar_l @ R`` (``R_0 = I`` or ``R_init``) [and ``R_sq`` likewise] in one call.

    ``attn_layers[l]`` / ``grad_layers[l]``: ``[B*H, N, N]`` or ``[B, H, N, N]`` (fp32/fp16/bf16).
    ``shared_attn=True``: ``attn_layers[l]`` holds ONE sample's heads (``[H, N, N]``) shared by all ``batch_size``
    samples of ``grad_layers[l]`` (shared-forward mode; read with batch stride 0).
    ``causal=True``: the probabilities come from causally masked attention (exact zeros above the diagonal, CLIP's text tower):
    the kernels do not read what lies above the diagonal (``MMX_CHAIN_CAUSAL``); same bits, about half the bytes.
    Returns ``R [B, N, N]`` (and ``R_sq [B, N, M]`` when ``R_sq_init`` is given).
    """
    if len(attn_layers) != len(grad_layers):
        raise MMXError("self_chain: %d attn layers vs %d grad layers" % (len(attn_layers), len(grad_layers)))
    if len(attn_layers) > _lib.MAX_LAYERS:
        raise MMXError("self_chain: more than %d layers" % _lib.MAX_LAYERS)
    _dev(*attn_layers, *grad_layers, R_init, R_sq_init)
    attn = [_capture(a) for a in attn_layers]
    grad = [_capture(g) for g in grad_layers]
    ref = attn[0] if attn else R_init
    if ref is None:
        raise MMXError("self_chain: no layers and no R_init")
    n = ref.shape[-1]
    device = ref.device
    dt = _DTYPES[attn[0].dtype] if attn else _lib.MMX_F32
    heads = 1
    for a, g in zip(attn, grad):
        if (a.shape != g.shape and not shared_attn) or a.dtype != attn[0].dtype or g.dtype != attn[0].dtype \
                or a.shape[-1] != n or a.shape[-2] != n or (shared_attn and a.numel() * batch_size != g.numel()):
            raise MMXError("self_chain: inconsistent layer shapes/dtypes")
    if attn:
        bh = grad[0].numel() // (n * n)
        if bh % batch_size:
            raise MMXError("self_chain: %d matrices not divisible by batch %d" % (bh, batch_size))
        heads = bh // batch_size
    R_out = torch.empty(batch_size, n, n, dtype=torch.float32, device=device)
    if R_init is not None:
        R_init = _f32c(R_init).expand(batch_size, n, n).contiguous()
    m = 0
    sq_out = None
    if R_sq_init is not None:
        R_sq_init = _f32c(R_sq_init)
        m = R_sq_init.shape[-1]
        R_sq_init = R_sq_init.expand(batch_size, n, m).contiguous()
        sq_out = torch.empty(batch_size, n, m, dtype=torch.float32, device=device)
    need = lib().mmx_self_chain_workspace_bytes(len(attn), batch_size, heads, n, m, dt)
    ws = _workspace(need, device)
    at, _k1 = _lib.ptr_table([a.data_ptr() for a in attn])
    gt, _k2 = _lib.ptr_table([g.data_ptr() for g in grad])
    check(lib().mmx_relevancy_self_chain_flags(at, gt, len(attn), batch_size, heads, n, dt, 0 if shared_attn else -1,
                                               _p(R_init), _p(R_out), _p(R_sq_init), _p(sq_out), m,
                                               _lib.CHAIN_CAUSAL if causal else 0, _p(ws), need,
                                               _stream()), "mmx_relevancy_self_chain_flags")
    return (R_out, sq_out) if sq_out is not None else R_out


def relevancy_chain_row(attn_layers, grad_layers, batch_size, rows, shared_attn=False):
    """Row ``rows[b]`` of sample b's ``relevancy_self_chain`` result, ``[B, N]`` -- what the ViT / VisualBERT generators
    return (``R[0, 1:]``, ViT notebook cell 7:34; ``R[cls_index]``, VisualBERT/.../ExplanationGenerator.py:95-97).

    ``R = (I + A_L) ... (I + A_1)``, so ``e_r^T R`` is a row vector carried from the TOP layer down,
    ``x <- x + x A_l`` (``mmx_chain_vecmat``): per layer one head-average pass over the slabs and one mat-vec, instead of
    the N^3 product the long-sequence split path runs.  N <= 128 keeps the one-launch fused kernel (all layers, R in
    registers) and picks the row afterwards -- that is faster there.  Same result up to fp32 summation order."""
    n = grad_layers[0].shape[-1]
    dev = grad_layers[0].device
    fixed = isinstance(rows, int)               # (a Python int needs no host -> device copy: capturable into a hipGraph)
    if not fixed:
        rows = torch.as_tensor(rows, device=dev).reshape(-1).expand(batch_size)
    if n <= 128:
        R = relevancy_self_chain(attn_layers, grad_layers, batch_size, shared_attn=shared_attn)
        return R[:, rows].contiguous() if fixed else R[torch.arange(batch_size, device=dev), rows]
    x = torch.zeros(batch_size, n, dtype=torch.float32, device=dev)
    if fixed:
        x[:, rows] = 1.0
    else:
        x.scatter_(1, rows.reshape(batch_size, 1), 1.0)
    for a, g in zip(reversed(list(attn_layers)), reversed(list(grad_layers))):
        x = chain_vecmat(x, avg_heads(a, g, batch_size=batch_size, shared_attn=shared_attn))
    return x


class _QuickGELU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        check(lib().mmx_quick_gelu_fwd(_p(x), _p(y), x.numel(), _stream()), "mmx_quick_gelu_fwd")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        check(lib().mmx_quick_gelu_bwd(_p(x), _p(dy), _p(dx), x.numel(), _stream()), "mmx_quick_gelu_bwd")
        return dx


def quick_gelu(x):
    """``x * sigmoid(1.702 x)`` as one fused pass forward and one backward (fp32 HIP tensors)."""
    _dev(x)
    if x.dtype != torch.float32:
        raise MMXError("quick_gelu: fp32 only")
    return _QuickGELU.apply(x)


def quick_gelu_fwd(x, out_dtype=torch.float32):
    """``x * sigmoid(1.702 x)``, no autograd (the hand-written backward passes keep ``x`` themselves).  ``out_dtype=torch.bfloat16``
    (a bf16 body: the activation only feeds the next GEMM): the kernel writes bf16, no conversion pass."""
    _dev(x)
    x = _f32c(x)
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise MMXError("quick_gelu_fwd: out_dtype is fp32 or bf16, got %s" % out_dtype)
    if out_dtype == torch.bfloat16 and x.numel() % 4 == 0:
        y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
        check(lib().mmx_quick_gelu_fwd_bf16(_p(x), _p(y), x.numel(), _stream()), "mmx_quick_gelu_fwd_bf16")
        return y
    y = torch.empty_like(x)
    check(lib().mmx_quick_gelu_fwd(_p(x), _p(y), x.numel(), _stream()), "mmx_quick_gelu_fwd")
    # (the bf16 kernel packs four elements a store; any other count takes the fp32 kernel, whose result is rounded once)
    return y if out_dtype == torch.float32 else y.to(torch.bfloat16)


def quick_gelu_bwd(x, dy):
    """``dy * QuickGELU'(x)`` in one pass.  ``x`` has ``dy``'s shape, or batch 1 where ``dy`` has batch B (shared-forward
    mode: the ONE activation tensor is broadcast over the B upstream gradients inside the kernel), or batch M where ``dy`` has
    batch K*M in K-major order (grouped mode: target t reads sample t % M)."""
    _dev(x, dy)
    if dy.dtype == torch.bfloat16:             # bf16 gradient stream: dy / dx bf16, x fp32 (broadcast over the batch)
        x, dy = _f32c(x), dy.contiguous()
        if dy.numel() % x.numel() or x.numel() % 8:
            raise MMXError("quick_gelu_bwd (bf16): x %s does not tile dy %s" % (tuple(x.shape), tuple(dy.shape)))
        dx = torch.empty_like(dy)
        check(lib().mmx_quick_gelu_bwd_bcast_bf16(_p(x), _p(dy), _p(dx), dy.numel(), x.numel(), _stream()),
              "mmx_quick_gelu_bwd_bcast_bf16")
        return dx
    x, dy = _f32c(x), _f32c(dy)
    dx = torch.empty_like(dy)
    if x.shape == dy.shape:
        check(lib().mmx_quick_gelu_bwd(_p(x), _p(dy), _p(dx), x.numel(), _stream()), "mmx_quick_gelu_bwd")
    elif x.shape[1:] == dy.shape[1:] and dy.shape[0] % x.shape[0] == 0 and x.numel() % 4 == 0:
        # (x of batch M < B: the targets are K-major over M samples, target t reading sample t % M)
        check(lib().mmx_quick_gelu_bwd_bcast(_p(x), _p(dy), _p(dx), dy.numel(), x.numel(), _stream()),
              "mmx_quick_gelu_bwd_bcast")
    else:
        raise MMXError("quick_gelu_bwd: x %s vs dy %s" % (tuple(x.shape), tuple(dy.shape)))
    return dx


def _affine(what, E, *vectors):
    """The per-feature operands of a LayerNorm kernel (``gamma``, ``beta``) as fp32 contiguous tensors; the kernel reads ``E`` floats of each."""
    out = []
    for t in vectors:
        if t.numel() != E:
            raise MMXError("%s: a row has %d elements, gamma / beta %d" % (what, E, t.numel()))
        out.append(_f32c(t))
    return out


def _row_stats(what, x_rows, mean, rstd):
    """``mean`` / ``rstd`` of a LayerNorm backward as fp32 contiguous tensors; the kernel reads one of each per row of ``x``."""
    if mean.numel() != x_rows or rstd.numel() != x_rows:
        raise MMXError("%s: %d / %d statistics (mean / rstd) for the %d rows of x" % (what, mean.numel(), rstd.numel(), x_rows))
    return _f32c(mean), _f32c(rstd)


def _bwd_rows(what, dy, x, d_res):
    """The row counts of a LayerNorm backward, checked before a pointer leaves: ``x`` and ``d_res`` have ``dy``'s row width, ``d_res``
    ``dy``'s row count (the kernel reads row ``r`` of both), and ``x``'s rows tile ``dy``'s (row ``r`` reads ``x``'s row ``r % x_rows``)."""
    E = dy.shape[-1] if dy.dim() else 0
    if E == 0 or x.dim() == 0 or x.shape[-1] != E:
        raise MMXError("%s: dy %s and x %s differ in their last dimension" % (what, tuple(dy.shape), tuple(x.shape)))
    rows, x_rows = dy.numel() // E, x.numel() // E
    if x_rows == 0 or rows % x_rows:
        raise MMXError("%s: the %d rows of x do not tile the %d rows of dy" % (what, x_rows, rows))
    if d_res is not None and (d_res.dim() == 0 or d_res.shape[-1] != E or d_res.numel() != dy.numel()):
        raise MMXError("%s: d_res %s is not dy's %d rows of %d" % (what, tuple(d_res.shape), rows, E))
    return E, rows, x_rows


def add_layernorm(x, y, gamma, beta, eps=1e-5, h_dtype=torch.float32):
    """``s = x + y; h = LayerNorm(s)`` in one pass -> ``(s, h, mean, rstd)`` (``y=None``: ``s`` is ``x`` itself).
    ``mean`` / ``rstd``: ``[rows]`` fp32, what ``layernorm_bwd_add`` takes.  ``h_dtype=torch.bfloat16``: ``h`` leaves the kernel
    as bf16 (a bf16 body feeds it to a half-precision GEMM only)."""
    _dev(x, y, gamma, beta)
    x = _f32c(x)
    E = x.shape[-1]
    rows = x.numel() // E
    if y is not None:
        y = _f32c(y)
        if y.shape != x.shape:
            raise MMXError("add_layernorm: x %s vs y %s" % (tuple(x.shape), tuple(y.shape)))
    gamma, beta = _affine("add_layernorm", E, gamma, beta)
    s = torch.empty_like(x) if y is not None else x
    h = torch.empty(x.shape, dtype=h_dtype, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib().mmx_add_layernorm_fwd_ex(_p(x), _p(y), _p(gamma), _p(beta), _p(s) if y is not None else _p(None),
                                         _p(h), _p(mean), _p(rstd), rows, E, float(eps), _DTYPES[h_dtype], _stream()),
          "mmx_add_layernorm_fwd")
    return s, h, mean, rstd


def layernorm_bwd_add(dy, x, mean, rstd, gamma, d_res=None):
    """``d_res + LayerNorm'(dy)`` with forward statistics shared across the batch: ``dy``/``d_res`` ``[B, N, E]``,
    ``x`` ``[1, N, E]`` (or ``[B, N, E]``), ``mean``/``rstd`` matching ``x``'s rows."""
    _dev(dy, x, mean, rstd, gamma, d_res)
    dy, x = _f32c(dy), _f32c(x)
    E, rows, x_rows = _bwd_rows("layernorm_bwd_add", dy, x, d_res)
    mean, rstd = _row_stats("layernorm_bwd_add", x_rows, mean, rstd)
    (gamma,) = _affine("layernorm_bwd_add", E, gamma)
    dx = torch.empty_like(dy)
    check(lib().mmx_layernorm_bwd_add(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma),
                                      _p(_f32c(d_res)) if d_res is not None else _p(None), _p(dx), rows, x_rows, E,
                                      _stream()), "mmx_layernorm_bwd_add")
    return dx


def layernorm_bwd_add_bf16(dy, x, mean, rstd, gamma, d_res=None, want_f32=True):
    """``layernorm_bwd_add`` for a bf16 upstream gradient ``dy``: returns ``(dx fp32 or None, dx bf16)`` -- the fp32 result
    is the next residual gradient, the bf16 copy the operand of the next bf16 GEMM (one pass writes both)."""
    _dev(dy, x, mean, rstd, gamma, d_res)
    if dy.dtype != torch.bfloat16:
        raise MMXError("layernorm_bwd_add_bf16: dy must be bf16")
    dy, x = dy.contiguous(), _f32c(x)
    E, rows, x_rows = _bwd_rows("layernorm_bwd_add_bf16", dy, x, d_res)
    dx = torch.empty(dy.shape, dtype=torch.float32, device=dy.device) if want_f32 else None
    dx_h = torch.empty_like(dy)
    mean, rstd = _row_stats("layernorm_bwd_add_bf16", x_rows, mean, rstd)
    (gamma,) = _affine("layernorm_bwd_add_bf16", E, gamma)
    check(lib().mmx_layernorm_bwd_add_bf16(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma),
                                           _p(_f32c(d_res)) if d_res is not None else _p(None), _p(dx), _p(dx_h), rows,
                                           x_rows, E, _stream()), "mmx_layernorm_bwd_add_bf16")
    return dx, dx_h


_GEMM_WEIGHTS = {}   # id(parameter) -> {dtype: (version, converted copy)}; the entry is dropped when the parameter dies


def _cached_weight(weight, key, make):
    """``make()``'s tensor for ``weight`` under ``key``: built again after an in-place modification of the parameter or its move to
    another device, ``(copy, True)`` then."""
    per_weight = _GEMM_WEIGHTS.get(id(weight))
    if per_weight is None:
        per_weight = _GEMM_WEIGHTS[id(weight)] = {}
        weakref.finalize(weight, _GEMM_WEIGHTS.pop, id(weight), None)
    hit = per_weight.get(key)
    fresh = hit is None or hit[0] != weight._version or hit[1].device != weight.device
    if fresh:
        hit = per_weight[key] = (weight._version, make())
    return hit[1], fresh


def _converted(weight, dtype):
    return _cached_weight(weight, dtype, lambda: weight.detach().to(dtype))[0]


def transposed_weight(weight):
    """Cached contiguous ``weight.t()`` (until the parameter is modified in place).  The input-gradient product ``dY . W`` of
    a Linear with few outputs and many inputs (DETR's ``linear2``: 256 -> 2048 on the way back) gets a poor library kernel in its
    natural NN layout (64x64x16 tiles: 140 us at 9500 rows); as ``F.linear(dY, W^T)`` the heuristic picks a 256-wide one
    (104 us) -- profiles/r03_detr_probe.txt."""
    return _cached_weight(weight, "t", lambda: weight.detach().t().contiguous())[0]


def sign_split_weight(weight, transposed=False):
    """Cached ``[clamp(W, min=0) | clamp(W, max=0)]`` (``[out, 2 in]``, until the parameter is modified in place): the weight
    operand of both GEMMs of the fused ``Linear.relprop`` (``lrp_linear``); ``transposed``: its contiguous ``[2 in, out]`` form."""
    def split():
        w = weight.detach().float()
        return torch.cat((w.clamp(min=0), w.clamp(max=0)), dim=1).contiguous()

    pn, fresh = _cached_weight(weight, "pn", split)
    if fresh:
        _GEMM_WEIGHTS[id(weight)].pop("pnT", None)   # (the transposed copy follows its source)
    if not transposed:
        return pn
    return _cached_weight(weight, "pnT", lambda: pn.t().contiguous())[0]


def lrp_fusable(*tensors):
    """The fused LRP rule kernels take fp32 CUDA tensors (anything else -- the CPU suite's host-logic tests -- runs the torch
    formulation in ``lrp.py``)."""
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def lrp_linear(R, X, weight, normalize):
    """``Linear.relprop`` (alpha = 1) as 2 GEMMs + 3 (4 with ``normalize``) launches: see ``csrc/lrp_kernels.hip``.
    ``R [..., out]``, ``X [..., in]``, ``weight [out, in]`` -> ``[..., in]``."""
    n_in, n_out = X.shape[-1], R.shape[-1]
    # the kernels index R by X's rows and the weight by (R, X)'s last dimensions: a mismatched or broadcastable R must not reach them
    if tuple(R.shape[:-1]) != tuple(X.shape[:-1]) or tuple(weight.shape) != (n_out, n_in):
        raise MMXError("lrp_linear: R %s, X %s, weight %s do not describe Linear.relprop (R [..., out], X [..., in], weight "
                       "[out, in] with equal leading dimensions)" % (tuple(R.shape), tuple(X.shape), tuple(weight.shape)))
    Xc, Rc = X.contiguous(), R.contiguous()
    rows = Xc.numel() // n_in
    WW = sign_split_weight(weight)                                   # [out, 2 in]
    st = _stream()
    XX = torch.empty(rows, 2 * n_in, dtype=torch.float32, device=X.device)
    check(lib().mmx_lrp_split_signs(_p(Xc), _p(XX), rows, n_in, st), "mmx_lrp_split_signs")

    def mm(a, wt_of, k, n):       # a [rows, k] . Wt [k, n]; few rows and a short contraction: the library's heuristic picks a
        if rows <= 128 and k <= 1024:   # 256-row tile on ONE workgroup (30-40 us, r04_lrp_probe.txt) -> our 32 x 32-tile kernel
            out_ = torch.empty(rows, n, dtype=torch.float32, device=a.device)
            check(lib().mmx_linear_f32(_p(a), _p(wt_of()), None, _p(out_), rows, n, k, st), "mmx_linear_f32")
            return out_
        return torch.mm(a, wt_of())
    Z = mm(XX, lambda: sign_split_weight(weight, transposed=True) if rows <= 128 and 2 * n_in <= 1024 else WW.t(), 2 * n_in, n_out)
    S = torch.empty_like(Z)                                          # Z [rows, out] = px pw^T + nx nw^T  (K = 2 in)
    check(lib().mmx_lrp_safe_divide(_p(Rc), _p(Z), _p(S), Z.numel(), st), "mmx_lrp_safe_divide")
    Y = mm(S, lambda: WW, n_out, 2 * n_in)                           # [rows, 2 in] = [S pw | S nw]
    out = torch.empty(X.shape, dtype=torch.float32, device=X.device)
    ws = _workspace(lib().mmx_lrp_workspace_bytes(), X.device, tag="lrp") if normalize else None
    check(lib().mmx_lrp_linear_combine(_p(XX), _p(Y), _p(out), rows, n_in, _p(Rc) if normalize else None, Rc.numel(),
                                       _p(ws), st), "mmx_lrp_linear_combine")
    return out


def lrp_mha_rescale(cam_v_pre, cam_v_post, cam_k, cam_q, cam_o):
    """The q / k rescale branch of ``MultiheadAttention.relprop`` (layers.py:791-799) in two launches; returns ``(cam_k, cam_q)``
    (fresh contiguous tensors, scaled in place when the branch applies)."""
    vp, vq = cam_v_pre.contiguous(), cam_v_post.contiguous()
    ck, cq, co = cam_k.contiguous().clone(), cam_q.contiguous().clone(), cam_o.contiguous()
    ws = _workspace(lib().mmx_lrp_workspace_bytes(), cam_k.device, tag="lrp")
    check(lib().mmx_lrp_mha_rescale(_p(vp), vp.numel(), _p(vq), vq.numel(), _p(ck), ck.numel(), _p(cq), cq.numel(), _p(co),
                                    co.numel(), _p(ws), _stream()), "mmx_lrp_mha_rescale")
    return ck, cq


def lrp_add(R, a, b, per_sample):
    """``Add.relprop`` in two launches -> ``(R_a, R_b)``; ``per_sample``: the rule's three sums per leading-dimension item."""
    Rc, ac, bc = R.contiguous(), a.contiguous(), b.contiguous()
    batch = Rc.shape[0] if (per_sample and Rc.dim() > 1) else 1
    if batch > 64:
        return None
    ra, rb = torch.empty_like(Rc), torch.empty_like(Rc)
    ws = _workspace(lib().mmx_lrp_workspace_bytes(), R.device, tag="lrp")
    check(lib().mmx_lrp_add_relprop(_p(Rc), _p(ac), _p(bc), _p(ra), _p(rb), batch, Rc.numel() // batch, _p(ws), _stream()),
          "mmx_lrp_add_relprop")
    return ra, rb


def lrp_clone(Rs, X):
    """``Clone.relprop`` in one launch (up to 8 relevance tensors)."""
    Xc = X.contiguous()
    rc = [r.contiguous() for r in Rs]
    out = torch.empty_like(Xc)
    tbl, _k = _lib.ptr_table([r.data_ptr() for r in rc])
    check(lib().mmx_lrp_clone_relprop(tbl, len(rc), _p(Xc), _p(out), Xc.numel(), _stream()), "mmx_lrp_clone_relprop")
    return out


_MM_OUT_DTYPE = [None]      # does torch.mm(a, b, out_dtype=torch.float32) work on this build / device?  probed once


def _mm_f32_out(a, b):
    """``a @ b`` for 2-D half-precision operands with an fp32 result straight from the GEMM's fp32 accumulators
    (``aten::mm.dtype``) -- no rounding of the result to bf16 and no conversion pass; falls back to ``.float()``."""
    if _MM_OUT_DTYPE[0] is None:
        try:
            torch.mm(a[:1], b, out_dtype=torch.float32)
            _MM_OUT_DTYPE[0] = True
        except (RuntimeError, TypeError):
            _MM_OUT_DTYPE[0] = False
    if _MM_OUT_DTYPE[0]:
        return torch.mm(a, b, out_dtype=torch.float32)
    return torch.mm(a, b).float()


def backward_gemm_bf16(x, weight):
    """``x (bf16) @ weight`` -> bf16: a GEMM of the bf16 gradient stream (fp32 accumulation inside the library kernel,
    result rounded once); the bf16 copy of ``weight`` is cached like ``backward_gemm``'s."""
    w = _converted(weight, torch.bfloat16)
    return torch.mm(x.reshape(-1, x.shape[-1]), w).view(*x.shape[:-1], w.shape[-1])


def backward_gemm(x, weight, dtype=torch.float32):
    """``x @ weight`` for the hand-written (shared-forward) backward passes.  ``dtype=torch.bfloat16`` (opt-in per tower /
    body, ``backward_gemm_dtype``) runs it on the bf16 MFMA with fp32 accumulation and an fp32 result; the converted
    weight is cached until the parameter is modified in place.  A plain library GEMM either way (hipBLASLt / rocBLAS)."""
    if dtype == torch.float32:
        return torch.matmul(x, weight)
    w = _converted(weight, dtype)
    return _mm_f32_out(x.reshape(-1, x.shape[-1]).to(dtype), w).view(*x.shape[:-1], w.shape[-1])


def linear(x, weight, bias=None, dtype=torch.float32):
    """``F.linear`` for the tape forward passes; ``dtype=torch.bfloat16`` (a bf16 body, ``forward_gemm_dtype``) rounds
    ``x`` and the (cached) weight to bf16, accumulates in fp32 and returns fp32."""
    if dtype == torch.float32:
        return torch.nn.functional.linear(x, weight, bias)
    w = _converted(weight, dtype)
    y = _mm_f32_out(x.reshape(-1, x.shape[-1]).to(dtype), w.t()).view(*x.shape[:-1], w.shape[0])
    return y if bias is None else y.add_(bias)


class ChainPlan:
    """A prepared ``relevancy_self_chain`` launch over persistent slabs: pointer tables, scratch and the output tensor are
    built once; ``launch()`` is a single C call (no per-call Python tensor plumbing).  The captured slabs of a tower
    keep their addresses from step to step, so the plan stays valid as long as the tensors it references are alive."""

    def __init__(self, attn_layers, grad_layers, batch_size, shared_attn=False, half_chain=False, causal=False):
        """``half_chain``: the reference's fp16 chain (``mmx_relevancy_self_chain_half``: every tensor-level result of the rule
        rounded to fp16, like the notebook's R on a model after ``convert_weights``); ``launch`` then returns an fp16 tensor."""
        _dev(*attn_layers, *grad_layers)
        self.half_chain = bool(half_chain)
        self.flags = _lib.CHAIN_CAUSAL if causal else 0     # ``causal``: see ``relevancy_self_chain``
        self.attn = [_capture(a) for a in attn_layers]
        self.grad = [_capture(g) for g in grad_layers]
        if not self.attn or len(self.attn) != len(self.grad) or len(self.attn) > _lib.MAX_LAYERS:
            raise MMXError("ChainPlan: need 1..%d (attn, grad) layer pairs" % _lib.MAX_LAYERS)
        g0 = self.grad[0]
        self.n = g0.shape[-1]
        self.batch = batch_size
        self.heads = g0.numel() // (self.n * self.n) // batch_size
        self.dt = _DTYPES[g0.dtype]
        self.shared = 0 if shared_attn else -1
        for a, g in zip(self.attn, self.grad):
            if g.shape != g0.shape or g.dtype != g0.dtype or a.dtype != g0.dtype or \
                    a.numel() * (batch_size if shared_attn else 1) != g.numel():
                raise MMXError("ChainPlan: inconsistent layer shapes/dtypes")
        self.device = g0.device
        if self.half_chain and g0.dtype == torch.bfloat16:
            raise MMXError("ChainPlan: the fp16 chain reads fp32 or fp16 slabs")
        self.need = lib().mmx_self_chain_workspace_bytes(len(self.attn), batch_size, self.heads, self.n, 0, self.dt)
        if self.half_chain and self.n <= 128:
            self.need = 0                                  # one fused launch per call, no scratch
        self.ws = torch.empty(max(self.need, 1), dtype=torch.uint8, device=g0.device)
        self.at, self._k1 = _lib.ptr_table([a.data_ptr() for a in self.attn])
        self.gt, self._k2 = _lib.ptr_table([g.data_ptr() for g in self.grad])

    def launch(self, out=None):
        """Enqueue on torch's current stream; returns ``R [B, N, N]`` (a fresh tensor unless ``out`` is given)."""
        if out is None:
            out = torch.empty(self.batch, self.n, self.n, dtype=torch.float32, device=self.device)
        if self.half_chain:
            check(lib().mmx_relevancy_self_chain_half(self.at, self.gt, len(self.attn), self.batch, self.heads, self.n, self.dt,
                                                      self.shared, _p(out), _p(self.ws), self.need, _stream()),
                  "mmx_relevancy_self_chain_half")
            return out.to(torch.float16)                   # lossless: the kernel rounds every result to fp16
        check(lib().mmx_relevancy_self_chain_flags(self.at, self.gt, len(self.attn), self.batch, self.heads, self.n, self.dt,
                                                   self.shared, None, _p(out), None, None, 0, self.flags, _p(self.ws), self.need,
                                                   _stream()), "mmx_relevancy_self_chain_flags")
        return out


# ------------------------------------------------------------------------------------------- matmul
def matmul(a, b, add_to=None, trans_a=False, nan_to_zero=False):
    """fp32 ``op(a) @ b (+ add_to)`` on the exact-fp32 MFMA; 2-D or batched 3-D (2-D operands broadcast)."""
    _dev(a, b, add_to)
    a, b = _f32c(a), _f32c(b)
    batch = 1
    for t in (a, b):
        if t.dim() == 3:
            batch = max(batch, t.shape[0])
    am, ak = (a.shape[-1], a.shape[-2]) if trans_a else (a.shape[-2], a.shape[-1])
    if b.shape[-2] != ak:
        raise MMXError("matmul: inner dims %d vs %d" % (ak, b.shape[-2]))
    n = b.shape[-1]
    sa = a.shape[-2] * a.shape[-1] if (a.dim() == 3 and a.shape[0] > 1) else 0
    sb = ak * n if (b.dim() == 3 and b.shape[0] > 1) else 0
    squeeze = a.dim() == 2 and b.dim() == 2
    out = torch.empty(batch, am, n, dtype=torch.float32, device=a.device)
    cin = None
    if add_to is not None:
        cin = _f32c(add_to).expand(batch, am, n).contiguous() if add_to.dim() == 2 or add_to.shape[0] != batch \
            else _f32c(add_to)
    check(lib().mmx_bmm_f32(_p(a), _p(b), _p(cin), _p(out), batch, am, n, ak, int(trans_a), sa, sb, am * n,
                            int(nan_to_zero), _stream()), "mmx_bmm_f32")
    return out[0] if squeeze else out


def rows_to_dense(vals, rows, n_tokens):
    """``out [B, n_tokens, E]`` = zeros with ``out[b, rows[b]] = vals[b]`` in ONE launch (``mmx_rows_to_dense``); a ``rows[b]`` outside
    ``[0, n_tokens)`` names no row: sample ``b`` is all zero."""
    _dev(vals, rows)
    vals, rows = _f32c(vals), rows.to(torch.long).contiguous()
    if vals.dim() != 2 or rows.numel() != vals.shape[0]:
        raise MMXError("rows_to_dense: vals [B, E] and rows [B] expected, got %s / %s" % (tuple(vals.shape), tuple(rows.shape)))
    B, E = vals.shape
    out = torch.empty(B, n_tokens, E, dtype=torch.float32, device=vals.device)
    check(lib().mmx_rows_to_dense(_p(vals), _p(rows), _p(out), B, n_tokens, E, _stream()), "mmx_rows_to_dense")
    return out


def rows_add_(dense, rows, vals):
    """``dense[b, rows[b]] += vals[b]`` in place (``mmx_rows_add``); ``dense [B, N, E]`` fp32 contiguous.  A ``rows[b]`` outside
    ``[0, N)`` leaves sample ``b`` as it is."""
    _dev(dense, rows, vals)
    if dense.dtype != torch.float32 or not dense.is_contiguous():
        raise MMXError("rows_add_: dense must be fp32 contiguous")
    B, N, E = dense.shape
    if tuple(vals.shape) != (B, E) or rows.numel() != B:
        raise MMXError("rows_add_: dense [B, N, E] needs vals [B, E] and rows [B], got %s / %s / %s"
                       % (tuple(dense.shape), tuple(vals.shape), tuple(rows.shape)))
    check(lib().mmx_rows_add(_p(dense), _p(rows.to(torch.long).contiguous()), _p(_f32c(vals)), B, N, E, _stream()), "mmx_rows_add")
    return dense


def clip_head_fused_enabled():
    """Option ``clip_head_fused`` (default 1): CLIP ``interpret`` / ``interpret_grouped`` take the similarity head's gradients from
    ``clip_head_grads``; 0 restores the autograd head over ``CLIP.logits``."""
    return bool(lib().mmx_clip_head_fused_enabled())


def clip_head_grads(img_feat, txt_feat, logit_scale, img_group=1, want_img=True, want_txt=True, want_diag=False):
    """Gradients of ``sum_b logits_per_image[b, b]`` (CLIP_explainability.ipynb cell 6:6-10; ``CLIP.logits``, CLIP/clip/model.py:369-378)
    with respect to the un-normalised features, in ONE launch (``mmx_clip_head_f32``) -> ``(d_img [B, D], d_txt [B, D], logit_diag [B])``,
    ``None`` where not wanted.  ``img_feat [Bi, D]``: pair b reads row 0 when ``Bi == 1``, else row ``b // img_group``
    (``Bi * img_group == B``); ``txt_feat [B, D]``; ``logit_scale``: the fp32 parameter itself, on the device (its ``exp`` is taken
    in the kernel)."""
    _dev(img_feat, txt_feat, logit_scale)
    for name, t in (("img_feat", img_feat), ("txt_feat", txt_feat)):
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise MMXError("clip_head_grads: %s must be fp32 contiguous [rows, D], got %s %s" % (name, t.dtype, tuple(t.shape)))
    if logit_scale.dtype != torch.float32 or logit_scale.numel() != 1:
        raise MMXError("clip_head_grads: logit_scale must be one fp32 value on the device")
    if img_feat.shape[1] != txt_feat.shape[1]:
        raise MMXError("clip_head_grads: img_feat %s vs txt_feat %s" % (tuple(img_feat.shape), tuple(txt_feat.shape)))
    B, D = txt_feat.shape
    d_img = torch.empty_like(txt_feat) if want_img else None
    d_txt = torch.empty_like(txt_feat) if want_txt else None
    diag = torch.empty(B, dtype=torch.float32, device=txt_feat.device) if want_diag else None
    check(lib().mmx_clip_head_f32(_p(img_feat), _p(txt_feat), _p(logit_scale), _p(d_img), _p(d_txt), _p(diag), B, D,
                                  img_feat.shape[0], int(img_group), _stream()), "mmx_clip_head_f32")
    return d_img, d_txt, diag


_const_rows = {}


def const_rows(batch, row, device):
    """``[batch]`` long tensor holding ``row`` everywhere -- "the same token of every sample" (a ViT's class token) for ``rows_to_dense``
    / ``rows_add_``.  A constant: built once per (device, batch, row) and kept, so no fill launch sits in a step (or in its hipGraph).
    Built and waited for on the stream of the first call, so every later stream may read it; a first call inside a stream capture
    gets a tensor of the capture's own (not kept)."""
    key = (str(device), int(batch), int(row))
    t = _const_rows.get(key)
    if t is None:
        t = torch.full((int(batch),), int(row), dtype=torch.long, device=device)
        if torch.cuda.is_current_stream_capturing():
            return t
        torch.cuda.current_stream().synchronize()
        _const_rows[key] = t
    return t


class LiveRows:
    """Device-side list of the live rows of a ``[B, N, *]`` gradient stream (``live_rows``): ``rows`` int32 ``[B * N]`` (the first
    ``count[0]`` entries are valid), ``count`` int32 ``[1]``; ``eot`` int64 ``[B]``: the last live position of every sample, what the list was
    built from and what the attention takes as its live lengths (``attn_capture_fwd(live=...)``); ``attn``: set by a forward whose
    attention did take them -- its ``qkv`` then holds the listed rows only, and the backward must take them too.  ``poison``: debug switch of the ``*_rows`` wrappers below -- their
    outputs start as NaN instead of uninitialised memory, so a consumer that reads an unlisted row shows up in the results."""
    poison = False

    def __init__(self, rows, count, batch, n_tokens, eot=None):
        self.rows, self.count, self.batch, self.n_tokens = rows, count, batch, n_tokens
        self.cap = batch * n_tokens
        self.eot, self.attn = eot, False

    def _out(self, like, width):
        shape = tuple(like.shape[:-1]) + (width,)
        if LiveRows.poison:
            return torch.full(shape, float("nan"), dtype=torch.float32, device=like.device)
        return torch.empty(shape, dtype=torch.float32, device=like.device)

    def _check(self, what, *tensors):
        for t in tensors:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() // t.shape[-1] != self.cap:
                raise MMXError("%s: fp32 contiguous tensors of %d rows expected, got %s %s" % (what, self.cap, t.dtype, tuple(t.shape)))


def live_rows(eot, n_tokens):
    """``eot [B]`` long -> ``LiveRows`` naming the rows ``b * n_tokens + p``, ``p <= eot[b]``, built on the device (``mmx_live_rows``:
    no read-back; per-call tensors, so a hipGraph capture owns them).  ``None`` when option ``text_live_rows`` is 0."""
    _dev(eot)
    eot = eot.to(torch.long).contiguous()
    B = eot.numel()
    buf = torch.empty(B * n_tokens + 1, dtype=torch.int32, device=eot.device)
    rc = lib().mmx_live_rows(_p(eot), B, n_tokens, _p(buf[1:]), _p(buf[:1]), _stream())
    if rc == _lib.MMX_ENOTSUP:
        return None
    check(rc, "mmx_live_rows")
    return LiveRows(buf[1:], buf[:1], B, n_tokens, eot)


def attn_live_shape(n_tokens, head_dim):
    """Is there a live-length instantiation of the whole-head attention kernels for a self-attention over ``n_tokens`` with this
    ``head_dim`` (``mmx_attn_live_shape``; today 65 ... 80 tokens, head_dim <= 64 and a multiple of 4 -- CLIP's text towers have 77), and is option
    ``text_live_attn`` on?  If not, the row-list route keeps the dense attention over a zero-filled ``qkv``."""
    return lib().mmx_attn_live_shape(n_tokens, n_tokens, head_dim) == 0


def _live_attn_check(what, live, B, Nq, Nk, probs):
    if live.eot is None or live.batch != B or live.n_tokens != Nq or Nq != Nk or probs.dtype != torch.float32:
        raise MMXError("%s: live= needs an fp32 self-attention over the %d x %d rows of the list, got batch %d, Nq %d, Nk %d, %s slab"
                       % (what, live.batch, live.n_tokens, B, Nq, Nk, str(probs.dtype).replace("torch.", "")))


def gemm_rows_eligible(*weights, dtype=torch.float32):
    """The eligibility rule of ``mmx_gemm_rows_f32`` for ``x @ weight``: fp32 contiguous 2-D weights, both widths multiples of 4
    (16-byte rows), 16-byte aligned storage.  ``dtype=torch.float16`` (``mmx_gemm_rows_f16``, which reads a cached fp16 copy of the
    same fp32 parameter): both widths multiples of 8 (16-byte rows of halves)."""
    if dtype not in (torch.float32, torch.float16):
        return False
    m = 4 if dtype == torch.float32 else 8
    return all(w.dtype == torch.float32 and w.dim() == 2 and w.is_contiguous() and w.shape[0] % m == 0 and w.shape[1] % m == 0
               and w.data_ptr() % 16 == 0 for w in weights)


def transposed_half_weight(weight):
    """Cached fp16 copy of ``weight.t().contiguous()`` (beside ``transposed_weight``, until the parameter is modified in place): the
    k-fastest operand ``mmx_gemm_rows_f16`` wants for the backward's ``x @ weight``.  The rounding is ``convert_weights``'
    (CLIP/clip/model.py:381-402); transposing moves the rounded values, it does not change them."""
    return _cached_weight(weight, "t16", lambda: weight.detach().t().to(torch.float16).contiguous())[0]


def gemm_rows(x, weight, live, out=None, dtype=torch.float32):
    """``out[r] = x[r] @ weight`` for the live rows ``r`` (``mmx_gemm_rows_f32``, exact fp32 on the MFMA); every other row of ``out``
    is left alone.  ``x [B, N, K]``, ``weight [K, M]`` (an ``nn.Linear`` weight as stored), ``out [B, N, M]``.
    ``dtype=torch.float16`` (an fp16 body): ``mmx_gemm_rows_f16`` -- ``x`` rounded to fp16 inside the kernel, the cached fp16 copy of
    ``weight.t()``, fp32 accumulation and an fp32 ``out``: the roundings of ``backward_gemm(x, weight, torch.float16)``."""
    _dev(x, weight, out)
    K, M = weight.shape
    if out is None:
        out = live._out(x, M)
    live._check("gemm_rows", x, out)
    if x.shape[-1] != K or out.shape[-1] != M or not gemm_rows_eligible(weight, dtype=dtype):
        raise MMXError("gemm_rows: x %s @ weight %s -> out %s (%s)" % (tuple(x.shape), tuple(weight.shape), tuple(out.shape), dtype))
    if dtype == torch.float16:
        check(lib().mmx_gemm_rows_f16(_p(x), _p(transposed_half_weight(weight)), _p(out), _p(live.rows), _p(live.count), live.cap, M, K,
                                      _stream()), "mmx_gemm_rows_f16")
        return out
    check(lib().mmx_gemm_rows_f32(_p(x), _p(weight), _p(out), _p(live.rows), _p(live.count), live.cap, M, K, _stream()),
          "mmx_gemm_rows_f32")
    return out


def live_rows_forward_enabled():
    """Options ``text_live_rows`` and ``text_live_rows_fwd`` are both on: the forward of a causal tower may take the row list too."""
    return bool(lib().mmx_text_live_rows_fwd_enabled())


def live_rows_half_enabled():
    """Options ``text_live_rows_half`` (default 0), ``text_live_rows`` and ``text_live_rows_fwd`` are all on: the text tower of an fp16
    body may take the row list, its GEMMs on ``mmx_gemm_rows_f16`` / ``mmx_gemm_rows_bias_f16``."""
    return bool(lib().mmx_text_live_rows_half_enabled())


def linear_rows(x, weight, bias, live, out=None, gelu=False, act_out=None, dtype=torch.float32):
    """``out[r] = x[r] @ weight.t() + bias`` for the live rows ``r`` (``mmx_gemm_rows_bias_f32``: a forward ``nn.Linear`` on the tiles of
    ``gemm_rows``, fed with the cached ``transposed_weight``); every other row of ``out`` is left alone.  ``x [B, N, in]``, ``weight
    [out, in]``.  ``gelu``: returns ``(out, act)`` with ``act = QuickGELU(out)`` on the live rows, written by the same kernel -- the bits
    ``quick_gelu_fwd(out)`` has there (``act_out``: the tensor to write it to).  ``dtype=torch.float16`` (an fp16 body):
    ``mmx_gemm_rows_bias_f16`` -- ``x`` rounded to fp16 inside the kernel, the cached fp16 copy ``linear(..., torch.float16)`` uses (no
    transposed copy), fp32 accumulation, fp32 bias and ``out``."""
    _dev(x, weight, bias, out, act_out)
    M, K = weight.shape
    if out is None:
        out = live._out(x, M)
    live._check("linear_rows", x, out)
    if x.shape[-1] != K or out.shape[-1] != M or not gemm_rows_eligible(weight, dtype=dtype) or bias is None or bias.numel() != M:
        raise MMXError("linear_rows: x %s @ weight %s^T + bias -> out %s (%s)"
                       % (tuple(x.shape), tuple(weight.shape), tuple(out.shape), dtype))
    act = (act_out if act_out is not None else live._out(x, M)) if gelu else None
    if act is not None:
        live._check("linear_rows", act)
        if act.shape[-1] != M or act.data_ptr() == out.data_ptr():
            raise MMXError("linear_rows: the activation needs a [.., %d] tensor of its own" % M)
    if dtype == torch.float16:
        check(lib().mmx_gemm_rows_bias_f16(_p(x), _p(_converted(weight, torch.float16).contiguous()), _p(_f32c(bias.detach())), _p(out),
                                           _p(act), _p(live.rows), _p(live.count), live.cap, M, K, _stream()),
              "mmx_gemm_rows_bias_f16")
        return (out, act) if gelu else out
    check(lib().mmx_gemm_rows_bias_f32(_p(x), _p(transposed_weight(weight)), _p(_f32c(bias.detach())), _p(out), _p(act), _p(live.rows),
                                       _p(live.count), live.cap, M, K, _stream()), "mmx_gemm_rows_bias_f32")
    return (out, act) if gelu else out


def add_layernorm_rows(x, y, gamma, beta, eps, live, out=None):
    """``add_layernorm`` on the live rows -> ``(s, h, mean, rstd)`` of the dense shapes; the rows outside the list are not written
    (``y=None``: ``s`` is ``x`` itself).  Listed rows have the bits of the dense kernel.  ``out``: ``(s, h, mean, rstd)`` to write to."""
    _dev(x, y, gamma, beta)
    live._check("add_layernorm_rows", x, *([y] if y is not None else []))
    E = x.shape[-1]
    gamma, beta = _affine("add_layernorm_rows", E, gamma, beta)
    if out is not None:
        s, h, mean, rstd = out
        _dev(s, h, mean, rstd)
        s = s if y is not None else x
        live._check("add_layernorm_rows", h, *([s] if y is not None else []))
        if h.shape[-1] != E or (y is not None and s.shape[-1] != E) or mean.numel() != live.cap or rstd.numel() != live.cap or \
                not (mean.is_contiguous() and rstd.is_contiguous() and mean.dtype == rstd.dtype == torch.float32):
            raise MMXError("add_layernorm_rows: out must be (s, h [.., %d], mean, rstd [%d]) fp32 contiguous" % (E, live.cap))
    else:
        s = live._out(x, E) if y is not None else x
        h = live._out(x, E)
        mean, rstd = live._out(x, 1).view(-1), live._out(x, 1).view(-1)
    check(lib().mmx_add_layernorm_fwd_rows(_p(x), _p(y), _p(gamma), _p(beta), _p(s) if y is not None else _p(None), _p(h),
                                           _p(mean), _p(rstd), _p(live.rows), _p(live.count), live.cap, E, float(eps), _stream()),
          "mmx_add_layernorm_fwd_rows")
    return s, h, mean, rstd


def quick_gelu_bwd_rows(x, dy, live, out=None):
    """``quick_gelu_bwd`` on the live rows (``x`` at the same row as ``dy``); every other row of the result is left alone.  ``out``: an
    fp32 contiguous tensor of ``dy``'s shape to write to."""
    _dev(x, dy, out)
    live._check("quick_gelu_bwd_rows", x, dy)
    dx = out if out is not None else live._out(dy, dy.shape[-1])
    if out is not None:
        live._check("quick_gelu_bwd_rows", out)
        if out.shape != dy.shape:
            raise MMXError("quick_gelu_bwd_rows: dy %s -> out %s" % (tuple(dy.shape), tuple(out.shape)))
    check(lib().mmx_quick_gelu_bwd_rows(_p(x), _p(dy), _p(dx), _p(live.rows), _p(live.count), live.cap, dy.shape[-1], _stream()),
          "mmx_quick_gelu_bwd_rows")
    return dx


def layernorm_bwd_add_rows(dy, x, mean, rstd, gamma, d_res, live, out=None):
    """``layernorm_bwd_add`` on the live rows (per-row ``x`` / ``mean`` / ``rstd``); every other row of the result is left alone.
    ``out``: an fp32 contiguous tensor of ``dy``'s shape to write to."""
    _dev(dy, x, mean, rstd, gamma, d_res, out)
    live._check("layernorm_bwd_add_rows", dy, x, *([d_res] if d_res is not None else []))
    _bwd_rows("layernorm_bwd_add_rows", dy, x, d_res)
    mean, rstd = _row_stats("layernorm_bwd_add_rows", live.cap, mean, rstd)
    (gamma,) = _affine("layernorm_bwd_add_rows", dy.shape[-1], gamma)
    dx = out if out is not None else live._out(dy, dy.shape[-1])
    if out is not None:
        live._check("layernorm_bwd_add_rows", out)
        if out.shape != dy.shape:
            raise MMXError("layernorm_bwd_add_rows: dy %s -> out %s" % (tuple(dy.shape), tuple(out.shape)))
    check(lib().mmx_layernorm_bwd_add_rows(_p(dy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(d_res), _p(dx), _p(live.rows),
                                           _p(live.count), live.cap, dy.shape[-1], _stream()), "mmx_layernorm_bwd_add_rows")
    return dx


def small_linear(x, lin):
    """``lin(x)`` for an ``nn.Linear`` applied to a FEW rows (a shared forward's 100 decoder queries) with a SQUARE weight of at
    most 256: the one shape family where the library's heuristic leaves the chip idle (a 256-row tile for 100 rows: 3
    workgroups, 30 us; ``mmx_linear_f32``: 9 us).  Anything else goes to ``lin`` itself -- also an ``x`` that carries an
    autograd graph (the kernel records none: this is an op of the tape passes, which differentiate by hand)."""
    rows = x.numel() // x.shape[-1]
    if not (x.is_cuda and x.dtype == torch.float32 and rows <= 128 and lin.in_features == lin.out_features <= 256) or \
            (torch.is_grad_enabled() and x.requires_grad):
        return lin(x)
    x2 = _f32c(x).view(rows, lin.in_features)
    out = torch.empty(rows, lin.out_features, dtype=torch.float32, device=x.device)
    check(lib().mmx_linear_f32(_p(x2), _p(transposed_weight(lin.weight)), _p(lin.bias.detach() if lin.bias is not None else None),
                               _p(out), rows, lin.out_features, lin.in_features, _stream()), "mmx_linear_f32")
    return out.view(*x.shape[:-1], lin.out_features)


def chain_matvec(A, y, base=None):
    """``base + A @ y`` for ``A [B, N, N]``, ``y`` / ``base [B, N]`` (fp32; ``base`` defaults to ``y``): one column of
    the chain ``R <- R + A R``."""
    _dev(A, y, base)
    A, y = _f32c(A), _f32c(y)
    base = y if base is None else _f32c(base)
    B, N = y.shape
    out = torch.empty_like(y)
    check(lib().mmx_chain_matvec(_p(A), _p(y), _p(base), _p(out), B, N, _stream()), "mmx_chain_matvec")
    return out


def chain_vecmat(x, A, base=None):
    """``base + x @ A`` for ``x`` / ``base [B, N]``, ``A [B, N, N]`` (fp32; ``base`` defaults to ``x``): one row of the
    chain carried top-down."""
    _dev(A, x, base)
    A, x = _f32c(A), _f32c(x)
    base = x if base is None else _f32c(base)
    B, N = x.shape
    out = torch.empty_like(x)
    need = lib().mmx_chain_vecmat_workspace_bytes(B, N)
    ws = _workspace(need, x.device, "vecmat")
    check(lib().mmx_chain_vecmat(_p(A), _p(x), _p(base), _p(out), B, N, _p(ws), need, _stream()), "mmx_chain_vecmat")
    return out


def avg_heads_vecmat(x, cam, grad, batch_size=1, shared_attn=False, base=None):
    """``base + x @ mean_h(clamp(grad * cam, 0))`` for ``x`` / ``base [B, N]`` fp32 (``base`` defaults to ``x``) and square slabs
    ``[B * H, N, N]``: ``chain_vecmat(x, avg_heads(cam, grad))`` without the ``[B, N, N]`` intermediate, two launches instead of
    three (``mmx_avg_heads_vecmat``).  ``shared_attn`` as in ``avg_heads``."""
    _dev(cam, grad, x, base)
    cam, grad, x = _capture(cam), _capture(grad), _f32c(x)
    base = x if base is None else _f32c(base)
    B, N = x.shape
    bh = grad.numel() // (N * N)
    ok = cam.numel() * batch_size == grad.numel() if shared_attn else cam.shape == grad.shape
    if not ok or B != batch_size or bh % B or tuple(grad.shape[-2:]) != (N, N) or cam.dtype != grad.dtype:
        raise MMXError("avg_heads_vecmat: x %s, cam %s/%s, grad %s/%s, batch %d" % (tuple(x.shape), tuple(cam.shape), cam.dtype,
                                                                                     tuple(grad.shape), grad.dtype, batch_size))
    out = torch.empty_like(x)
    need = lib().mmx_avg_heads_vecmat_workspace_bytes(B, N)
    ws = _workspace(need, x.device, "ahv")
    check(lib().mmx_avg_heads_vecmat(_p(cam), _p(grad), _p(x), _p(base), _p(out), B, bh // B, N, _DTYPES[cam.dtype],
                                     0 if shared_attn else -1, _p(ws), need, _stream()), "mmx_avg_heads_vecmat")
    return out


# ------------------------------------------------------------------------------------------- eq. 8-9
def handle_residual(R, check_diag=True):
    """Eq. 8-9 on ``[.., N, N]``.  ``check_diag``: ``True`` asserts ``min diag(R - I) >= 0`` now, like the reference's
    assert (one device->host read); ``False`` skips the check; ``"defer"`` returns ``(out, diag_min)`` with the device
    word, so that a caller can check many calls with ONE read (or none, inside a hipGraph)."""
    _dev(R)
    R = _f32c(R)
    n = R.shape[-1]
    batch = R.numel() // (n * n)
    out = torch.empty_like(R)
    dmin = torch.empty(1, dtype=torch.float32, device=R.device) if check_diag else None
    check(lib().mmx_handle_residual(_p(R), _p(out), batch, n, _p(dmin), _stream()), "mmx_handle_residual")
    if check_diag == "defer":
        return out, dmin
    if check_diag:
        assert dmin.item() >= 0  # same contract as the reference's assert (it also syncs)
    return out


# ------------------------------------------------------------------------------------------- rules 10/11
def mm_attention_rules(R_ss, R_qq, cam_sq, R_qs=None, apply_normalization=True, apply_self_in_rule_10=True,
                       nan_to_zero=False, check_diag=True):
    """Returns ``R_sq_addition`` (and ``R_ss_addition`` when ``R_qs`` is given)."""
    _dev(R_ss, R_qq, cam_sq, R_qs)
    R_ss, R_qq, cam_sq = _f32c(R_ss), _f32c(R_qq), _f32c(cam_sq)
    ns, nq = cam_sq.shape[-2], cam_sq.shape[-1]
    if R_ss.shape[-1] != ns or R_qq.shape[-1] != nq:
        raise MMXError("mm_attention_rules: R_ss %s, R_qq %s, cam_sq %s" % (tuple(R_ss.shape), tuple(R_qq.shape), tuple(cam_sq.shape)))
    flags = (_lib.MM_NORMALIZE if apply_normalization else 0) | (_lib.MM_SELF_IN_RULE10 if apply_self_in_rule_10 else 0) \
        | (_lib.MM_NAN_TO_ZERO if nan_to_zero else 0)
    sq_add = torch.empty(ns, nq, dtype=torch.float32, device=cam_sq.device)
    ss_add = None
    if R_qs is not None:
        R_qs = _f32c(R_qs)
        ss_add = torch.empty(ns, ns, dtype=torch.float32, device=cam_sq.device)
    want_diag = check_diag and apply_normalization      # the reference asserts in handle_residual even when the
    dmin = torch.empty(1, dtype=torch.float32, device=cam_sq.device) if want_diag else None   # self terms are unused
    need = lib().mmx_mm_rules_workspace_bytes(ns, nq)
    ws = _workspace(need, cam_sq.device)
    check(lib().mmx_mm_attention_rules(_p(R_ss), _p(R_qq), _p(R_qs), _p(cam_sq), _p(sq_add), _p(ss_add), ns, nq,
                                       flags, _p(dmin), _p(ws), need, _stream()), "mmx_mm_attention_rules")
    if want_diag:
        assert dmin.item() >= 0
    return (sq_add, ss_add) if R_qs is not None else sq_add


LXMERT_FUSED_MAX_TOKENS = 48


def lxmert_schedule(lang, vis, x_lang_cross, x_img_cross, x_lang_self, x_img_self, apply_normalization=True,
                    apply_self_in_rule_10=True, check_diag=True, text_len=None):
    """The whole LXMERT rule schedule in one launch.  Every argument is a list of ``(attn, grad)`` pairs of fp32
    ``[B, H, Nq, Nk]`` tensors (``x_img_*`` may omit the last cross layer).  Returns ``(R_tt, R_ti, R_ii, R_it)``
    with a leading batch dim.

    ``text_len`` (``[B]`` int tensor, optional): the batch is padded to ``T`` question tokens and sample ``b`` has
    ``text_len[b]`` real ones; its rules run on that leading block, the rest of its outputs is zero.
    ``check_diag``: ``True`` asserts the reference's ``handle_residual`` contract right away (one device->host read, like
    the reference's own assert); ``"defer"`` returns the device word as a fifth value instead -- nothing synchronises,
    the call can be captured into a hipGraph, and the caller asserts ``diag_min >= 0`` when it reads the results."""
    groups = [lang, vis, x_lang_cross, x_img_cross, x_lang_self, x_img_self]
    flat = [t for grp in groups for pair in grp for t in pair]
    _dev(*flat)
    if any(t.dtype != torch.float32 for t in flat):
        raise MMXError("lxmert_schedule: fp32 capture slabs only")
    keep = [[(a.contiguous(), g.contiguous()) for a, g in grp] for grp in groups]
    a0 = keep[2][0][0]                                     # [B, H, T, I]
    B, H, T, I = a0.shape
    n_x = len(keep[2])
    if len(keep[4]) != n_x or len(keep[3]) < n_x - 1 or len(keep[5]) < n_x - 1:
        raise MMXError("lxmert_schedule: inconsistent cross-layer lists")
    dev = a0.device
    R_tt = torch.empty(B, T, T, dtype=torch.float32, device=dev)
    R_ti = torch.empty(B, T, I, dtype=torch.float32, device=dev)
    R_ii = torch.empty(B, I, I, dtype=torch.float32, device=dev)
    R_it = torch.empty(B, I, T, dtype=torch.float32, device=dev)
    want_diag = bool(check_diag) and apply_normalization and apply_self_in_rule_10
    dmin = torch.empty(1, dtype=torch.float32, device=dev) if want_diag else None
    if text_len is not None:
        _dev(text_len)
        text_len = text_len.to(dtype=torch.int32).contiguous()
        if text_len.numel() != B:
            raise MMXError("lxmert_schedule: text_len needs one entry per sample")
    tables, alive = [], []
    for grp in keep:
        for which in (0, 1):
            tbl, arr = _lib.ptr_table([pair[which].data_ptr() for pair in grp])
            tables.append(tbl)
            alive.append(arr)
    flags = (_lib.MM_NORMALIZE if apply_normalization else 0) | (_lib.MM_SELF_IN_RULE10 if apply_self_in_rule_10 else 0)
    la, lg, va, vg, xlca, xlcg, xica, xicg, xlsa, xlsg, xisa, xisg = tables
    # two phases in one launch: chip-wide head averages, the last arriver of a sample runs the rules on the MFMA
    need = lib().mmx_lxmert_schedule_workspace_bytes(len(keep[0]), len(keep[1]), n_x, B, T, I)
    ws = _workspace(need, dev, tag="lxmert_schedule")
    check(lib().mmx_lxmert_schedule(la, lg, len(keep[0]), va, vg, len(keep[1]), xlca, xlcg, xica, xicg, xlsa, xlsg,
                                    xisa, xisg, n_x, B, H, T, I, flags, _p(text_len), _p(R_tt), _p(R_ti), _p(R_ii),
                                    _p(R_it), _p(dmin), _p(ws), need, _stream()), "mmx_lxmert_schedule")
    if check_diag == "defer":
        return R_tt, R_ti, R_ii, R_it, dmin
    if want_diag:
        assert dmin.item() >= 0   # the reference's handle_residual assert
    return R_tt, R_ti, R_ii, R_it


# ------------------------------------------------------------------------------------------- bi-modal baselines, padded batches
def _lengths(what, lens, B):
    """A per-sample length array for the C-ABI: ``None`` or a device ``int32 [B]`` tensor (clamped to the extent by the kernel)."""
    if lens is None:
        return None
    _dev(lens)
    lens = lens.to(dtype=torch.int32).contiguous()
    if lens.numel() != B:
        raise MMXError("%s: a length array needs one entry per sample (%d), got %d" % (what, B, lens.numel()))
    return lens


def _slab(what, t):
    _dev(t)
    if t.dtype != torch.float32 or t.dim() != 4:
        raise MMXError("%s: fp32 [B, H, Nq, Nk] capture slabs only, got %s %s" % (what, t.dtype, tuple(t.shape)))
    return t.contiguous()


def _head_mean_live(what, attn, grad, q_len, k_len, zero_cls):
    attn = _slab(what, attn)
    B, H, Nq, Nk = attn.shape
    if grad is not None:
        grad = _slab(what, grad)
        if grad.shape != attn.shape:
            raise MMXError("%s: gradient slab %s does not match %s" % (what, tuple(grad.shape), tuple(attn.shape)))
    q_len, k_len = _lengths(what, q_len, B), _lengths(what, k_len, B)
    out = torch.empty(B, Nq, Nk, dtype=torch.float32, device=attn.device)
    check(lib().mmx_head_mean_live(_p(attn), _p(grad), _p(out), B, H, Nq, Nk, _p(q_len), _p(k_len),
                                   _lib.HEAD_MEAN_ZERO_CLS if zero_cls else 0, _stream()), "mmx_head_mean_live")
    return out


def head_mean_live(attn, q_len=None, k_len=None, zero_cls=False):
    """``mean_h attn[b, h]`` on sample b's leading ``q_len[b] x k_len[b]`` block of a padded ``[B, H, Nq, Nk]`` fp32 slab, exact
    zeros outside it -> ``[B, Nq, Nk]``.  Lengths: device int tensors ``[B]`` or ``None`` (the full extent); ``zero_cls``:
    ``out[b, 0, 0] = 0``.  One launch, nothing synchronises."""
    return _head_mean_live("head_mean_live", attn, None, q_len, k_len, zero_cls)


def attn_gradcam_live(attn, grad, q_len=None, k_len=None, zero_cls=False):
    """GradCAM of a padded batch: ``clamp(mean_h(attn[b, h] * w[b, h]), 0)`` with ``w[b, h]`` the mean of ``grad[b, h]`` over sample
    b's LIVE block only (a padded batch's gradient is not zero at padded key columns).  Arguments as ``head_mean_live``."""
    return _head_mean_live("attn_gradcam_live", attn, grad, q_len, k_len, zero_cls)


def lxmert_rollout(text_attn, img_attn, cross_attn, text_len=None):
    """Rollout of a padded LXMERT batch in two launches.  ``text_attn``: the fp32 ``[B, H, T, T]`` slabs of the language layers, then
    every x-layer's language self-attention (the last x-layer's LAST); ``img_attn``: ``[B, H, I, I]`` slabs of ``r_layers``, then the
    image self-attention of every x-layer but the last; ``cross_attn``: the last x-layer's ``[B, H, T, I]`` slab; ``text_len``: device
    int ``[B]`` or ``None``.  Returns ``(R_tt [B, T, T], R_ti [B, T, I], R_ii [B, I, I])``."""
    what = "lxmert_rollout"
    text = [_slab(what, t) for t in text_attn]
    img = [_slab(what, t) for t in img_attn]
    cross = _slab(what, cross_attn)
    B, H, T, I = cross.shape
    if any(t.shape != (B, H, T, T) for t in text) or any(t.shape != (B, H, I, I) for t in img):
        raise MMXError("lxmert_rollout: the tables do not match the cross slab %s" % (tuple(cross.shape),))
    text_len = _lengths(what, text_len, B)
    dev = cross.device
    R_tt = torch.empty(B, T, T, dtype=torch.float32, device=dev)
    R_ti = torch.empty(B, T, I, dtype=torch.float32, device=dev)
    R_ii = torch.empty(B, I, I, dtype=torch.float32, device=dev)
    tt, _k0 = _lib.ptr_table([t.data_ptr() for t in text])
    ti, _k1 = _lib.ptr_table([t.data_ptr() for t in img])
    need = lib().mmx_lxmert_rollout_workspace_bytes(len(text), len(img), B, T, I)
    if need == 0:
        raise MMXError("lxmert_rollout: needs 2..%d text slabs, 1..%d image slabs and T, I <= %d (got %d, %d, T=%d, I=%d)"
                       % (_lib.BASELINES_MAX_TABLE, _lib.BASELINES_MAX_TABLE, LXMERT_FUSED_MAX_TOKENS, len(text), len(img), T, I))
    ws = _workspace(need, dev, tag="lxmert_rollout")        # grow-only scratch: pinned_state keeps it alive for graphs
    check(lib().mmx_lxmert_rollout(tt, len(text), ti, len(img), _p(cross), B, H, T, I, _p(text_len), _p(R_tt), _p(R_ti),
                                   _p(R_ii), _p(ws), need, _stream()), "mmx_lxmert_rollout")
    return R_tt, R_ti, R_ii


def head_minmax_live(cam, q_len=None, k_len=None, zero_cls=False):
    """The per-map step of partial LRP on a padded batch: ``m = mean_h cam[b, h]`` on sample b's leading ``q_len[b] x k_len[b]`` block
    of a ``[B, H, Nq, Nk]`` fp32 slab, ``(m - min m) / (max m - min m)`` with the extremes over that block, exact zeros outside it
    -> ``[B, Nq, Nk]``.  ``max == min`` gives NaN over the block and a NaN in the block spreads over it, as in the reference's
    expression; ``zero_cls`` writes ``out[b, 0, 0] = 0`` afterwards.  Arguments as ``head_mean_live``; one launch."""
    what = "head_minmax_live"
    cam = _slab(what, cam)
    B, H, Nq, Nk = cam.shape
    q_len, k_len = _lengths(what, q_len, B), _lengths(what, k_len, B)
    out = torch.empty(B, Nq, Nk, dtype=torch.float32, device=cam.device)
    check(lib().mmx_head_minmax_live(_p(cam), _p(out), B, H, Nq, Nk, _p(q_len), _p(k_len),
                                     _lib.HEAD_MEAN_ZERO_CLS if zero_cls else 0, _stream()), "mmx_head_minmax_live")
    return out


def lxmert_transformer_attr(text_pairs, img_pairs, cross_pair, text_len=None):
    """Transformer attribution of a padded LXMERT batch in two launches.  ``text_pairs``: ``(cam, grad)`` pairs of fp32
    ``[B, H, T, T]`` slabs, the language layers, then every x-layer's language self-attention; ``img_pairs``: ``[B, H, I, I]`` pairs of
    ``r_layers``, then the image self-attention of every x-layer but the last; ``cross_pair``: the last x-layer's ``[B, H, T, I]``
    pair; ``text_len``: device int ``[B]`` or ``None``.  Returns ``(R_tt [B, T, T], R_ti [B, T, I], R_ii [B, I, I])``."""
    what = "lxmert_transformer_attr"
    text = [(_slab(what, c), _slab(what, g)) for c, g in text_pairs]
    img = [(_slab(what, c), _slab(what, g)) for c, g in img_pairs]
    cross_c, cross_g = _slab(what, cross_pair[0]), _slab(what, cross_pair[1])
    B, H, T, I = cross_c.shape
    if cross_g.shape != cross_c.shape or any(t.shape != (B, H, T, T) for pair in text for t in pair) or \
            any(t.shape != (B, H, I, I) for pair in img for t in pair):
        raise MMXError("lxmert_transformer_attr: the tables do not match the cross slab %s" % (tuple(cross_c.shape),))
    text_len = _lengths(what, text_len, B)
    dev = cross_c.device
    R_tt = torch.empty(B, T, T, dtype=torch.float32, device=dev)
    R_ti = torch.empty(B, T, I, dtype=torch.float32, device=dev)
    R_ii = torch.empty(B, I, I, dtype=torch.float32, device=dev)
    tc, _k0 = _lib.ptr_table([c.data_ptr() for c, _ in text])
    tg, _k1 = _lib.ptr_table([g.data_ptr() for _, g in text])
    ic, _k2 = _lib.ptr_table([c.data_ptr() for c, _ in img])
    ig, _k3 = _lib.ptr_table([g.data_ptr() for _, g in img])
    need = lib().mmx_lxmert_attr_workspace_bytes(len(text), len(img), B, T, I)
    if need == 0:
        raise MMXError("lxmert_transformer_attr: needs 1..%d text pairs, 1..%d image pairs and T, I <= %d (got %d, %d, T=%d, I=%d)"
                       % (_lib.BASELINES_MAX_TABLE, _lib.BASELINES_MAX_TABLE, LXMERT_FUSED_MAX_TOKENS, len(text), len(img), T, I))
    ws = _workspace(need, dev, tag="lxmert_attr")
    check(lib().mmx_lxmert_attr(tc, tg, len(text), ic, ig, len(img), _p(cross_c), _p(cross_g), B, H, T, I, _p(text_len), _p(R_tt),
                                _p(R_ti), _p(R_ii), _p(ws), need, _stream()), "mmx_lxmert_attr")
    return R_tt, R_ti, R_ii


# ------------------------------------------------------------------------------------------- single-stream baselines, padded batches
SELFATTN_MAX_TOKENS = _lib.SELFATTN_MAX_TOKENS       # T + V of mmx_selfattn_row_live / mmx_selfattn_rollout_row


def _selfattn_shape(what, attn, n_text):
    """``(B, H, T, V)`` of a ``[B, H, N, N]`` slab whose sequence is ``n_text`` padded text positions followed by regions."""
    B, H, N, Nk = attn.shape
    if n_text is None:
        raise MMXError("%s: n_text (the padded text width T; V = N - T) is required" % what)
    T = int(n_text)
    if N != Nk or T < 2 or N - T < 1 or N > _lib.SELFATTN_MAX_TOKENS:
        raise MMXError("%s: needs square slabs with T >= 2, V = N - T >= 1 and N <= %d (got %s, n_text=%d)"
                       % (what, _lib.SELFATTN_MAX_TOKENS, tuple(attn.shape), T))
    return B, H, T, N - T


def _selfattn_row(what, attn, grad, text_len, vis_len, n_text):
    attn = _slab(what, attn)
    B, H, T, V = _selfattn_shape(what, attn, n_text)
    ws, need = None, 0
    if grad is not None:
        grad = _slab(what, grad)
        if grad.shape != attn.shape:
            raise MMXError("%s: gradient slab %s does not match %s" % (what, tuple(grad.shape), tuple(attn.shape)))
        need = lib().mmx_selfattn_row_live_workspace_bytes(B, H, T, V)
        ws = _workspace(need, attn.device, tag="selfattn_row")       # grow-only scratch: pinned_state keeps it alive for graphs
    text_len, vis_len = _lengths(what, text_len, B), _lengths(what, vis_len, B)
    out = torch.empty(B, T + V, dtype=torch.float32, device=attn.device)
    check(lib().mmx_selfattn_row_live(_p(attn), _p(grad), _p(out), B, H, T, V, _p(text_len), _p(vis_len), _p(ws), need, _stream()),
          "mmx_selfattn_row_live")
    return out


def selfattn_raw_row(attn, text_len=None, vis_len=None, n_text=None):
    """Raw attention of a padded single-stream batch: row ``c_b = text_len[b] - 2`` of ``mean_h attn[b, h]`` on sample b's live
    positions ``[0, text_len[b]) u [T, T + vis_len[b])`` of a ``[B, H, N, N]`` fp32 slab, ``T = n_text`` (the padded text width),
    exact zeros elsewhere and at ``c_b`` -> ``[B, N]``.  Lengths: device int tensors ``[B]`` or ``None`` (the full extent).  One
    launch, nothing synchronises."""
    return _selfattn_row("selfattn_raw_row", attn, None, text_len, vis_len, n_text)


def selfattn_gradcam_row(attn, grad, text_len=None, vis_len=None, n_text=None):
    """Attention GradCAM of a padded single-stream batch, min-max normalised over sample b's LIVE block only (the gradient of a padded
    batch is not zero at padded keys), row ``c_b`` -> ``[B, N]``.  Arguments as ``selfattn_raw_row``; three launches."""
    return _selfattn_row("selfattn_gradcam_row", attn, grad, text_len, vis_len, n_text)


def selfattn_rollout_row(attn_layers, text_len=None, vis_len=None, n_text=None):
    """Row ``c_b`` of the un-normalised rollout ``(I + A_{L-1}) ... (I + A_0)`` of a padded single-stream batch, ``A_l`` the head mean
    of ``attn_layers[l]`` (fp32 ``[B, H, N, N]`` slabs, already sliced to ``start_layer:``) -> ``[B, N]``.  Two launches."""
    what = "selfattn_rollout_row"
    layers = [_slab(what, t) for t in attn_layers]
    if not layers or any(t.shape != layers[0].shape for t in layers):
        raise MMXError("%s: needs 1..%d slabs of one shape" % (what, _lib.BASELINES_MAX_TABLE))
    B, H, T, V = _selfattn_shape(what, layers[0], n_text)
    text_len, vis_len = _lengths(what, text_len, B), _lengths(what, vis_len, B)
    need = lib().mmx_selfattn_rollout_row_workspace_bytes(len(layers), B, T, V)
    if need == 0:
        raise MMXError("%s: needs 1..%d slabs (got %d)" % (what, _lib.BASELINES_MAX_TABLE, len(layers)))
    dev = layers[0].device
    out = torch.empty(B, T + V, dtype=torch.float32, device=dev)
    tbl, _k = _lib.ptr_table([t.data_ptr() for t in layers])
    ws = _workspace(need, dev, tag="selfattn_rollout")               # grow-only scratch: pinned_state keeps it alive for graphs
    check(lib().mmx_selfattn_rollout_row(tbl, len(layers), B, H, T, V, _p(text_len), _p(vis_len), _p(out), _p(ws), need, _stream()),
          "mmx_selfattn_rollout_row")
    return out


def selfattn_ours_row(attn_layers, grad_layers, text_len=None, vis_len=None, n_text=None):
    """``generate_ours`` (reference :68-107) of a padded single-stream batch: row ``c_b`` of ``(I + A_{L-1}) ... (I + A_0)`` with
    ``A_l = mean_h clamp(grad_layers[l] * attn_layers[l], min=0)`` (the clamp per head, before the mean) on sample b's live set, exact
    zeros elsewhere and at ``c_b`` -> ``[B, T + V]``.  Both tables: fp32 ``[B, H, N, N]`` slabs of one shape, entry ``l`` of both from
    one layer; the gradient's padding may hold anything.  Any cam slab may stand in for ``attn``: the rows of
    ``generate_transformer_att`` (reference :42-56) are the same arithmetic on the LRP cams.  Lengths and ``n_text`` as
    ``selfattn_raw_row``.  Two launches, nothing synchronises."""
    what = "selfattn_ours_row"
    layers = [_slab(what, t) for t in attn_layers]
    grads = [_slab(what, t) for t in grad_layers]
    if not layers or len(layers) != len(grads):
        raise MMXError("%s: needs 1..%d probability slabs and as many gradient slabs (got %d and %d)"
                       % (what, _lib.BASELINES_MAX_TABLE, len(layers), len(grads)))
    if any(t.shape != layers[0].shape for t in layers + grads):
        raise MMXError("%s: every slab of both tables must have the shape %s" % (what, tuple(layers[0].shape)))
    B, H, T, V = _selfattn_shape(what, layers[0], n_text)
    text_len, vis_len = _lengths(what, text_len, B), _lengths(what, vis_len, B)
    need = lib().mmx_selfattn_ours_row_workspace_bytes(len(layers), B, T, V)
    if need == 0:
        raise MMXError("%s: needs 1..%d slabs per table (got %d)" % (what, _lib.BASELINES_MAX_TABLE, len(layers)))
    dev = layers[0].device
    out = torch.empty(B, T + V, dtype=torch.float32, device=dev)
    at, _k0 = _lib.ptr_table([t.data_ptr() for t in layers])
    gt, _k1 = _lib.ptr_table([t.data_ptr() for t in grads])
    ws = _workspace(need, dev, tag="selfattn_ours")                  # grow-only scratch: pinned_state keeps it alive for graphs
    check(lib().mmx_selfattn_ours_row(at, gt, len(layers), B, H, T, V, _p(text_len), _p(vis_len), _p(out), _p(ws), need, _stream()),
          "mmx_selfattn_ours_row")
    return out


# ------------------------------------------------------------------------------------------- rollout
def rollout_chain(layers, normalize):
    """``layers``: list of ``[B, N, N]`` (or ``[N, N]``) fp32 maps, already sliced to ``start_layer:``."""
    _dev(*layers)
    mats = [_f32c(m) for m in layers]
    n = mats[0].shape[-1]
    batch = mats[0].numel() // (n * n)
    out = torch.empty(batch, n, n, dtype=torch.float32, device=mats[0].device)
    need = lib().mmx_rollout_workspace_bytes(batch, n)
    ws = _workspace(need, mats[0].device)
    tbl, _k = _lib.ptr_table([m.data_ptr() for m in mats])
    check(lib().mmx_rollout_chain(tbl, len(mats), batch, n, int(normalize), _p(out), _p(ws), need, _stream()),
          "mmx_rollout_chain")
    return out


# ------------------------------------------------------------------------------------------- attention capture
def _bhnd_strides(t, layout):
    """Element strides (batch, head, token) of a ``[B, N, H, D]``-viewable tensor with contiguous D; ``(0, 0, 0)`` for ``None``."""
    if t is None:
        return 0, 0, 0
    s = t.stride()                                   # one walk per operand: these run on every eager call
    if s[-1] != 1:
        raise MMXError("attention operands need a contiguous head_dim")
    if layout == "bnhd":
        return s[0], s[2], s[1]
    if layout == "bhnd":
        return s[0], s[1], s[2]
    raise MMXError("layout %r" % layout)


def _attn_dims(q, k, layout):
    """``(B, H, Nq, Nk, D)`` of the operands ``q`` and ``k`` in ``layout``."""
    if layout == "bnhd":
        B, Nq, H, D = q.shape
        return B, H, Nq, k.shape[1], D
    if layout == "bhnd":
        B, H, Nq, D = q.shape
        return B, H, Nq, k.shape[2], D
    raise MMXError("layout %r" % layout)


def _strided(t, layout):
    """``(pointer, batch stride, head stride, token stride)`` of an optional operand: a null pointer and zeros for ``None``."""
    return (_p(t), *_bhnd_strides(t, layout))


def _qkv_args(q, k, v, layout):
    """The prefix of every attention entry: the three pointers, then the three stride triples (of ``None`` s: nulls and zeros)."""
    return (_p(q), _p(k), _p(v), *_bhnd_strides(q, layout), *_bhnd_strides(k, layout), *_bhnd_strides(v, layout))


def _attn_bwd_args(layout, qkv, probs, probs_sb, slab_dtype, d_o, o, dprobs, grads, dims, scale, scale_mode, need_dqkv):
    """The operand block every backward entry starts with, up to ``need_dqkv``: ``qkv`` / ``grads`` are ``(q, k, v)`` / ``(dq, dk,
    dv)`` (``None`` s without ``need_dqkv``), ``dims`` is ``(B, H, Nq, Nk, D)``; ``o=False``: the entry takes no forward output."""
    return (*_qkv_args(*qkv, layout), _p(probs), probs_sb, slab_dtype, _p(d_o), *_bhnd_strides(d_o, layout),
            *(() if o is False else _strided(o, layout)), _p(dprobs), *_qkv_args(*grads, layout), *dims, float(scale), scale_mode,
            int(need_dqkv))


def _mask_strides(mask, Nk):
    """``(mask fp32 contiguous, batch stride, query stride)`` of an additive ``[Nq, Nk]`` or ``[B, Nq | 1, Nk]`` mask."""
    if mask is None:
        return None, 0, 0
    mask = _f32c(mask)
    if mask.dim() == 2:          # [Nq, Nk]
        return mask, 0, Nk
    if mask.dim() == 3:          # [B, Nq or 1, Nk]
        return mask, (mask.shape[1] * Nk if mask.shape[0] > 1 else 0), (Nk if mask.shape[1] > 1 else 0)
    raise MMXError("mask must be [Nq,Nk] or [B,Nq|1,Nk]")


def attn_capture_fwd(q, k, v, probs_out, scale, scale_mode=_lib.SCALE_Q_FIRST, mask=None, layout="bnhd", mma_bf16=False, live=None,
                     out=None):
    """``q``: ``[B, Nq, H, D]`` view (``layout='bnhd'``) or ``[B, H, Nq, D]``; writes P into ``probs_out``
    (``[B, H, Nq, Nk]`` fp32 contiguous, caller-owned slab) and returns O in the same layout as q.
    ``mma_bf16``: products on the bf16 matrix cores (``MMX_ATTN_MMA_BF16``: operands rounded to bf16, fp32 accumulate
    and softmax; long-sequence streaming kernels only).
    ``live`` (a ``LiveRows`` over the ``B x N`` rows; CAUSAL ``mask``, ``attn_live_shape``): ``mmx_attn_capture_fwd_live`` -- the rows
    past ``live.eot[b]`` of q / k / v are not read and those of O are not written; the live rows of P and O get the bits of the dense
    call on a q / k / v with zeros in the dead rows, and so do the dead rows of P (the softmax of zero scores under the mask).
    ``out``: a caller-owned fp32 tensor of q's shape (contiguous head_dim) to write O into."""
    _dev(q, k, v, probs_out, mask, out)
    if q.dtype != torch.float32 or k.dtype != torch.float32 or v.dtype != torch.float32:
        raise MMXError("attention capture op is fp32 in this ABI version")
    B, H, Nq, Nk, D = _attn_dims(q, k, layout)
    if probs_out.dtype not in _DTYPES or not probs_out.is_contiguous() or probs_out.numel() != B * H * Nq * Nk:
        raise MMXError("probs_out must be a contiguous fp32 / fp16 / bf16 [B,H,Nq,Nk] slab")
    if out is not None and (out.dtype != torch.float32 or out.shape != q.shape):
        raise MMXError("attn_capture_fwd: out must be fp32 of q's shape %s" % (tuple(q.shape),))
    mask, msb, msq = _mask_strides(mask, Nk)
    if live is not None:
        _live_attn_check("attn_capture_fwd", live, B, Nq, Nk, probs_out)
        if mask is None or mma_bf16:
            raise MMXError("attn_capture_fwd: live= stands on a causal mask and the exact-fp32 kernels")
        o = out if out is not None else live._out(q, D)
        check(lib().mmx_attn_capture_fwd_live(*_qkv_args(q, k, v, layout), _p(mask), msb, msq, _p(probs_out), _DTYPES[probs_out.dtype],
                                              *_strided(o, layout), B, H, Nq, Nk, D, float(scale), scale_mode,
                                              _p(live.eot), _stream()), "mmx_attn_capture_fwd_live")
        return o
    o = out if out is not None else torch.empty(q.shape, dtype=torch.float32, device=q.device)
    check(lib().mmx_attn_capture_fwd_ex(*_qkv_args(q, k, v, layout), _p(mask), msb, msq, _p(probs_out),
                                        _DTYPES[probs_out.dtype] | (_lib.MMX_ATTN_MMA_BF16 if mma_bf16 else 0),
                                        *_strided(o, layout), B, H, Nq, Nk, D, float(scale), scale_mode, _stream()),
          "mmx_attn_capture_fwd")
    return o


def attn_fwd(q, k, v, scale, scale_mode=_lib.SCALE_Q_FIRST, mask=None, layout="bnhd", out=None, live=None):
    """Attention forward WITHOUT a capture slab (``mmx_attn_fwd``): operands, mask and scale modes as ``attn_capture_fwd``;
    returns O in the layout of q.  Exact fp32.  Up to 128 keys it is the capture forward's whole-head kernel with the P store
    compiled out (O bit-identical); beyond, one sweep over the keys with a running row maximum.  ``out``: a caller-owned fp32
    tensor of q's shape (contiguous head_dim) to write O into.
    ``live`` (a ``LiveRows`` over the ``B x N`` rows; CAUSAL ``mask``, ``attn_live_shape``): ``mmx_attn_fwd_live`` -- the rows past
    ``live.eot[b]`` of q / k / v are not read and those of O are not written; the live rows of O get the bits of
    ``attn_capture_fwd(live=...)``, which are those of the dense call on a q / k / v with zeros in the dead rows.  Outside
    ``attn_live_shape`` it raises (``MMX_ENOTSUP``; nothing is launched)."""
    _dev(q, k, v, mask, out)
    if q.dtype != torch.float32 or k.dtype != torch.float32 or v.dtype != torch.float32:
        raise MMXError("attn_fwd is exact fp32 (no bf16 / fp16 mode yet), got %s" % str(q.dtype).replace("torch.", ""))
    B, H, Nq, Nk, D = _attn_dims(q, k, layout)
    if out is not None and (out.dtype != torch.float32 or out.shape != q.shape):
        raise MMXError("attn_fwd: out must be fp32 of q's shape %s" % (tuple(q.shape),))
    mask, msb, msq = _mask_strides(mask, Nk)
    if live is not None:
        _live_attn_check("attn_fwd", live, B, Nq, Nk, q)
        if mask is None:
            raise MMXError("attn_fwd: live= stands on a causal mask")
        o = out if out is not None else live._out(q, D)
        check(lib().mmx_attn_fwd_live(*_qkv_args(q, k, v, layout), _p(mask), msb, msq, *_strided(o, layout), B, H, Nq, Nk, D,
                                      float(scale), scale_mode, _p(live.eot), _stream()), "mmx_attn_fwd_live")
        return o
    o = out if out is not None else torch.empty(q.shape, dtype=torch.float32, device=q.device)
    check(lib().mmx_attn_fwd(*_qkv_args(q, k, v, layout), _p(mask), msb, msq, *_strided(o, layout), B, H, Nq, Nk, D, float(scale),
                             scale_mode, _stream()), "mmx_attn_fwd")
    return o


def patch_ranks(scores, out=None):
    """``scores [B, P]`` fp32 -> ``ranks [B, P]`` int32: position of every patch in ONE stable descending order of its row
    (``torch.sort(descending=True, stable=True)``: ties by ascending index, ``+0.0 == -0.0``, NaN first).  ``P <= 4096``."""
    _dev(scores, out)
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise MMXError("patch_ranks: scores must be [B, P] fp32, got %s %s" % (tuple(scores.shape), scores.dtype))
    scores = scores.contiguous()
    if out is not None and (out.dtype != torch.int32 or out.shape != scores.shape or not out.is_contiguous()):
        raise MMXError("patch_ranks: out must be a contiguous int32 tensor of the scores' shape")
    ranks = out if out is not None else torch.empty(scores.shape, dtype=torch.int32, device=scores.device)
    check(lib().mmx_patch_ranks(_p(scores), _p(ranks), scores.shape[0], scores.shape[1], _stream()), "mmx_patch_ranks")
    return ranks


def perturb_patches(images, ranks, counts, fill, out=None):
    """``images [B, C, R, R]`` fp32, ``ranks [B, (R / patch)^2]`` int32, ``counts [S]`` int32 (device), ``fill [C]`` fp32 ->
    ``[S, B, C, R, R]``: copy s keeps the pixels of the patches ranked below ``counts[s]`` and sets the others to ``fill[c]``
    (one launch).  The patch size follows from ``ranks``' width."""
    _dev(images, ranks, counts, fill, out)
    if images.dim() != 4 or images.shape[2] != images.shape[3] or images.dtype != torch.float32:
        raise MMXError("perturb_patches: images must be [B, C, R, R] fp32, got %s %s" % (tuple(images.shape), images.dtype))
    B, C, R, _ = images.shape
    if ranks.dtype != torch.int32 or ranks.dim() != 2 or ranks.shape[0] != B or counts.dtype != torch.int32 or counts.dim() != 1:
        raise MMXError("perturb_patches: ranks must be [B, P] int32 and counts [S] int32")
    grid = int(round(ranks.shape[1] ** 0.5))
    if grid < 1 or grid * grid != ranks.shape[1] or R % grid:
        raise MMXError("perturb_patches: %d patches are not a square grid that divides the resolution %d" % (ranks.shape[1], R))
    fill = _f32c(fill).reshape(-1)
    if fill.numel() != C:
        raise MMXError("perturb_patches: fill needs one value per channel (%d), got %d" % (C, fill.numel()))
    S = counts.shape[0]
    images, ranks, counts = images.contiguous(), ranks.contiguous(), counts.contiguous()
    if out is None:
        out = torch.empty(S, B, C, R, R, dtype=torch.float32, device=images.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != S * B * C * R * R:
        raise MMXError("perturb_patches: out must be a contiguous fp32 [S, B, C, R, R] tensor")
    check(lib().mmx_perturb_patches(_p(images), _p(ranks), _p(counts), _p(fill), _p(out), B, C, R, R // grid, S, _stream()),
          "mmx_perturb_patches")
    return out


def perturb_tokens(ids, scores, counts, want_ranks=False, out=None):
    """The S perturbed copies of B captions in one launch (``mmx_perturb_tokens``).  ``ids [B, N]`` int64 token ids, ``scores [B, N]``
    fp32 (one per position), ``counts [S, N - 1]`` int32 on the device (``clip_text_perturbation.token_step_counts``) ->
    ``(out_ids [S, B, N] int64, out_eot [S, B] int64)``, with ``want_ranks`` also ``ranks [B, N]`` int32.  A caption's EOT is the first
    maximum of its ids, its words the positions between position 0 and EOT; step s keeps the ``counts[s][W]`` best-scored of its W
    words (ONE stable descending order, the one of ``patch_ranks``) in their original order between the first token and EOT, zeros
    behind; ``out_eot`` is where EOT lands (``== out_ids.argmax(-1)``).  ``2 <= N <= 256``, ``S <= 64``.  ``out``: contiguous
    ``(out_ids, out_eot)`` or, with ``want_ranks``, ``(out_ids, out_eot, ranks)`` to write to."""
    _dev(ids, scores, counts, *(out or ()))
    if ids.dim() != 2 or ids.dtype != torch.int64 or scores.dtype != torch.float32 or scores.shape != ids.shape:
        raise MMXError("perturb_tokens: ids [B, N] int64 and scores [B, N] fp32 expected, got %s %s / %s %s"
                       % (tuple(ids.shape), ids.dtype, tuple(scores.shape), scores.dtype))
    B, N = ids.shape
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != N - 1:
        raise MMXError("perturb_tokens: counts must be [S, %d] int32 (one count per word count), got %s %s"
                       % (N - 1, tuple(counts.shape), counts.dtype))
    S = counts.shape[0]
    ids, scores, counts = ids.contiguous(), scores.contiguous(), counts.contiguous()
    if out is not None:
        if len(out) != (3 if want_ranks else 2):
            raise MMXError("perturb_tokens: out must be (out_ids, out_eot%s)" % (", ranks" if want_ranks else ""))
        out_ids, out_eot, ranks = tuple(out) + (() if want_ranks else (None,))
        for t, shape, dt in ((out_ids, (S, B, N), torch.int64), (out_eot, (S, B), torch.int64), (ranks, (B, N), torch.int32)):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous()):
                raise MMXError("perturb_tokens: out needs contiguous out_ids [S, B, N] int64, out_eot [S, B] int64, ranks [B, N] int32")
    else:
        out_ids = torch.empty(S, B, N, dtype=torch.int64, device=ids.device)
        out_eot = torch.empty(S, B, dtype=torch.int64, device=ids.device)
        ranks = torch.empty(B, N, dtype=torch.int32, device=ids.device) if want_ranks else None
    check(lib().mmx_perturb_tokens(_p(ids), _p(scores), _p(counts), _p(out_ids), _p(out_eot), _p(ranks), B, N, S, _stream()),
          "mmx_perturb_tokens")
    return (out_ids, out_eot, ranks) if want_ranks else (out_ids, out_eot)


def _perturb_rows(what, cam, text_len, T):
    """The operands the two single-stream builders share: ``cam [B, T + V]`` fp32 in the padded layout, ``text_len [B]`` int32 on the
    device, the padded text width ``T`` -> ``(cam, text_len, B, T, V)``."""
    if cam.dim() != 2 or cam.dtype != torch.float32:
        raise MMXError("%s: cam must be [B, T + V] fp32 in the padded layout, got %s %s" % (what, tuple(cam.shape), cam.dtype))
    B, N = cam.shape
    T = int(T)
    if T < 3 or N - T < 1 or N > _lib.SELFATTN_MAX_TOKENS:
        raise MMXError("%s: needs T >= 3, V = N - T >= 1 and N <= %d (got N=%d, T=%d)" % (what, _lib.SELFATTN_MAX_TOKENS, N, T))
    if text_len.dtype != torch.int32 or tuple(text_len.shape) != (B,):
        raise MMXError("%s: text_len must be [%d] int32 on the device, got %s %s" % (what, B, tuple(text_len.shape), text_len.dtype))
    return cam.contiguous(), text_len.contiguous(), B, T, N - T


def selfattn_perturb_regions(emb, cam, text_len, counts, rows, n_text, positive=False, want_ranks=False, out=None):
    """The packed input of the image perturbation test of a padded single-stream batch in one launch (``mmx_selfattn_perturb_regions``).
    ``emb [B, T + V, E]`` fp32 (embedded + LayerNorm-ed rows), ``cam [B, T + V]`` fp32, ``text_len [B]`` int32, ``counts [G]`` int32 on
    the device (the DISTINCT keep counts, descending), ``rows`` = ``B * sum_g (T + c_g)`` as the host computed it from the same counts,
    ``n_text = T`` -> ``(x [rows, E] fp32, mask [rows] fp32, pooled [G, B] int64)``, with ``want_ranks`` also ``ranks [B, V]`` int32.
    Sequence (g, b) starts at row ``off_g + b * (T + c_g)``: item b's T text rows, then its ``c_g`` best regions in rank order (the
    stable order of ``patch_ranks``; ``positive`` ranks the negated scores); ``mask`` is ``-10000`` at padded text positions;
    ``pooled`` is the packed row of token ``text_len[b] - 2``.  ``E <= 2**20`` and ``B * G < 2**31`` (the entry refuses more).  ``out``: contiguous ``(x, mask, pooled[, ranks])`` to write to."""
    what = "selfattn_perturb_regions"
    _dev(emb, cam, text_len, counts, *(out or ()))
    cam, text_len, B, T, V = _perturb_rows(what, cam, text_len, n_text)
    if emb.dim() != 3 or emb.dtype != torch.float32 or tuple(emb.shape[:2]) != (B, T + V) or emb.shape[2] < 1:
        raise MMXError("%s: emb must be [%d, %d, E] fp32, got %s %s" % (what, B, T + V, tuple(emb.shape), emb.dtype))
    if counts.dtype != torch.int32 or counts.dim() != 1 or not 1 <= counts.shape[0] <= 64:
        raise MMXError("%s: counts must be [G] int32 with 1 <= G <= 64, got %s %s" % (what, tuple(counts.shape), counts.dtype))
    E, G, rows = emb.shape[2], counts.shape[0], int(rows)
    if not B * G * T <= rows <= B * G * (T + V):
        raise MMXError("%s: %d packed rows outside B * G * T .. B * G * (T + V) = %d .. %d" % (what, rows, B * G * T, B * G * (T + V)))
    emb, counts = emb.contiguous(), counts.contiguous()
    shapes = (((rows, E), torch.float32), ((rows,), torch.float32), ((G, B), torch.int64), ((B, V), torch.int32))
    if out is not None:
        if len(out) != (4 if want_ranks else 3):
            raise MMXError("%s: out must be (x, mask, pooled%s)" % (what, ", ranks" if want_ranks else ""))
        for t, (shape, dt) in zip(out, shapes):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise MMXError("%s: out needs contiguous x [R, E] fp32, mask [R] fp32, pooled [G, B] int64, ranks [B, V] int32" % what)
        x, mask, pooled, ranks = tuple(out) + (() if want_ranks else (None,))
    else:
        x, mask, pooled, ranks = (torch.empty(shape, dtype=dt, device=emb.device) for shape, dt in shapes)
        if not want_ranks:
            ranks = None
    check(lib().mmx_selfattn_perturb_regions(_p(emb), _p(cam), _p(text_len), _p(counts), _p(x), _p(mask), _p(pooled), _p(ranks), B, T, V,
                                             E, G, rows, int(bool(positive)), _stream()), "mmx_selfattn_perturb_regions")
    return (x, mask, pooled, ranks) if want_ranks else (x, mask, pooled)


def selfattn_perturb_text(ids, segments, cam, text_len, counts, positive=False, out=None):
    """The S perturbed copies of B padded questions of a single-stream batch in one launch (``mmx_selfattn_perturb_text``).
    ``ids`` / ``segments [B, T]`` int64, ``cam [B, T + V]`` fp32, ``text_len [B]`` int32, ``counts [S, T]`` int32 on the device
    (``counts[s][w] = int((1 - step_s) * w)``) -> ``(ids, segments, mask [S, B, T] int64, new_len [S, B] int64)``.  With ``n`` the
    length of question b (clamped to 3 .. T): positions 0, n - 2 and n - 1 always stay, step s keeps the ``counts[s][n - 3]`` best of
    the words 1 .. n - 3 (the stable order of ``patch_ranks``; ``positive`` ranks the negated scores) in their original order,
    left-aligned, zeros behind; ``new_len = 3 + kept``.  ``out``: the four contiguous tensors to write to."""
    what = "selfattn_perturb_text"
    _dev(ids, segments, cam, text_len, counts, *(out or ()))
    if ids.dim() != 2 or ids.dtype != torch.int64 or segments.dtype != torch.int64 or segments.shape != ids.shape:
        raise MMXError("%s: ids and segments must be [B, T] int64, got %s %s / %s %s"
                       % (what, tuple(ids.shape), ids.dtype, tuple(segments.shape), segments.dtype))
    cam, text_len, B, T, V = _perturb_rows(what, cam, text_len, ids.shape[1])
    if ids.shape[0] != B:
        raise MMXError("%s: %d questions but %d relevancy rows" % (what, ids.shape[0], B))
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != T or not 1 <= counts.shape[0] <= 64:
        raise MMXError("%s: counts must be [S, %d] int32 with 1 <= S <= 64, got %s %s" % (what, T, tuple(counts.shape), counts.dtype))
    S = counts.shape[0]
    ids, segments, counts = ids.contiguous(), segments.contiguous(), counts.contiguous()
    shapes = ((S, B, T), (S, B, T), (S, B, T), (S, B))
    if out is not None:
        if len(out) != 4 or any(tuple(t.shape) != s or t.dtype != torch.int64 or not t.is_contiguous() for t, s in zip(out, shapes)):
            raise MMXError("%s: out needs contiguous int64 ids, segments, mask [S, B, T] and new_len [S, B]" % what)
        o_ids, o_seg, o_mask, new_len = out
    else:
        o_ids, o_seg, o_mask, new_len = (torch.empty(s, dtype=torch.int64, device=ids.device) for s in shapes)
    check(lib().mmx_selfattn_perturb_text(_p(ids), _p(segments), _p(cam), _p(text_len), _p(counts), _p(o_ids), _p(o_seg), _p(o_mask),
                                          _p(new_len), B, T, V, S, int(bool(positive)), _stream()), "mmx_selfattn_perturb_text")
    return o_ids, o_seg, o_mask, new_len


def text_placement(place):
    """A placement table of ``lxmert_perturb_text`` -- S rows ``(base, stride, width)`` -- as the HOST int64 array the entry reads
    (build it once per shape and pass it again: a call then creates nothing)."""
    rows = [tuple(int(v) for v in row) for row in place]
    if not rows or any(len(row) != 3 for row in rows):
        raise MMXError("text_placement: S >= 1 rows of (base, stride, width) expected")
    return (C.c_int64 * (3 * len(rows)))(*[v for row in rows for v in row])


def lxmert_perturb_text(ids, types, cam, text_len, counts, place, out_elems, positive=False, want_ranks=False, out=None):
    """The S perturbed copies of B padded questions of a two-stream batch in one launch, written where ``place`` puts them
    (``mmx_lxmert_perturb_text``).  ``ids`` / ``types [B, T]`` int64, ``cam [B, T]`` fp32, ``text_len [B]`` int32 and ``counts
    [S, T - 1]`` int32 on the device (``counts[s][w] = int((1 - step_s) * w)``), ``place``: S rows ``(base, stride, width)`` on the
    host (a list, or what ``text_placement`` made of one) -> ``(ids, types [out_elems] int64, mask [out_elems] fp32, new_len [S, B]
    int64)``, with ``want_ranks`` also ``ranks [B, T]`` int32.  With ``n`` the length of question b (clamped to 2 .. T): positions 0
    and n - 1 always stay, step s keeps the ``counts[s][n - 2]`` best of the words 1 .. n - 2 (the stable order of ``patch_ranks``;
    ``positive`` ranks the negated scores) in their original order; sequence (s, b) is the ``width_s`` elements at ``base_s + b *
    stride_s``: the kept positions, zeros behind, truncated at the width; ``new_len = 2 + kept`` is not truncated.  Elements no
    sequence covers are not written.  ``2 <= T <= 256``, ``S <= 64``.  ``out``: the contiguous tensors to write to."""
    what = "lxmert_perturb_text"
    _dev(ids, types, cam, text_len, counts, *(out or ()))
    if ids.dim() != 2 or ids.dtype != torch.int64 or types.dtype != torch.int64 or types.shape != ids.shape:
        raise MMXError("%s: ids and types must be [B, T] int64, got %s %s / %s %s"
                       % (what, tuple(ids.shape), ids.dtype, tuple(types.shape), types.dtype))
    B, T = ids.shape
    if not 2 <= T <= 256 or B < 1:
        raise MMXError("%s: needs B >= 1 and 2 <= T <= 256 (got B=%d, T=%d)" % (what, B, T))
    if cam.dtype != torch.float32 or tuple(cam.shape) != (B, T):
        raise MMXError("%s: cam must be [%d, %d] fp32, got %s %s" % (what, B, T, tuple(cam.shape), cam.dtype))
    if text_len.dtype != torch.int32 or tuple(text_len.shape) != (B,):
        raise MMXError("%s: text_len must be [%d] int32 on the device, got %s %s" % (what, B, tuple(text_len.shape), text_len.dtype))
    if counts.dtype != torch.int32 or counts.dim() != 2 or counts.shape[1] != T - 1 or not 1 <= counts.shape[0] <= 64:
        raise MMXError("%s: counts must be [S, %d] int32 with 1 <= S <= 64, got %s %s" % (what, T - 1, tuple(counts.shape), counts.dtype))
    S, out_elems = counts.shape[0], int(out_elems)
    if not isinstance(place, C.Array):
        place = text_placement(place)
    if len(place) != 3 * S:
        raise MMXError("%s: %d placement rows for %d steps" % (what, len(place) // 3, S))
    if out_elems < 1:
        raise MMXError("%s: out_elems = %d < 1" % (what, out_elems))
    ids, types, cam, text_len, counts = ids.contiguous(), types.contiguous(), cam.contiguous(), text_len.contiguous(), counts.contiguous()
    shapes = (((out_elems,), torch.int64), ((out_elems,), torch.int64), ((out_elems,), torch.float32), ((S, B), torch.int64),
              ((B, T), torch.int32))
    if out is not None:
        if len(out) != (5 if want_ranks else 4):
            raise MMXError("%s: out must be (ids, types, mask, new_len%s)" % (what, ", ranks" if want_ranks else ""))
        for t, (shape, dt) in zip(out, shapes):
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise MMXError("%s: out needs contiguous ids / types [out_elems] int64, mask [out_elems] fp32, new_len [S, B] int64, "
                               "ranks [B, T] int32" % what)
        o_ids, o_types, o_mask, new_len, ranks = tuple(out) + (() if want_ranks else (None,))
    else:
        o_ids, o_types, o_mask, new_len, ranks = (torch.empty(shape, dtype=dt, device=ids.device) for shape, dt in shapes)
        if not want_ranks:
            ranks = None
    check(lib().mmx_lxmert_perturb_text(_p(ids), _p(types), _p(cam), _p(text_len), _p(counts), place, _p(o_ids), _p(o_types), _p(o_mask),
                                        _p(new_len), _p(ranks), out_elems, B, T, S, int(bool(positive)), _stream()),
          "mmx_lxmert_perturb_text")
    return (o_ids, o_types, o_mask, new_len, ranks) if want_ranks else (o_ids, o_types, o_mask, new_len)


def head_kernel_shape(n_q, n_k, head_dim, slab_dtype=torch.float32):
    """Does the register-resident whole-head backward (``attention_head.hip``) serve this shape?  (Its eligibility test, host side:
    what decides whether a bf16 gradient stream can pass through an exact-fp32 attention without conversion passes.)"""
    if not (slab_dtype == torch.float32 and 1 <= n_k <= 128 and 1 <= n_q <= 256 and head_dim % 4 == 0 and head_dim <= 64):
        return False
    # the kernel's own exclusions (attention_head.hip, attn_bwd_head_try): its LDS image must fit a CU, and the widest key
    # side is not instantiated beyond 8 query strips
    dp, ntk, ntq = (32 if head_dim <= 32 else 64), (n_k + 15) // 16, (n_q + 15) // 16
    lds = 4 * max(ntk * 16 * (2 * dp + 12), ntq * 16 * (ntk * 16 + 4 + dp + 4))
    return lds <= 160 * 1024 and not (ntk >= 7 and ntq > 8)


def _attn_capture_bwd_grouped(q, k, probs, d_o, dprobs_out, layout, mma_bf16, rel_row, images):
    """The refusals of ``attn_capture_bwd(images=M)``, the grouped row mode (per-image forward operands, per-target everything
    else); the call itself is the exact-fp32 ``rel_row`` branch's, over the ``T`` targets."""
    if rel_row is None or mma_bf16:
        raise MMXError("attn_capture_bwd: images= is the grouped exact-fp32 row mode: it needs rel_row and mma_bf16=False")
    M, _H, Nq, Nk, _D = _attn_dims(q, k, layout)
    T = d_o.shape[0]
    if images != M or probs.shape[0] != M or images < 1 or T % images:
        raise MMXError("attn_capture_bwd: images=%d needs q/k/v/probs of batch %d and a d_o batch that is a multiple of it "
                       "(q batch %d, probs batch %d, d_o batch %d)" % (images, images, M, probs.shape[0], T))
    if rel_row.dtype != torch.float32 or tuple(rel_row.shape) != (T, Nq) or Nq != Nk or probs.dtype != torch.float32:
        raise MMXError("attn_capture_bwd: grouped rel_row needs fp32 [T, N] rows and fp32 slabs of a self-attention")
    if d_o.dtype != torch.float32:
        raise MMXError("attn_capture_bwd: grouped rel_row needs an fp32 d_o")
    if dprobs_out is not None and (dprobs_out.dtype != torch.float32 or dprobs_out.shape[0] != T):
        raise MMXError("attn_capture_bwd: grouped dprobs_out must be fp32 with batch %d" % T)
    if probs.stride(-1) != 1 or not probs.is_contiguous():
        raise MMXError("attn_capture_bwd: grouped probs must be a contiguous [M, H, N, N] slab")
    return T


def attn_capture_bwd(q, k, v, probs, d_o, dprobs_out, scale, scale_mode=_lib.SCALE_Q_FIRST, need_dqkv=True,
                     layout="bnhd", out=None, batch=None, o=None, mma_bf16=False, rel_row=None, images=None, live=None):
    """Writes dP into ``dprobs_out`` and returns ``(dq, dk, dv)`` (``None`` when ``need_dqkv`` is False).
    ``live`` (the backward of ``attn_capture_fwd(live=...)``, ``mmx_attn_capture_bwd_live``; fp32 ``d_o``, none of ``batch`` /
    ``rel_row`` / ``images`` / ``mma_bf16``): the rows past ``live.eot[b]`` of q / k / v / d_o are not read and those of dq / dk / dv
    are not written; ``dprobs_out`` is written whole, exact zeros in the dead rows; every live value has the bits of the dense call
    on operands with zeros in the dead rows.
    ``out=(dq, dk, dv)`` lets the caller hand in (strided) views, e.g. of one packed dqkv tensor.
    ``batch``: shared-forward mode -- q/k/v/probs come from ONE forward (batch 1) and are broadcast (stride 0) over the
    ``batch`` upstream gradients in ``d_o``; dq/dk/dv/dprobs are per sample.
    ``o``: the forward's output (same layout as ``q``), optional: saves the long-sequence kernels a sweep over the keys.
    ``rel_row`` (``[B, N]`` fp32; row-relevancy mode, ``mmx_attn_capture_bwd_rowrel`` with ``mma_bf16=True``,
    ``mmx_attn_capture_bwd_rowrel_f32`` on the exact-fp32 kernels otherwise): returns
    ``(dq, dk, dv, rel_row + rel_row . mean_h clamp(dP * P, 0))``; ``dprobs_out`` may then be ``None`` (dP is not stored;
    exact fp32 beyond the whole-head shapes with ``need_dqkv``: the key-side kernel reads dP back, from a scratch slab).
    ``images=M`` (with an exact-fp32 ``rel_row``; grouped row mode, ``mmx_attn_capture_bwd_rowrel_f32_grouped``): q/k/v/probs/o
    come from ONE forward over M distinct images (batch M); ``d_o``, ``rel_row``, dq/dk/dv and ``dprobs_out`` have batch T, a
    multiple of M, in K-major order -- target t explains image t % M."""
    _dev(q, k, v, probs, d_o, dprobs_out, rel_row)
    if live is not None and (images is not None or rel_row is not None or mma_bf16 or dprobs_out is None
                             or (batch is not None and batch != q.shape[0]) or d_o.dtype != torch.float32):
        raise MMXError("attn_capture_bwd: live= is the plain fp32 capture backward (a dprobs slab, an fp32 d_o, one forward per "
                       "gradient; no rel_row / images / mma_bf16)")
    targets = None
    if images is not None:
        images = int(images)
        targets = _attn_capture_bwd_grouped(q, k, probs, d_o, dprobs_out, layout, mma_bf16, rel_row, images)
    if probs.dtype not in _DTYPES or (dprobs_out is not None and probs.dtype != dprobs_out.dtype):
        raise MMXError("attn_capture_bwd: probs / dprobs slabs must share one of fp32 / fp16 / bf16")
    if dprobs_out is None and rel_row is None:
        raise MMXError("attn_capture_bwd: no dprobs slab (only the row-relevancy mode runs without one)")
    B, H, Nq, Nk, D = _attn_dims(q, k, layout)
    shared = targets is None and batch is not None and batch != B
    if shared:
        if B != 1:
            raise MMXError("shared-forward backward needs batch-1 q/k/v")
        B = batch
        q, k, v = (t.expand(B, *t.shape[1:]) for t in (q, k, v))      # stride-0 views, no copy
        if o is not None:
            o = o.expand(B, *o.shape[1:])
    if targets is not None:
        B = targets                                  # per target from here on; q / k / v / probs / o keep their batch of images
    probs_sb = 0 if shared else H * Nq * Nk
    if d_o.stride(-1) != 1:
        d_o = d_o.contiguous()
    io_bf16 = d_o.dtype == torch.bfloat16            # bf16 gradient stream: dq / dk / dv come back as bf16 too
    if io_bf16 and not mma_bf16 and not head_kernel_shape(Nq, Nk, D, probs.dtype):
        raise MMXError("attn_capture_bwd: a bf16 d_o needs mma_bf16=True (MMX_ATTN_IO_BF16) or a whole-head shape "
                       "(fp32 slabs, Nk <= 128, Nq <= 256, head_dim % 4 == 0 and <= 64: exact-fp32 arithmetic on the bf16 stream)")
    flags = (_lib.MMX_ATTN_MMA_BF16 if mma_bf16 else 0) | (_lib.MMX_ATTN_IO_BF16 if io_bf16 else 0)
    dq = dk = dv = None
    ws = None
    need = 0
    if need_dqkv:
        if out is not None:
            dq, dk, dv = out
        else:
            dq, dk, dv = (torch.empty((B,) + tuple(t.shape[1:]), dtype=d_o.dtype, device=t.device) for t in (q, k, v))
        if rel_row is None:                                    # (the row modes size their own workspace: delta is its first part)
            need = lib().mmx_attn_capture_bwd_workspace_bytes(B, H, Nq)
            ws = _workspace(need, q.device, "attn_bwd")
    if o is not None and (o.dtype != torch.float32 or o.stride(-1) != 1):
        o = None                                               # only a hint: fall back to the two-sweep form
    slab = _DTYPES[probs.dtype]

    def operands(slab_dtype, dprobs, d_o_=d_o, grads=(dq, dk, dv), fwd_o=o):
        return _attn_bwd_args(layout, (q, k, v), probs, probs_sb, slab_dtype, d_o_, fwd_o, dprobs, grads, (B, H, Nq, Nk, D), scale,
                              scale_mode, need_dqkv)
    if rel_row is not None:
        if not mma_bf16:
            if rel_row.dtype != torch.float32 or tuple(rel_row.shape) != (B, Nq) or Nq != Nk or probs.dtype != torch.float32:
                raise MMXError("attn_capture_bwd: exact-fp32 rel_row needs fp32 [B, N] rows and fp32 slabs of a self-attention")
            if io_bf16:
                raise MMXError("attn_capture_bwd: exact-fp32 rel_row needs an fp32 d_o")
            name, tail, dprobs = "mmx_attn_capture_bwd_rowrel_f32", (), dprobs_out
            if targets is not None:
                name, tail = name + "_grouped", (images,)
            if dprobs is None and need_dqkv and not head_kernel_shape(Nq, Nk, D, probs.dtype):
                dprobs = _workspace(4 * B * H * Nq * Nk, q.device, "attn_rowrel_dp").view(torch.float32)
        else:
            if rel_row.dtype != torch.float32 or tuple(rel_row.shape) != (B, Nq) or Nq != Nk:
                raise MMXError("attn_capture_bwd: rel_row must be fp32 [B, N] of a self-attention, with mma_bf16=True")
            name, tail, slab, dprobs = "mmx_attn_capture_bwd_rowrel", (), slab | flags, dprobs_out
        rel_row = rel_row.contiguous()
        rel_out = torch.empty_like(rel_row)
        need = getattr(lib(), name + "_workspace_bytes")(B, H, Nq, Nk)
        ws = _workspace(need, q.device, "attn_bwd")
        check(getattr(lib(), name)(*operands(slab, dprobs), _p(rel_row), _p(rel_out), *tail, _p(ws), need, _stream()), name)
        return dq, dk, dv, rel_out
    if live is not None:
        _live_attn_check("attn_capture_bwd", live, B, Nq, Nk, probs)
        check(lib().mmx_attn_capture_bwd_live(*operands(slab, dprobs_out, fwd_o=False), _p(live.eot), _p(ws), need, _stream()),
              "mmx_attn_capture_bwd_live")
        return dq, dk, dv
    rc = lib().mmx_attn_capture_bwd_ex(*operands(slab | flags, dprobs_out), _p(ws), need, _stream())
    if rc == _lib.MMX_ENOTSUP and io_bf16 and not mma_bf16:
        # the whole-head kernel is the only exact-fp32 kernel with bf16 gradient I/O; it turned this call down at run time (a view
        # it cannot load 8 bytes at a time, or option attn_head = 0): same arithmetic on an fp32 d_o, results rounded once to bf16
        f32 = [torch.empty(tuple(t.shape), dtype=torch.float32, device=t.device) for t in (q, k, v)] if need_dqkv else [None] * 3
        check(lib().mmx_attn_capture_bwd_ex(*operands(slab | flags & ~_lib.MMX_ATTN_IO_BF16, dprobs_out, d_o.float(), f32), _p(ws),
                                            need, _stream()), "mmx_attn_capture_bwd")
        if need_dqkv:
            for dst, src in zip((dq, dk, dv), f32):
                dst.copy_(src)
        return dq, dk, dv
    check(rc, "mmx_attn_capture_bwd")
    return dq, dk, dv


def attn_relprop(q, k, v, probs, o, cam_o, scale, scale_mode=_lib.SCALE_Q_FIRST, layout="bnhd", phase=3, cam_scores=None):
    """LRP relevance through the attention core (``mmx_attn_relprop[_phase]``; the two halved matmul / ``einsum`` relprops of
    DETR/modules/layers.py:770-781, lxmert_lrp.py:422-461, BERT_ours.py:345-395).  ``q [B, Nq, H, D]``, ``k`` / ``v [B, Nk,
    H, D]``, ``o`` / ``cam_o [B, Nq, H, D]`` (strided views ok), ``probs [B, H, Nq, Nk]`` fp32 contiguous.  Returns ``(cam_probs
    [B, H, Nq, Nk], cam_q, cam_k, cam_v)`` with the cams of q / k / v contiguous in ``layout``.

    ``phase``: ``_lib.LRP_VALUES`` -> ``(cam_probs, None, None, cam_v)`` from ``cam_o``; ``_lib.LRP_SCORES`` -> ``(None, cam_q,
    cam_k, None)`` from ``cam_scores [B, H, Nq, Nk]`` (the relevance of the pre-softmax scores; ``v / probs / o / cam_o`` may be
    ``None``); both (default) with ``cam_scores=None``: the fused core."""
    values, scores = bool(phase & _lib.LRP_VALUES), bool(phase & _lib.LRP_SCORES)
    given = [t for t in (q, k, v, probs, o, cam_o, cam_scores) if t is not None]
    _dev(*given)
    if any(t.dtype != torch.float32 for t in given):
        raise MMXError("attn_relprop: fp32 operands only")
    B, H, Nq, Nk, D = _attn_dims(q, k, layout)
    for name, t in (("probs", probs if values else None), ("cam_scores", cam_scores)):
        if t is not None and (not t.is_contiguous() or t.numel() != B * H * Nq * Nk):
            raise MMXError("attn_relprop: %s must be a contiguous [B,H,Nq,Nk] slab" % name)
    if scores and not values and cam_scores is None:
        raise MMXError("attn_relprop: the scores phase alone needs cam_scores")
    if values and cam_o.stride(-1) != 1:
        cam_o = cam_o.contiguous()
    new = lambda t: torch.empty(tuple(t.shape), dtype=torch.float32, device=q.device)          # noqa: E731
    cam_probs = torch.empty(B, H, Nq, Nk, dtype=torch.float32, device=q.device) if values else None
    cam_q, cam_k = (new(q), new(k)) if scores else (None, None)
    cam_v = new(v) if values else None
    qkv, (po, *so), (pc, *sc) = _qkv_args(q, k, v, layout), _strided(o, layout), _strided(cam_o, layout)
    check(lib().mmx_attn_relprop_phase(*qkv[:3], po, pc, *qkv[3:], *so, *sc, _p(probs), _p(cam_probs),
                                       *_qkv_args(cam_q, cam_k, cam_v, layout), B, H, Nq, Nk, D, float(scale), scale_mode,
                                       _p(cam_scores), int(phase), _stream()), "mmx_attn_relprop_phase")
    return cam_probs, cam_q, cam_k, cam_v


def detr_decoder_rows(self_pairs, cross_pairs, targets, shared_attn=False):
    """K2-DETR (``mmx_detr_decoder_rows``): the decoder half of DETR's rules for ROWS of ``R_q_i`` in four launches.
    ``self_pairs[l]`` / ``cross_pairs[l]``: ``(attn, grad)`` of decoder layer l's self- / cross-attention, fp32, gradient
    slabs ``[K*H, Q, *]``, probability slabs the same or ``[H, Q, *]`` when ``shared_attn`` (one forward for the K samples).
    ``targets``: ``[K]`` long.  Returns ``(s [K, Ni], diag_min [1])`` -- see include/mmx_relevancy.h."""
    targets = targets.reshape(-1).to(torch.long).contiguous()
    K = targets.numel()
    tens = [t for pair in list(self_pairs) + list(cross_pairs) for t in pair]
    _dev(targets, *tens)
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in tens):
        raise MMXError("detr_decoder_rows: fp32 contiguous slabs only")
    g0, c0 = self_pairs[0][1], cross_pairs[0][1]
    Q, Ni = g0.shape[-1], c0.shape[-1]
    H = g0.numel() // (K * Q * Q)
    if H * K * Q * Q != g0.numel() or c0.numel() != K * H * Q * Ni:
        raise MMXError("detr_decoder_rows: slab shapes %s / %s do not fit K = %d" % (tuple(g0.shape), tuple(c0.shape), K))
    L = len(self_pairs)
    s_out = torch.empty(K, Ni, dtype=torch.float32, device=g0.device)
    dmin = torch.empty(1, dtype=torch.float32, device=g0.device)
    need = lib().mmx_detr_decoder_rows_workspace_bytes(L, K, Q, Ni)
    ws = _workspace(need, g0.device, "detr_rows")
    tables = [_lib.ptr_table([pair[w].data_ptr() for pair in grp]) for grp in (self_pairs, cross_pairs) for w in (0, 1)]
    (sa, _k0), (sg, _k1), (ca, _k2), (cg, _k3) = tables
    check(lib().mmx_detr_decoder_rows(sa, sg, ca, cg, L, K, H, Q, Ni, 0 if shared_attn else H * Q * Q,
                                      0 if shared_attn else H * Q * Ni, _p(targets), _p(s_out), _p(dmin), _p(ws), need,
                                      _stream()), "mmx_detr_decoder_rows")
    return s_out, dmin


# ------------------------------------------------------------------------------------------- DETR baselines, all kept queries at once
DETR_BASELINES_MAX_TOKENS = 2048       # Ni of mmx_detr_cross_rows / mmx_detr_rollout_rows (Q <= 128, H <= 32)


def _detr_slab(what, t, tail=None):
    """An fp32 ``[H, rows, cols]`` capture slab of ONE image (``get_attn()`` of a DETR attention module)."""
    _dev(t)
    if t.dtype != torch.float32 or t.dim() != 3 or (tail is not None and tuple(t.shape[1:]) != tuple(tail)):
        raise MMXError("%s: fp32 [H, rows, cols] capture slabs of one image only, got %s %s%s"
                       % (what, t.dtype, tuple(t.shape), "" if tail is None else " (expected [*, %d, %d])" % tuple(tail)))
    return t.contiguous()


def _detr_targets(what, targets):
    _dev(targets)
    targets = targets.reshape(-1).to(torch.long).contiguous()
    if targets.numel() < 1:
        raise MMXError("%s: needs at least one target" % what)
    return targets


def _detr_cross_rows(what, cross_attn, cross_grad, targets):
    P = _detr_slab(what, cross_attn)
    targets = _detr_targets(what, targets)
    K, (H, Q, Ni) = targets.numel(), P.shape
    bstride, ws, need = 0, None, 0
    if cross_grad is not None:
        cross_grad = _detr_slab(what, cross_grad, (Q, Ni))
        if cross_grad.shape[0] == K * H:
            bstride = H * Q * Ni
        elif cross_grad.shape[0] != H:
            raise MMXError("%s: the gradient slab is [K * H, Q, Ni] or, shared by every target, [H, Q, Ni]; got %s for K = %d, H = %d"
                           % (what, tuple(cross_grad.shape), K, H))
        need = lib().mmx_detr_cross_rows_workspace_bytes(K, H, Q, Ni)
        ws = _workspace(need, P.device, tag="detr_cross_rows")      # grow-only scratch: pinned_state keeps it alive for graphs
    out = torch.empty(K, Ni, dtype=torch.float32, device=P.device)
    check(lib().mmx_detr_cross_rows(_p(P), _p(cross_grad), bstride, _p(targets), _p(out), K, H, Q, Ni, _p(ws), need, _stream()),
          "mmx_detr_cross_rows")
    return out


def detr_raw_rows(cross_attn, targets):
    """Raw attention for all kept queries of one image: row ``targets[k]`` of the head mean of the last decoder layer's
    cross-attention slab ``[H, Q, Ni]`` (fp32) -> ``[K, Ni]``.  ``targets``: device ``[K]`` integers, clamped to ``0 .. Q - 1`` by the
    kernel.  One launch, nothing synchronises."""
    return _detr_cross_rows("detr_raw_rows", cross_attn, None, targets)


def detr_gradcam_rows(cross_attn, cross_grad, targets):
    """Attention GradCAM for all kept queries of one image: ``max(0, mean_h(P[h, t_k] * w[k, h]))`` with ``w[k, h]`` the mean of
    target k's gradient block ``[Q, Ni]`` of head h -> ``[K, Ni]``.  ``cross_grad``: ``[K * H, Q, Ni]``, or ``[H, Q, Ni]`` when one
    gradient slab serves every target.  Two launches."""
    return _detr_cross_rows("detr_gradcam_rows", cross_attn, cross_grad, targets)


def detr_rollout_rows(enc_attn_list, dec_self_attn_list, cross_attn, targets):
    """Rollout for all kept queries of one image: row ``targets[k]`` of ``R_qq^T . (mean_h cross_attn . R_ii)`` with ``R_ii`` / ``R_qq``
    the normalised rollouts of the encoder / decoder self-attention slabs (``[H, Ni, Ni]`` / ``[H, Q, Q]`` fp32, first layer first),
    carried as row vectors: no ``Ni x Ni`` product is formed -> ``[K, Ni]``.  See include/mmx_relevancy.h."""
    what = "detr_rollout_rows"
    P = _detr_slab(what, cross_attn)
    H, Q, Ni = P.shape
    enc = [_detr_slab(what, t, (Ni, Ni)) for t in enc_attn_list]
    dec = [_detr_slab(what, t, (Q, Q)) for t in dec_self_attn_list]
    if any(t.shape[0] != H for t in enc + dec):
        raise MMXError("%s: every slab needs the %d heads of the cross-attention slab" % (what, H))
    targets = _detr_targets(what, targets)
    K = targets.numel()
    need = lib().mmx_detr_rollout_rows_workspace_bytes(len(enc), len(dec), K, Q, Ni)
    if need == 0:
        raise MMXError("%s: needs 1..%d encoder and decoder slabs, Q <= 128 and Ni <= %d (got %d, %d, Q=%d, Ni=%d)"
                       % (what, _lib.BASELINES_MAX_TABLE, DETR_BASELINES_MAX_TOKENS, len(enc), len(dec), Q, Ni))
    out = torch.empty(K, Ni, dtype=torch.float32, device=P.device)
    et, _k0 = _lib.ptr_table([t.data_ptr() for t in enc])
    dt, _k1 = _lib.ptr_table([t.data_ptr() for t in dec])
    ws = _workspace(need, P.device, tag="detr_rollout_rows")        # grow-only scratch: pinned_state keeps it alive for graphs
    check(lib().mmx_detr_rollout_rows(et, len(enc), dt, len(dec), _p(P), _p(targets), _p(out), K, H, Q, Ni, _p(ws), need, _stream()),
          "mmx_detr_rollout_rows")
    return out
