"""-m gpu: explaining K targets per image over a batch of DISTINCT images in one pass.

Kernel: the grouped exact-fp32 row mode of the capture backward (``mmx_attn_capture_bwd_rowrel_f32_grouped``: q / k / v / P / O
per image, everything else per target, target t explaining image t % M) against ``mmx_attn_capture_bwd_rowrel_f32`` on
materialised per-target copies -- bit for bit.  Then the ViT / CLIP entries built on it against per-image loops and the oracles.
"""
import pytest
import torch

from test_gpu_batch_images import _clip_inputs, _clip_models, _clip_oracle_example, _close, _guarded, _vit

pytestmark = pytest.mark.gpu

H, D = 4, 64


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    return _ops


def _inputs(N, M, K, causal, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(M, N, 3, H, D, generator=g).cuda()
    mask = torch.full((N, N), float("-inf")).triu_(1).cuda() if causal else None
    d_o = (torch.randn(K * M, N, H, D, generator=g) * 1e-2).cuda()
    return qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], mask, d_o, torch.rand(K * M, N, generator=g).cuda()


def _run(ops, q, k, v, probs, d_o, rel, need, o, **kw):
    T, N = rel.shape
    bufs = [_guarded((T, N, H, D)) for _ in range(3)] if need else None
    res = ops.attn_capture_bwd(q, k, v, probs, d_o, None, D ** -0.5, need_dqkv=need, rel_row=rel, o=o,
                               out=tuple(b[0] for b in bufs) if need else None, **kw)
    return res[3], bufs


def _same(a, b):
    (row_a, bufs_a), (row_b, bufs_b) = a, b
    assert torch.equal(row_a, row_b)
    if bufs_a is not None:
        for (x, gx), (y, gy) in zip(bufs_a, bufs_b):
            assert torch.equal(x, y)
            assert torch.isnan(gx).all() and torch.isnan(gy).all()          # nothing written past the outputs


@pytest.mark.parametrize("N,causal", [(50, False), (77, True), (128, False), (129, False), (197, False), (257, False)])
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("need", [True, False])
def test_grouped_equals_rowrel_f32_on_copies(ops, N, causal, M, K, need):
    q, k, v, mask, d_o, rel = _inputs(N, M, K, causal, N * 37 + M * 5 + K)
    probs = torch.empty(M, H, N, N, device="cuda")
    o = ops.attn_capture_fwd(q, k, v, probs, D ** -0.5, mask=mask)
    got = _run(ops, q, k, v, probs, d_o, rel, need, o, images=M)
    img = torch.arange(K * M, device="cuda") % M                            # K-major: target t explains image t % M
    want = _run(ops, q[img], k[img], v[img], probs[img].contiguous(), d_o, rel, need, o[img])
    torch.cuda.synchronize()
    assert got[0].shape == (K * M, N) and torch.isfinite(got[0]).all()
    _same(got, want)
    if K == 1:                                                              # the per-sample call on the images themselves
        _same(got, _run(ops, q, k, v, probs, d_o, rel, need, o))
    if M == 1:                                                              # the shared-forward (stride-0) call
        _same(got, _run(ops, q, k, v, probs, d_o, rel, need, o, batch=K))


@pytest.mark.parametrize("N,causal", [(50, False), (77, True), (197, False)])
@pytest.mark.parametrize("need", [True, False])
def test_grouped_nan_reaches_only_its_image(ops, N, causal, need):
    """clamp(NaN, 0) = NaN: a NaN planted in image 1's P shows up in exactly that image's K rows, as on the copies."""
    M, K = 3, 4
    q, k, v, mask, d_o, rel = _inputs(N, M, K, causal, N + 3)
    probs = torch.empty(M, H, N, N, device="cuda")
    o = ops.attn_capture_fwd(q, k, v, probs, D ** -0.5, mask=mask)
    probs[1, 2, N // 2, 3] = float("nan")
    row, _ = _run(ops, q, k, v, probs, d_o, rel, need, o, images=M)
    img = torch.arange(K * M, device="cuda") % M
    want, _ = _run(ops, q[img], k[img], v[img], probs[img].contiguous(), d_o, rel, need, o[img])
    torch.cuda.synchronize()
    assert torch.equal(torch.isnan(row).any(-1), img == 1)
    assert torch.equal(torch.isnan(row), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert torch.equal(row[ok], want[ok])


def test_grouped_refuses_bad_arguments(ops):
    import ctypes as C
    from transformer_mm_explainability_amd import _lib
    M, K, N = 2, 3, 50
    q, k, v, _, d_o, rel = _inputs(N, M, K, False, 1)
    probs = torch.empty(M, H, N, N, device="cuda")
    ops.attn_capture_fwd(q, k, v, probs, D ** -0.5)
    with pytest.raises(_lib.MMXError):                                      # q / probs batch is not `images`
        ops.attn_capture_bwd(q, k, v, probs, d_o, None, D ** -0.5, rel_row=rel, images=3)
    with pytest.raises(_lib.MMXError):                                      # 5 targets over 2 images
        ops.attn_capture_bwd(q, k, v, probs, d_o[:5], None, D ** -0.5, rel_row=rel[:5], images=M)
    with pytest.raises(_lib.MMXError):                                      # the grouped mode is a row mode
        ops.attn_capture_bwd(q, k, v, probs, d_o, torch.empty(K * M, H, N, N, device="cuda"), D ** -0.5, images=M)
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_bwd(q, k, v, probs, d_o, None, D ** -0.5, rel_row=rel[:, :49], images=M)
    with pytest.raises(_lib.MMXError):                                      # exact fp32 only
        ops.attn_capture_bwd(q, k, v, probs, d_o, None, D ** -0.5, rel_row=rel, images=M, mma_bf16=True)
    h = _lib.lib()
    p = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731
    ws = torch.empty(h.mmx_attn_capture_bwd_rowrel_f32_grouped_workspace_bytes(K * M, H, N, N), dtype=torch.uint8,
                     device="cuda")
    out = torch.empty_like(rel)
    s = (N * 3 * H * D, D, 3 * H * D)
    so = (N * H * D, D, H * D)
    for T, n_img in ((K * M, 0), (K * M, 4), (5, M)):
        rc = h.mmx_attn_capture_bwd_rowrel_f32_grouped(
            p(q), p(k), p(v), *s, *s, *s, p(probs), H * N * N, 0, p(d_o), *so, None, 0, 0, 0, None, None, None, None,
            0, 0, 0, 0, 0, 0, 0, 0, 0, T, H, N, N, D, C.c_float(D ** -0.5), 1, 0, p(rel), p(out), n_img, p(ws), ws.numel(), None)
        assert rc == -22, (T, n_img, rc)


# ------------------------------------------------------------------------------------------------------------ ViT
@pytest.mark.parametrize("img,patch,dim,depth,heads,classes", [(96, 16, 128, 3, 2, 11), (224, 16, 768, 12, 12, 1000)])
def test_vit_generate_relevance_batch_multi(img, patch, dim, depth, heads, classes):
    """(96, 16): N = 37, whole-head kernel; (224, 16) is ViT-B/16, N = 197: the streaming kernels."""
    from oracle import vit_torch
    from transformer_mm_explainability_amd import vit_model
    B, K = 4, 3
    model = _vit(img, patch, dim, depth, heads, classes)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(6))
    indices = torch.tensor([[3, 7, 0], [10, 1, 3], [2, 2, 9], [0, 5, 8]])
    model = model.cuda()
    xc, ic = x.cuda(), indices.cuda()
    got = vit_model.generate_relevance_batch_multi(model, xc, ic)
    assert got.shape == (B, K, (img // patch) ** 2)
    for b in range(B):
        _close(got[b], vit_model.generate_relevance_multi(model, xc[b:b + 1], ic[b]))
    for b, k in (((0, 1), (2, 2)) if dim <= 128 else ((1, 0),)):          # the CPU oracle (one map at full size: slow there)
        want, _ = vit_torch.generate_relevance(sd, x[b:b + 1], heads, int(indices[b, k]))
        _close(got[b, k], want)
    logits, _ = model.forward_tape(xc, grads=False)
    top = logits.topk(K, dim=-1).indices
    assert torch.equal(vit_model.generate_relevance_batch_multi(model, xc, top_k=K),
                       vit_model.generate_relevance_batch_multi(model, xc, top))
    assert torch.equal(vit_model.generate_relevance_batch_multi(model, xc, ic[:, :1])[:, 0],
                       vit_model.generate_relevance_batch(model, xc, ic[:, 0]))


_GRAPH_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
from test_gpu_batch_images import _vit
from transformer_mm_explainability_amd import vit_model
B, K = 4, 3
model = _vit(96, 16, 128, 3, 2, 11).cuda()
g = torch.Generator().manual_seed(19)
x1 = torch.randn(B, 3, 96, 96, generator=g).cuda()
x2 = torch.randn(B, 3, 96, 96, generator=g).cuda()
i1 = torch.tensor([[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 0, 1]]).cuda()
i2 = torch.tensor([[0, 0, 9], [9, 1, 10], [4, 2, 2], [3, 3, 3]]).cuda()
run = vit_model.GraphedRelevanceBatchMulti(model, x1, indices=i1)
got = run(x2, i2).clone()
top = vit_model.GraphedRelevanceBatchMulti(model, x1, top_k=K)
got_top = top(x2).clone()
torch.cuda.synchronize()
assert got.shape == (B, K, 36)
assert torch.equal(got, vit_model.generate_relevance_batch_multi(model, x2, i2)), "indices"
assert torch.equal(got_top, vit_model.generate_relevance_batch_multi(model, x2, top_k=K)), "top_k"
print("graphed batch multi ok")
"""


def test_vit_graphed_relevance_batch_multi_replays_new_images():
    """``GraphedRelevanceBatchMulti`` replay on new images / classes (and with device-side top-K classes) == the eager call.
    In a child process, as test_gpu_batch_images.py's graph test (the suite's later multi-stream graphs keep their streams)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _GRAPH_CHILD, root], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "graphed batch multi ok" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])


# ------------------------------------------------------------------------------------------------------------ CLIP
@pytest.mark.parametrize("which", ["tiny", "vitb32"])
def test_clip_interpret_batch_multi(golden, which):
    from oracle import clip_torch
    from transformer_mm_explainability_amd import clip_explainability as ce
    B, C, K = 5, 6, 3
    cfg, model = _clip_models(golden, which)
    images, texts = _clip_inputs(cfg, B, C, 23)
    sd = clip_torch.prepare_state_dict(model.state_dict(), cfg["transformer_heads"])
    model = model.cuda()
    ic, tc = images.cuda(), texts.cuda()
    index = torch.tensor([[0, 3, 5], [1, 2, 0], [4, 4, 1], [5, 0, 2], [3, 1, 4]])
    got = ce.interpret_batch_multi(ic, tc, model, "cuda", index=index.cuda())
    assert got.shape == (B, K, (cfg["image_resolution"] // cfg["vision_patch_size"]) ** 2)
    for k in range(K):
        _close(got[:, k], ce.interpret_batch(ic, tc, model, "cuda", index=index[:, k].cuda()))
    assert torch.equal(ce.interpret_batch_multi(ic, tc, model, "cuda", index=index[:, :1].cuda())[:, 0],
                       ce.interpret_batch(ic, tc, model, "cuda", index=index[:, 0].cuda()))
    for b, k in (((0, 2),) if which == "vitb32" else ((0, 1), (3, 2), (4, 0))):
        _close(got[b, k], _clip_oracle_example(sd, images[b:b + 1], texts, int(index[b, k])))
    got_top = ce.interpret_batch_multi(ic, tc, model, "cuda", top_k=K)
    assert got_top.shape == got.shape and torch.isfinite(got_top).all()
    _close(got_top[:, 0], ce.interpret_batch(ic, tc, model, "cuda"))      # the best prompt first
    assert all(p.grad is None for p in model.parameters())             # no weight gradients were computed


@pytest.mark.parametrize("which,start", [("tiny", -1), ("tiny", 0), ("vitb32", 0)])
def test_clip_interpret_grouped(golden, which, start):
    """K captions per image: equals the notebook's ``interpret`` on the images repeated K times each (two towers, per-caption
    text relevancy), and the CPU oracle per image with that image's captions."""
    from oracle import clip_torch
    from transformer_mm_explainability_amd import clip_explainability as ce
    M, K = 3, 2
    cfg, model = _clip_models(golden, which)
    images, texts = _clip_inputs(cfg, M, M * K, 29)
    sd = clip_torch.prepare_state_dict(model.state_dict(), cfg["transformer_heads"])
    model = model.cuda()
    ic, tc = images.cuda(), texts.cuda()
    R_text, R_image = ce.interpret_grouped(ic, tc, model, "cuda", start_layer=start, start_layer_text=start)
    want_text, want_image = ce.interpret(ic.repeat_interleave(K, 0), tc, model, "cuda", start, start, share_image_forward=False)
    assert R_text.shape == want_text.shape and R_image.shape == want_image.shape
    _close(R_text, want_text)
    _close(R_image, want_image)
    for m in (range(M) if which == "tiny" else (1,)):
        ot, oi = clip_torch.interpret(sd, images[m:m + 1], texts[m * K:(m + 1) * K], start, start)
        _close(R_text[m * K:(m + 1) * K], ot)
        _close(R_image[m * K:(m + 1) * K], oi)


def test_batch_targets_refusals(golden):
    from transformer_mm_explainability_amd import _lib
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import vit_model
    model = _vit(96, 16, 128, 3, 2, 11).cuda()
    x = torch.randn(2, 3, 96, 96, device="cuda")
    for bad in (torch.tensor([1, 2]), torch.tensor([[1, 2]]), torch.tensor([[[1]], [[2]]])):
        with pytest.raises(ValueError):
            vit_model.generate_relevance_batch_multi(model, x, bad.cuda())
    model.backward_gemm_dtype = torch.bfloat16
    with pytest.raises(_lib.MMXError, match="bfloat16"):
        vit_model.generate_relevance_batch_multi(model, x, top_k=2)
    model.backward_gemm_dtype = torch.float32
    cfg, clip = _clip_models(golden, "tiny")
    images, texts = _clip_inputs(cfg, 2, 4, 3)
    clip = clip.cuda()
    ic, tc = images.cuda(), texts.cuda()
    with pytest.raises(ValueError):
        ce.interpret_batch_multi(ic, tc, clip, "cuda", index=torch.tensor([[0, 1], [1, 2], [2, 3]]).cuda())
    with pytest.raises(ValueError):
        ce.interpret_batch_multi(ic, tc, clip, "cuda", index=torch.tensor([0, 1]).cuda())
    with pytest.raises(ValueError):
        ce.interpret_grouped(ic, tc[:3], clip, "cuda")
    clip.set_body_dtype(torch.bfloat16)
    try:
        with pytest.raises(_lib.MMXError, match="bfloat16"):
            ce.interpret_batch_multi(ic, tc, clip, "cuda", top_k=2)
        with pytest.raises(_lib.MMXError, match="bfloat16"):
            ce.interpret_grouped(ic, tc, clip, "cuda")
    finally:
        clip.set_body_dtype(torch.float32)
