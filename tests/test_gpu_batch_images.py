"""-m gpu: explaining a batch of DISTINCT images in one pass.

Kernel: the exact-fp32 row-relevancy mode of the capture backward (``mmx_attn_capture_bwd_rowrel_f32``; whole-head kernel for
N <= 128, streaming query-side kernel beyond) against the slab route it replaces (dP stored, then ``avg_heads_vecmat``).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

H, D = 4, 64
GUARD = 64


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    return _ops


def _guarded(shape):
    """A NaN-filled buffer with GUARD elements after ``shape``'s elements: (view, guard)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), float("nan"), device="cuda")
    return buf[:n].view(*shape), buf[n:]


def _inputs(N, B, causal, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, 3, H, D, generator=g).cuda()
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    mask = torch.full((N, N), float("-inf")).triu_(1).cuda() if causal else None
    return q, k, v, mask, (torch.randn(B, N, H, D, generator=g) * 1e-2).cuda(), torch.rand(B, N, generator=g).cuda()


def _slab_route(ops, q, k, v, probs, d_o, rel, need):
    B, N = rel.shape
    dprobs = torch.empty(B, H, N, N, device="cuda")
    res = ops.attn_capture_bwd(q, k, v, probs, d_o, dprobs, D ** -0.5, need_dqkv=need, o=None)
    row = ops.avg_heads_vecmat(rel, probs.view(B * H, N, N), dprobs.view(B * H, N, N), batch_size=B)
    return res, row


def _row_route(ops, q, k, v, probs, d_o, rel, need, dprobs=None):
    B, N = rel.shape
    bufs = [_guarded((B, N, H, D)) for _ in range(3)] if need else None
    res = ops.attn_capture_bwd(q, k, v, probs, d_o, dprobs, D ** -0.5, need_dqkv=need, rel_row=rel,
                               out=tuple(b[0] for b in bufs) if need else None)
    return res, bufs


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("N,causal", [(50, False), (77, True), (128, False), (129, False), (197, False), (257, False)])
@pytest.mark.parametrize("need", [True, False])
def test_rowrel_f32_equals_slab_route(ops, N, causal, B, need):
    q, k, v, mask, d_o, rel = _inputs(N, B, causal, N * 131 + B)
    probs = torch.empty(B, H, N, N, device="cuda")
    ops.attn_capture_fwd(q, k, v, probs, D ** -0.5, mask=mask)
    (dq0, dk0, dv0), want = _slab_route(ops, q, k, v, probs, d_o, rel, need)
    res, bufs = _row_route(ops, q, k, v, probs, d_o, rel, need)
    res2, bufs2 = _row_route(ops, q, k, v, probs, d_o, rel, need)
    torch.cuda.synchronize()
    row, row2 = res[3], res2[3]
    assert row.shape == (B, N) and torch.isfinite(row).all()
    top = float(want.abs().max())
    assert float((row - want).abs().max()) <= 1e-6 * top, (float((row - want).abs().max()), top)
    assert torch.equal(row, row2)                                           # deterministic reduction order
    if need:
        for (got, guard), (got2, _), ref in zip(bufs, bufs2, (dq0, dk0, dv0)):
            assert torch.equal(got, ref)                                    # the row is extra work, not another schedule
            assert torch.equal(got2, ref)
            assert torch.isnan(guard).all()


@pytest.mark.parametrize("N,causal", [(50, False), (77, True), (197, False)])
def test_rowrel_f32_keeps_dprobs_and_guard(ops, N, causal):
    """With a dprobs slab handed in, it holds the slab route's dP bit for bit and nothing past it is written."""
    B = 3
    q, k, v, mask, d_o, rel = _inputs(N, B, causal, N + 7)
    probs = torch.empty(B, H, N, N, device="cuda")
    ops.attn_capture_fwd(q, k, v, probs, D ** -0.5, mask=mask)
    want_dp = torch.empty(B, H, N, N, device="cuda")
    ops.attn_capture_bwd(q, k, v, probs, d_o, want_dp, D ** -0.5, need_dqkv=True)
    dp, guard = _guarded((B, H, N, N))
    _row_route(ops, q, k, v, probs, d_o, rel, True, dprobs=dp)
    torch.cuda.synchronize()
    assert torch.equal(dp, want_dp)
    assert torch.isnan(guard).all()


@pytest.mark.parametrize("N,causal", [(50, False), (77, True), (129, False), (197, False)])
@pytest.mark.parametrize("need", [True, False])
def test_rowrel_f32_nan_policy(ops, N, causal, need):
    """clamp(NaN, 0) is NaN, as on the slab route: a NaN planted in dO gives the same NaN pattern in the row."""
    B = 5
    q, k, v, mask, d_o, rel = _inputs(N, B, causal, N * 3 + 1)
    d_o[2, N // 3, 1, 5] = float("nan")
    probs = torch.empty(B, H, N, N, device="cuda")
    ops.attn_capture_fwd(q, k, v, probs, D ** -0.5, mask=mask)
    _, want = _slab_route(ops, q, k, v, probs, d_o, rel, need)
    res, _ = _row_route(ops, q, k, v, probs, d_o, rel, need)
    torch.cuda.synchronize()
    row = res[3]
    assert torch.isnan(want).any()
    assert torch.equal(torch.isnan(row), torch.isnan(want))
    ok = ~torch.isnan(want)
    assert float((row[ok] - want[ok]).abs().max()) <= 1e-6 * float(want[ok].abs().max())


def test_rowrel_f32_refuses_bad_arguments(ops):
    from transformer_mm_explainability_amd import _lib
    q, k, v, _, d_o, rel = _inputs(50, 2, False, 1)
    probs = torch.empty(2, H, 50, 50, device="cuda")
    ops.attn_capture_fwd(q, k, v, probs, D ** -0.5)
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_bwd(q, k, v, probs, d_o, None, D ** -0.5, rel_row=rel[:, :49])
    with pytest.raises(_lib.MMXError):
        ops.attn_capture_bwd(q, k, v, probs.half(), d_o, None, D ** -0.5, rel_row=rel)


# ------------------------------------------------------------------------------------------------------------ ViT
def _vit(img, patch, dim, depth, heads, classes, seed=0):
    from transformer_mm_explainability_amd import vit_model
    torch.manual_seed(seed)
    model = vit_model.VisionTransformer(img_size=img, patch_size=patch, embed_dim=dim, depth=depth, num_heads=heads,
                                        num_classes=classes).float().eval()
    with torch.no_grad():               # non-trivial biases / head, as in test_gpu_vit.py
        for p in model.parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.02)
        model.head.weight.mul_(10)
    return model


def _close(got, want):
    want = want.to(got.device)
    err = float((got - want).abs().max())
    assert err <= max(1e-5, 1e-4 * float(want.abs().max())), err


@pytest.mark.parametrize("img,patch,dim,depth,heads,classes", [(96, 16, 128, 3, 2, 11), (224, 16, 768, 12, 12, 1000)])
def test_vit_generate_relevance_batch(img, patch, dim, depth, heads, classes):
    """(96, 16): N = 37, whole-head kernel; (224, 16) is ViT-B/16, N = 197: the streaming kernels."""
    from oracle import vit_torch
    from transformer_mm_explainability_amd import vit_explainability as ve
    from transformer_mm_explainability_amd import vit_model
    B = 8
    model = _vit(img, patch, dim, depth, heads, classes)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(B, 3, img, img, generator=torch.Generator().manual_seed(5))
    indices = torch.tensor([3, 7, 0, 3, 10, 1, 7, 2])
    model = model.cuda()
    xc = x.cuda()
    got = vit_model.generate_relevance_batch(model, xc, indices.cuda())
    got_top = vit_model.generate_relevance_batch(model, xc)
    assert got.shape == (B, (img // patch) ** 2)
    for b in range(B):
        _close(got[b], ve.generate_relevance(model, xc[b:b + 1], index=int(indices[b])))
        _close(got_top[b], ve.generate_relevance(model, xc[b:b + 1]))
    for b in (range(B) if dim <= 128 else (0, 5)):      # the CPU oracle (two images at full size: slow there)
        want, _ = vit_torch.generate_relevance(sd, x[b:b + 1], heads, int(indices[b]))
        _close(got[b], want)
        want_top, _ = vit_torch.generate_relevance(sd, x[b:b + 1], heads, None)
        _close(got_top[b], want_top)


_GRAPH_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
from test_gpu_batch_images import _vit
from transformer_mm_explainability_amd import vit_model
B = 8
model = _vit(96, 16, 128, 3, 2, 11).cuda()
g = torch.Generator().manual_seed(9)
x1 = torch.randn(B, 3, 96, 96, generator=g).cuda()
x2 = torch.randn(B, 3, 96, 96, generator=g).cuda()
i1 = torch.tensor([1, 2, 3, 4, 5, 6, 7, 8]).cuda()
i2 = torch.tensor([0, 0, 9, 9, 1, 10, 4, 2]).cuda()
run = vit_model.GraphedRelevanceBatch(model, x1, indices=i1)
got = run(x2, i2).clone()
top = vit_model.GraphedRelevanceBatch(model, x1)
got_top = top(x2).clone()
torch.cuda.synchronize()
assert torch.equal(got, vit_model.generate_relevance_batch(model, x2, i2)), "indices"
assert torch.equal(got_top, vit_model.generate_relevance_batch(model, x2)), "arg-max"
print("graphed batch ok")
"""


def test_vit_graphed_relevance_batch_replays_new_images():
    """``GraphedRelevanceBatch`` replay on new images / classes (and with device-side arg-max classes) == the eager call.
    Runs in a child process: every capture takes pool streams (``ops.graph_capture``), and the suite's later multi-stream
    graphs (DETR, CLIP) are captured on whichever pool streams come next -- this test leaves that sequence as it was."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _GRAPH_CHILD, root], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "graphed batch ok" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])


# ------------------------------------------------------------------------------------------------------------ CLIP
def _clip_oracle_example(sd, image, texts, index):
    """CLIP/example.py:8-32 restated on the CPU oracle's forward (oracle/clip_torch.forward): one image, C prompts."""
    from oracle import clip_torch
    logits, img_probs, _ = clip_torch.forward(sd, image, texts)
    if index is None:
        index = int(logits[0].argmax())
    one_hot = torch.zeros_like(logits)
    one_hot[0, index] = 1
    grads = torch.autograd.grad(torch.sum(one_hot * logits), img_probs)
    n = img_probs[0].shape[-1]
    R = torch.eye(n)
    for a, g in zip(img_probs, grads):
        cam = (g.reshape(-1, n, n) * a.detach().reshape(-1, n, n)).clamp(min=0).mean(dim=0)
        R = R + cam @ R
    return R[0, 1:]


def _clip_inputs(cfg, B, C, seed):
    g = torch.Generator().manual_seed(seed)
    res, ctx, vocab = cfg["image_resolution"], cfg["context_length"], cfg["vocab_size"]
    images = torch.randn(B, 3, res, res, generator=g)
    texts = torch.zeros(C, ctx, dtype=torch.long)
    for c in range(C):
        n = 2 + (c * 3) % (ctx - 3)
        texts[c, 0] = vocab - 2
        texts[c, 1:1 + n] = torch.randint(1, vocab - 2, (n,), generator=g)
        texts[c, 1 + n] = vocab - 1                                     # EOT: the highest id
    return images, texts


def _clip_models(golden, which):
    from transformer_mm_explainability_amd import clip_model
    if which == "tiny":
        import json
        g = golden("clip_tiny")
        cfg = json.loads(str(g["cfg_json"]))
        model = clip_model.CLIP(**cfg).float().eval()
        model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w__")})
    else:
        model = clip_model.random_init("ViT-B/32", seed=0)
        names = ["embed_dim", "image_resolution", "vision_layers", "vision_width", "vision_patch_size", "context_length",
                 "vocab_size", "transformer_width", "transformer_heads", "transformer_layers"]
        cfg = dict(zip(names, clip_model.CONFIGS["ViT-B/32"]))
    return cfg, model


@pytest.mark.parametrize("which", ["tiny", "vitb32"])
def test_clip_interpret_batch(golden, which):
    from oracle import clip_torch
    from transformer_mm_explainability_amd import clip_example
    from transformer_mm_explainability_amd import clip_explainability as ce
    B, C = 6, 4
    cfg, model = _clip_models(golden, which)
    images, texts = _clip_inputs(cfg, B, C, 17)
    sd = clip_torch.prepare_state_dict(model.state_dict(), cfg["transformer_heads"])
    model = model.cuda()
    ic, tc = images.cuda(), texts.cuda()
    index = torch.tensor([0, 3, 1, 2, 3, 0])
    got = ce.interpret_batch(ic, tc, model, "cuda", index=index.cuda())
    got_top = ce.interpret_batch(ic, tc, model, "cuda")
    assert got.shape == (B, (cfg["image_resolution"] // cfg["vision_patch_size"]) ** 2)
    for b in range(B):
        single = ce.interpret_single(ic[b:b + 1], tc, model, "cuda", index=int(index[b]))
        _close(got[b], single)
        _close(got_top[b], ce.interpret_single(ic[b:b + 1], tc, model, "cuda"))
    for b in ((0, 4) if which == "vitb32" else range(B)):
        _close(got[b], _clip_oracle_example(sd, images[b:b + 1], texts, int(index[b])))
        _close(got_top[b], _clip_oracle_example(sd, images[b:b + 1], texts, None))
    assert all(p.grad is None for p in model.parameters())             # no weight gradients were computed
    assert torch.equal(clip_example.interpret(ic[2:3], tc, model, "cuda", index=1),
                       ce.interpret_single(ic[2:3], tc, model, "cuda", index=1))
