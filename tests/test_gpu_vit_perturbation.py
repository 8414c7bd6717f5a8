"""-m gpu: the perturbation test for ViT and CLIP zero-shot maps (``vit_perturbation.py``) and its three kernels:
``mmx_patch_ranks``, ``mmx_perturb_patches`` and the attention forward without a capture slab, ``mmx_attn_fwd``.

One case of the long-sequence matrix below differs from the others: head_dim 80.  The fp32 capture forward serves head_dim <= 64
only (``check_attn_dims``: MMX_ENOTSUP beyond), and the no-capture forward serves the capture forward's shape space, so at 80 there
is no capture output to measure ``e_cap`` on; that case asserts the refusal of both entries.  The general tiled kernel (the one
that serves what the other two families do not) is covered by head_dim 50 instead (not a multiple of 4: neither the whole-head
nor the streaming kernels take it), with both conditions asserted.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402
from test_gpu_batch_images import _clip_inputs, _clip_models, _vit  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
H = 4


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    return _ops


def _guarded(shape, dtype=torch.float32):
    """A sentinel-filled buffer (NaN / INT_MIN) with GUARD elements after ``shape``'s elements: (view, guard, sentinel test)."""
    n = 1
    for s in shape:
        n *= s
    if dtype == torch.float32:
        buf = torch.full((n + GUARD,), float("nan"), device="cuda")
        return buf[:n].view(*shape), buf[n:], lambda g: bool(torch.isnan(g).all())
    buf = torch.full((n + GUARD,), -2 ** 31, dtype=dtype, device="cuda")
    return buf[:n].view(*shape), buf[n:], lambda g: bool((g == -2 ** 31).all())


def _cpu_ranks(scores):
    from transformer_mm_explainability_amd.lxmert_perturbation import _ranks, ranking
    return _ranks(ranking(scores))


def _cpu_perturb(images, ranks, counts, fill, patch):
    """The torch restatement: where(rank[patch of pixel] < counts[s], image, fill[c]) -> [S, B, C, R, R]."""
    B, C, R, _ = images.shape
    G = R // patch
    pix = ranks.view(B, G, G).repeat_interleave(patch, dim=1).repeat_interleave(patch, dim=2)          # [B, R, R]
    keep = pix.view(1, B, 1, R, R) < torch.as_tensor(counts).view(-1, 1, 1, 1, 1)
    return torch.where(keep, images.unsqueeze(0), fill.view(1, 1, C, 1, 1).expand(len(counts), B, C, R, R))


# ------------------------------------------------------------------------------------------------------------ 1. ranks
@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("P", [1, 16, 49, 196, 576, 1024, 4096])
@pytest.mark.parametrize("kind", ["random", "ties", "special"])
def test_patch_ranks_equal_stable_descending_sort(ops, B, P, kind):
    g = torch.Generator().manual_seed(P * 7 + B)
    x = torch.randn(B, P, generator=g)
    if kind == "ties":
        x = torch.floor(torch.rand(B, P, generator=g) * 8) / 8                      # 8 levels
    elif kind == "special":
        vals = [float("inf"), float("-inf"), 0.0, -0.0, float("nan"), -0.0, 0.0, float("nan"), float("inf")]
        for b in range(B):
            pos = torch.randperm(P, generator=g)[:len(vals)]
            for p, v in zip(pos.tolist(), vals):
                x[b, p] = v
    want = _cpu_ranks(x)
    out, guard, intact = _guarded((B, P), torch.int32)
    got = ops.patch_ranks(x.cuda(), out=out)
    again = ops.patch_ranks(x.cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.int32
    assert torch.equal(got.cpu().long(), want)
    assert torch.equal(again, got)
    assert intact(guard)
    # the positive test ranks the negated map (-NaN stays NaN)
    assert torch.equal(ops.patch_ranks(-x.cuda()).cpu().long(), _cpu_ranks(-x))


# ------------------------------------------------------------------------------------------------------------ 2. perturbed images
@pytest.mark.parametrize("R,patch", [(32, 8), (96, 16), (224, 16), (224, 32), (336, 14)])
@pytest.mark.parametrize("B", [1, 5])
def test_perturb_patches_equal_torch_restatement(ops, R, patch, B):
    S, C, P = 9, 3, (R // patch) ** 2
    g = torch.Generator().manual_seed(R + patch + B)
    images = torch.randn(B, C, R, R, generator=g)
    ranks = _cpu_ranks(torch.rand(B, P, generator=g))
    counts = [P, 0] + sorted(torch.randint(0, P + 1, (S - 2,), generator=g).tolist(), reverse=True)
    fill = torch.tensor([0.5, -1.25, 2.0])
    want = _cpu_perturb(images, ranks, counts, fill, patch)
    out, guard, intact = _guarded((S, B, C, R, R))
    got = ops.perturb_patches(images.cuda(), ranks.int().cuda(), torch.tensor(counts, dtype=torch.int32).cuda(), fill.cuda(), out=out)
    torch.cuda.synchronize()
    assert got.shape == (S, B, C, R, R)
    assert torch.equal(got.cpu(), want)
    assert intact(guard)
    assert torch.equal(got[0].cpu(), images) and bool((got[1].cpu() == fill.view(1, C, 1, 1)).all())


def test_perturb_patches_refuses_bad_arguments(ops):
    from transformer_mm_explainability_amd._lib import MMXError
    images = torch.randn(2, 3, 32, 32).cuda()
    counts = torch.tensor([16, 0], dtype=torch.int32).cuda()
    with pytest.raises(MMXError):
        ops.perturb_patches(images, torch.zeros(2, 15, dtype=torch.int32).cuda(), counts, torch.zeros(3).cuda())      # no square grid
    with pytest.raises(MMXError):
        ops.perturb_patches(images, torch.zeros(2, 9, dtype=torch.int32).cuda(), counts, torch.zeros(3).cuda())       # 3 does not divide 32
    with pytest.raises(MMXError):
        ops.perturb_patches(images, torch.zeros(2, 16, dtype=torch.int32).cuda(), counts, torch.zeros(2).cuda())      # fill per channel
    with pytest.raises(MMXError):
        ops.patch_ranks(torch.rand(2, 4097).cuda())


# ------------------------------------------------------------------------------------------------------------ 3. / 4. attention
def _qkv(B, N, heads, D, layout, seed):
    g = torch.Generator().manual_seed(seed)
    if layout == "bnhd":
        qkv = torch.randn(B, N, 3, heads, D, generator=g).cuda()
        return qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    return tuple(torch.randn(B, heads, N, D, generator=g).cuda() for _ in range(3))


def _mask(kind, B, N, seed):
    if kind == "none":
        return None
    if kind == "causal":
        return torch.full((N, N), float("-inf")).triu_(1).cuda()
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(B, 1, N)
    for b in range(B):
        m[b, 0, N - int(torch.randint(1, N // 2, (1,), generator=g)):] = float("-inf")
    if kind == "padding_one_dead":
        m[0] = float("-inf")                                                         # a fully masked sample: NaN rows
    return m.cuda()


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("N,mask_kind", [(17, "none"), (50, "none"), (77, "causal"), (128, "none"), (50, "padding_one_dead")])
@pytest.mark.parametrize("scale_mode", [0, 1])
def test_attn_fwd_short_is_bit_identical_to_capture(ops, N, mask_kind, B, D, layout, scale_mode):
    q, k, v = _qkv(B, N, H, D, layout, N * 31 + B + D)
    mask = _mask(mask_kind, B, N, N + B)
    scale = D ** -0.5 if scale_mode == 0 else D ** 0.5
    probs = torch.empty(B, H, N, N, device="cuda")
    want = ops.attn_capture_fwd(q, k, v, probs, scale, scale_mode, mask, layout=layout)
    out, guard, intact = _guarded(tuple(q.shape))
    got = ops.attn_fwd(q, k, v, scale, scale_mode, mask, layout=layout, out=out)
    torch.cuda.synchronize()
    nan_w, nan_g = torch.isnan(want), torch.isnan(got)
    assert torch.equal(nan_w, nan_g)
    assert torch.equal(got[~nan_g], want[~nan_w])                                    # bit for bit on every finite entry
    assert intact(guard)
    if mask_kind == "padding_one_dead":
        assert bool(nan_g[0].all()) and not bool(nan_g[1:].any())
    else:
        assert not bool(nan_g.any())
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def _attn64(q, k, v, scale, scale_mode, mask, layout):
    """The same attention in fp64 on the CPU -> O in q's layout."""
    q, k, v = (t.detach().cpu().double() for t in (q, k, v))
    if layout == "bnhd":
        q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    s = (q * scale) @ k.transpose(-1, -2) if scale_mode == 0 else (q @ k.transpose(-1, -2)) / scale
    if mask is not None:
        m = mask.detach().cpu().double()
        s = s + (m if m.dim() == 2 else m.unsqueeze(1))
    o = torch.softmax(s, dim=-1) @ v
    return o.permute(0, 2, 1, 3) if layout == "bnhd" else o


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("D", [32, 64, 50, 80])
@pytest.mark.parametrize("N", [129, 197, 257, 577])
@pytest.mark.parametrize("mask_kind", ["none", "padding"])
def test_attn_fwd_long_against_fp64(ops, N, D, B, mask_kind):
    """12 heads: at B = 8 every N runs the one-sweep streaming kernel (D 32 / 64), at B = 1 the small-grid kernel with the store
    compiled out; D = 50 runs the general tiled kernel; D = 80: see the module docstring."""
    from transformer_mm_explainability_amd._lib import MMXError
    heads = 12
    q, k, v = _qkv(B, N, heads, D, "bnhd", N * 13 + B + D)
    mask = _mask(mask_kind, B, N, N + D)
    scale = D ** -0.5
    if D > 64:
        with pytest.raises(MMXError):
            ops.attn_capture_fwd(q, k, v, torch.empty(B, heads, N, N, device="cuda"), scale, 0, mask)
        with pytest.raises(MMXError):
            ops.attn_fwd(q, k, v, scale, 0, mask)
        return
    o64 = _attn64(q, k, v, scale, 0, mask, "bnhd")
    o_cap = ops.attn_capture_fwd(q, k, v, torch.empty(B, heads, N, N, device="cuda"), scale, 0, mask)
    out, guard, intact = _guarded(tuple(q.shape))
    o_new = ops.attn_fwd(q, k, v, scale, 0, mask, out=out)
    again = ops.attn_fwd(q, k, v, scale, 0, mask)
    torch.cuda.synchronize()
    e_new = float((o_new.cpu().double() - o64).abs().max())
    e_cap = float((o_cap.cpu().double() - o64).abs().max())
    print("attn_fwd N=%d D=%d B=%d mask=%s: e_new %.3e e_cap %.3e" % (N, D, B, mask_kind, e_new, e_cap))
    parity.note("e_new", e_new, scale=float(o64.abs().max()))
    parity.note("e_cap", e_cap, scale=float(o64.abs().max()))
    assert intact(guard)
    assert torch.equal(again, o_new)
    parity.close(o_new, o64.float(), what="o_new_vs_fp64")
    assert e_new <= 2 * e_cap, (e_new, e_cap)


def test_attn_fwd_long_fully_masked_row_is_nan(ops):
    """A fully masked sample ends as NaN on the one-sweep kernel, like torch.softmax and the capture forward."""
    B, N, D, heads = 8, 197, 64, 12
    q, k, v = _qkv(B, N, heads, D, "bnhd", 5)
    mask = _mask("padding_one_dead", B, N, 3)
    want = ops.attn_capture_fwd(q, k, v, torch.empty(B, heads, N, N, device="cuda"), D ** -0.5, 0, mask)
    got = ops.attn_fwd(q, k, v, D ** -0.5, 0, mask)
    torch.cuda.synchronize()
    assert bool(torch.isnan(got[0]).all()) and not bool(torch.isnan(got[1:]).any())
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    parity.close(got[1:], want[1:], what="live_samples")


# ------------------------------------------------------------------------------------------------------------ 5. bodies
@pytest.mark.parametrize("cfg", [(96, 16, 128, 3, 2, 11), (224, 16, 192, 2, 3, 10)])
def test_vit_forward_nocapture_equals_tape_forward(cfg):
    model = _vit(*cfg).cuda()
    x = torch.randn(4, 3, cfg[0], cfg[0], generator=torch.Generator().manual_seed(2)).cuda()
    got = model.forward_nocapture(x)
    assert model.buffers_ is None                                                   # no capture slab was allocated
    want, _ = model.forward_tape(x, grads=False)
    torch.cuda.synchronize()
    assert got.shape == (4, cfg[5])
    parity.close(got, want, what="logits")
    tokens = model._embed(x)
    parity.close(model.forward_nocapture(tokens=tokens), want, what="logits_from_tokens")
    with pytest.raises(ValueError):
        model.forward_nocapture()


@pytest.mark.parametrize("which", ["tiny", "vitb32"])
def test_clip_encode_nocapture_equals_tape_forward(golden, which):
    cfg, model = _clip_models(golden, which)
    images, texts = _clip_inputs(cfg, 3, 4, 11)
    model = model.cuda()
    got = model.visual.encode_nocapture(images.cuda())
    assert model.visual.transformer.buffers is None
    text_f = model.encode_text_nocapture(texts.cuda())
    assert model.transformer.buffers is None
    want, _ = model.visual.forward_tape(images.cuda(), grads=False)
    want_t, _ = model.encode_text_tape(texts.cuda())
    torch.cuda.synchronize()
    parity.close(got, want, what="image_features")
    parity.close(text_f, want_t, what="text_features")
    y = model.visual.transformer.forward_nocapture(model.visual._embed(images.cuda()))          # all rows
    assert y.shape[:2] == (3, model.visual.positional_embedding.shape[0])


def test_nocapture_refuses_half_bodies(golden):
    from transformer_mm_explainability_amd._lib import MMXError
    from transformer_mm_explainability_amd import vit_perturbation as vp
    cfg, model = _clip_models(golden, "tiny")
    images, texts = _clip_inputs(cfg, 2, 3, 1)
    model = model.cuda()
    model.set_body_dtype(torch.bfloat16)
    with pytest.raises(MMXError, match="bfloat16"):
        model.visual.encode_nocapture(images.cuda())
    with pytest.raises(MMXError, match="bfloat16"):
        vp.ClipZeroShotScorer(model, texts.cuda())
    vit = _vit(96, 16, 128, 3, 2, 11).cuda().half()
    with pytest.raises(MMXError, match="float16"):
        vit.forward_nocapture(torch.randn(1, 3, 96, 96).cuda().half())


# ------------------------------------------------------------------------------------------------------------ 6. - 8. end to end
def _oracle_curves(logits, targets):
    prob = torch.softmax(logits, dim=-1)
    S, B, _ = logits.shape
    return prob.gather(2, targets.view(1, B, 1).expand(S, B, 1)).squeeze(2), prob


def _check_result(res, want_logits, labels, tag):
    """logits / target_prob with parity.close; pred == the oracle's arg-max wherever its top-2 probability gap >= 1e-4."""
    S, B, _ = want_logits.shape
    want_targets = want_logits[0].argmax(dim=-1)                     # step 0 keeps every patch: the unperturbed image
    want_tp, prob = _oracle_curves(want_logits, want_targets)
    assert res.logits.shape == want_logits.shape and res.target_prob.shape == (S, B) and res.pred.shape == (S, B)
    parity.close(res.logits, want_logits, what=tag + "_logits")
    assert torch.equal(res.targets.cpu(), want_targets)
    parity.close(res.target_prob, want_tp, what=tag + "_target_prob")
    top2 = prob.topk(2, dim=-1).values
    sure = (top2[..., 0] - top2[..., 1]) >= 1e-4
    print("%s: smallest top-2 gap %.3e, %d of %d cases compared" % (tag, float((top2[..., 0] - top2[..., 1]).min()),
                                                                     int(sure.sum()), S * B))
    assert int((~sure).sum()) <= 0.1 * S * B
    assert torch.equal(res.pred.cpu()[sure], want_logits.argmax(dim=-1)[sure])
    assert torch.equal(res.correct, res.pred == labels.cuda().view(1, B))
    assert torch.equal(res.accuracy, res.correct.float().mean(dim=1))


@pytest.mark.parametrize("cfg,seed", [((96, 16, 128, 3, 2, 11), 6), ((224, 16, 192, 2, 3, 10), 8)])
@pytest.mark.parametrize("positive", [False, True])
def test_vit_zero_mode_against_cpu_oracle(cfg, seed, positive):
    from oracle import vit_torch
    from transformer_mm_explainability_amd import vit_perturbation as vp
    img, patch, _, _, heads, classes = cfg
    B, P = 4, (img // patch) ** 2
    model = _vit(*cfg)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, img, img, generator=g)
    cam = torch.rand(B, P, generator=g)
    labels = torch.randint(0, classes, (B,), generator=g)
    fill = torch.tensor([0.25, -0.5, 0.0])
    model = model.cuda()
    pert = vp.PatchPerturbation(vp.VitScorer(model), fill=fill)
    res = pert(images.cuda(), cam.cuda(), labels=labels.cuda(), is_positive_pert=positive)
    assert model.buffers_ is None
    ranks = _cpu_ranks(-cam if positive else cam)
    x = _cpu_perturb(images, ranks, vp.step_counts(vp.PERT_STEPS, P), fill, patch)
    with torch.no_grad():
        want = torch.stack([vit_torch.forward(sd, x[s], heads)[0] for s in range(x.shape[0])])
    _check_result(res, want, labels, "vit_zero")
    # explicit targets: the probability of THAT class is followed
    res_t = pert(images.cuda(), cam.cuda(), targets=labels.cuda(), is_positive_pert=positive)
    parity.close(res_t.target_prob, _oracle_curves(want, labels)[0], what="vit_zero_given_targets")
    with pytest.raises(ValueError):
        pert(images.cuda(), cam.cuda()[:, :-1])


@pytest.mark.parametrize("positive", [False, True])
def test_clip_zero_mode_against_cpu_oracle(golden, positive):
    from oracle import clip_torch
    from transformer_mm_explainability_amd import vit_perturbation as vp
    cfg, model = _clip_models(golden, "tiny")
    images, texts = _clip_inputs(cfg, 5, 6, 23)
    sd = clip_torch.prepare_state_dict(model.state_dict(), cfg["transformer_heads"])
    patch = cfg["vision_patch_size"]
    P = (cfg["image_resolution"] // patch) ** 2
    g = torch.Generator().manual_seed(3)
    cam = torch.rand(5, P, generator=g)
    labels = torch.randint(0, 6, (5,), generator=g)
    model = model.cuda()
    pert = vp.PatchPerturbation(vp.ClipZeroShotScorer(model, texts.cuda()))
    res = pert(images.cuda(), cam.cuda(), labels=labels.cuda(), is_positive_pert=positive)
    assert model.visual.transformer.buffers is None
    x = _cpu_perturb(images, _cpu_ranks(-cam if positive else cam), vp.step_counts(vp.PERT_STEPS, P), torch.zeros(3), patch)
    with torch.no_grad():
        want = torch.stack([clip_torch.forward(sd, x[s], texts)[0] for s in range(x.shape[0])])
    _check_result(res, want, labels, "clip_zero")


def test_clip_vitb32_zero_mode_against_cpu_oracle(golden):
    from oracle import clip_torch
    from transformer_mm_explainability_amd import vit_perturbation as vp
    cfg, model = _clip_models(golden, "vitb32")
    images, texts = _clip_inputs(cfg, 1, 3, 29)
    sd = clip_torch.prepare_state_dict(model.state_dict(), cfg["transformer_heads"])
    patch, steps = cfg["vision_patch_size"], (0, 0.5)
    P = (cfg["image_resolution"] // patch) ** 2
    cam = torch.rand(1, P, generator=torch.Generator().manual_seed(4))
    labels = torch.tensor([1])
    model = model.cuda()
    res = vp.PatchPerturbation(vp.ClipZeroShotScorer(model, texts.cuda()), steps=steps)(images.cuda(), cam.cuda(), labels=labels.cuda())
    x = _cpu_perturb(images, _cpu_ranks(cam), vp.step_counts(steps, P), torch.zeros(3), patch)
    with torch.no_grad():
        want = torch.stack([clip_torch.forward(sd, x[s], texts)[0] for s in range(2)])
    _check_result(res, want, labels, "clip_vitb32_zero")


def _kept_rows(ranks, n):
    """Token rows of a step: the class token, then the n top-ranked patches in their original order -> [B, 1 + n]."""
    keep = [torch.nonzero(ranks[b] < n).flatten() + 1 for b in range(ranks.shape[0])]
    return torch.stack([torch.cat([torch.zeros(1, dtype=torch.long), kb]) for kb in keep])


def _vit_oracle_from_tokens(sd, x, heads):
    """oracle/vit_torch.forward from the position embedding on, over the given token rows ``x [B, n, E]``."""
    B, N, E = x.shape
    d = E // heads
    depth = len([k for k in sd if k.endswith(".attn.qkv.weight")])
    for l in range(depth):
        pre = "blocks.%d." % l
        h = F.layer_norm(x, (E,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], 1e-6)
        qkv = F.linear(h, sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]).reshape(B, N, 3, heads, d).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn = ((q @ k.transpose(-2, -1)) * (d ** -0.5)).softmax(dim=-1)
        o = (attn @ v).transpose(1, 2).reshape(B, N, E)
        x = x + F.linear(o, sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"])
        h = F.layer_norm(x, (E,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], 1e-6)
        h = F.gelu(F.linear(h, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"]))
        x = x + F.linear(h, sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"])
    x = F.layer_norm(x, (E,), sd["norm.weight"], sd["norm.bias"], 1e-6)
    return F.linear(x[:, 0], sd["head.weight"], sd["head.bias"])


@pytest.mark.parametrize("positive", [False, True])
def test_vit_drop_mode_against_token_subset_oracle(positive):
    from oracle import vit_torch
    from transformer_mm_explainability_amd import vit_perturbation as vp
    cfg = (96, 16, 128, 3, 2, 11)
    img, patch, _, _, heads, _ = cfg
    B, P = 4, (img // patch) ** 2
    model = _vit(*cfg)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(12)
    images = torch.randn(B, 3, img, img, generator=g)
    cam = torch.rand(B, P, generator=g)
    ranks = _cpu_ranks(-cam if positive else cam)
    with torch.no_grad():
        tok = F.conv2d(images, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=patch).flatten(2).transpose(1, 2)
        tok = torch.cat([sd["cls_token"].expand(B, -1, -1), tok], dim=1) + sd["pos_embed"]
        want = []
        for n in vp.step_counts(vp.PERT_STEPS, P):
            rows = _kept_rows(ranks, n)
            want.append(_vit_oracle_from_tokens(sd, torch.gather(tok, 1, rows.unsqueeze(-1).expand(B, n + 1, tok.shape[-1])), heads))
        want = torch.stack(want)
        full = vit_torch.forward(sd, images, heads)[0]
    model = model.cuda()
    res = vp.PatchPerturbation(vp.VitScorer(model), mode="drop")(images.cuda(), cam.cuda(), is_positive_pert=positive)
    assert model.buffers_ is None
    parity.close(res.logits, want, what="vit_drop_logits")
    # a step that keeps all P patches is the unperturbed image, in both modes
    parity.close(res.logits[0], full, what="vit_drop_keeps_all")
    zero = vp.PatchPerturbation(vp.VitScorer(model), mode="zero", fill=3.0)(images.cuda(), cam.cuda(), is_positive_pert=positive)
    parity.close(zero.logits[0], full, what="vit_zero_keeps_all")


def test_clip_drop_mode_against_token_subset_oracle(golden):
    from oracle import clip_torch
    from transformer_mm_explainability_amd import vit_perturbation as vp
    cfg, model = _clip_models(golden, "tiny")
    images, texts = _clip_inputs(cfg, 5, 6, 23)
    sd = clip_torch.prepare_state_dict(model.state_dict(), cfg["transformer_heads"])
    patch, B = cfg["vision_patch_size"], 5
    P = (cfg["image_resolution"] // patch) ** 2
    cam = torch.rand(B, P, generator=torch.Generator().manual_seed(7))
    ranks = _cpu_ranks(cam)
    width = sd["visual.conv1.weight"].shape[0]
    with torch.no_grad():
        full, _, _ = clip_torch.forward(sd, images, texts)
        # the oracle's forward, cut open after ln_pre: the image tower over the kept rows, the text side as it is
        x = F.conv2d(images, sd["visual.conv1.weight"], stride=patch).flatten(2).transpose(1, 2)
        x = torch.cat([sd["visual.class_embedding"].expand(B, 1, -1), x], dim=1) + sd["visual.positional_embedding"]
        x = clip_torch._layer_norm(x, sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"])
        ctx = sd["positional_embedding"].shape[0]
        t = F.embedding(texts, sd["token_embedding.weight"]) + sd["positional_embedding"]
        for l in range(clip_torch._n_layers(sd, "transformer.resblocks.")):
            t = clip_torch._block(sd, "transformer.resblocks.%d." % l, t, sd["__text_heads__"], torch.full((ctx, ctx), float("-inf")).triu_(1), [])
        t = clip_torch._layer_norm(t, sd["ln_final.weight"], sd["ln_final.bias"])
        tf = t[torch.arange(t.shape[0]), texts.argmax(dim=-1)] @ sd["text_projection"]
        tf = tf / tf.norm(dim=-1, keepdim=True)
        want = []
        for n in vp.step_counts(vp.PERT_STEPS, P):
            rows = _kept_rows(ranks, n)
            y = torch.gather(x, 1, rows.unsqueeze(-1).expand(B, n + 1, width))
            for l in range(clip_torch._n_layers(sd, "visual.transformer.resblocks.")):
                y = clip_torch._block(sd, "visual.transformer.resblocks.%d." % l, y, width // 64, None, [])
            f = clip_torch._layer_norm(y[:, 0, :], sd["visual.ln_post.weight"], sd["visual.ln_post.bias"]) @ sd["visual.proj"]
            f = f / f.norm(dim=-1, keepdim=True)
            want.append(sd["logit_scale"].exp() * f @ tf.t())
        want = torch.stack(want)
    model = model.cuda()
    scorer = vp.ClipZeroShotScorer(model, texts.cuda())
    res = vp.PatchPerturbation(scorer, mode="drop")(images.cuda(), cam.cuda())
    assert model.visual.transformer.buffers is None
    parity.close(res.logits, want, what="clip_drop_logits")
    parity.close(res.logits[0], full, what="clip_drop_keeps_all")
    zero = vp.PatchPerturbation(scorer, mode="zero", fill=-2.0)(images.cuda(), cam.cuda())
    parity.close(zero.logits[0], full, what="clip_zero_keeps_all")


# ------------------------------------------------------------------------------------------------------------ 9. determinism, chunks
@pytest.mark.parametrize("mode", ["zero", "drop"])
def test_determinism_and_chunking(mode):
    from transformer_mm_explainability_amd import vit_perturbation as vp
    cfg = (96, 16, 128, 3, 2, 11)
    model = _vit(*cfg).cuda()
    g = torch.Generator().manual_seed(21)
    images = torch.randn(4, 3, 96, 96, generator=g).cuda()
    cam = torch.rand(4, 36, generator=g).cuda()
    pert = vp.PatchPerturbation(vp.VitScorer(model), mode=mode)
    a, b = pert(images, cam), pert(images, cam)
    assert torch.equal(a.logits, b.logits) and torch.equal(a.target_prob, b.target_prob) and torch.equal(a.pred, b.pred)
    c = pert(images, cam, max_batch=7 if mode == "zero" else 3)                     # not a divisor of S * B = 36 resp. B = 4
    parity.close(c.logits, a.logits, what="chunked_logits")
    assert torch.equal(c.pred, a.pred)


# ------------------------------------------------------------------------------------------------------------ 10. pipeline
def test_pipeline_vit_relevance_batch_to_perturbation():
    from transformer_mm_explainability_amd import vit_model
    from transformer_mm_explainability_amd import vit_perturbation as vp
    cfg = (96, 16, 128, 3, 2, 11)
    model = _vit(*cfg).cuda()
    images = torch.randn(6, 3, 96, 96, generator=torch.Generator().manual_seed(30)).cuda()
    cam = vit_model.generate_relevance_batch(model, images)
    labels = torch.tensor([0, 1, 2, 3, 4, 5]).cuda()
    for mode in ("zero", "drop"):
        for positive in (False, True):
            res = vp.PatchPerturbation(vp.VitScorer(model), mode=mode)(images, cam, labels=labels, is_positive_pert=positive)
            S = len(vp.PERT_STEPS)
            assert res.logits.shape == (S, 6, 11) and res.target_prob.shape == (S, 6) and res.pred.shape == (S, 6)
            assert res.correct.shape == (S, 6) and res.accuracy.shape == (S,) and res.auc().shape == (6,)
            assert bool(torch.isfinite(res.logits).all()) and bool(torch.isfinite(res.target_prob).all())
            assert bool(torch.isfinite(res.auc()).all())


def test_pipeline_clip_interpret_batch_to_perturbation(golden):
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import vit_perturbation as vp
    cfg, model = _clip_models(golden, "tiny")
    images, texts = _clip_inputs(cfg, 6, 4, 31)
    model = model.cuda()
    ic, tc = images.cuda(), texts.cuda()
    cam = ce.interpret_batch(ic, tc, model, "cuda")
    scorer = vp.ClipZeroShotScorer(model, tc)
    for mode in ("zero", "drop"):
        res = vp.PatchPerturbation(scorer, mode=mode)(ic, cam, labels=torch.zeros(6, dtype=torch.long).cuda())
        S = len(vp.PERT_STEPS)
        assert res.logits.shape == (S, 6, 4) and res.accuracy.shape == (S,)
        assert bool(torch.isfinite(res.logits).all()) and bool(torch.isfinite(res.target_prob).all())


_GRAPH_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch
from transformer_mm_explainability_amd import ops
B, R, patch, S = 5, 96, 16, 9
P = (R // patch) ** 2
g = torch.Generator().manual_seed(40)
cam = torch.rand(B, P, generator=g).cuda()
images = torch.randn(B, 3, R, R, generator=g).cuda()
counts = torch.tensor([36, 27, 18, 9, 7, 5, 3, 1, 0], dtype=torch.int32).cuda()
fill = torch.tensor([0.1, 0.2, 0.3]).cuda()
ops.perturb_patches(images, ops.patch_ranks(cam), counts, fill)          # warm-up outside the capture
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with ops.graph_capture(graph):
    ranks = ops.patch_ranks(cam)
    out = ops.perturb_patches(images, ranks, counts, fill)
cam2 = torch.rand(B, P, generator=g).cuda()
images2 = torch.randn(B, 3, R, R, generator=g).cuda()
cam.copy_(cam2)
images.copy_(images2)
graph.replay()
torch.cuda.synchronize()
want_r = ops.patch_ranks(cam2)
want = ops.perturb_patches(images2, want_r, counts, fill)
torch.cuda.synchronize()
assert torch.equal(ranks, want_r), "ranks"
assert torch.equal(out, want), "perturbed images"
print("graphed zero-mode kernels ok")
"""


def test_zero_mode_kernels_replay_under_a_graph():
    """``patch_ranks`` + ``perturb_patches`` captured with ``ops.graph_capture`` replay bit-equal to eager on new inputs.  In a
    child process, like the other capture tests: a capture takes pool streams, and the suite's later multi-stream graphs are
    captured on whichever pool streams come next."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _GRAPH_CHILD, root], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "graphed zero-mode kernels ok" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
