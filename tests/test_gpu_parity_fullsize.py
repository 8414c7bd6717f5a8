"""-m gpu: parity against the ORACLE at the sizes BASELINE.json measures (VERDICT r01 "next" item 1).

  * cfg 2 exactly as ``bench.py`` runs it: CLIP ViT-B/32, batch 64, all 12+12 layers, bench.py's seeds -- eager with
    the shared image forward, eager with B image copies, and the hipGraph replay, each vs ``oracle/clip_torch.interpret``
    (the notebook algorithm: one ``autograd.grad`` per layer) at 1e-5;
  * cfg 5's token count (ViT-L/14@336: 577 image tokens, 16 heads; the streaming attention kernels and the N > 128
    chain), reduced depth/batch so the CPU oracle finishes in seconds;
  * cfg 3's DETR encoder size (Ni = 25x38 = 950, d = 32, 8 heads; 100 queries): the capture op vs
    ``oracle/attention_torch`` and the rule schedule vs ``oracle/relevancy_np.detr_generate_ours_chain`` on the slabs.
Tolerances are the north star's: relevancy maps 1e-5 abs; probabilities 2e-6, gradients 2e-5.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


from parity import close  # noqa: E402  (atol only: rtol = 0)


def bench_inputs(batch, seed=0, context=77, vocab_hi=49405, sot=49406, eot=49407, res=224):
    """``bench.synthetic_inputs`` restated (bench.py sets process-wide TunableOp env at import, so it is not imported)."""
    g = torch.Generator().manual_seed(1 + seed)
    image = torch.randn(1, 3, res, res, generator=g)
    texts = torch.zeros(batch, context, dtype=torch.long)
    g2 = torch.Generator().manual_seed(2 + seed)
    for b in range(batch):
        n = int(torch.randint(3, 11, (1,), generator=g2))
        texts[b, 0] = sot
        texts[b, 1:1 + n] = torch.randint(1, vocab_hi, (n,), generator=g2)
        texts[b, 1 + n] = eot
    return image, texts


def test_cfg2_batch64_vs_oracle():
    """The measured configuration at its own size: every map of the 64-pair batch within 1e-5 of the oracle, for all
    three ways bench.py can run the step (layer-group split G = 4 and the shared-forward backward at B = 64 included)."""
    from oracle import clip_torch
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import clip_model
    model = clip_model.random_init("ViT-B/32", seed=0)
    image, texts = bench_inputs(64)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    sd = clip_torch.prepare_state_dict(model.state_dict(), 8)
    want_text, want_img = clip_torch.interpret(sd, image, texts, 0, 0)
    model = model.cuda()
    image, texts = image.cuda(), texts.cuda()
    for share in (True, False):
        R_text, R_image = ce.interpret(image, texts, model, "cuda", 0, 0, share_image_forward=share)
        close(R_text, want_text, what="R_text")
        close(R_image, want_img, what="R_image")
    run = ce.GraphedInterpret(model, image, texts, start_layer=0, start_layer_text=0)
    R_text, R_image = run()
    close(R_text, want_text, what="R_text")
    close(R_image, want_img, what="R_image")
    run_ns = ce.GraphedInterpret(model, image, texts, start_layer=0, start_layer_text=0, share_image_forward=False)
    R_text, R_image = run_ns()
    close(R_text, want_text, what="R_text")
    close(R_image, want_img, what="R_image")


def test_fp16_mode_at_vit_b32_vs_the_references_fp16_model(golden):
    """The reference's own half-precision mode at the headline geometry (CLIP ViT-B/32, all 12 + 12 layers, B = 8):
    ``set_body_dtype(torch.float16)`` vs the reference's model after ``convert_weights`` + notebook cell 6 (fixture
    clip_vitb32_fp16.npz: made on the CPU by tests/golden/make_golden.py from the same ``random_init`` weights and inputs; it also
    holds the reference's fp32 result).  Bar: 6e-3 of the largest off-diagonal entry of the map -- the reference's fp16 and fp32
    results are themselves 2e-3 (text) / 1.5e-3 (image) apart; our body keeps the residual stream in fp32, so it lands between
    them.  The hipGraph replay reproduces the eager call bit for bit."""
    import faulthandler
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import clip_model
    faulthandler.dump_traceback_later(300, exit=False)                # a stall here names its line in the log (does not stop the run)
    try:
        g = golden("clip_vitb32_fp16")
        model = clip_model.random_init("ViT-B/32", seed=0).cuda()
        image, texts = bench_inputs(8)
        assert torch.equal(texts, torch.from_numpy(g["texts"]))
        model.set_body_dtype(torch.float16)
        got = ce.interpret(image.cuda(), texts.cuda(), model, "cuda", 0, 0)
        torch.cuda.synchronize()
        assert got[0].dtype == torch.float16 and got[1].dtype == torch.float16
        off = torch.eye(77, dtype=torch.bool).logical_not()
        errs = {}
        for k, name in enumerate(("R_text", "R_image")):
            for tag in ("fp16", "fp32"):
                w, g_ = torch.from_numpy(g[name + "_" + tag]).float(), got[k].float().cpu()
                if k == 0:
                    w, g_ = w[:, off], g_[:, off]                      # (the unit diagonal would set the scale)
                errs[(name, tag)] = float((g_ - w).abs().max()) / float(w.abs().max())
                assert errs[(name, tag)] <= 6e-3, (name, tag, errs)
        print("fp16 mode, relative errors:", errs, flush=True)
        run = ce.GraphedInterpret(model, image.cuda(), texts.cuda(), start_layer=0, start_layer_text=0)
        R_text, R_image = run()
        torch.cuda.synchronize()
        assert torch.equal(R_text, got[0]) and torch.equal(R_image, got[1])
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_cfg5_token_count_vs_oracle():
    """ViT-L/14@336 geometry (577 image tokens, width 1024 / 16 heads; text width 768 / 12 heads), 2 + 2 layers, B = 2."""
    from oracle import clip_torch
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import clip_model
    torch.manual_seed(0)
    model = clip_model.CLIP(768, 336, 2, 1024, 14, 77, 49408, 768, 12, 2).float().eval()
    image, texts = bench_inputs(2, res=336)
    sd = clip_torch.prepare_state_dict(model.state_dict(), 12)
    want_text, want_img = clip_torch.interpret(sd, image, texts, 0, 0)
    assert want_img.shape == (2, 576)
    model = model.cuda()
    for share in (True, False):
        R_text, R_image = ce.interpret(image.cuda(), texts.cuda(), model, "cuda", 0, 0, share_image_forward=share)
        close(R_text, want_text, what="R_text")
        close(R_image, want_img, what="R_image")


def test_cfg5_bf16_body_vs_oracle():
    """BASELINE config 5's bf16 body (``CLIP.set_body_dtype(torch.bfloat16)``: GEMMs and the image tower's attention
    products on the bf16 matrix cores, fp32 accumulation, fp32 LayerNorm / softmax / relevancy) at the ViT-L/14@336
    geometry, 3 + 2 layers, B = 3, vs the fp32 oracle.  Stated tolerance (bf16 has 8 significant bits and the maps are
    products of ~1e-3-sized gradients through the layers): per sample max |diff| <= 3e-2 * max |map| and cosine
    similarity >= 0.999.  The row-relevancy mode (no gradient slab; the class-token row of R carried through the
    backward) must agree with the slab + chain route of the same bf16 body to 2e-3 of max |map| (they differ by the
    slab's bf16 rounding of dP only), and a hipGraph replay must reproduce the eager call bit for bit."""
    from oracle import clip_torch
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import clip_model
    torch.manual_seed(0)
    model = clip_model.CLIP(768, 336, 3, 1024, 14, 77, 49408, 768, 12, 2).float().eval()
    image, texts = bench_inputs(3, res=336)
    sd = clip_torch.prepare_state_dict(model.state_dict(), 12)
    want_text, want_img = clip_torch.interpret(sd, image, texts, 0, 0)
    model = model.cuda()
    model.set_body_dtype(torch.bfloat16)
    assert model.visual.row_relevancy_ok()
    R_text, R_image = ce.interpret(image.cuda(), texts.cuda(), model, "cuda", 0, 0)
    assert model.visual.transformer.buffers.grads is None            # row mode: no gradient slab was allocated

    def near(got, want, tol, cos_min):
        got, want = got.float().cpu().reshape(got.shape[0], -1), want.float().reshape(want.shape[0], -1)
        for b in range(got.shape[0]):
            assert float((got[b] - want[b]).abs().max()) <= tol * float(want[b].abs().max())
            assert float(torch.nn.functional.cosine_similarity(got[b], want[b], dim=0)) >= cos_min

    near(R_image, want_img, 3e-2, 0.999)
    off = torch.eye(77, dtype=torch.bool).logical_not()
    near(R_text[:, off], want_text[:, off], 3e-2, 0.999)
    row = R_image.clone()
    model.visual.row_relevancy_ok = lambda: False                    # slab + chain route of the same bf16 body
    _, R_slab = ce.interpret(image.cuda(), texts.cuda(), model, "cuda", 0, 0)
    assert model.visual.transformer.buffers.grads is not None
    near(row, R_slab.cpu(), 2e-3, 0.99999)
    del model.visual.row_relevancy_ok
    run = ce.GraphedInterpret(model, image.cuda(), texts.cuda(), start_layer=0, start_layer_text=0)
    _, R_graph = run()
    assert torch.equal(R_graph, row)


def _cfg5_model(vision_layers, text_layers=12, seed=0):
    from transformer_mm_explainability_amd import clip_model
    torch.manual_seed(seed)
    return clip_model.CLIP(768, 336, vision_layers, 1024, 14, 77, 49408, 768, 12, text_layers).float().eval()


_CFG5_ORACLE = {}


def _cfg5_oracle(vision_layers, text_layers, batch):
    """fp32 CPU oracle maps of the ViT-L/14@336 architecture at the given depth (cached per session: the fp32 and the
    bf16 test of one depth share it)."""
    from oracle import clip_torch
    key = (vision_layers, text_layers, batch)
    if key not in _CFG5_ORACLE:
        model = _cfg5_model(vision_layers, text_layers)
        image, texts = bench_inputs(batch, res=336)
        torch.set_num_threads(min(32, torch.get_num_threads()))
        sd = clip_torch.prepare_state_dict(model.state_dict(), 12)
        _CFG5_ORACLE[key] = clip_torch.interpret(sd, image, texts, 0, 0)
    return _CFG5_ORACLE[key]


def test_cfg5_full_depth_fp32_vs_oracle():
    """BASELINE config 5's architecture at its REAL depth --
    ``CLIP(768, 336, 24, 1024, 14, 77, 49408, 768, 12, 12)`` (CLIP/clip/model.py:405-428 sizes), B = 2, all 24 + 12 layers --
    on the exact fp32 path (streaming attention kernels at N = 577, split chain) vs ``oracle/clip_torch.interpret`` at the
    north star's 1e-5 absolute, shared image forward and B copies."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    want_text, want_img = _cfg5_oracle(24, 12, 2)
    model = _cfg5_model(24, 12).cuda()
    image, texts = bench_inputs(2, res=336)
    for share in (True, False):
        R_text, R_image = ce.interpret(image.cuda(), texts.cuda(), model, "cuda", 0, 0, share_image_forward=share)
        close(R_text, want_text, what="R_text")
        close(R_image, want_img, what="R_image")


# measured on an MI355X (profiles/r03_parity.json, keys ``...bf16_error_by_depth[L]::R_image_rel`` / ``R_text_rel``): the bf16
# body's error relative to max |map| is 5.3e-3 / 4.0e-3 / 2.8e-3 / 2.3e-3 at L = 3 / 6 / 12 / 24 image-tower layers (text
# tower: 3.4e-3 .. 4.2e-3) -- it does NOT grow with depth on these inputs (the map is dominated by the top layers, whose
# gradients have passed through the fewest bf16 roundings); cosine distance <= 4.2e-6.  Bound = ~3x the measured value.
CFG5_BF16_REL_BOUND = {3: 1.5e-2, 6: 1.2e-2, 12: 1.0e-2, 24: 1.0e-2}


@pytest.mark.parametrize("depth", [3, 6, 12, 24])
def test_cfg5_bf16_error_by_depth(depth):
    """the bf16 body (what ``bench.py --workload cfg5`` times) vs the fp32 oracle as a CURVE over the
    image tower's depth (text tower at its real 12 layers, B = 2): per sample max |diff| / max |map| and the cosine
    similarity are recorded per depth (``parity.note``) and bounded by ``CFG5_BF16_REL_BOUND``."""
    from parity import note
    from transformer_mm_explainability_amd import clip_explainability as ce
    want_text, want_img = _cfg5_oracle(depth, 12, 2)
    model = _cfg5_model(depth, 12).cuda()
    model.set_body_dtype(torch.bfloat16)
    image, texts = bench_inputs(2, res=336)
    R_text, R_image = ce.interpret(image.cuda(), texts.cuda(), model, "cuda", 0, 0)
    off = torch.eye(77, dtype=torch.bool).logical_not()
    worst = {}
    for name, got, want in (("R_image", R_image.float().cpu(), want_img), ("R_text", R_text.float().cpu()[:, off], want_text[:, off])):
        got, want = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
        rel = max(float((got[b] - want[b]).abs().max() / want[b].abs().max()) for b in range(got.shape[0]))
        cos = min(float(torch.nn.functional.cosine_similarity(got[b], want[b], dim=0)) for b in range(got.shape[0]))
        note(name + "_rel", rel)
        note(name + "_one_minus_cos", 1.0 - cos)
        worst[name] = (rel, cos)
    assert worst["R_image"][0] <= CFG5_BF16_REL_BOUND[depth] and worst["R_image"][1] >= 0.9999, worst
    assert worst["R_text"][0] <= 1.2e-2 and worst["R_text"][1] >= 0.9999, worst


def test_cfg5_graph_replay_after_other_interpret():
    """a captured row-relevancy graph (bf16 body: probabilities-only buffers, ``grads is None``) must
    re-install its pinned slabs when another interpret() with a different batch replaced them in between."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    model = _cfg5_model(2, 2).cuda()
    model.set_body_dtype(torch.bfloat16)
    image, texts = bench_inputs(3, res=336)
    image, texts = image.cuda(), texts.cuda()
    run = ce.GraphedInterpret(model, image, texts, start_layer=0, start_layer_text=0)
    first = [t.clone() for t in run()]
    ce.interpret(image, texts[:2], model, "cuda", 0, 0)                 # another batch size: new slabs on both towers
    again = run()
    assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    assert model.visual.transformer.resblocks[0].attn_grad is None      # probabilities-only buffers: no gradient view


@pytest.mark.parametrize("Nq,Nk", [(950, 950), (100, 950), (577, 577)])
def test_capture_op_at_size_vs_oracle(Nq, Nk):
    """The capture op at the DETR-encoder / DETR-cross / ViT-L token counts vs the oracle's hooked attention core."""
    from oracle import attention_torch as oat
    from transformer_mm_explainability_amd import ops
    H, D = (8, 32) if Nk == 950 else (4, 64)
    g = torch.Generator().manual_seed(Nq + Nk)
    q, k, v, d_o = (torch.randn(1, n, H, D, generator=g) for n in (Nq, Nk, Nk, Nq))
    bh = lambda t: t.permute(0, 2, 1, 3)
    P, O, dP, dq, dk, dv = oat.capture(bh(q), bh(k), bh(v), bh(d_o), D ** -0.5)
    probs = torch.empty(1, H, Nq, Nk, device="cuda")
    dprobs = torch.empty_like(probs)
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    o = ops.attn_capture_fwd(qc, kc, vc, probs, D ** -0.5)
    close(probs, P, atol=2e-6, rtol=1e-4, what="intermediate")
    close(bh(o), O, rtol=1e-4, what="intermediate")
    gq, gk, gv = ops.attn_capture_bwd(qc, kc, vc, probs, d_o.cuda(), dprobs, D ** -0.5, o=o)
    close(dprobs, dP, atol=2e-5, rtol=1e-4, what="intermediate")
    close(bh(gq), dq, atol=2e-5, rtol=1e-4, what="intermediate")
    close(bh(gk), dk, atol=2e-5, rtol=1e-4, what="intermediate")
    close(bh(gv), dv, atol=2e-5, rtol=1e-4, what="intermediate")


@pytest.mark.parametrize("Nq,Nk,slab", [(577, 577, torch.bfloat16), (577, 577, torch.float32), (100, 950, torch.bfloat16),
                                        (200, 130, torch.float32)])
def test_capture_op_bf16_matrix_cores_vs_oracle(Nq, Nk, slab):
    """``MMX_ATTN_MMA_BF16`` (BASELINE config 5's bf16 body): attention products on v_mfma_f32_16x16x32_bf16, operands
    rounded to bf16 as they are read, fp32 accumulation / softmax / dS.  Oracle: the fp32 hooked-attention core on the
    bf16-ROUNDED q, k, v, dO.  Stated tolerances, relative to each tensor's max |x|: what is a product of exactly
    representable operands (S -> P, dP = dO.V^T) 1e-4 (+ the slab's own rounding, 2^-8, when the slab is bf16); what has a
    second, re-rounded operand (O = P.V, dQ = dS.K, dK = dS^T.Q, dV = P^T.dO) 2^-7 = 8e-3.  Shared-forward mode too."""
    from oracle import attention_torch as oat
    from transformer_mm_explainability_amd import ops
    H, D = (8, 32) if Nk == 950 else (4, 64)
    B = 2
    g = torch.Generator().manual_seed(Nq * 3 + Nk)
    rb = lambda t: t.to(torch.bfloat16).float()
    q, k, v = (rb(torch.randn(1, n, H, D, generator=g)) for n in (Nq, Nk, Nk))
    d_o = rb(torch.randn(B, Nq, H, D, generator=g))
    bh = lambda t: t.permute(0, 2, 1, 3)

    def rel(got, want, tol):
        got, want = got.float().cpu(), want.float()
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= tol * float(want.abs().max()), \
            (float((got - want).abs().max()), float(want.abs().max()))

    slab_tol = 2.0 ** -8 if slab == torch.bfloat16 else 0.0
    p_tol = 1e-4 + slab_tol if D == 64 else 2.0 ** -7    # d = 32: q * 32^-0.5 is rounded AFTER scaling (not a power of two)
    probs = torch.empty(1, H, Nq, Nk, device="cuda", dtype=slab)
    dprobs = torch.empty(B, H, Nq, Nk, device="cuda", dtype=slab)
    qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
    o = ops.attn_capture_fwd(qc, kc, vc, probs, D ** -0.5, mma_bf16=True)
    for use_o in (True, False):
        gq, gk, gv = ops.attn_capture_bwd(qc, kc, vc, probs, d_o.cuda(), dprobs, D ** -0.5, batch=B,
                                          o=o if use_o else None, mma_bf16=True)
        for b in range(B):
            P, O, dP, dq, dk, dv = oat.capture(bh(q), bh(k), bh(v), bh(d_o[b:b + 1]), D ** -0.5)
            if b == 0 and use_o:
                rel(probs, P, p_tol)
                rel(bh(o), O, 2.0 ** -7)
            rel(dprobs[b:b + 1], dP, 1e-4 + slab_tol)        # dO, V are used as rounded by the caller: exact products
            rel(bh(gq[b:b + 1]), dq, 2.0 ** -7)
            rel(bh(gk[b:b + 1]), dk, 2.0 ** -7)
            rel(bh(gv[b:b + 1]), dv, 2.0 ** -7)


def test_detr_ni950_rules_vs_oracle():
    """cfg 3 at its real size: the rule schedule of ``generate_ours`` (encoder chain at N = 950, decoder rules 6/7/10)
    on the slabs captured by the same run vs ``oracle/relevancy_np.detr_generate_ours_chain``; the batched-target route
    (``generate_ours_multi``) must agree as well."""
    from oracle import relevancy_np as onp
    from transformer_mm_explainability_amd import detr_model
    from transformer_mm_explainability_amd.detr_explainability import Generator
    torch.manual_seed(0)
    model = detr_model.detr_resnet50_head().cuda().eval()
    feats = torch.randn(1, 2048, 25, 38, device="cuda") * 0.5
    gen = Generator(model)
    tgt = torch.tensor([57], device="cuda")               # one kept query per call, as DETR/mask_generator.py:91 does
    out = gen.generate_ours(feats, tgt, use_lrp=False).clone()
    enc, dec = model.transformer.encoder.layers, model.transformer.decoder.layers
    slab = lambda m: (m.get_attn().cpu().numpy(), m.get_attn_gradients().cpu().numpy())
    ea, eg = zip(*[slab(b.self_attn) for b in enc])
    sa, sg = zip(*[slab(b.self_attn) for b in dec])
    ca, cg = zip(*[slab(b.multihead_attn) for b in dec])
    want = onp.detr_generate_ours_chain(ea, eg, sa, sg, ca, cg, tgt.cpu().numpy())
    assert want.shape == out.shape == (1, 1, 1, 950)
    close(out, want, atol=1e-5, relmax=3e-4)   # measured 1.05e-4 of the largest entry (950-term fp32 dot products, two summation orders)
    both = torch.tensor([3, 57], device="cuda")
    multi = Generator(model).generate_ours_multi(feats, both)
    close(multi[:, :, 1:2], want, atol=1e-5, relmax=3e-4)
    # the row-vector form of the same rules (``rows_only``: no R_i_i, mat-vecs only) vs the oracle, and both routes vs an
    # fp64 evaluation of the schedule on the captured slabs (referee only): the vector form carries rho = R_ii 1 - 1 as a
    # deviation, the matrix form gets it through diag(R_ii) - 1 and loses 2-3 digits there
    rows = Generator(model).generate_ours_multi(feats, both, rows_only=True)
    close(rows[:, :, 1:2], want, atol=1e-5, relmax=3e-4)
    gen2 = Generator(model)
    gen2.generate_ours_multi(feats, both, share_forward=False)              # per-sample slabs of sample 1 (query 57)
    dd = lambda t: t.double()
    H = 8
    avg = lambda m: (dd(m.get_attn().reshape(2, H, *m.get_attn().shape[-2:])[1]) *
                     dd(m.get_attn_gradients().reshape(2, H, *m.get_attn().shape[-2:])[1])).clamp(min=0).mean(0)

    def residual(R):
        n = R.shape[-1]
        eye = torch.eye(n, dtype=R.dtype, device=R.device)
        return (R - eye) / (R - eye).sum(-1, keepdim=True) + eye

    R_ii = torch.eye(950, dtype=torch.float64, device="cuda")
    for b in enc:
        R_ii = R_ii + avg(b.self_attn) @ R_ii
    R_qq = torch.eye(100, dtype=torch.float64, device="cuda")
    R_qi = torch.zeros(100, 950, dtype=torch.float64, device="cuda")
    for b in dec:
        cam = avg(b.self_attn)
        R_qq, R_qi = R_qq + cam @ R_qq, R_qi + cam @ R_qi
        R_qi = R_qi + residual(R_qq).T @ (avg(b.multihead_attn) @ residual(R_ii))
    exact = R_qi[57].float()
    scale = float(exact.abs().max())
    err_rows = float((rows[0, 0, 1] - exact).abs().max()) / scale
    err_matrix = float((multi[0, 0, 1] - exact).abs().max()) / scale
    assert err_rows <= 2e-5 and err_matrix <= 2e-3, (err_rows, err_matrix)
    # who owns the 1.05e-4 between the device result and the fp32 oracle above: the oracle's own distance from
    # the fp64 evaluation of the same slabs goes to the record beside the device's two routes
    err_oracle = float((torch.from_numpy(want[0, 0, 0]).cuda() - exact).abs().max()) / scale
    from parity import note
    note("fp32 oracle (matrix route) vs fp64 schedule, query 57", err_oracle * scale, None, scale)
    note("device rows-only route vs fp64 schedule, query 57", err_rows * scale, 2e-5 * scale, scale)
    note("device matrix route vs fp64 schedule, query 57", err_matrix * scale, 2e-3 * scale, scale)


@pytest.mark.parametrize("N,B,need", [(577, 3, True), (197, 2, True), (577, 2, False), (64, 2, True), (130, 1, True), (300, 2, True),
                                      (640, 1, True)])
def test_bf16_backward_third_generation_equals_second(N, B, need):
    """``attention_bf16_v3.hip`` (shared forward + bf16 gradient stream + row-relevancy mode: the cfg-5 path; bf16 images of
    the shared operands prepared once per call, padded / transposed probability images, 4 waves per SIMD) runs the SAME
    tile arithmetic in the SAME order as the second generation (``attention_bf16.hip``, pinned on the oracle above and, per element on
    counted float64 bounds with all three generations held to the reference directly, by ``tests/test_gpu_attention_bf16.py``), so dq /
    dk / dv (bf16) agree up to isolated last-place flips and the carried relevancy row to 1e-6 (``attn_bf16_v3`` = 0 is the
    second generation, 2 the third-generation pair, 3 -- the default since round 6 -- the third-generation query side with the
    fourth-generation key side ``attn_bwd_kv_v4_kernel``)."""
    from transformer_mm_explainability_amd import ops
    H, D = 4, 64
    g = torch.Generator().manual_seed(N * 7 + B)
    qkv = torch.randn(1, N, 3, H, D, generator=g).cuda()
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    probs = torch.empty(1, H, N, N, device="cuda", dtype=torch.bfloat16)
    o = ops.attn_capture_fwd(q, k, v, probs, D ** -0.5, mma_bf16=True)
    d_o = (torch.randn(B, N, H, D, generator=g) * 1e-2).to(torch.bfloat16).cuda()
    rel = torch.rand(B, N, generator=g).cuda()
    results = {}
    try:
        for mode in (0, 2, 3):
            ops.set_option("attn_bf16_v3", mode)
            out = torch.full((B, N, 3, H, D), float("nan"), device="cuda", dtype=torch.bfloat16) if need else None
            res = ops.attn_capture_bwd(q, k, v, probs, d_o, None, D ** -0.5, batch=B, o=o, need_dqkv=need, mma_bf16=True,
                                       rel_row=rel, out=(out[:, :, 0], out[:, :, 1], out[:, :, 2]) if need else None)
            torch.cuda.synchronize()
            results[mode] = (out, res[3])
    finally:
        ops.set_option("attn_bf16_v3", 3)
    want_out, want_rel = results[0]
    assert torch.isfinite(want_rel).all()
    for mode in (2, 3):
        got_out, got_rel = results[mode]
        if need:
            assert torch.isfinite(got_out.float()).all()
            # same products in the same order; what may differ is how the compiler contracts the fp32 arithmetic around
            # them (delta = rowsum(dO * O), dS) in the two kernels, i.e. a last-place flip of a bf16 result here and there
            diff = (got_out.float() - want_out.float()).abs()
            top = float(want_out.float().abs().max())
            assert float(diff.max()) <= 2.0 ** -7 * top, (mode, float(diff.max()), top)        # <= one bf16 ulp of the largest entries
            # mode 3 (round 6: key side on v_mfma_f32_32x32x16_bf16, 16 query rows per instruction instead of 32): the SAME bf16
            # products, fp32-accumulated in another grouping -> more last-place flips of the bf16 results, never more than one ulp
            assert float((diff > 0).float().mean()) < (0.01 if mode == 2 else 0.05), (mode, float((diff > 0).float().mean()))
        # (the relevancy sum is fp32 VALU work: same terms, but the compiler may contract / order the fmas differently)
        assert float((got_rel - want_rel).abs().max()) <= (1e-6 if mode == 2 else 3e-6) * float(want_rel.abs().max()), mode
