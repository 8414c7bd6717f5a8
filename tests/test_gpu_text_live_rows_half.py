"""-m gpu: the text tower of an fp16 body (``set_body_dtype(torch.float16)``, the reference's ``convert_weights`` mode,
CLIP/clip/model.py:381-402) on the rows up to each caption's EOT token -- option ``text_live_rows_half`` (default 0), the GEMMs on
``mmx_gemm_rows_f16`` / ``mmx_gemm_rows_bias_f16``, everything else the fp32 row kernels of the fp32 route.  The rounding points are
the dense fp16 path's (every GEMM input rounded to fp16 once, fp32 accumulation); the two differ in the order of the fp32 sums only.

Pinned on the reference's fp16 model (the bar of ``test_fp16_mode_matches_the_references_fp16_model``), on the dense fp16 path through
their distances to the fp32 maps (the 1.5 x margin ``tests/test_gpu_text_perturbation.py`` gives a path that differs from its
neighbour by summation order only; measured on the 77-token model of this file: see ``DESIGN.md``), and bit for bit on itself: graph
replays, the poison switch, the accessors.  bf16 and fp32 bodies do not notice the option."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture
def options():
    """``options(text_live_rows_half=1, ...)`` sets process-wide switches; the defaults are back afterwards, the poison switch off."""
    from transformer_mm_explainability_amd import ops

    def set_options(**kw):
        for key, value in kw.items():
            ops.set_option(key, value)
    yield set_options
    set_options(text_live_rows=1, text_live_rows_fwd=1, text_live_attn=1, text_live_rows_half=0)
    ops.LiveRows.poison = False


def load_tiny(golden):
    from transformer_mm_explainability_amd import clip_model
    g = golden("clip_tiny")
    cfg = json.loads(str(g["cfg_json"]))
    model = clip_model.CLIP(**cfg).float().eval()
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w__")})
    return g, cfg, model.cuda()


def captions(lengths, context, vocab, seed=0):
    """Token ids ``[B, context]`` with ``lengths[b]`` tokens each: start token, words, EOT (the largest id: the arg-max, model.py:360)."""
    g = torch.Generator().manual_seed(seed)
    texts = torch.zeros(len(lengths), context, dtype=torch.long)
    for b, n in enumerate(lengths):
        assert 2 <= n <= context
        texts[b, 0] = vocab - 2
        texts[b, 1:n - 1] = torch.randint(1, vocab - 2, (n - 2,), generator=g)
        texts[b, n - 1] = vocab - 1
    return texts


_MODEL = {}
LENGTHS = [77, 2, 16, 17, 33, 6]             # EOT at position 76 (no dead row) and at position 1 among them


def model77(golden):
    """The tiny configuration (3 layers, width 64, 2 heads) at 77 tokens with random weights: the live-length attention is on."""
    if not _MODEL:
        from transformer_mm_explainability_amd import clip_model
        g = golden("clip_tiny")
        cfg = dict(json.loads(str(g["cfg_json"])), context_length=77)
        torch.manual_seed(41)
        model = clip_model.CLIP(**cfg).float().eval().cuda()
        _MODEL.update(cfg=cfg, model=model, image=torch.from_numpy(g["image"]).cuda(),
                      texts=captions(LENGTHS, 77, cfg["vocab_size"], seed=42).cuda())
    return _MODEL["cfg"], _MODEL["model"], _MODEL["image"], _MODEL["texts"]


def maps(model, image, texts):
    from transformer_mm_explainability_amd import clip_explainability as ce
    R_text, R_image = ce.interpret(image, texts, model, "cuda", 0, 0)
    return R_text.clone(), R_image.clone()


@pytest.mark.parametrize("tag,sl,slt", [("last", -1, -1), ("all", 0, 0), ("mid", 1, 2)])
def test_route_matches_the_references_fp16_model(golden, options, tag, sl, slt):
    """12 tokens: the attention stays dense over a zero-filled ``qkv``.  Exactly the assertion of
    ``tests/test_gpu_clip.py::test_fp16_mode_matches_the_references_fp16_model``; and the route is what ran."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    g, cfg, model = load_tiny(golden)
    g16 = golden("clip_tiny_fp16")
    image, texts = torch.from_numpy(g["image"]).cuda(), torch.from_numpy(g["texts"]).cuda()
    model.set_body_dtype(torch.float16)
    _, state = model.encode_text_tape(texts)
    assert state[6] is None                                          # option off (the default): the dense tower
    options(text_live_rows_half=1)
    _, state = model.encode_text_tape(texts)
    assert state[6] is not None and not state[6].attn                # the route, dense attention inside it
    R_text, R_image = ce.interpret(image, texts, model, "cuda", start_layer=sl, start_layer_text=slt)
    assert model.transformer._probs_pending is not None              # interpret took it as well
    assert R_text.dtype == torch.float16 and R_image.dtype == torch.float16
    for got, name in ((R_text, "R_text_" + tag), (R_image, "R_image_" + tag)):
        want16, want32 = torch.from_numpy(g16[name]).float(), torch.from_numpy(g[name])
        top = float(want32.abs().max())
        err16 = float((got.float().cpu() - want16).abs().max())
        err32 = float((got.float().cpu() - want32).abs().max())
        print("%s: to the reference's fp16 %.3g, to its fp32 %.3g (bar %.3g)" % (name, err16, err32, 4e-3 * top))
        assert err16 <= 4e-3 * top and err32 <= 4e-3 * top, (name, err16, err32, top)


def test_route_is_as_close_to_fp32_as_the_dense_fp16_path(golden, options):
    """77 tokens, live-length attention on, captions with EOT at positions 76 and 1 among them: the route's distance to the fp32 maps is
    at most 1.5 x the dense fp16 path's, and ``R_text`` outside each caption's live block is exactly the identity."""
    from transformer_mm_explainability_amd import ops
    cfg, model, image, texts = model77(golden)
    assert ops.attn_live_shape(77, cfg["transformer_width"] // cfg["transformer_heads"])
    model.set_body_dtype(torch.float32)
    exact = maps(model, image, texts)
    try:
        model.set_body_dtype(torch.float16)
        dense = maps(model, image, texts)
        assert model.transformer._probs_pending is None
        options(text_live_rows_half=1)
        route = maps(model, image, texts)
        pending = model.transformer._probs_pending
        assert pending is not None and pending["live"].attn
    finally:
        model.set_body_dtype(torch.float32)
    for name, want, a, b in (("R_text", exact[0], dense[0], route[0]), ("R_image", exact[1], dense[1], route[1])):
        d_dense = float((a.float() - want).abs().max())
        d_route = float((b.float() - want).abs().max())
        print("%s: distance to the fp32 maps: dense fp16 %.4g, route %.4g (largest entry %.4g)"
              % (name, d_dense, d_route, float(want.abs().max())))
        assert bool(torch.isfinite(b).all())
        assert d_route <= 1.5 * d_dense, (name, d_route, d_dense)
    eye = torch.eye(77, device="cuda")
    for b, ln in enumerate(LENGTHS):
        outside = torch.ones(77, 77, dtype=torch.bool, device="cuda")
        outside[:ln, :ln] = False
        assert bool((route[0][b].float()[outside] == eye[outside]).all()), "R_text outside the live block of sample %d" % b


def test_graph_replays_follow_the_caption_lengths(golden, options):
    """One ``GraphedInterpret`` on the fp16 body, captured on short captions and replayed with longer ones, full-length ones and short
    ones again: every replay equals the eager route result on the same captions bit for bit."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    cfg, model, image, _ = model77(golden)
    ctx, vocab = cfg["context_length"], cfg["vocab_size"]
    short = captions([3, 4, 2, 5], ctx, vocab, seed=31).cuda()
    longer = captions([40, 17, 33, 16], ctx, vocab, seed=32).cuda()
    full = captions([ctx, ctx, ctx, ctx], ctx, vocab, seed=34).cuda()
    options(text_live_rows_half=1)
    try:
        model.set_body_dtype(torch.float16)
        eager = [maps(model, image, texts) for texts in (short, longer, full)]
        run = ce.GraphedInterpret(model, image, short, 0, 0)
        assert run._txt_pending is not None and run._txt_pending["live"].attn       # the route was captured, live attention included
        for texts, (want_t, want_i) in zip((short, longer, full, short), eager + [eager[0]]):
            got_t, got_i = run(image, texts)
            print("replay against eager: max |dR_text| %.3g, max |dR_image| %.3g"
                  % (float((got_t.float() - want_t.float()).abs().max()), float((got_i.float() - want_i.float()).abs().max())))
            assert torch.equal(got_t, want_t) and torch.equal(got_i, want_i)
    finally:
        model.set_body_dtype(torch.float32)


def test_poisoned_intermediates_change_nothing(golden, options):
    """``LiveRows.poison``: every per-call intermediate of the route starts as NaN -- same bits, no NaN anywhere."""
    from transformer_mm_explainability_amd import ops
    cfg, model, image, texts = model77(golden)
    options(text_live_rows_half=1)
    try:
        model.set_body_dtype(torch.float16)
        plain = maps(model, image, texts)
        ops.LiveRows.poison = True
        poisoned = maps(model, image, texts)
        assert model.transformer._probs_pending is not None
    finally:
        ops.LiveRows.poison = False
        model.set_body_dtype(torch.float32)
    for a, b in zip(plain, poisoned):
        assert bool(torch.isfinite(b).all())
        assert torch.equal(a, b)


def test_accessors_complete_the_slabs(golden, options):
    """Reading ``blk.attn_probs`` / ``blk.attn_grad`` after a route call runs the dense fp16 pass into the same slabs; the maps of the
    next call are unchanged."""
    cfg, model, image, texts = model77(golden)
    options(text_live_rows_half=1)
    try:
        model.set_body_dtype(torch.float16)
        before = maps(model, image, texts)
        tr = model.transformer
        assert tr._probs_pending is not None
        probs = [blk.attn_probs.clone() for blk in tr.resblocks]
        grads = [blk.attn_grad.clone() for blk in tr.resblocks]
        assert tr._probs_pending is None
        for t in probs + grads:
            assert bool(torch.isfinite(t.float()).all())
        rows = probs[0].float().reshape(-1, 77).sum(-1)
        assert torch.allclose(rows, torch.ones_like(rows), atol=1e-3)                  # every row a distribution, dead rows included
        after = maps(model, image, texts)
    finally:
        model.set_body_dtype(torch.float32)
    for a, b in zip(before, after):
        assert torch.equal(a, b)


def test_other_bodies_do_not_notice_the_option(golden, options):
    """bf16 body: no route, option or not.  fp32 body: the maps are bit-equal with the option on and off."""
    cfg, model, image, texts = model77(golden)
    tr = model.transformer
    x = torch.zeros(len(LENGTHS), 77, cfg["transformer_width"], device="cuda")
    eot = texts.argmax(dim=-1)
    try:
        model.set_body_dtype(torch.float32)
        off = maps(model, image, texts)
        options(text_live_rows_half=1)
        on = maps(model, image, texts)
        for a, b in zip(off, on):
            assert torch.equal(a, b)
        assert tr.live_rows_for_forward(x, eot) is not None                            # fp32: the route as before
        model.set_body_dtype(torch.bfloat16)
        assert tr.live_rows_for_forward(x, eot) is None
        model.set_body_dtype(torch.float16)
        assert tr.live_rows_for_forward(x, eot) is not None
        options(text_live_rows_half=0)
        assert tr.live_rows_for_forward(x, eot) is None
        options(text_live_rows_half=1, text_live_rows_fwd=0)
        assert tr.live_rows_for_forward(x, eot) is None
    finally:
        model.set_body_dtype(torch.float32)
