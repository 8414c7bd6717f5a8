"""-m gpu: the row-list FORWARD of the causally masked text tower (``clip_model.Transformer.forward_tape(live=...)``: LayerNorms, the
four GEMMs with their bias and QuickGELU run on the rows up to each caption's EOT token, picked on the device; the attention stays
dense on a ``qkv`` whose other rows are zeros) against the dense forward (options ``text_live_rows`` / ``text_live_rows_fwd``), the
golden fixture and the torch CPU oracle, and the completion of ``blk.attn_probs`` / ``blk.attn_grad`` on their first read."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


from parity import close, note  # noqa: E402

DENSE, BACKWARD_ONLY, ROUTE = (0, 1), (1, 0), (1, 1)       # (text_live_rows, text_live_rows_fwd)


def load_tiny(golden):
    from transformer_mm_explainability_amd import clip_model
    g = golden("clip_tiny")
    cfg = json.loads(str(g["cfg_json"]))
    model = clip_model.CLIP(**cfg).float().eval()
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w__")}
    model.load_state_dict(sd)
    return g, cfg, model.cuda()


@pytest.fixture
def route():
    """``route(mode)`` sets the two process-wide switches; the defaults (both on) are restored afterwards, and so are the tile
    height and the poison debug switch."""
    from transformer_mm_explainability_amd import ops

    def set_mode(mode):
        ops.set_option("text_live_rows", mode[0])
        ops.set_option("text_live_rows_fwd", mode[1])
    yield set_mode
    set_mode(ROUTE)
    ops.set_option("gemm_rows_tm", 32)
    ops.LiveRows.poison = False


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


def live_list():
    from transformer_mm_explainability_amd import ops
    B, N = 7, 77
    eot = torch.tensor([2, 76, 0, 11, 74, 5, 40], device="cuda")
    live = ops.live_rows(eot, N)
    listed = torch.zeros(B * N, dtype=torch.bool, device="cuda")
    listed[torch.tensor([b * N + p for b in range(B) for p in range(int(eot[b]) + 1)], device="cuda")] = True
    assert int(live.count.item()) == int(listed.sum())
    return B, N, live, listed


def same_bits(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def test_linear_rows_kernel_with_bias_and_quick_gelu(route):
    """``ops.linear_rows`` on the four Linears of a ViT-B/32 text block (and two tiny shapes that are no multiple of a tile) with
    both tile heights and a random bias.  Bound against float64: for ANY order of an fp32 sum of K products, |err| <= gamma_K *
    sum |a_k| |w_k| with gamma_K = K u / (1 - K u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1),
    plus one ulp of the result for the bias add.  Unlisted rows of both outputs keep the bits they had, and the activation output
    has the bits of ``ops.quick_gelu_fwd`` on the pre-activation output."""
    from transformer_mm_explainability_amd import ops
    route(ROUTE)
    B, N, live, listed = live_list()
    g = torch.Generator(device="cuda").manual_seed(3)
    u = 2.0 ** -24
    for tm in (32, 64):
        ops.set_option("gemm_rows_tm", tm)
        for K, M in ((512, 1536), (512, 512), (512, 2048), (2048, 512), (64, 16), (20, 36)):
            x = torch.randn(B, N, K, device="cuda", generator=g)
            w = torch.randn(M, K, device="cuda", generator=g) / K ** 0.5          # an nn.Linear weight as stored: [out, in]
            bias = torch.randn(M, device="cuda", generator=g)
            ref = x.view(B * N, K).double() @ w.double().t() + bias.double()
            mag = x.view(B * N, K).double().abs() @ w.double().abs().t()
            for gelu in (False, True):
                out = torch.full((B, N, M), 7.25, device="cuda")
                act = torch.full((B, N, M), -3.5, device="cuda")
                if gelu:
                    ops.linear_rows(x, w, bias, live, out=out, gelu=True, act_out=act)
                else:
                    ops.linear_rows(x, w, bias, live, out=out)
                out2, act2 = out.view(B * N, M), act.view(B * N, M)
                assert bool((out2[~listed] == 7.25).all()), (tm, K, M, gelu)
                assert bool((act2[~listed] == -3.5).all()), (tm, K, M, gelu)
                err = (out2.double() - ref).abs()[listed]
                ulp = torch.from_numpy(np.spacing(np.abs(out2.cpu().numpy()))).cuda().double()[listed]
                bound = (K * u / (1 - K * u)) * mag[listed] + ulp
                note("linear_rows tm%d %dx%d" % (tm, K, M), float(err.max()), float(bound.max()))
                assert bool((err <= bound).all()), (tm, K, M, gelu, float(err.max()), float(bound.max()))
                if gelu:
                    assert same_bits(act2[listed], ops.quick_gelu_fwd(out).view(B * N, M)[listed]), (tm, K, M)
                else:
                    assert bool((act2 == -3.5).all())


def test_add_layernorm_rows_equals_the_dense_kernel_bit_for_bit(route):
    """Row widths on every register-tile count of the kernel that a text tower can have here (1, 2 and 4 chunks of 64 x 4 floats,
    a width that leaves lanes idle), with and without the residual operand."""
    from transformer_mm_explainability_amd import ops
    route(ROUTE)
    B, N, live, listed = live_list()
    g = torch.Generator(device="cuda").manual_seed(4)
    for E in (512, 64, 20, 772):
        x = torch.randn(B, N, E, device="cuda", generator=g) * 3 + 1
        gamma, beta = torch.randn(E, device="cuda", generator=g), torch.randn(E, device="cuda", generator=g)
        for y in (torch.randn(B, N, E, device="cuda", generator=g), None):
            want = ops.add_layernorm(x, y, gamma, beta, 1e-5)
            out = (torch.full((B, N, E), 7.25, device="cuda"), torch.full((B, N, E), -3.5, device="cuda"),
                   torch.full((B * N,), 1.5, device="cuda"), torch.full((B * N,), 2.5, device="cuda"))
            got = ops.add_layernorm_rows(x, y, gamma, beta, 1e-5, live, out=out)
            if y is None:
                assert got[0] is x
            for i, (a, b, fill) in enumerate(zip(got, want, (7.25, -3.5, 1.5, 2.5))):
                if i == 0 and y is None:
                    assert bool((out[0] == 7.25).all())                      # no sum without a second operand
                    continue
                a2, b2 = a.reshape(B * N, -1), b.reshape(B * N, -1)
                assert same_bits(a2[listed], b2[listed]), (E, i)
                assert bool((a2[~listed] == fill).all()), (E, i)


def test_golden_parity_and_lazy_slab_accessors_on_the_tiny_model(golden, route):
    from transformer_mm_explainability_amd import clip_explainability as ce
    g, _, model = load_tiny(golden)
    image, texts = torch.from_numpy(g["image"]).cuda(), torch.from_numpy(g["texts"]).cuda()
    for mode, name in ((ROUTE, "on"), (DENSE, "off"), (BACKWARD_ONLY, "forward off")):
        route(mode)
        R_text, R_image = ce.interpret(image, texts, model, "cuda", 0, 0)
        assert (model.transformer._probs_pending is not None) == (mode == ROUTE)
        close(R_text, g["R_text_all"], what="R_text route %s" % name)
        close(R_image, g["R_image_all"], what="R_image route %s" % name)
        first = (R_text.clone(), R_image.clone())
        # the slabs as the pass left them: the gradients at and below the diagonal (all the chain reads; above it P is masked and a
        # row-list forward has no value rows of padded positions to form dO . V^T with)
        raw = model.transformer.buffers.grads
        n = raw.shape[-1]
        tril = torch.ones(n, n, dtype=torch.bool, device="cuda").tril_()
        for l in range(raw.shape[0]):
            close(raw[l].reshape(-1, n, n)[:, tril], g["txt_grad"][l][:, tril.cpu().numpy()], atol=5e-6, rtol=1e-4, what="intermediate")
        assert (model.transformer._probs_pending is not None) == (mode == ROUTE)
        for l, blk in enumerate(model.transformer.resblocks):
            close(blk.attn_grad, g["txt_grad"][l], atol=5e-6, rtol=1e-4, what="intermediate")       # every entry: the lazy completion
        assert model.transformer._probs_pending is None
        for l, blk in enumerate(model.transformer.resblocks):
            close(blk.attn_probs, g["txt_attn"][l], atol=2e-6, rtol=1e-4, what="intermediate")     # all rows: the lazy completion
        assert model.transformer._probs_pending is None
        again = ce.interpret(image, texts, model, "cuda", 0, 0)                   # the completion left nothing behind
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])


_ORACLE = {}


def vit_b32_case():
    """Random-init ViT-B/32 and the CPU oracle's maps for B = 8 captions of 3 ... 77 tokens, computed once per session."""
    if not _ORACLE:
        from oracle import clip_torch
        from transformer_mm_explainability_amd import clip_model
        model = clip_model.random_init("ViT-B/32", seed=0)
        image = torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(1))
        texts = captions([3, 75, 77, 5, 9, 12, 20, 40], 77, 49408, seed=2)
        sd = clip_torch.prepare_state_dict(model.state_dict(), 8)
        _ORACLE["case"] = (model.cuda(), image, texts, clip_torch.interpret(sd, image, texts, 0, 0))
    return _ORACLE["case"]


def test_vit_b32_against_the_oracle(route):
    """The route re-orders fp32 sums (another GEMM tiling in the forward), so its largest error against the CPU oracle may be at
    most 1.5 x the dense path's largest error against the same oracle (the project's rule for a re-ordered fp32 sum,
    tests/test_gpu_lrp.py).  One caption has its EOT at position 76: every row of that sample is live."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    model, image, texts, (want_text, want_img) = vit_b32_case()
    assert int(texts[2].argmax()) == 76
    errs = {}
    for mode in (DENSE, ROUTE):
        route(mode)
        R_text, R_image = ce.interpret(image.cuda(), texts.cuda(), model, "cuda", 0, 0)
        close(R_text, want_text.numpy(), what="R_text %s" % (mode,))
        close(R_image, want_img.numpy(), what="R_image %s" % (mode,))
        errs[mode] = (float((R_text.cpu() - want_text).abs().max()), float((R_image.cpu() - want_img).abs().max()))
    print("largest error against the oracle (R_text, R_image): dense %s, row-list forward and backward %s" % (errs[DENSE], errs[ROUTE]))
    assert errs[ROUTE][0] <= 1.5 * errs[DENSE][0], errs
    assert errs[ROUTE][1] <= 1.5 * errs[DENSE][1], errs


def test_graph_replays_follow_the_caption_lengths(golden, route):
    """A ``GraphedInterpret`` captured with short captions, replayed with longer ones, full-length ones (every row live) and short
    ones again: every replay equals the eager dense result, ``R_text`` outside each live block is exactly the identity, and reading
    ``blk.attn_probs`` after a replay gives the dense probabilities of ALL rows without disturbing the next replay."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    g, cfg, model = load_tiny(golden)
    image = torch.from_numpy(g["image"]).cuda()
    B, ctx, vocab = g["texts"].shape[0], cfg["context_length"], cfg["vocab_size"]
    short = captions([3 + b % 2 for b in range(B)], ctx, vocab, seed=5).cuda()
    longer = captions([(ctx, ctx - 1, 3, max(3, ctx // 2))[b % 4] for b in range(B)], ctx, vocab, seed=6).cuda()
    full = captions([ctx] * B, ctx, vocab, seed=7).cuda()
    short2 = captions([4 - b % 2 for b in range(B)], ctx, vocab, seed=8).cuda()
    sequence = [short, longer, full, short2]
    route(DENSE)
    dense = []
    for texts in sequence:
        R_text, R_image = ce.interpret(image, texts, model, "cuda", 0, 0)
        dense.append((R_text.clone(), R_image.clone(), [blk.attn_probs.clone() for blk in model.transformer.resblocks],
                      [blk.attn_grad.clone() for blk in model.transformer.resblocks]))
    route(ROUTE)
    run = ce.GraphedInterpret(model, image, short, 0, 0)
    assert run._txt_pending is not None                                          # the route was captured
    n = ctx
    eye = torch.eye(n, device="cuda")
    for step, (texts, (want_t, want_i, want_p, want_g)) in enumerate(zip(sequence, dense)):
        got_t, got_i = run(image, texts)
        close(got_t, want_t.cpu().numpy(), atol=2e-6, rtol=1e-4, what="intermediate")
        close(got_i, want_i.cpu().numpy(), atol=2e-6, rtol=1e-4, what="intermediate")
        for b, ln in enumerate((texts.argmax(dim=-1) + 1).tolist()):
            outside = torch.ones(n, n, dtype=torch.bool, device="cuda")
            outside[:ln, :ln] = False
            assert bool((got_t[b][outside] == eye[outside]).all()), "R_text outside the live block of sample %d" % b
        if step != 2:                                                            # (step 2 is followed by a replay without a read)
            keep = (got_t.clone(), got_i.clone())
            for blk, want in zip(model.transformer.resblocks, want_p):
                close(blk.attn_probs, want.cpu().numpy(), atol=2e-6, rtol=1e-4, what="intermediate")
            for blk, want in zip(model.transformer.resblocks, want_g):
                close(blk.attn_grad, want.cpu().numpy(), atol=5e-6, rtol=1e-4, what="intermediate")
            again_t, again_i = run(image, texts)                                 # the replay after a completion
            assert torch.equal(again_t, keep[0]) and torch.equal(again_i, keep[1])


def test_no_stale_reads_from_unlisted_rows(golden, route):
    """Every per-call intermediate of the route, forward and backward, starts as NaN (``ops.LiveRows.poison``): unlisted rows are
    never written, so a consumer that read one would carry the NaN into the slabs and the maps.  The results do not change by a bit."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import ops
    g, _, model = load_tiny(golden)
    image, texts = torch.from_numpy(g["image"]).cuda(), torch.from_numpy(g["texts"]).cuda()
    route(ROUTE)

    def run():
        R_text, R_image = ce.interpret(image, texts, model, "cuda", 0, 0)
        assert model.transformer._probs_pending is not None
        buffers = model.transformer.buffers                                     # the raw slabs: what the route itself wrote
        return [R_text.clone(), R_image.clone(), buffers.grads.clone(), buffers.probs.clone()]

    plain = run()
    ops.LiveRows.poison = True
    poisoned = run()
    for a, b in zip(plain, poisoned):
        assert not bool(torch.isnan(b).any())
        assert torch.equal(a, b)
    close(poisoned[0], g["R_text_all"])
    assert np.isfinite(poisoned[1].cpu().numpy()).all()


def test_completion_inside_a_stream_capture_raises(golden, route):
    """Reading ``blk.attn_probs`` of a pending tower while a stream is capturing would record the completion's kernels into someone
    else's graph: it raises instead, leaves the slabs pending, and the read works once the capture has ended."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import ops
    g, _, model = load_tiny(golden)
    image, texts = torch.from_numpy(g["image"]).cuda(), torch.from_numpy(g["texts"]).cuda()
    route(ROUTE)
    ce.interpret(image, texts, model, "cuda", 0, 0)
    blk = model.transformer.resblocks[0]
    assert model.transformer._probs_pending is not None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(ops.MMXError, match="stream capture"):
        with ops.graph_capture(graph):
            torch.zeros(4, device="cuda")
            blk.attn_probs
    del graph
    assert model.transformer._probs_pending is not None
    close(blk.attn_probs, g["txt_attn"][0], atol=2e-6, rtol=1e-4, what="intermediate")
