"""-m gpu: the attention of the causally masked text tower on the rows up to each caption's EOT token (``ops.attn_capture_fwd(live=...)``
/ ``ops.attn_capture_bwd(live=...)``: the live-length instantiations of the whole-head kernels, ``csrc/attention_head.hip``) against the
dense kernels on operands whose dead rows are zeros -- bit for bit --, and ``clip_model.Transformer.forward_tape(live=...)`` with it
against option ``text_live_attn = 0`` (dense attention over a zero-filled ``qkv``), the all-dense path and the torch CPU oracle."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from parity import close  # noqa: E402

B, H, N, D = 6, 2, 77, 64
EOT = [0, 15, 16, 31, 76, 5]          # L = 1, a strip boundary on either side, two strips, no dead row at all, a short one
SENTINEL = 7.25


@pytest.fixture
def options():
    """``options(text_live_rows=..., ...)`` sets process-wide switches; all of them are back on afterwards, the poison switch off."""
    from transformer_mm_explainability_amd import ops

    def set_options(**kw):
        for key, value in kw.items():
            ops.set_option(key, value)
    yield set_options
    set_options(text_live_rows=1, text_live_rows_fwd=1, text_live_attn=1)
    ops.LiveRows.poison = False


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return bool((bits(a) == bits(b)).all())


def causal_mask(n):
    return torch.full((n, n), float("-inf"), device="cuda").triu_(1)


_OPS = {}


def op_case():
    """Operands of the op-level tests, made once: ``qkv`` / ``d_o`` with zeros in the dead rows and with NaN there, the list, the dense
    kernels' ``P``, ``O``, ``dP`` and ``dq | dk | dv`` on the zeroed operands (the reference; never modified)."""
    if not _OPS:
        from transformer_mm_explainability_amd import _lib, ops
        g = torch.Generator(device="cuda").manual_seed(11)
        eot = torch.tensor(EOT, device="cuda")
        dead = torch.arange(N, device="cuda")[None, :] > eot[:, None]                       # [B, N]
        qkv = torch.randn(B, N, 3, H, D, device="cuda", generator=g)
        d_o = torch.randn(B, N, H, D, device="cuda", generator=g)
        zeroed, poisoned = qkv.clone(), qkv.clone()
        zeroed[dead], poisoned[dead] = 0.0, float("nan")
        d_o_zeroed, d_o_poisoned = d_o.clone(), d_o.clone()
        d_o_zeroed[dead], d_o_poisoned[dead] = 0.0, float("nan")
        mask, scale = causal_mask(N), D ** -0.5
        probs = torch.full((B, H, N, N), SENTINEL, device="cuda")
        o = ops.attn_capture_fwd(zeroed[:, :, 0], zeroed[:, :, 1], zeroed[:, :, 2], probs, scale, _lib.SCALE_Q_FIRST, mask)
        dprobs = torch.full((B, H, N, N), SENTINEL, device="cuda")
        dq, dk, dv = ops.attn_capture_bwd(zeroed[:, :, 0], zeroed[:, :, 1], zeroed[:, :, 2], probs, d_o_zeroed, dprobs, scale,
                                          _lib.SCALE_Q_FIRST, need_dqkv=True)
        _OPS.update(eot=eot, dead=dead, poisoned=poisoned, d_o_poisoned=d_o_poisoned, mask=mask, scale=scale, probs=probs, o=o,
                    dprobs=dprobs, dqkv=(dq, dk, dv), live=ops.live_rows(eot, N))
        assert ops.attn_live_shape(N, D)
    return _OPS


def test_forward_reads_no_dead_row_and_equals_the_dense_kernel_bit_for_bit(options):
    """``P``: the whole slab has the dense kernel's bits (dead rows: the softmax of zero scores under the mask, ``1 / (i + 1)`` over
    ``j <= i``).  ``O``: the dense bits on live rows, untouched elsewhere.  ``q``, ``k``, ``v`` hold NaN in every dead row."""
    from transformer_mm_explainability_amd import _lib, ops
    c = op_case()
    x = c["poisoned"]
    probs = torch.full((B, H, N, N), -3.5, device="cuda")
    out = torch.full((B, N, H, D), SENTINEL, device="cuda")
    o = ops.attn_capture_fwd(x[:, :, 0], x[:, :, 1], x[:, :, 2], probs, c["scale"], _lib.SCALE_Q_FIRST, c["mask"], live=c["live"], out=out)
    assert o is out
    assert not bool(torch.isnan(probs).any())
    assert same_bits(probs, c["probs"])
    assert same_bits(o[~c["dead"]], c["o"][~c["dead"]])
    assert bool((o[c["dead"]] == SENTINEL).all())
    # the filler itself, spelled out: row i of a dead query is 1 / (i + 1) on the keys j <= i
    i = N - 1
    want = torch.full((N,), 1.0 / N, device="cuda")
    assert int(c["eot"][0]) < i and torch.allclose(probs[0, 0, i], want, rtol=1e-6, atol=0)


@pytest.mark.parametrize("need_dqkv", [True, False], ids=["dqkv", "lowest_block"])
def test_backward_reads_no_dead_row_and_equals_the_dense_kernel_bit_for_bit(options, need_dqkv):
    """NaN in the dead rows of ``q``, ``k``, ``v``, ``dO`` and ``O``.  ``dP``: the dense kernel's bits over the whole slab, exact zeros in
    the dead rows.  ``dq``, ``dk``, ``dv``: the dense bits on live rows, untouched elsewhere.  ``need_dqkv=False`` is the lowest block
    of a tower: ``dP`` only."""
    from transformer_mm_explainability_amd import _lib, ops
    c = op_case()
    x, dead = c["poisoned"], c["dead"]
    o_poisoned = c["o"].clone()
    o_poisoned[dead] = float("nan")
    dprobs = torch.full((B, H, N, N), -3.5, device="cuda")
    dqkv = torch.full((B, N, 3, H, D), SENTINEL, device="cuda")
    res = ops.attn_capture_bwd(x[:, :, 0], x[:, :, 1], x[:, :, 2], c["probs"], c["d_o_poisoned"], dprobs, c["scale"], _lib.SCALE_Q_FIRST,
                               need_dqkv=need_dqkv, out=(dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]) if need_dqkv else None,
                               o=o_poisoned, live=c["live"])
    assert same_bits(dprobs, c["dprobs"])
    dead_rows = dead[:, None, :].expand(B, H, N)
    assert bool((dprobs[dead_rows] == 0).all())
    if not need_dqkv:
        assert res == (None, None, None) and bool((dqkv == SENTINEL).all())
        return
    for i, want in enumerate(c["dqkv"]):
        got = dqkv[:, :, i]
        assert same_bits(got[~dead], want[~dead]), "dq dk dv"[3 * i:3 * i + 2]
        assert bool((got[dead] == SENTINEL).all()), "dq dk dv"[3 * i:3 * i + 2]


def test_a_shape_without_a_live_instantiation_is_an_error_not_a_dense_run(options):
    from transformer_mm_explainability_amd import _lib, ops
    n, d = 20, 32
    assert not ops.attn_live_shape(n, d)
    qkv = torch.randn(2, n, 3, 2, d, device="cuda")
    live = ops.live_rows(torch.tensor([3, 19], device="cuda"), n)
    probs = torch.empty(2, 2, n, n, device="cuda")
    with pytest.raises(ops.MMXError, match="live"):
        ops.attn_capture_fwd(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], probs, d ** -0.5, _lib.SCALE_Q_FIRST, causal_mask(n), live=live)
    options(text_live_attn=0)
    assert not ops.attn_live_shape(N, D)


# ------------------------------------------------------------------------------------------------------------------ tower level

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


_TOWER = {}


def small_clip(golden, context):
    """The configuration of the golden tiny model (the one the other live-rows suites use) at another context length, random
    weights; with its image, captions whose lengths sit on and around the 16-row strips, and the CPU oracle's maps.  Once per length."""
    if context not in _TOWER:
        from oracle import clip_torch
        from transformer_mm_explainability_amd import clip_model
        g = golden("clip_tiny")
        cfg = dict(json.loads(str(g["cfg_json"])), context_length=context)
        torch.manual_seed(21)
        model = clip_model.CLIP(**cfg).float().eval()
        image = torch.from_numpy(g["image"])
        lengths = [2, 16, 17, 32, context, 6, 33] if context >= 33 else [2, 16, 17, context, 6]
        texts = captions(lengths, context, cfg["vocab_size"], seed=22)
        sd = clip_torch.prepare_state_dict(model.state_dict(), cfg["transformer_heads"])
        _TOWER[context] = (cfg, model.cuda(), image.cuda(), texts.cuda(), clip_torch.interpret(sd, image, texts, 0, 0))
    return _TOWER[context]


def run_tower(model, image, texts):
    """The maps, the raw slabs as the pass left them, then every block's completed ``attn_probs`` / ``attn_grad``."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    R_text, R_image = ce.interpret(image, texts, model, "cuda", 0, 0)
    tr = model.transformer
    out = dict(R_text=R_text.clone(), R_image=R_image.clone(), pending=tr._probs_pending is not None,
               raw_probs=tr.buffers.probs.clone(), raw_grads=tr.buffers.grads.clone())
    out["probs"] = [blk.attn_probs.clone() for blk in tr.resblocks]
    out["grads"] = [blk.attn_grad.clone() for blk in tr.resblocks]
    return out


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
def test_tower_with_live_attention_equals_the_zero_filled_dense_attention(golden, options, poison):
    """77 tokens: the live instantiation runs.  Default options against ``text_live_attn = 0`` bit for bit (maps and raw slabs), the
    1e-5 contract of the CPU oracle, and the completed accessors against an all-dense run under the forward-route suite's tolerances
    (tests/test_gpu_text_forward_live_rows.py).  ``poisoned``: every per-call intermediate of the route starts as NaN, ``qkv`` and
    ``dqkv`` included now -- same bits, no NaN anywhere."""
    from transformer_mm_explainability_amd import ops
    cfg, model, image, texts, (want_text, want_image) = small_clip(golden, 77)
    assert ops.attn_live_shape(77, cfg["transformer_width"] // cfg["transformer_heads"])
    options(text_live_rows=0)
    dense = run_tower(model, image, texts)
    assert not dense["pending"]
    options(text_live_rows=1, text_live_attn=0)
    ops.LiveRows.poison = poison
    filled = run_tower(model, image, texts)
    options(text_live_attn=1)
    live = run_tower(model, image, texts)
    assert filled["pending"] and live["pending"]
    for key in ("R_text", "R_image", "raw_probs", "raw_grads"):
        assert not bool(torch.isnan(live[key]).any()), key
        assert torch.equal(live[key], filled[key]), key
    close(live["R_text"], want_text.numpy(), what="R_text live attention")
    close(live["R_image"], want_image.numpy(), what="R_image live attention")
    for l in range(len(dense["probs"])):
        close(live["probs"][l], dense["probs"][l].cpu().numpy(), atol=2e-6, rtol=1e-4, what="intermediate")
        close(live["grads"][l], dense["grads"][l].cpu().numpy(), atol=5e-6, rtol=1e-4, what="intermediate")
    if poison:
        ops.LiveRows.poison = False
        plain = run_tower(model, image, texts)
        for key in ("R_text", "R_image", "raw_probs", "raw_grads"):
            assert torch.equal(live[key], plain[key]), key


def test_graph_replays_follow_the_caption_lengths(golden, options):
    """One ``GraphedInterpret`` captured on short captions, replayed with longer ones, then shorter ones: the lengths are read on the
    device, so every replay equals the eager call on the same inputs, bit for bit (same kernels in the same order), and rows that were
    live in the replay before leave nothing behind: ``R_text`` outside each live block is exactly the identity, and a replay of the
    first captions after all the others returns the first replay's bits."""
    from transformer_mm_explainability_amd import clip_explainability as ce
    cfg, model, image, _, _ = small_clip(golden, 77)
    ctx, vocab = cfg["context_length"], cfg["vocab_size"]
    short = captions([3, 4, 2, 5], ctx, vocab, seed=31).cuda()
    longer = captions([ctx, 17, 40, 16], ctx, vocab, seed=32).cuda()
    shorter = captions([2, 3, 2, 2], ctx, vocab, seed=33).cuda()
    eager = [tuple(t.clone() for t in ce.interpret(image, texts, model, "cuda", 0, 0)) for texts in (short, longer, shorter)]
    run = ce.GraphedInterpret(model, image, short, 0, 0)
    assert run._txt_pending is not None and run._txt_pending["live"].attn           # the route was captured, live attention included
    eye = torch.eye(ctx, device="cuda")
    first = None
    for texts, (want_t, want_i) in zip((short, longer, shorter, short), eager + [eager[0]]):
        got_t, got_i = run(image, texts)
        print("replay against eager: max |dR_text| %.3g, max |dR_image| %.3g"
              % (float((got_t - want_t).abs().max()), float((got_i - want_i).abs().max())))
        assert torch.equal(got_t, want_t) and torch.equal(got_i, want_i)
        for b, ln in enumerate((texts.argmax(dim=-1) + 1).tolist()):
            outside = torch.ones(ctx, ctx, dtype=torch.bool, device="cuda")
            outside[:ln, :ln] = False
            assert bool((got_t[b][outside] == eye[outside]).all()), "R_text outside the live block of sample %d" % b
        if first is None:
            first = (got_t.clone(), got_i.clone())
    assert torch.equal(got_t, first[0]) and torch.equal(got_i, first[1])


def test_fallback_shape_keeps_the_dense_attention_inside_the_route(golden, options):
    """20 tokens: no live instantiation, so the route zero-fills ``qkv`` and runs the dense attention as before; it agrees with the
    all-dense path under the tolerance the forward-route suite uses for that comparison, and with the CPU oracle."""
    from transformer_mm_explainability_amd import ops
    cfg, model, image, texts, (want_text, want_image) = small_clip(golden, 20)
    assert not ops.attn_live_shape(20, cfg["transformer_width"] // cfg["transformer_heads"])
    options(text_live_rows=0)
    dense = run_tower(model, image, texts)
    options(text_live_rows=1)
    route = run_tower(model, image, texts)
    assert route["pending"] and not dense["pending"]
    assert not model.transformer.__dict__.get("_probs_pending")                      # (the accessors were read: completed)
    close(route["R_text"], dense["R_text"].cpu().numpy(), atol=2e-6, rtol=1e-4, what="intermediate")
    close(route["R_image"], dense["R_image"].cpu().numpy(), atol=2e-6, rtol=1e-4, what="intermediate")
    close(route["R_text"], want_text.numpy(), what="R_text fallback shape")
    close(route["R_image"], want_image.numpy(), what="R_image fallback shape")
    for l in range(len(dense["probs"])):
        close(route["probs"][l], dense["probs"][l].cpu().numpy(), atol=2e-6, rtol=1e-4, what="intermediate")
        close(route["grads"][l], dense["grads"][l].cpu().numpy(), atol=5e-6, rtol=1e-4, what="intermediate")
