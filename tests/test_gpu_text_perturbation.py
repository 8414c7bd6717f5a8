"""-m gpu: the token perturbation test for CLIP captions (``clip_text_perturbation.py``) and what it stands on: ``mmx_perturb_tokens``
against the plain-loop restatement of its rule, the live-length attention forward without a capture slab (``mmx_attn_fwd_live``,
``ops.attn_fwd(live=...)``) against the capture pair and the dense kernel, the row-list inference forward of the text tower
(``Transformer.forward_nocapture(live=...)``, ``CLIP.encode_text_nocapture(live=True)``) against a float64 referee, and the evaluator
against the torch CPU oracle."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import parity  # noqa: E402
import text_perturbation_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
H = 3
SENTINEL = 7.25


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    return _ops


@pytest.fixture
def restore():
    """Process-wide switches back to their defaults after a test that moves them."""
    from transformer_mm_explainability_amd import ops as _ops
    yield
    for key in ("text_live_rows", "text_live_rows_fwd", "text_live_attn"):
        _ops.set_option(key, 1)
    _ops.LiveRows.poison = False


def _guarded(shape, dtype):
    """An INT_MIN-filled buffer with GUARD elements after ``shape``'s elements: (view, guard, sentinel test)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), -2 ** 31, dtype=dtype, device="cuda")
    return buf[:n].view(*shape), buf[n:], lambda g: bool((g == -2 ** 31).all())


def same_bits(a, b):
    return bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


# ------------------------------------------------------------------------------------------------------------ 1. perturb_tokens
SOT, EOT_ID = 49406, 49407
SPECIAL = [float("inf"), float("-inf"), 0.0, -0.0, float("nan"), -0.0, 0.0, float("nan"), float("inf")]


def _token_case(N, B, kind, g):
    """Caption lengths cycle through 2 tokens (no word), 3 (one word), N (EOT in the last position), an all-zero row (e = 0), a row
    whose largest id appears twice (the first one is EOT) and a random length."""
    ids = torch.zeros(B, N, dtype=torch.long)
    for b in range(B):
        c = b % 6
        if c == 3:
            continue
        n = (2, min(3, N), N, 0, max(2, N // 2), int(torch.randint(2, N + 1, (1,), generator=g)))[c]
        ids[b, 0] = SOT
        ids[b, 1:n - 1] = torch.randint(1, 1000, (n - 2,), generator=g)
        ids[b, n - 1] = EOT_ID
        if c == 4 and n < N:
            ids[b, n:] = torch.randint(1, 1000, (N - n,), generator=g)              # (what follows the first EOT is dropped)
            ids[b, N - 1] = EOT_ID
    x = torch.randn(B, N, generator=g)
    if kind == "ties":
        x = torch.floor(torch.rand(B, N, generator=g) * 8) / 8                      # 8 levels
    elif kind == "special":
        for b in range(B):
            e = int(ids[b].argmax())
            words = torch.arange(1, max(e, 1))[torch.randperm(max(e - 1, 0), generator=g)][:len(SPECIAL)]
            for p, v in zip(words.tolist(), SPECIAL):
                x[b, p] = v
            x[b, 0] = float("nan")                                                  # outside the words: never ranked
            x[b, e:] = float("inf")
            x[b, e::2] = float("nan")
    return ids, x


@pytest.mark.parametrize("B", [1, 5, 64])
@pytest.mark.parametrize("N", [2, 3, 12, 64, 65, 77, 256])
@pytest.mark.parametrize("kind", ["random", "ties", "special"])
def test_perturb_tokens_equal_the_loop_restatement(ops, N, B, kind):
    from transformer_mm_explainability_amd.clip_text_perturbation import token_step_counts
    from transformer_mm_explainability_amd.lxmert_perturbation import PERT_STEPS
    ids, x = _token_case(N, B, kind, torch.Generator().manual_seed(N * 7 + B))
    for steps in (PERT_STEPS, (0,)):
        table = token_step_counts(steps, N)
        counts = torch.tensor(table, dtype=torch.int32, device="cuda")
        S = len(steps)
        for sign in (1.0, -1.0):                                                    # the positive test ranks the negated scores
            want_ids, want_eot, want_ranks = cases.restate(ids, sign * x, table)
            (o_ids, g0, ok0), (o_eot, g1, ok1), (o_rk, g2, ok2) = (_guarded((S, B, N), torch.int64), _guarded((S, B), torch.int64),
                                                                   _guarded((B, N), torch.int32))
            got = ops.perturb_tokens(ids.cuda(), (sign * x).cuda(), counts, want_ranks=True, out=(o_ids, o_eot, o_rk))
            again = ops.perturb_tokens(ids.cuda(), (sign * x).cuda(), counts, want_ranks=True)
            no_ranks = ops.perturb_tokens(ids.cuda(), (sign * x).cuda(), counts)
            torch.cuda.synchronize()
            assert got[0] is o_ids and got[1] is o_eot and got[2] is o_rk
            assert torch.equal(o_ids.cpu(), want_ids), (S, sign)
            assert torch.equal(o_eot.cpu(), want_eot), (S, sign)
            assert torch.equal(o_rk.cpu(), want_ranks), (S, sign)
            assert ok0(g0) and ok1(g1) and ok2(g2)
            assert all(torch.equal(a, b) for a, b in zip(again, got))
            assert len(no_ranks) == 2 and torch.equal(no_ranks[0], o_ids) and torch.equal(no_ranks[1], o_eot)
            assert torch.equal(o_ids.argmax(dim=-1), o_eot)
            tail = torch.arange(N, device="cuda").view(1, 1, N) > o_eot.unsqueeze(-1)
            assert bool((o_ids[tail] == 0).all())
        if S == 1:      # step 0 removes nothing: the caption itself wherever it holds zeros past its EOT
            e = ids.argmax(dim=-1)
            clean = torch.tensor([bool((ids[b, int(e[b]) + 1:] == 0).all()) for b in range(B)])
            assert torch.equal(o_ids.cpu()[0][clean], ids[clean])


def test_perturb_tokens_refuses_wrong_operands(ops):
    from transformer_mm_explainability_amd._lib import MMXError
    ids = torch.zeros(2, 12, dtype=torch.long, device="cuda")
    x = torch.zeros(2, 12, device="cuda")
    with pytest.raises(MMXError):
        ops.perturb_tokens(ids, x, torch.zeros(9, 12, dtype=torch.int32, device="cuda"))       # counts: [S, N - 1]
    with pytest.raises(MMXError):
        ops.perturb_tokens(ids.int(), x, torch.zeros(9, 11, dtype=torch.int32, device="cuda"))
    with pytest.raises(MMXError):
        ops.perturb_tokens(ids, x[:, :-1], torch.zeros(9, 11, dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------------------------------------------------ 2. attn_fwd(live=)
def _lengths(N):
    """One sample per live length, then the two clamped ones -> eot [13]."""
    return [L - 1 for L in (1, 15, 16, 17, 32, 33, 48, 49, 64, 65, N)] + [-3, N + 5]


def _rows(t, layout):
    """[B, N, H, D] view of an operand in either layout."""
    return t if layout == "bnhd" else t.transpose(1, 2)


@pytest.mark.parametrize("N", [65, 77, 80])
@pytest.mark.parametrize("D", [20, 32, 64])
@pytest.mark.parametrize("layout", ["bnhd", "bhnd"])
@pytest.mark.parametrize("mode", ["q_first", "scores"])
def test_attn_fwd_live_equals_the_capture_pair_and_the_dense_kernel(ops, N, D, layout, mode):
    from transformer_mm_explainability_amd import _lib
    scale_mode = _lib.SCALE_Q_FIRST if mode == "q_first" else _lib.SCALE_SCORES
    scale = D ** -0.5 if mode == "q_first" else D ** 0.5                       # (SCALE_SCORES divides the scores by `scale`)
    eot = torch.tensor(_lengths(N), device="cuda")
    B = eot.numel()
    live = ops.live_rows(eot, N)
    assert ops.attn_live_shape(N, D)
    dead = torch.arange(N, device="cuda")[None, :] > eot.clamp(0, N - 1)[:, None]          # [B, N]
    g = torch.Generator(device="cuda").manual_seed(N * 100 + D)
    shape = (B, N, H, D) if layout == "bnhd" else (B, H, N, D)
    q, k, v = (torch.randn(shape, device="cuda", generator=g) for _ in range(3))
    mask = torch.full((N, N), float("-inf"), device="cuda").triu_(1)
    zeroed, poisoned = [], []
    for t in (q, k, v):
        z, p = t.clone(), t.clone()
        _rows(z, layout)[dead] = 0.0
        _rows(p, layout)[dead] = float("nan")
        zeroed.append(z)
        poisoned.append(p)
    out = torch.full(shape, SENTINEL, device="cuda")
    o = ops.attn_fwd(q, k, v, scale, scale_mode, mask, layout=layout, live=live, out=out)
    assert o is out
    probs = torch.empty(B, H, N, N, device="cuda")
    o_cap = ops.attn_capture_fwd(q, k, v, probs, scale, scale_mode, mask, layout=layout, live=live)
    o_dense = ops.attn_fwd(*zeroed, scale, scale_mode, mask, layout=layout)
    o_nan = ops.attn_fwd(*poisoned, scale, scale_mode, mask, layout=layout, live=live)
    torch.cuda.synchronize()
    got = _rows(o, layout)
    assert not bool(torch.isnan(got[~dead]).any())
    assert same_bits(got[~dead], _rows(o_cap, layout)[~dead])
    assert same_bits(got[~dead], _rows(o_dense, layout)[~dead])
    assert bool((got[dead] == SENTINEL).all())
    assert same_bits(_rows(o_nan, layout)[~dead], got[~dead])


def test_attn_fwd_live_outside_its_shapes_is_an_error_not_a_dense_run(ops, restore):
    from transformer_mm_explainability_amd._lib import MMXError
    for N, option in ((12, 1), (77, 0)):
        eot = torch.tensor([3, 7], device="cuda")
        q, k, v = (torch.randn(2, N, H, 32, device="cuda") for _ in range(3))
        mask = torch.full((N, N), float("-inf"), device="cuda").triu_(1)
        live = ops.live_rows(eot, N)
        out = torch.full((2, N, H, 32), SENTINEL, device="cuda")
        try:
            ops.set_option("text_live_attn", option)
            assert not ops.attn_live_shape(N, 32)
            with pytest.raises(MMXError, match="live"):
                ops.attn_fwd(q, k, v, 32 ** -0.5, mask=mask, live=live, out=out)
        finally:
            ops.set_option("text_live_attn", 1)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    with pytest.raises(MMXError, match="mask"):
        ops.attn_fwd(q, k, v, 32 ** -0.5, live=live)


# ------------------------------------------------------------------------------------------------------------ 3. row-list inference forward
_MODELS = {}


def _model(golden, which):
    """``(cfg, model on the GPU, oracle state dict, lengths)``, built once per session."""
    if which not in _MODELS:
        from oracle import clip_torch
        from transformer_mm_explainability_amd import clip_model
        if which == "tiny":
            g = golden("clip_tiny")
            cfg = cases.tiny_cfg(golden)
            model = clip_model.CLIP(**cfg).float().eval()
            model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("w__")})
            lengths = cases.TINY_LENGTHS
        else:
            cfg = cases.CTX77_CFG
            torch.manual_seed(0)
            model = clip_model.CLIP(**cfg).float().eval()
            lengths = cases.CTX77_LENGTHS
        sd = clip_torch.prepare_state_dict(model.state_dict(), cfg["transformer_heads"])
        _MODELS[which] = (cfg, model.cuda(), sd, lengths)
    return _MODELS[which]


def _oracle_text_features(sd, texts, dtype):
    """The text half of ``oracle.clip_torch.forward`` (its ``_block`` with the causal mask, ``ln_final``, the EOT row, the projection)
    on a ``dtype`` copy of the state dict -> un-normalised features ``[B, embed_dim]``."""
    w = {k: v.detach().to(dtype) for k, v in sd.items() if torch.is_tensor(v)}
    heads = sd["__text_heads__"]
    ctx, E = w["positional_embedding"].shape
    d = E // heads
    mask = torch.full((ctx, ctx), float("-inf")).triu_(1).to(dtype)
    t = F.embedding(texts, w["token_embedding.weight"]) + w["positional_embedding"]
    B, N, _ = t.shape
    layers = len([k for k in w if k.startswith("transformer.resblocks.") and k.endswith(".attn.in_proj_weight")])
    for l in range(layers):
        pre = "transformer.resblocks.%d." % l
        h = F.layer_norm(t, (E,), w[pre + "ln_1.weight"], w[pre + "ln_1.bias"])
        q, k, v = F.linear(h, w[pre + "attn.in_proj_weight"], w[pre + "attn.in_proj_bias"]).chunk(3, dim=-1)
        q = q * (float(d) ** -0.5)
        q, k, v = (x.view(B, N, heads, d).permute(0, 2, 1, 3).reshape(B * heads, N, d) for x in (q, k, v))
        p = F.softmax(torch.bmm(q, k.transpose(1, 2)) + mask, dim=-1)
        o = torch.bmm(p, v).view(B, heads, N, d).permute(0, 2, 1, 3).reshape(B, N, E)
        t = t + F.linear(o, w[pre + "attn.out_proj.weight"], w[pre + "attn.out_proj.bias"])
        h = F.layer_norm(t, (E,), w[pre + "ln_2.weight"], w[pre + "ln_2.bias"])
        h = F.linear(h, w[pre + "mlp.c_fc.weight"], w[pre + "mlp.c_fc.bias"])
        h = h * torch.sigmoid(1.702 * h)
        t = t + F.linear(h, w[pre + "mlp.c_proj.weight"], w[pre + "mlp.c_proj.bias"])
    t = F.layer_norm(t, (E,), w["ln_final.weight"], w["ln_final.bias"])
    return t[torch.arange(B), texts.argmax(dim=-1)] @ w["text_projection"]


@pytest.mark.parametrize("which", ["tiny", "ctx77"])
def test_row_list_inference_forward_against_a_float64_referee(golden, ops, restore, monkeypatch, which):
    """The route re-orders fp32 sums (another GEMM tiling), so its largest error against the float64 referee may be at most 1.5 x the
    dense path's largest error against the same referee (the project's rule, tests/test_gpu_text_forward_live_rows.py)."""
    cfg, model, sd, lengths = _model(golden, which)
    texts = cases.captions(lengths, cfg["context_length"], cfg["vocab_size"], torch.Generator().manual_seed(31))
    with torch.no_grad():
        ref64 = _oracle_text_features(sd, texts, torch.float64)
        ref32 = _oracle_text_features(sd, texts, torch.float32)
    head_dim = cfg["transformer_width"] // cfg["transformer_heads"]
    assert ops.attn_live_shape(cfg["context_length"], head_dim) == (which == "ctx77")
    buffers = model.transformer.buffers
    calls = {"rows": 0, "live_attn": 0}
    linear_rows, attn_fwd = ops.linear_rows, ops.attn_fwd

    def count_rows(*a, **kw):
        calls["rows"] += 1
        return linear_rows(*a, **kw)

    def count_attn(*a, **kw):
        calls["live_attn"] += kw.get("live") is not None
        return attn_fwd(*a, **kw)
    monkeypatch.setattr(ops, "linear_rows", count_rows)
    monkeypatch.setattr(ops, "attn_fwd", count_attn)
    dense = model.encode_text_nocapture(texts.cuda(), live=False)
    assert calls == {"rows": 0, "live_attn": 0}
    route = model.encode_text_nocapture(texts.cuda(), live=True)
    layers = cfg["transformer_layers"]
    # every block's in_proj on the row list, the lower blocks' other three Linears too; the live attention where it has a kernel
    assert calls == {"rows": layers + 3 * (layers - 1), "live_attn": layers if which == "ctx77" else 0}
    monkeypatch.undo()
    assert model.transformer.buffers is buffers
    err_dense = float((dense.cpu().double() - ref64).abs().max())
    err_route = float((route.cpu().double() - ref64).abs().max())
    print("%s: largest error against the float64 referee: dense %.3e, row-list route %.3e" % (which, err_dense, err_route))
    parity.note("dense_vs_f64", err_dense)
    parity.note("route_vs_f64", err_route)
    parity.close(dense, ref32, what="dense_features")
    parity.close(route, ref32, what="route_features")
    assert err_route <= 1.5 * err_dense, (err_route, err_dense)
    # option text_live_attn = 0: the dense attention over a zero-filled qkv, the same bits (live queries see live keys only)
    ops.set_option("text_live_attn", 0)
    assert same_bits(model.encode_text_nocapture(texts.cuda(), live=True), route)
    ops.set_option("text_live_attn", 1)
    # no unlisted row is read: the intermediates start as NaN
    ops.LiveRows.poison = True
    try:
        poisoned = model.encode_text_nocapture(texts.cuda(), live=True)
    finally:
        ops.LiveRows.poison = False
    assert bool(torch.isfinite(poisoned).all()) and same_bits(poisoned, route)
    # the default call is the dense path: it builds no row list
    def no_list(*a, **kw):
        raise AssertionError("the default encode_text_nocapture built a row list")
    monkeypatch.setattr(ops, "live_rows", no_list)
    assert same_bits(model.encode_text_nocapture(texts.cuda()), dense)
    monkeypatch.undo()
    # row-list forward switched off process-wide: live=True falls back to the dense forward
    ops.set_option("text_live_rows_fwd", 0)
    assert same_bits(model.encode_text_nocapture(texts.cuda(), live=True), dense)


def test_row_list_inference_forward_refuses_a_bf16_body(golden):
    from transformer_mm_explainability_amd._lib import MMXError
    cfg, model, _, lengths = _model(golden, "ctx77")
    texts = cases.captions(lengths, 77, cfg["vocab_size"], torch.Generator().manual_seed(31)).cuda()
    model.set_body_dtype(torch.bfloat16)
    try:
        with pytest.raises(MMXError, match="bfloat16"):
            model.encode_text_nocapture(texts, live=True)
        with pytest.raises(MMXError, match="bfloat16"):
            model.encode_text_nocapture(texts)
    finally:
        model.set_body_dtype(torch.float32)
    x = torch.randn(2, 77, 64, device="cuda")
    eot = torch.tensor([3, 9], device="cuda")
    with pytest.raises(ValueError):
        model.transformer.forward_nocapture(x, out_rows=None, live=model.transformer.live_rows_for_forward(x, eot))


# ------------------------------------------------------------------------------------------------------------ 4. evaluator
def _oracle_curves(logits, targets):
    prob = torch.softmax(logits, dim=-1)
    S, B, _ = logits.shape
    return prob.gather(2, targets.view(1, B, 1).expand(S, B, 1)).squeeze(2), prob


def _check_result(res, want_logits, labels, tag):
    """logits / target_prob with parity.close; pred == the oracle's arg-max wherever its top-2 probability gap >= 1e-4."""
    S, B, _ = want_logits.shape
    want_targets = want_logits[0].argmax(dim=-1)                     # step 0 keeps every word: the unperturbed caption
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


_WANT = {}


def _evaluator_case(golden, which, positive):
    """Inputs, the restated captions of every step and the CPU oracle's logits for them ``[S, B, n_images]``; once per session."""
    key = (which, positive)
    if key not in _WANT:
        from oracle import clip_torch
        from transformer_mm_explainability_amd.clip_text_perturbation import token_step_counts
        from transformer_mm_explainability_amd.lxmert_perturbation import PERT_STEPS
        cfg, model, sd, lengths = _model(golden, which)
        images, cam, texts = cases.evaluator_inputs(cfg, lengths, *((23, 24) if which == "tiny" else (29, 30)))
        ids, eot, _ = cases.restate(texts, -cam if positive else cam, token_step_counts(PERT_STEPS, texts.shape[1]))
        with torch.no_grad():
            want = torch.stack([clip_torch.forward(sd, images, ids[s])[0].t() for s in range(ids.shape[0])])
        labels = torch.randint(0, images.shape[0], (texts.shape[0],), generator=torch.Generator().manual_seed(5))
        _WANT[key] = (model, images, cam, texts, ids, eot, want, labels)
    return _WANT[key]


@pytest.mark.parametrize("which", ["tiny", "ctx77"])
@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("live", [False, True])
def test_token_perturbation_against_cpu_oracle(golden, which, positive, live):
    from transformer_mm_explainability_amd import clip_text_perturbation as tp
    model, images, cam, texts, ids, eot, want, labels = _evaluator_case(golden, which, positive)
    buffers = model.transformer.buffers
    pert = tp.TokenPerturbation(tp.ClipCaptionScorer(model, images.cuda()), live=live)
    res = pert(texts.cuda(), cam.cuda(), labels=labels.cuda(), is_positive_pert=positive)
    assert model.transformer.buffers is buffers
    assert torch.equal(res.texts.cpu(), ids) and torch.equal(res.eot.cpu(), eot)
    _check_result(res, want, labels, "text_%s_%s" % (which, "live" if live else "dense"))
    # explicit targets: the probability of THAT image is followed
    res_t = pert(texts.cuda(), cam.cuda(), targets=labels.cuda(), is_positive_pert=positive)
    assert res_t.correct is None and res_t.accuracy is None
    parity.close(res_t.target_prob, _oracle_curves(want, labels)[0], what="text_given_targets")
    with pytest.raises(ValueError):
        pert(texts.cuda(), cam.cuda()[:, :-1])
    with pytest.raises(ValueError):
        pert(texts.cuda(), cam.cuda()[:-1])


def test_caption_scorer_refuses_a_bf16_body(golden):
    from transformer_mm_explainability_amd import clip_text_perturbation as tp
    from transformer_mm_explainability_amd._lib import MMXError
    model, images = _evaluator_case(golden, "tiny", False)[:2]
    model.set_body_dtype(torch.bfloat16)
    try:
        with pytest.raises(MMXError, match="bfloat16"):
            tp.ClipCaptionScorer(model, images.cuda())
    finally:
        model.set_body_dtype(torch.float32)


# ------------------------------------------------------------------------------------------------------------ 5. determinism, chunks
@pytest.mark.parametrize("live", [False, True])
def test_determinism_and_chunking(golden, live):
    """Two calls give equal bits.  Chunks: ``max_batch = S * B`` is the unchunked call (equal bits, asserted); ``max_batch = 7`` (no
    divisor of S * B = 90) gives the same logits to ``parity.close`` and the same predictions on BOTH routes -- bit equality is not
    asserted for it: the dense route's library GEMMs and the route's row-list tiles both see other row counts per chunk, and either
    may then sum in another order."""
    from transformer_mm_explainability_amd import clip_text_perturbation as tp
    model, images, cam, texts = _evaluator_case(golden, "ctx77", False)[:4]
    scorer = tp.ClipCaptionScorer(model, images.cuda())
    pert = tp.TokenPerturbation(scorer, live=live)
    a, b = pert(texts.cuda(), cam.cuda()), pert(texts.cuda(), cam.cuda())
    assert torch.equal(a.logits, b.logits) and torch.equal(a.target_prob, b.target_prob) and torch.equal(a.pred, b.pred)
    S, B = a.logits.shape[:2]
    whole = tp.TokenPerturbation(scorer, live=live, max_batch=S * B)(texts.cuda(), cam.cuda())
    assert torch.equal(whole.logits, a.logits)
    c = tp.TokenPerturbation(scorer, live=live, max_batch=7)(texts.cuda(), cam.cuda())
    print("max_batch 7, live=%s: logits bit-equal to the unchunked call: %s" % (live, torch.equal(c.logits, a.logits)))
    parity.close(c.logits, a.logits, what="chunked_logits")
    assert torch.equal(c.pred, a.pred)


# ------------------------------------------------------------------------------------------------------------ 6. pipeline
def test_pipeline_interpret_to_token_perturbation(golden):
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import clip_text_perturbation as tp
    model, images, _, texts = _evaluator_case(golden, "ctx77", False)[:4]
    images, texts = images.cuda(), texts.cuda()
    B, N = texts.shape
    R_text, _ = ce.interpret(images[:1], texts, model, "cuda", 0, 0)
    cam = tp.text_cams(texts, R_text)
    assert cam.shape == (B, N) and bool(torch.isfinite(cam).all())
    eot = texts.argmax(dim=-1)
    assert torch.equal(cam, torch.stack([R_text[b, int(eot[b])] for b in range(B)]))
    text_buffers, image_buffers = model.transformer.buffers, model.visual.transformer.buffers
    assert text_buffers is not None
    for live in (False, True):
        res = tp.TokenPerturbation(tp.ClipCaptionScorer(model, images), live=live)(texts, cam)
        S = len(tp.PERT_STEPS)
        assert res.logits.shape == (S, B, images.shape[0]) and res.target_prob.shape == (S, B) and res.auc().shape == (B,)
        assert bool(torch.isfinite(res.logits).all()) and bool(torch.isfinite(res.target_prob).all())
        _, per_text = model.logits(model.visual.encode_nocapture(images=images), model.encode_text_nocapture(texts))
        want = torch.softmax(per_text, dim=-1).gather(1, res.targets.view(B, 1)).squeeze(1)
        parity.close(res.target_prob[0], want, what="step0_target_prob")
        assert torch.equal(res.targets, per_text.argmax(dim=-1))
        # no capture slab is allocated (or replaced) by the evaluator
        assert model.transformer.buffers is text_buffers and model.visual.transformer.buffers is image_buffers
    with pytest.raises(ValueError):
        tp.text_cams(texts, R_text[:, :-1])
