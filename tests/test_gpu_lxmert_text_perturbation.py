"""-m gpu: the LXMERT text perturbation test on device-built step groups (``LxmertPerturbation.perturbation_text_grouped``,
``GraphedTextPerturbation``) == the current route (``perturbation_text``) on the same padded batch, == every item alone and unpadded,
== the reference's sequential loop (lxmert/lxmert/perturbation.py:160-188, restated: physically remove the tokens, one forward per
step), and == the reference evaluator's own scores (``tests/golden/lxmert_perturbation.npz``) from inside a padded batch.  The tiny
LXMERT of ``tests/test_gpu_perturbation.py``, restated: hidden 96, 4 heads, 3 / 2 / 2 layers; T = 12, 20 regions, B = 4 questions of
12, 5, 2 and 9 tokens, cams given directly.

The tests print their distances and whether the graph replay was bit-equal to the eager route (``-s``)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, I, LENS = 12, 20, [12, 5, 2, 9]
_shared = {}


def _model():
    from transformer_mm_explainability_amd import lxmert_model as lm
    if "model" not in _shared:
        torch.manual_seed(5)
        cfg = lm.LxmertConfig(hidden_size=96, num_attention_heads=4, intermediate_size=192, l_layers=3, x_layers=2,
                              r_layers=2, visual_feat_dim=40, vocab_size=200, num_qa_labels=31,
                              max_position_embeddings=64)
        model = lm.LxmertForQuestionAnswering(cfg).cuda().eval()
        with torch.no_grad():                                     # default init leaves the scores nearly flat
            for p in model.parameters():
                if p.dim() > 1:
                    p.mul_(3.0)
        _shared["model"] = model
    return _shared["model"]


def _ragged_batch(g, lens, n_text=T, regions=I):
    B = len(lens)
    ids = torch.zeros(B, n_text, dtype=torch.long)
    mask = torch.zeros(B, n_text)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, 200, (n,), generator=g)
        mask[b, :n] = 1
    return dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), token_type_ids=torch.zeros(B, n_text, dtype=torch.long).cuda(),
                visual_feats=torch.randn(B, regions, 40, generator=g).cuda(), visual_pos=torch.rand(B, regions, 4, generator=g).cuda())


def _case():
    """The batch, its cams and the CURRENT route's scores for both signs: computed once, shared, never modified."""
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    if "case" not in _shared:
        g = torch.Generator().manual_seed(21)
        batch = _ragged_batch(g, LENS)
        cam = (torch.rand(len(LENS), T, generator=g).cuda() * batch["attention_mask"]).contiguous()
        pert = lp.LxmertPerturbation(_model())
        current = {positive: pert.perturbation_text(batch, cam, positive).clone() for positive in (False, True)}
        _shared["case"] = (batch, cam, current)
    return _shared["case"]


def _one(batch, b, n):
    return {k: v[b:b + 1, :n] if k in ("input_ids", "attention_mask", "token_type_ids") else v[b:b + 1] for k, v in batch.items()}


@pytest.mark.parametrize("max_groups", [1, 2, 3])
@pytest.mark.parametrize("positive", [False, True])
def test_grouped_equals_the_current_route_padded_and_unpadded(positive, max_groups):
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    model = _model()
    batch, cam, current = _case()
    pert = lp.LxmertPerturbation(model)
    got = pert.perturbation_text_grouped(batch, cam, positive, max_groups=max_groups)
    assert got.shape == (len(LENS), len(lp.PERT_STEPS), 31) and torch.isfinite(got).all()
    print("grouped(%d) vs perturbation_text, positive=%s: max abs diff %.3e" % (max_groups, positive,
                                                                                 float((got - current[positive]).abs().max())))
    torch.testing.assert_close(got, current[positive], rtol=1e-4, atol=1e-5)
    for b, n in enumerate(LENS):
        alone = pert.perturbation_text(_one(batch, b, n), cam[b, :n], positive)
        torch.testing.assert_close(got[b], alone, rtol=1e-4, atol=1e-5)
    assert not torch.allclose(got[0, 0], got[0, -1], atol=1e-3)        # the perturbation does change the answer scores


@pytest.mark.parametrize("positive", [False, True])
def test_grouped_equals_the_sequential_physical_removal_loop(positive):
    """The loop of ``test_text_perturbation_batched_equals_sequential`` (tests/test_gpu_perturbation.py), per item of the batch."""
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    model = _model()
    batch, cam, _ = _case()
    got = lp.LxmertPerturbation(model).perturbation_text_grouped(batch, cam, positive)
    with torch.no_grad():
        for b, n in enumerate(LENS):
            one = _one(batch, b, n)
            c = (-cam if positive else cam)[b, :n]
            for s, step in enumerate(lp.PERT_STEPS):
                pure = c[1:-1]
                top = pure.topk(k=int((1 - step) * (n - 2)), dim=-1).indices.tolist()
                kept = sorted([0, n - 1] + [i + 1 for i in top])
                want = model(input_ids=one["input_ids"][:, kept], attention_mask=one["attention_mask"][:, kept],
                             token_type_ids=one["token_type_ids"][:, kept], visual_feats=one["visual_feats"],
                             visual_pos=one["visual_pos"]).question_answering_score[0]
                torch.testing.assert_close(got[b, s], want, rtol=1e-4, atol=1e-5)


def test_scores_with_encoded_regions_equal_the_plain_call():
    model = _model()
    batch, _, _ = _case()
    plain = model.scores_no_grad(**batch)
    visn = model.encode_vision(batch["visual_feats"], batch["visual_pos"])
    assert visn.shape == (len(LENS), I, 96)
    text = {k: batch[k] for k in ("input_ids", "attention_mask", "token_type_ids")}
    got = model.scores_no_grad(visn_encoded=visn, **text)
    print("visn_encoded vs plain: max abs diff %.3e, bit-equal %s" % (float((got - plain).abs().max()), torch.equal(got, plain)))
    torch.testing.assert_close(got, plain, rtol=1e-5, atol=1e-5)
    # with a region mask, and repeated for questions that come 3 per sample (the evaluator's call)
    vmask = torch.ones(len(LENS), I, device="cuda")
    vmask[:, 13:] = 0
    plain = model.scores_no_grad(visual_attention_mask=vmask, **batch)
    visn = model.encode_vision(batch["visual_feats"], batch["visual_pos"], vmask)
    torch.testing.assert_close(model.scores_no_grad(visn_encoded=visn, visual_attention_mask=vmask, **text), plain, rtol=1e-5, atol=1e-5)
    rep = {k: v.repeat_interleave(3, dim=0) for k, v in text.items()}
    got = model.scores_no_grad(visn_encoded=visn, visual_attention_mask=vmask, visn_repeat=3, **rep)
    torch.testing.assert_close(got, plain.repeat_interleave(3, dim=0), rtol=1e-5, atol=1e-5)
    with pytest.raises(ValueError):
        model.scores_no_grad(visn_encoded=visn[:, :0], **text)


@pytest.mark.parametrize("positive", [False, True])
def test_reference_evaluator_text_scores_from_inside_a_padded_batch(golden, positive):
    """The 9 score vectors the reference's own ``perturbation_text`` produced on the reference body, reproduced for that item as row 1
    of a batch padded 3 tokens past its length, between two shorter random questions (tolerances of the existing golden test)."""
    from transformer_mm_explainability_amd import lxmert_model as lm
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    gm, g = golden("lxmert_model"), golden("lxmert_perturbation")
    hidden, heads, inter, ll, xl, rl, feat, vocab, labels, max_pos, n_text, regions = (int(x) for x in gm["dims"])
    if "golden_model" not in _shared:
        model = lm.LxmertForQuestionAnswering(lm.LxmertConfig(
            hidden_size=hidden, num_attention_heads=heads, intermediate_size=inter, l_layers=ll, x_layers=xl, r_layers=rl,
            visual_feat_dim=feat, vocab_size=vocab, num_qa_labels=labels, max_position_embeddings=max_pos))
        model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in gm.items() if k.startswith("w__")}, strict=True)
        _shared["golden_model"] = model.cuda().eval()
    model = _shared["golden_model"]
    item = {k[4:]: torch.from_numpy(np.asarray(v)) for k, v in gm.items() if k.startswith("in__")}
    pad, B, row = n_text + 3, 3, 1
    gen = torch.Generator().manual_seed(33)
    ids = torch.zeros(B, pad, dtype=torch.long)
    mask = torch.zeros(B, pad)
    types = torch.zeros(B, pad, dtype=torch.long)
    feats = torch.randn(B, regions, feat, generator=gen)
    pos = torch.rand(B, regions, 4, generator=gen)
    cam = torch.zeros(B, pad)
    for b, n in ((0, max(n_text - 2, 2)), (2, 2)):
        ids[b, :n] = torch.randint(1, vocab, (n,), generator=gen)
        mask[b, :n] = 1
        cam[b, :n] = torch.rand(n, generator=gen)
    ids[row, :n_text], mask[row, :n_text], types[row, :n_text] = item["input_ids"][0], 1, item["token_type_ids"][0]
    feats[row], pos[row], cam[row, :n_text] = item["visual_feats"][0], item["visual_pos"][0], torch.from_numpy(g["cam_text"])
    batch = dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), token_type_ids=types.cuda(), visual_feats=feats.cuda(),
                 visual_pos=pos.cuda())
    pert = lp.LxmertPerturbation(model)
    tag = "text_%s" % ("pos" if positive else "neg")
    for max_groups in (1, 2, 3):
        scores = pert.perturbation_text_grouped(batch, cam.cuda(), positive, max_groups=max_groups)[row]
        torch.testing.assert_close(scores.cpu(), torch.from_numpy(g["scores_" + tag]), rtol=1e-4, atol=1e-5)
        acc = pert.accuracy(scores, torch.from_numpy(g["label_scores"]).cuda())
        torch.testing.assert_close(acc.cpu(), torch.from_numpy(g["acc_" + tag]), rtol=0, atol=1e-6)


def test_graphed_text_perturbation_replays_any_lengths_and_refuses_another_shape():
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    model = _model()
    g = torch.Generator().manual_seed(44)
    pert = lp.LxmertPerturbation(model)
    run, bit_equal = None, []
    for lens in ([12, 12, 12, 12], [6, 11, 2, 7], LENS):
        batch = _ragged_batch(g, lens)
        R_t_t = torch.rand(len(lens), T, T, generator=g).cuda() * batch["attention_mask"][:, None, :]
        R_t_i = torch.rand(len(lens), T, I, generator=g).cuda()
        labels = torch.rand(len(lens), 31, generator=g).cuda()
        _, cam_text = lp.normalize_cams_batch(R_t_t, R_t_i, batch["attention_mask"])
        want = pert.perturbation_text_grouped(batch, cam_text).clone()
        want_acc = lp.LxmertPerturbation.accuracy(want, labels)
        if run is None:
            run = lp.GraphedTextPerturbation(pert, batch, R_t_t, R_t_i, labels)
        got_acc = run(batch, R_t_t, R_t_i, labels)
        assert got_acc.shape == (len(lens), len(lp.PERT_STEPS))
        torch.testing.assert_close(run.scores, want, rtol=1e-5, atol=1e-6)
        assert torch.equal(got_acc, want_acc), (got_acc, want_acc)
        bit_equal.append(torch.equal(run.scores, want))
    print("graph replay vs eager, bit-equal per batch:", bit_equal)
    short = _ragged_batch(g, [5, 5, 5])
    with pytest.raises(ValueError, match="captured"):
        run(short, R_t_t[:3], R_t_i[:3], labels[:3])


def test_no_host_synchronisation_after_the_first_call():
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    model = _model()
    batch, cam, current = _case()
    pert = lp.LxmertPerturbation(model)
    pert.perturbation_text_grouped(batch, cam)                           # builds the shape's constants (host lists -> device)
    other = _ragged_batch(torch.Generator().manual_seed(55), [3, 12, 7, 2])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = pert.perturbation_text_grouped(batch, cam)
        pert.perturbation_text_grouped(other, cam, True)
        no_mask = {k: v for k, v in other.items() if k != "attention_mask"}
        pert.perturbation_text_grouped(no_mask, cam)                     # without a mask every question has T tokens
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.testing.assert_close(got, current[False], rtol=1e-4, atol=1e-5)
