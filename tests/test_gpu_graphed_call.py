"""-m gpu: ``graphed.capture`` on a toy call, and the two things the shared helpers changed or carry for the wrappers: ``GraphedRelevance``
keeps the ViT's slabs like the batch wrappers always did, and DETR's chunked K-slot replay runs through ``graphed.replay_slots``.
The helpers' host side (checked copies, slot filling) is ``tests/test_graphed_host.py``."""
import pytest
import torch

from test_gpu_detr_baselines_multi import _body as detr_body
from test_gpu_vit import build as build_vit

pytestmark = pytest.mark.gpu


def test_capture_on_a_toy_call():
    from transformer_mm_explainability_amd import graphed, ops
    gen = torch.Generator().manual_seed(0)
    cam, grad = torch.rand(2, 3, 5, 5, generator=gen).cuda(), torch.randn(2, 3, 5, 5, generator=gen).cuda()
    bias = torch.randn(2, 5, 5, generator=gen).cuda()
    calls = [0]

    def call():
        calls[0] += 1
        return ops.avg_heads(cam, grad, batch_size=2) + bias

    graph, out, pinned = graphed.capture(call, warmup=2, keep=(cam, grad))
    assert calls[0] == 2 + 1                                            # the warm-up calls and the captured one
    assert isinstance(pinned, list) and len(pinned) >= 2 and pinned[-2] is cam and pinned[-1] is grad
    assert hasattr(graph, "_mmx_private")                               # captured through ops.graph_capture
    for seed in (1, 2):
        gen = torch.Generator().manual_seed(seed)
        cam.copy_(torch.rand(2, 3, 5, 5, generator=gen))
        grad.copy_(torch.randn(2, 3, 5, 5, generator=gen))
        graph.replay()
        assert calls[0] == 3                                            # a replay runs no Python
        assert torch.equal(out, ops.avg_heads(cam, grad, batch_size=2) + bias)


def test_graphed_relevance_keeps_the_slabs_its_graph_was_captured_on():
    """An eager call at another batch size makes the model install new slabs; the wrapper still holds the ones its graph reads and
    writes, and replays the same bits.  (Nothing here frees or overwrites the old slabs: the reference and the values are what is
    asserted.)"""
    from transformer_mm_explainability_amd import vit_model
    model = build_vit(64, 16, 128, 3, 2, classes=11).cuda()
    image = torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    run = vit_model.GraphedRelevance(model, image, indices=[3, 7])
    slabs = model.buffers_
    assert slabs is not None and run.buffers is slabs
    before = run(image, [3, 7]).clone()
    vit_model.generate_relevance_batch(model, torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(2)).cuda())
    assert model.buffers_ is not slabs                                  # (the eager call did replace them)
    assert run.buffers is slabs
    assert torch.equal(run(image, [3, 7]), before)


def test_graphed_baselines_multi_chunks_through_the_shared_loop():
    """K = 2 slots, 3 targets: two replays, the second with a spare slot.  Raw attention has no batch size in it, so the eager call on
    the plain list gives the same bits (``test_replays_are_bit_equal_to_the_eager_multi_call``)."""
    from transformer_mm_explainability_amd.detr_explainability import Generator, GraphedBaselinesMulti
    model, feats, _ = detr_body("small")
    targets = torch.tensor([8, 0, 3], device="cuda")
    run = GraphedBaselinesMulti(model, feats, "raw_attn", K=2)
    got = run(feats, targets)
    want = Generator(model).generate_raw_attn_multi(feats, targets)
    assert got.shape == want.shape == (1, 1, 3, feats.shape[-1] * feats.shape[-2])
    assert torch.equal(got, want)
