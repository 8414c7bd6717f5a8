"""Probe (GPU box): explaining a batch of DISTINCT images in one pass, against the per-image entries.

    python tools/probe_batch_images.py            # interleaved A/B, medians of 7 after warm-up
    python tools/probe_batch_images.py --kernels  # only the attention backward calls, for rocprofv3 --kernel-trace --stats

A/B pairs (same process, alternated call by call):
  * ViT-B/16 (random init), B = 64 distinct images: GraphedRelevanceBatch vs a loop of 64 GraphedRelevance (K = 1) replays;
    eager generate_relevance_batch (fused exact-fp32 row) vs the same tape backward with dP slabs + avg_heads_vecmat per layer;
  * CLIP ViT-B/32 (random init), C = 100 prompts, B = 64 images: interpret_batch vs a loop of interpret_single.
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from transformer_mm_explainability_amd import clip_explainability as ce  # noqa: E402
from transformer_mm_explainability_amd import clip_model, ops, vit_model  # noqa: E402

B, C, REPS = 64, 100, 7


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def ab(name_a, fa, name_b, fb, reps=REPS, per=B):
    for _ in range(2):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(wall(fa))
        tb.append(wall(fb))
    ma, mb = statistics.median(ta), statistics.median(tb)
    print("  A %-52s median %8.2f ms  (%7.1f maps/s)  min %8.2f" % (name_a, ma * 1e3, per / ma, min(ta) * 1e3))
    print("  B %-52s median %8.2f ms  (%7.1f maps/s)  min %8.2f" % (name_b, mb * 1e3, per / mb, min(tb) * 1e3))
    print("  A / B = %.3f" % (ma / mb))
    return ma, mb


def vit_slab_route(model, images, idx):
    """generate_relevance_batch's tape forward / backward with dP slabs and avg_heads_vecmat per layer (the slab route)."""
    logits, state = model.forward_tape(images, grads=True)
    d_logits = torch.zeros(B, logits.shape[-1], device=images.device).scatter_(1, idx.reshape(B, 1), 1.0)
    buf = model.buffers_
    N = buf.probs.shape[-1]
    row = [torch.zeros(B, N, device=images.device)]
    row[0][:, 0] = 1.0

    def rule(l):
        row[0] = ops.avg_heads_vecmat(row[0], buf.probs[l], buf.grads[l], batch_size=B)
    model.backward_tape(state, d_logits, on_layer_done=rule)
    return row[0][:, 1:]


def clip_texts(cfg_ctx, vocab, n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(n, cfg_ctx, dtype=torch.long)
    for c in range(n):
        L = 4 + c % 12
        t[c, 0] = vocab - 2
        t[c, 1:1 + L] = torch.randint(1, vocab - 2, (L,), generator=g)
        t[c, 1 + L] = vocab - 1
    return t


def main():
    kernels_only = "--kernels" in sys.argv
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    vit = vit_model.vit_base_patch16_224().float().eval().to(dev)
    for p in vit.parameters():
        p.requires_grad_(False)
    images = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    idx = torch.randint(0, 1000, (B,), generator=g).to(dev)
    clip = clip_model.random_init("ViT-B/32", seed=0).to(dev)
    cimages = torch.randn(B, 3, 224, 224, generator=g).to(dev)
    texts = clip_texts(77, 49408, C, 1).to(dev)
    cidx = torch.randint(0, C, (B,), generator=g).to(dev)

    if kernels_only:
        # 3 calls of each route: the kernel table tells the rowrel instantiations (REL = true) from the plain ones
        for _ in range(3):
            vit_model.generate_relevance_batch(vit, images, idx)
            vit_slab_route(vit, images, idx)
            ce.interpret_batch(cimages, texts, clip, dev, index=cidx)
            # CLIP image tower with slabs: same tape, grads stored, then the slab rule
            with torch.no_grad():
                feat, st = clip.visual.forward_tape(cimages, first_grad_layer=0, grads=True)
                clip.visual.backward_tape(st, torch.randn_like(feat), 0)
        torch.cuda.synchronize()
        print("kernels run done")
        return

    print("== ViT-B/16, B = %d distinct images, one class each" % B)
    err = float((vit_model.generate_relevance_batch(vit, images, idx) - vit_slab_route(vit, images, idx)).abs().max())
    print("  max |fused row - slab route| = %.3g" % err)
    ab("generate_relevance_batch (eager, fused fp32 row)", lambda: vit_model.generate_relevance_batch(vit, images, idx),
       "tape backward + dP slabs + avg_heads_vecmat (eager)", lambda: vit_slab_route(vit, images, idx))
    run_b = vit_model.GraphedRelevanceBatch(vit, images, indices=idx)
    run_1 = vit_model.GraphedRelevance(vit, images[:1], indices=idx[:1])
    pinned = run_b.buffers        # noqa: F841  (the per-image graph re-installed other slabs on the model)

    def loop_1():
        for b in range(B):
            run_1(images[b:b + 1], idx[b:b + 1])
    ab("GraphedRelevanceBatch replay (B = 64)", lambda: run_b(images, idx),
       "64 x GraphedRelevance replay (K = 1)", loop_1)

    print("== CLIP ViT-B/32, C = %d prompts, B = %d distinct images" % (C, B))
    got = ce.interpret_batch(cimages, texts, clip, dev, index=cidx)
    ref = torch.stack([ce.interpret_single(cimages[b:b + 1], texts, clip, dev, index=int(cidx[b])) for b in range(B)])
    print("  max |interpret_batch - interpret_single loop| = %.3g" % float((got - ref).abs().max()))
    cl = [int(i) for i in cidx.cpu()]

    def loop_single():
        for b in range(B):
            ce.interpret_single(cimages[b:b + 1], texts, clip, dev, index=cl[b])
    ab("interpret_batch (text encoded once, fused row)", lambda: ce.interpret_batch(cimages, texts, clip, dev, index=cidx),
       "64 x interpret_single", loop_single, reps=5)


if __name__ == "__main__":
    main()
