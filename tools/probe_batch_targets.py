"""Probe (GPU box): K targets per image over a batch of DISTINCT images in one pass, against K calls of the batch entries.

    python tools/probe_batch_targets.py            # interleaved A/B, medians of 7 after warm-up
    python tools/probe_batch_targets.py --kernels  # only the attention backward calls, for rocprofv3 --kernel-trace --stats

K = 5 targets per image, M = 64 images (T = 320 targets).  A/B pairs (same process, alternated call by call):
  * ViT-B/16 (random init): generate_relevance_batch_multi vs 5 x generate_relevance_batch (eager);
  * CLIP ViT-B/32 (random init), C = 100 prompts: interpret_batch_multi vs 5 x interpret_batch;
  * CLIP ViT-B/32, 5 captions per image: interpret_grouped vs interpret on the 320 repeated images (share_image_forward=False);
  * the capture backward alone at T = 320 (ViT-B/16 and CLIP ViT-B/32 image-tower shapes, need_dqkv): the grouped row mode
    (images = 64) vs the per-sample row mode on materialised per-target copies -- time per target.
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from transformer_mm_explainability_amd import clip_explainability as ce  # noqa: E402
from transformer_mm_explainability_amd import clip_model, ops, vit_model  # noqa: E402

M, K, C, REPS = 64, 5, 100, 7
T = M * K


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def ab(name_a, fa, name_b, fb, reps=REPS, per=T):
    for _ in range(2):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(wall(fa))
        tb.append(wall(fb))
    ma, mb = statistics.median(ta), statistics.median(tb)
    print("  A %-58s median %8.2f ms  (%7.1f maps/s)  min %8.2f" % (name_a, ma * 1e3, per / ma, min(ta) * 1e3))
    print("  B %-58s median %8.2f ms  (%7.1f maps/s)  min %8.2f" % (name_b, mb * 1e3, per / mb, min(tb) * 1e3))
    print("  A / B = %.3f" % (ma / mb))
    return ma, mb


def clip_texts(ctx, vocab, n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(n, ctx, dtype=torch.long)
    for c in range(n):
        L = 4 + c % 12
        t[c, 0] = vocab - 2
        t[c, 1:1 + L] = torch.randint(1, vocab - 2, (L,), generator=g)
        t[c, 1 + L] = vocab - 1
    return t


def attn_case(H, N, D, seed, dev):
    """One layer's capture backward at T = K * M targets over M images: (grouped call, per-sample call on copies)."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(M, N, 3, H, D, generator=g).to(dev)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    probs = torch.empty(M, H, N, N, device=dev)
    o = ops.attn_capture_fwd(q, k, v, probs, D ** -0.5)
    d_o = (torch.randn(T, N, H, D, generator=g) * 1e-2).to(dev)
    rel = torch.rand(T, N, generator=g).to(dev)
    img = torch.arange(T, device=dev) % M
    qc, kc, vc, pc, oc = q[img], k[img], v[img], probs[img].contiguous(), o[img]
    out = [torch.empty(T, N, H, D, device=dev) for _ in range(3)]

    def grouped():
        return ops.attn_capture_bwd(q, k, v, probs, d_o, None, D ** -0.5, rel_row=rel, o=o, out=out, images=M)[3]

    def copies():
        return ops.attn_capture_bwd(qc, kc, vc, pc, d_o, None, D ** -0.5, rel_row=rel, o=oc, out=out)[3]
    return grouped, copies


def main():
    kernels_only = "--kernels" in sys.argv
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    cases = {"ViT-B/16 layer (H 12, N 197, D 64)": attn_case(12, 197, 64, 1, dev),
             "CLIP ViT-B/32 image layer (H 12, N 50, D 64)": attn_case(12, 50, 64, 2, dev)}
    if kernels_only:
        for _ in range(3):
            for grouped, copies in cases.values():
                grouped()
                copies()
        torch.cuda.synchronize()
        print("kernels run done")
        return

    print("== capture backward alone, T = %d targets over M = %d images (need_dqkv, eager, 20 calls per sample)" % (T, M))
    for name, (grouped, copies) in cases.items():
        assert torch.equal(grouped(), copies())
        print(" %s: grouped == per-sample on copies, bit for bit" % name)

        def rep(fn):
            return lambda: [fn() for _ in range(20)]
        ta, tb = ab("grouped row mode (images = 64)", rep(grouped), "per-sample row mode on copies", rep(copies), per=20 * T)
        print("  per target: grouped %.3f us, per-sample %.3f us" % (ta / 20 / T * 1e6, tb / 20 / T * 1e6))

    vit = vit_model.vit_base_patch16_224().float().eval().to(dev)
    for p in vit.parameters():
        p.requires_grad_(False)
    images = torch.randn(M, 3, 224, 224, generator=g).to(dev)
    idx = torch.randint(0, 1000, (M, K), generator=g).to(dev)
    print("== ViT-B/16, M = %d distinct images, K = %d classes each" % (M, K))
    got = vit_model.generate_relevance_batch_multi(vit, images, idx)
    ref = torch.stack([vit_model.generate_relevance_batch(vit, images, idx[:, k]) for k in range(K)], 1)
    print("  max |batch_multi - 5 x batch| = %.3g" % float((got - ref).abs().max()))

    def five_vit():
        for k in range(K):
            vit_model.generate_relevance_batch(vit, images, idx[:, k])
    ab("generate_relevance_batch_multi (one forward, grouped bwd)", lambda: vit_model.generate_relevance_batch_multi(vit, images, idx),
       "5 x generate_relevance_batch", five_vit)
    del vit
    torch.cuda.empty_cache()

    clip = clip_model.random_init("ViT-B/32", seed=0).to(dev)
    cimages = torch.randn(M, 3, 224, 224, generator=g).to(dev)
    texts = clip_texts(77, 49408, C, 1).to(dev)
    cidx = torch.randint(0, C, (M, K), generator=g).to(dev)
    print("== CLIP ViT-B/32, C = %d prompts, M = %d distinct images, K = %d prompts each" % (C, M, K))
    got = ce.interpret_batch_multi(cimages, texts, clip, dev, index=cidx)
    ref = torch.stack([ce.interpret_batch(cimages, texts, clip, dev, index=cidx[:, k]) for k in range(K)], 1)
    print("  max |interpret_batch_multi - 5 x interpret_batch| = %.3g" % float((got - ref).abs().max()))

    def five_clip():
        for k in range(K):
            ce.interpret_batch(cimages, texts, clip, dev, index=cidx[:, k])
    ab("interpret_batch_multi (text once, one image fwd, grouped)", lambda: ce.interpret_batch_multi(cimages, texts, clip, dev, index=cidx),
       "5 x interpret_batch", five_clip)

    captions = clip_texts(77, 49408, T, 2).to(dev)
    rep_images = cimages.repeat_interleave(K, 0)
    print("== CLIP ViT-B/32, M = %d images x %d captions each (T = %d)" % (M, K, T))
    rt, ri = ce.interpret_grouped(cimages, captions, clip, dev)
    wt, wi = ce.interpret(rep_images, captions, clip, dev, share_image_forward=False)
    print("  max |R_text - interpret| = %.3g, max |R_image - interpret| = %.3g"
          % (float((rt - wt).abs().max()), float((ri - wi).abs().max())))
    ab("interpret_grouped (image fwd at M = 64, grouped row bwd)", lambda: ce.interpret_grouped(cimages, captions, clip, dev),
       "interpret on the 320 repeated images", lambda: ce.interpret(rep_images, captions, clip, dev, share_image_forward=False))


if __name__ == "__main__":
    main()
