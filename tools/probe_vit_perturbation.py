"""Probe (GPU box): the image perturbation test (vit_perturbation.py) and its three kernels.

    python tools/probe_vit_perturbation.py attn       # mmx_attn_fwd vs mmx_attn_capture_fwd_ex, A/A spread first
    python tools/probe_vit_perturbation.py patches    # mmx_patch_ranks / mmx_perturb_patches vs the torch composition
    python tools/probe_vit_perturbation.py evaluator  # PatchPerturbation vs the route a user can assemble without it

Each part is its own process (run each under its own `timeout`).  Device events around every timed call, every shape warmed,
A and B alternated call by call, medians of REPS = 20.  The A/A line times the SAME call against itself in that interleaving:
a difference between two variants means something only beyond it.
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from transformer_mm_explainability_amd import clip_model, ops, vit_model  # noqa: E402
from transformer_mm_explainability_amd import vit_perturbation as vp  # noqa: E402
from transformer_mm_explainability_amd.lxmert_perturbation import _ranks, ranking  # noqa: E402

REPS = 20
DEV = "cuda"


def timed(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner                                      # ms per call


def interleaved(fns, reps=REPS, warm=3, inner=1):
    """Medians (ms per call) of ``fns`` (a dict name -> callable), alternated sample by sample; a sample is ``inner`` calls
    back to back between two events (kernels of tens of microseconds: a single launch would time the launch gap too)."""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(timed(f, inner))
    return {k: statistics.median(v) for k, v in t.items()}


def part_attn():
    H, D = 12, 64
    print("== mmx_attn_fwd (no slab) vs mmx_attn_capture_fwd_ex (fp32 slab), H = %d, D = %d; ms per call are medians of %d samples of 10 calls" % (H, D, REPS))
    print("   bytes = q, k, v, o; FLOP = 2 products (4 B H N^2 D); 'A/A' = the capture call timed against itself")
    for B in (64, 576):
        for N, causal in ((50, False), (77, True), (197, False), (577, False)):
            g = torch.Generator().manual_seed(N + B)
            qkv = torch.randn(B, N, 3, H, D, generator=g).to(DEV)
            q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
            mask = torch.full((N, N), float("-inf")).triu_(1).to(DEV) if causal else None
            probs = torch.empty(B, H, N, N, device=DEV)
            out = torch.empty(B, N, H, D, device=DEV)
            cap = lambda: ops.attn_capture_fwd(q, k, v, probs, D ** -0.5, mask=mask)          # noqa: E731
            new = lambda: ops.attn_fwd(q, k, v, D ** -0.5, mask=mask, out=out)                 # noqa: E731
            m = interleaved({"cap_a": cap, "new": new, "cap_b": cap}, inner=10)
            spread = abs(m["cap_a"] - m["cap_b"]) / min(m["cap_a"], m["cap_b"])
            capt = 0.5 * (m["cap_a"] + m["cap_b"])
            nbytes, flop = 4.0 * B * N * H * D * 4, 4.0 * B * H * N * N * D
            print("  B %3d N %3d%s  capture %8.3f ms  no-capture %8.3f ms  new/capture %.3f  A/A spread %.1f %%  |  no-capture: "
                  "%6.1f GB/s  %6.2f TFLOP/s   capture slab %7.1f MB not written"
                  % (B, N, " causal" if causal else "       ", capt, m["new"], m["new"] / capt, 100 * spread,
                     nbytes / m["new"] / 1e6, flop / m["new"] / 1e9, probs.numel() * 4 / 1e6))
            del qkv, probs, out
            torch.cuda.empty_cache()


def torch_composition(images, cam, counts, fill, patch):
    """What produces the same tensors without the two kernels: sort + scatter_ (ranks), comparison + where (copies)."""
    B, C, R, _ = images.shape
    G = R // patch
    ranks = _ranks(ranking(cam))
    pix = ranks.view(B, G, G).repeat_interleave(patch, dim=1).repeat_interleave(patch, dim=2)
    keep = pix.view(1, B, 1, R, R) < counts.view(-1, 1, 1, 1, 1)
    return ranks, torch.where(keep, images.unsqueeze(0), fill.view(1, 1, C, 1, 1))


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:                                             # the count is a side note: not measured is an answer
        return "not measured (%s)" % type(exc).__name__


def part_patches():
    S, C = 9, 3
    print("== mmx_patch_ranks + mmx_perturb_patches vs the torch composition (sort, scatter_, repeat_interleave, <, where), S = %d; samples of 10 calls" % S)
    for B, P, R, patch in ((64, 196, 224, 16), (64, 576, 336, 14)):
        g = torch.Generator().manual_seed(P)
        images = torch.randn(B, C, R, R, generator=g).to(DEV)
        cam = torch.rand(B, P, generator=g).to(DEV)
        counts = torch.tensor(vp.step_counts(vp.PERT_STEPS, P), dtype=torch.int32, device=DEV)
        fill = torch.tensor([0.1, 0.2, 0.3], device=DEV)
        ranks = ops.patch_ranks(cam)
        out = torch.empty(S, B, C, R, R, device=DEV)
        want_r, want = torch_composition(images, cam, counts, fill, patch)
        assert torch.equal(ranks.long(), want_r) and torch.equal(ops.perturb_patches(images, ranks, counts, fill, out=out), want)
        del want
        f_rank = lambda: ops.patch_ranks(cam)                                                   # noqa: E731
        f_pert = lambda: ops.perturb_patches(images, ranks, counts, fill, out=out)              # noqa: E731
        f_torch = lambda: torch_composition(images, cam, counts, fill, patch)                   # noqa: E731
        m = interleaved({"ranks_a": f_rank, "perturb": f_pert, "torch": f_torch, "ranks_b": f_rank}, inner=10)
        wbytes = 4.0 * S * B * C * R * R
        print("  B %d P %d R %d patch %d: same tensors, bit for bit" % (B, P, R, patch))
        print("    mmx_patch_ranks     %8.3f ms (A/A %8.3f)   1 launch" % (m["ranks_a"], m["ranks_b"]))
        print("    mmx_perturb_patches %8.3f ms   %7.1f GB/s written (%.0f MB), %7.1f GB/s with the read   1 launch"
              % (m["perturb"], wbytes / m["perturb"] / 1e6, wbytes / 1e6, (wbytes + wbytes / S) / m["perturb"] / 1e6))
        print("    torch composition   %8.3f ms   device launches: %s" % (m["torch"], count_launches(f_torch)))
        del images, out
        torch.cuda.empty_cache()


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20, base / 2 ** 20


def report(name, ms, n_images, mem):
    print("    %-64s %9.2f ms per batch  %7.1f images/s  peak %8.0f MiB (resident before the call %6.0f)"
          % (name, ms, n_images / ms * 1e3, mem[0], mem[1]))


def part_evaluator():
    B = 64
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    images = torch.randn(B, 3, 224, 224, generator=g).to(DEV)
    fill = torch.zeros(3, device=DEV)
    print("== the evaluator, %d images, default steps (S = %d): ms are medians of %d, alternated" % (B, len(vp.PERT_STEPS), REPS))

    vit = vit_model.vit_base_patch16_224().float().eval().to(DEV)
    for p in vit.parameters():
        p.requires_grad_(False)
    cam = torch.rand(B, 196, generator=g).to(DEV)
    counts = torch.tensor(vp.step_counts(vp.PERT_STEPS, 196), device=DEV)

    def baseline_vit():
        _, pert = torch_composition(images, cam, counts, fill, 16)
        return torch.stack([vit.forward_tape(pert[s], grads=False)[0] for s in range(pert.shape[0])])

    scorer = vp.VitScorer(vit)
    zero, drop = vp.PatchPerturbation(scorer, mode="zero"), vp.PatchPerturbation(scorer, mode="drop")
    zero64 = vp.PatchPerturbation(scorer, mode="zero", max_batch=B)
    err = float((zero(images, cam).logits - baseline_vit()).abs().max())
    print("  ViT-B/16 (random weights): max |zero-mode logits - baseline logits| = %.3g" % err)
    fns = {"base_a": baseline_vit, "zero": lambda: zero(images, cam), "zero64": lambda: zero64(images, cam),
           "drop": lambda: drop(images, cam), "base_b": baseline_vit}
    m = interleaved(fns, warm=2)
    print("    A/A spread of the baseline: %.1f %%" % (100 * abs(m["base_a"] - m["base_b"]) / min(m["base_a"], m["base_b"])))
    report("baseline: torch ranking + masking, forward_tape(grads=False) per step", 0.5 * (m["base_a"] + m["base_b"]), B, peak(baseline_vit))
    vit.buffers_ = None
    report("PatchPerturbation zero mode (576 images in one batch)", m["zero"], B, peak(fns["zero"]))
    report("PatchPerturbation zero mode, max_batch = 64", m["zero64"], B, peak(fns["zero64"]))
    report("PatchPerturbation drop mode", m["drop"], B, peak(fns["drop"]))
    del vit, scorer, zero, drop, zero64, fns
    torch.cuda.empty_cache()

    clip = clip_model.random_init("ViT-B/32", seed=0).to(DEV)
    for p in clip.parameters():
        p.requires_grad_(False)
    texts = torch.zeros(100, 77, dtype=torch.long)
    for c in range(100):
        L = 4 + c % 12
        texts[c, 0], texts[c, 1 + L] = 49406, 49407
        texts[c, 1:1 + L] = torch.randint(1, 49406, (L,), generator=g)
    texts = texts.to(DEV)
    cam = torch.rand(B, 49, generator=g).to(DEV)
    counts = torch.tensor(vp.step_counts(vp.PERT_STEPS, 49), device=DEV)
    tf, _ = clip.encode_text_tape(texts)
    tf = tf / tf.norm(dim=-1, keepdim=True)
    clip.transformer.buffers = None
    scale = clip.logit_scale.exp()

    def baseline_clip():
        _, pert = torch_composition(images, cam, counts, fill, 32)
        rows = []
        for s in range(pert.shape[0]):
            f, _ = clip.visual.forward_tape(pert[s], grads=False)
            rows.append(scale * (f / f.norm(dim=-1, keepdim=True)) @ tf.t())
        return torch.stack(rows)

    scorer = vp.ClipZeroShotScorer(clip, texts)
    zero, drop = vp.PatchPerturbation(scorer, mode="zero"), vp.PatchPerturbation(scorer, mode="drop")
    err = float((zero(images, cam).logits - baseline_clip()).abs().max())
    print("  CLIP ViT-B/32 (random weights), 100 prompts: max |zero-mode logits - baseline logits| = %.3g" % err)
    fns = {"base_a": baseline_clip, "zero": lambda: zero(images, cam), "drop": lambda: drop(images, cam), "base_b": baseline_clip}
    m = interleaved(fns, warm=2)
    print("    A/A spread of the baseline: %.1f %%" % (100 * abs(m["base_a"] - m["base_b"]) / min(m["base_a"], m["base_b"])))
    report("baseline: torch ranking + masking, visual.forward_tape(grads=False) per step", 0.5 * (m["base_a"] + m["base_b"]), B,
           peak(baseline_clip))
    clip.visual.transformer.buffers = None
    report("PatchPerturbation zero mode (576 images in one batch)", m["zero"], B, peak(fns["zero"]))
    report("PatchPerturbation drop mode", m["drop"], B, peak(fns["drop"]))


if __name__ == "__main__":
    parts = {"attn": part_attn, "patches": part_patches, "evaluator": part_evaluator}
    if len(sys.argv) != 2 or sys.argv[1] not in parts:
        raise SystemExit("usage: python tools/probe_vit_perturbation.py attn | patches | evaluator")
    print("device: %s" % torch.cuda.get_device_name(0))
    parts[sys.argv[1]]()
