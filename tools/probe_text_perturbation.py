"""Probe (GPU box): the caption perturbation test (clip_text_perturbation.py) on ViT-B/32 with the 64 captions of
bench.synthetic_inputs and the default S = 9 steps.

    python tools/probe_text_perturbation.py tokens      # ops.perturb_tokens vs lxmert_perturbation.text_keep_batches on the device
    python tools/probe_text_perturbation.py forward     # encode_text_nocapture on the 576 perturbed captions: live=True vs live=False
    python tools/probe_text_perturbation.py evaluator   # TokenPerturbation vs text_keep_batches + the dense forward per step

Each part is its own process (run each under its own `timeout`).  Device events around every timed call, every shape warmed,
A and B alternated call by call, medians of REPS = 20.  The A/A line times the SAME call against itself in that interleaving:
a difference between two variants means something only beyond it.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from transformer_mm_explainability_amd import clip_model, ops  # noqa: E402
from transformer_mm_explainability_amd import clip_text_perturbation as tp  # noqa: E402
from transformer_mm_explainability_amd.lxmert_perturbation import PERT_STEPS, text_keep_batches  # noqa: E402

REPS = 20
DEV = "cuda"
B = 64
S = len(PERT_STEPS)


def timed(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner                                      # ms per call


def interleaved(fns, reps=REPS, warm=3, inner=1):
    """Medians (ms per call) of ``fns`` (a dict name -> callable), alternated sample by sample; a sample is ``inner`` calls back
    to back between two events."""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(timed(f, inner))
    return {k: statistics.median(v) for k, v in t.items()}


def spread(a, b):
    return 100 * abs(a - b) / min(a, b)


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


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() / 2 ** 20, base / 2 ** 20


def inputs():
    _, texts = bench.synthetic_inputs(B, DEV, 0)
    cam = torch.rand(B, 77, generator=torch.Generator().manual_seed(7)).to(DEV)
    counts = torch.tensor(tp.token_step_counts(PERT_STEPS, 77), dtype=torch.int32, device=DEV)
    return texts, cam, counts


def torch_composition(texts, cam, lens, types):
    """The S perturbed copies by the project's torch statement of the rule -> ids [B * S, 77], a caption's copies adjacent."""
    return text_keep_batches(texts, types, cam, PERT_STEPS, False, n_tokens=lens)[0]


def part_tokens():
    texts, cam, counts = inputs()
    lens = (texts.argmax(dim=-1) + 1).tolist()                            # (read once, outside the timed calls: the caller's knowledge)
    types = torch.zeros_like(texts)
    ids, eot = ops.perturb_tokens(texts, cam, counts)
    want = torch_composition(texts, cam, lens, types).view(B, S, 77).transpose(0, 1)
    assert torch.equal(ids, want) and torch.equal(eot, want.argmax(dim=-1))
    f_new = lambda: ops.perturb_tokens(texts, cam, counts)                # noqa: E731
    f_old = lambda: torch_composition(texts, cam, lens, types)            # noqa: E731
    m = interleaved({"new_a": f_new, "torch": f_old, "new_b": f_new}, inner=10)
    print("== ops.perturb_tokens vs text_keep_batches on the device, %d captions x %d steps; same ids, bit for bit; samples of 10 calls" % (B, S))
    print("    mmx_perturb_tokens  %8.4f ms (A/A %8.4f, spread %.1f %%)   device launches: %s"
          % (m["new_a"], m["new_b"], spread(m["new_a"], m["new_b"]), count_launches(f_new)))
    print("    text_keep_batches   %8.4f ms   device launches: %s   (builds two tensors from host lists per call)"
          % (m["torch"], count_launches(f_old)))


def part_forward():
    texts, cam, counts = inputs()
    model = clip_model.random_init("ViT-B/32", seed=0).to(DEV)
    for p in model.parameters():
        p.requires_grad_(False)
    ids, eot = ops.perturb_tokens(texts, cam, counts)
    flat, flat_eot = ids.view(S * B, 77), eot.view(S * B)
    share = float((flat_eot + 1).sum()) / (S * B * 77)
    dense = lambda: model.encode_text_nocapture(flat, live=False, eot=flat_eot)       # noqa: E731
    route = lambda: model.encode_text_nocapture(flat, live=True, eot=flat_eot)        # noqa: E731
    err = float((dense() - route()).abs().max())
    m = interleaved({"dense_a": dense, "route": route, "dense_b": dense})
    d = 0.5 * (m["dense_a"] + m["dense_b"])
    print("== encode_text_nocapture on the %d perturbed captions (ViT-B/32 text tower): live rows %.1f %% of %d" % (S * B, 100 * share, S * B * 77))
    print("    max |route features - dense features| = %.3g" % err)
    print("    live=False (dense)  %8.3f ms   A/A spread %.1f %%   peak %6.0f MiB" % (d, spread(m["dense_a"], m["dense_b"]), peak(dense)[0]))
    print("    live=True  (route)  %8.3f ms   route / dense %.3f   peak %6.0f MiB" % (m["route"], m["route"] / d, peak(route)[0]))
    ops.set_option("text_live_attn", 0)
    m2 = interleaved({"route_dense_attn": route, "dense": dense})
    ops.set_option("text_live_attn", 1)
    print("    live=True, option text_live_attn 0 (dense attention over a zero-filled qkv)  %8.3f ms (dense in the same interleaving %8.3f)"
          % (m2["route_dense_attn"], m2["dense"]))
    # the unperturbed captions alone (what the default targets cost)
    m3 = interleaved({"dense_a": lambda: model.encode_text_nocapture(texts, live=False), "route": lambda: model.encode_text_nocapture(texts, live=True),
                      "dense_b": lambda: model.encode_text_nocapture(texts, live=False)})
    print("    the %d unperturbed captions (live rows %.1f %%): dense %8.3f ms (A/A %8.3f), route %8.3f ms"
          % (B, 100 * float((texts.argmax(-1) + 1).sum()) / (B * 77), m3["dense_a"], m3["dense_b"], m3["route"]))


def part_evaluator():
    texts, cam, counts = inputs()
    model = clip_model.random_init("ViT-B/32", seed=0).to(DEV)
    for p in model.parameters():
        p.requires_grad_(False)
    images = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
    scorer = tp.ClipCaptionScorer(model, images)
    lens = (texts.argmax(dim=-1) + 1).tolist()
    types = torch.zeros_like(texts)

    def baseline():
        ids = torch_composition(texts, cam, lens, types).view(B, S, 77)
        return torch.stack([scorer.logits(ids[:, s]) for s in range(S)])

    dense, route = tp.TokenPerturbation(scorer, live=False), tp.TokenPerturbation(scorer, live=True)
    print("== TokenPerturbation, %d captions against 8 images, S = %d: ms are medians of %d, alternated" % (B, S, REPS))
    print("    max |dense logits - baseline logits| = %.3g, max |route logits - baseline logits| = %.3g"
          % (float((dense(texts, cam).logits - baseline()).abs().max()), float((route(texts, cam).logits - baseline()).abs().max())))
    fns = {"base_a": baseline, "dense": lambda: dense(texts, cam), "route": lambda: route(texts, cam), "base_b": baseline}
    m = interleaved(fns, warm=2)
    base = 0.5 * (m["base_a"] + m["base_b"])
    print("    A/A spread of the baseline: %.1f %%" % spread(m["base_a"], m["base_b"]))
    for name, ms, fn in (("baseline: text_keep_batches + the dense forward per step", base, baseline),
                         ("TokenPerturbation live=False (576 captions in one batch + the 64 targets)", m["dense"], fns["dense"]),
                         ("TokenPerturbation live=True", m["route"], fns["route"])):
        mem = peak(fn)
        print("    %-78s %9.2f ms per batch  %7.1f captions/s  peak %7.0f MiB (resident before %6.0f)" % (name, ms, B / ms * 1e3, mem[0], mem[1]))


if __name__ == "__main__":
    parts = {"tokens": part_tokens, "forward": part_forward, "evaluator": part_evaluator}
    if len(sys.argv) != 2 or sys.argv[1] not in parts:
        raise SystemExit("usage: python tools/probe_text_perturbation.py tokens | forward | evaluator")
    print("device: %s" % torch.cuda.get_device_name(0))
    parts[sys.argv[1]]()
