"""Probe (GPU box): the perturbation test of VisualBERT at the shape of the evaluator (``examples/visualbert_pert_eval.py``: BERT-base
VisualBERT, B = 32 questions of 8..20 tokens padded to 24, 100 regions).

    python tools/probe_visualbert_perturbation.py perturb image       # | text
    python tools/probe_visualbert_perturbation.py kernels
    python tools/probe_visualbert_perturbation.py oracle
    python tools/probe_visualbert_perturbation.py evaluator rollout   # | any --method of the evaluator

``perturb``: the 9-step test of 32 items three ways -- a loop of 32 ``perturbation_image`` / ``perturbation_text`` calls (the parent's
route, the yardstick), ``perturbation_*_batch`` eager, and ``GraphedVisualBertPerturbation`` replayed.
``kernels``: the two builder launches alone (``ops.selfattn_perturb_regions`` / ``ops.selfattn_perturb_text``) against the torch
composition the per-item route runs per item (``image_keep_masks`` / ``text_keep_batch``), here for the 32 items.
``oracle``: the distance of the batched and of the per-item scores from a float64 run of ``oracle.visualbert_torch.forward`` on the same
physically perturbed inputs (two items, both tests).  A record, not a gate.
``evaluator``: ``examples/visualbert_pert_eval.py --num-samples 256 --explain-batch 32`` end to end, as child processes, with
``--perturb-batch 32`` and without, alternated, ``samples_per_s`` as the evaluator prints it.

Each invocation is its own process (run each under its own `timeout`).  A host clock around work that ends in a device synchronise,
device events for the kernels; every variant warmed, variants alternated sample by sample inside the process, medians of REPS = 20.  The
A/A lines time the SAME variant twice in that interleaving: a difference between two variants means something only beyond that spread.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from transformer_mm_explainability_amd import ops  # noqa: E402
from transformer_mm_explainability_amd import visualbert_explainability as vb  # noqa: E402
from transformer_mm_explainability_amd import visualbert_model as vm  # noqa: E402
from transformer_mm_explainability_amd import visualbert_perturbation as vp  # noqa: E402
from transformer_mm_explainability_amd.lxmert_perturbation import image_keep_masks  # noqa: E402

REPS = 20
DEV = "cuda"
B, T_PAD, REGIONS, FEAT = 32, 24, 100, 2048
KEYS = ("input_ids", "input_mask", "segment_ids", "image_feature_0")


def spread(a, b):
    return 100 * abs(a - b) / min(a, b)


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_timed(fn, inner=10):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def interleaved(fns, timer, reps=REPS, warm=3):
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t[k].append(timer(f))
    return {k: statistics.median(v) for k, v in t.items()}


def batch_and_cams(cfg, seed=0):
    """The evaluator's synthetic questions (8..20 tokens padded to 24) and a random relevancy row per item, zeros at the padding."""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(8, 21, (B,), generator=g).tolist()
    ids, mask = torch.zeros(B, T_PAD, dtype=torch.long), torch.zeros(B, T_PAD, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, cfg.vocab_size, (n,), generator=g)
        mask[b, :n] = 1
    batch = {"input_ids": ids.to(DEV), "input_mask": mask.to(DEV), "segment_ids": torch.zeros(B, T_PAD, dtype=torch.long, device=DEV),
             "image_feature_0": torch.randn(B, REGIONS, FEAT, generator=g).to(DEV)}
    cams = torch.rand(B, T_PAD + REGIONS, generator=g) * mask_row(mask)
    return batch, cams.to(DEV), lens


def mask_row(mask):
    return torch.cat((mask.float(), torch.ones(mask.shape[0], REGIONS)), dim=1)


def model_and_pert():
    cfg = vm.VisualBertConfig()
    torch.manual_seed(0)
    model = vm.VisualBERT(cfg).to(DEV).eval()
    return cfg, model, vp.VisualBertPerturbation(model)


def per_item_scores(pert, batch, cams, lens, modality, positive=False, items=None):
    run = pert.perturbation_image if modality == "image" else pert.perturbation_text
    return [run({k: batch[k][b:b + 1] for k in KEYS}, vb.unpad_row(cams, b, lens[b], padded_text=T_PAD), positive)
            for b in (range(B) if items is None else items)]


def part_perturb(modality):
    cfg, model, pert = model_and_pert()
    batch, cams, lens = batch_and_cams(cfg)
    batched = pert.perturbation_image_batch if modality == "image" else pert.perturbation_text_batch
    rows = [vb.unpad_row(cams, b, n, padded_text=T_PAD) for b, n in enumerate(lens)]       # (the evaluator holds these per item)
    run = pert.perturbation_image if modality == "image" else pert.perturbation_text

    def per_item():
        return [run({k: batch[k][b:b + 1] for k in KEYS}, rows[b]) for b in range(B)]

    def eager():
        return batched(batch, cams)

    graphed = vp.GraphedVisualBertPerturbation(pert, batch, cams, modality)

    def replay():
        return graphed(batch, cams)

    want, got_e, got_g = torch.stack(per_item()), eager().clone(), replay().clone()
    print("== %s test, BERT-base VisualBERT, B = %d questions of %d..%d tokens padded to %d, %d regions, 9 steps"
          % (modality, B, min(lens), max(lens), T_PAD, REGIONS))
    print("    max |batched - per item| over the scores = %.3g (largest score %.3g); same arg-max answers: %s; graphed == eager bit for bit: %s"
          % (float((got_e - want).abs().max()), float(want.abs().max()), bool(torch.equal(got_e.argmax(-1), want.argmax(-1))),
             bool(torch.equal(got_e, got_g))))
    m = interleaved({"item_a": per_item, "eager_a": eager, "graph_a": replay, "item_b": per_item, "eager_b": eager, "graph_b": replay},
                    host_timed, warm=2)
    item, eag, graph = (0.5 * (m[k + "_a"] + m[k + "_b"]) for k in ("item", "eager", "graph"))
    print("    per-item loop (%d calls)   %9.2f ms per batch  %8.1f samples/s   A/A %9.2f / %9.2f ms, spread %.1f %%"
          % (B, item, B / item * 1e3, m["item_a"], m["item_b"], spread(m["item_a"], m["item_b"])))
    print("    batched, eager             %9.2f ms per batch  %8.1f samples/s   per-item / batched %.1fx   A/A %9.2f / %9.2f ms, spread %.1f %%"
          % (eag, B / eag * 1e3, item / eag, m["eager_a"], m["eager_b"], spread(m["eager_a"], m["eager_b"])))
    print("    batched, graph replay      %9.2f ms per batch  %8.1f samples/s   per-item / graphed %.1fx   A/A %9.2f / %9.2f ms, spread %.1f %%"
          % (graph, B / graph * 1e3, item / graph, m["graph_a"], m["graph_b"], spread(m["graph_a"], m["graph_b"])))
    if modality == "image":
        k = pert._batch_constants(T_PAD, REGIONS, B, torch.device(DEV))
        print("    packed rows per batch: %d in %d segments (the masked per-item route runs %d)" % (k["rows"], len(k["segments"]), 9 * sum(n + REGIONS for n in lens)))


def part_kernels():
    cfg = vm.VisualBertConfig()
    batch, cams, lens = batch_and_cams(cfg, seed=1)
    E = cfg.hidden_size
    emb = torch.randn(B, T_PAD + REGIONS, E, device=DEV)
    text_len = batch["input_mask"].sum(dim=1).to(torch.int32)
    groups, _ = vp.image_step_groups(vp.IMAGE_STEPS, REGIONS)
    counts = torch.tensor(groups, dtype=torch.int32, device=DEV)
    rows = vp.group_offsets(groups, T_PAD, B)[1]
    text_counts = torch.tensor(vp.text_step_counts(vp.TEXT_STEPS, T_PAD), dtype=torch.int32, device=DEV)
    out_r = ops.selfattn_perturb_regions(emb, cams, text_len, counts, rows, T_PAD)
    out_t = ops.selfattn_perturb_text(batch["input_ids"], batch["segment_ids"], cams, text_len, text_counts)

    def regions_hip():
        return ops.selfattn_perturb_regions(emb, cams, text_len, counts, rows, T_PAD, out=out_r)

    def regions_torch():                                # what perturbation_image builds per item: the [S, V] keep masks
        return [image_keep_masks(cams[b, T_PAD:], vp.IMAGE_STEPS) for b in range(B)]

    def text_hip():
        return ops.selfattn_perturb_text(batch["input_ids"], batch["segment_ids"], cams, text_len, text_counts, out=out_t)

    def text_torch():                                   # what perturbation_text builds per item (lengths already on the host)
        return [vp.text_keep_batch(batch["input_ids"][b:b + 1, :n], batch["segment_ids"][b:b + 1, :n], cams[b, 1:n - 2], n, vp.TEXT_STEPS)
                for b, n in enumerate(lens)]

    print("== the builder launches alone, B = %d, T = %d, V = %d, E = %d; samples of 10 calls between two events" % (B, T_PAD, REGIONS, E))
    print("    regions: %d packed rows of %d floats written (%.1f MiB), %d x %d read" % (rows, E, rows * E * 4 / 2 ** 20, B * (T_PAD + REGIONS), E))
    # (image_keep_masks builds masks only -- the per-item route gathers nothing -- so that line carries no ratio: not like for like)
    for name, new, old, what, like in (("perturb_regions (1 launch)", regions_hip, regions_torch, "image_keep_masks x 32 (masks only, no gather)", False),
                                       ("perturb_text (1 launch)", text_hip, text_torch, "text_keep_batch x 32", True)):
        m = interleaved({"new_a": new, "torch": old, "new_b": new}, event_timed)
        ratio = "   torch / HIP %.1fx" % (m["torch"] / (0.5 * (m["new_a"] + m["new_b"]))) if like else ""
        print("    %-28s HIP %8.4f ms (A/A %8.4f, spread %.1f %%)   %s %8.4f ms%s"
              % (name, m["new_a"], m["new_b"], spread(m["new_a"], m["new_b"]), what, m["torch"], ratio))


def part_oracle(items=(0, 1)):
    from oracle import visualbert_torch as oracle
    cfg, model, pert = model_and_pert()
    batch, cams, lens = batch_and_cams(cfg)
    sd = {k: v.detach().double().cpu() for k, v in model.state_dict().items() if v.is_floating_point()}
    host = {k: batch[k].cpu() for k in KEYS}
    cams_h = cams.cpu()
    print("== distance from a float64 run of oracle/visualbert_torch.forward on the same physically perturbed inputs, items %s of the batch"
          % (list(items),))
    for modality, steps in (("image", vp.IMAGE_STEPS), ("text", vp.TEXT_STEPS)):
        batched = (pert.perturbation_image_batch if modality == "image" else pert.perturbation_text_batch)(batch, cams).double().cpu()
        single = torch.stack(per_item_scores(pert, batch, cams, lens, modality, items=items)).double().cpu()
        worst = {"batched": 0.0, "per item": 0.0}
        scale = 0.0
        for at, b in enumerate(items):
            n = lens[b]
            ids, mask, feats = host["input_ids"][b:b + 1, :n], host["input_mask"][b:b + 1, :n], host["image_feature_0"][b:b + 1].double()
            for s, step in enumerate(steps):
                if modality == "image":                 # evaluation_loop.py:111-117
                    top = torch.sort(cams_h[b, T_PAD:], descending=True, stable=True).indices[:int((1 - step) * REGIONS)]
                    ref = oracle.forward(sd, cfg.num_attention_heads, ids, mask, feats[:, top])[0][0]
                else:                                   # evaluation_loop.py:135-156
                    scores = cams_h[b, 1:n - 2]
                    top = torch.sort(scores, descending=True, stable=True).indices[:int((1 - step) * scores.shape[0])].tolist()
                    kept = sorted([0, n - 2, n - 1] + [i + 1 for i in top])
                    ref = oracle.forward(sd, cfg.num_attention_heads, ids[:, kept], mask[:, :len(kept)], feats)[0][0]
                worst["batched"] = max(worst["batched"], float((batched[b, s] - ref).abs().max()))
                worst["per item"] = max(worst["per item"], float((single[at, s] - ref).abs().max()))
                scale = max(scale, float(ref.abs().max()))
        print("    %-5s test: max |batched - float64| = %.3e   max |per item - float64| = %.3e   (largest score %.3f)"
              % (modality, worst["batched"], worst["per item"], scale))


def part_evaluator(method, reps=3):
    script = os.path.join(ROOT, "examples", "visualbert_pert_eval.py")

    def run(perturb):
        res = subprocess.run([sys.executable, script, "--method", method, "--num-samples", "256", "--explain-batch", "32",
                              "--perturb-batch", str(perturb)], cwd=ROOT, capture_output=True, text=True, timeout=300, check=True)
        return json.loads(res.stdout.strip().splitlines()[-1])

    rows = {"item_a": [], "batch_a": [], "item_b": [], "batch_b": []}
    acc = {}
    for _ in range(reps):
        for key, perturb in (("item_a", 0), ("batch_a", 32), ("item_b", 0), ("batch_b", 32)):
            out = run(perturb)
            rows[key].append(out["samples_per_s"])
            acc[key] = out["step_accuracy_percent"]
            print("%s: %.1f samples/s" % (key, out["samples_per_s"]), file=sys.stderr, flush=True)
    m = {k: statistics.median(v) for k, v in rows.items()}
    item, batch = 0.5 * (m["item_a"] + m["item_b"]), 0.5 * (m["batch_a"] + m["batch_b"])
    print("== evaluator, --method %s --num-samples 256 --explain-batch 32, image perturbation, medians of %d alternated child processes" % (method, reps))
    print("    --perturb-batch 0   %8.1f samples/s   A/A %8.1f / %8.1f, spread %.1f %%" % (item, m["item_a"], m["item_b"], spread(m["item_a"], m["item_b"])))
    print("    --perturb-batch 32  %8.1f samples/s   A/A %8.1f / %8.1f, spread %.1f %%   batched / per-item %.2fx   same step accuracies: %s"
          % (batch, m["batch_a"], m["batch_b"], spread(m["batch_a"], m["batch_b"]), batch / item, acc["batch_a"] == acc["item_a"] == acc["item_b"]))


if __name__ == "__main__":
    a = sys.argv[1:]
    ok = (len(a) == 2 and a[0] == "perturb" and a[1] in ("image", "text")) or a in (["kernels"], ["oracle"]) or (len(a) == 2 and a[0] == "evaluator")
    if not ok:
        raise SystemExit("usage: python tools/probe_visualbert_perturbation.py perturb image|text  |  kernels  |  oracle  |  evaluator <method>")
    if a[0] == "evaluator":                             # (children only: this process never opens the GPU)
        part_evaluator(a[1])
    else:
        print("device: %s" % torch.cuda.get_device_name(0))
        {"perturb": lambda: part_perturb(a[1]), "kernels": part_kernels, "oracle": part_oracle}[a[0]]()
