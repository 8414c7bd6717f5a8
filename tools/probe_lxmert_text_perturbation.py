"""Probe (GPU box): the text perturbation test of LXMERT at the cfg-4 shape (LXMERT-base, random weights, B = 32 questions of 8..20
tokens padded to 20, 36 regions) -- the record is ``profiles/lxmert_text_perturbation_probe.txt``.

    python tools/probe_lxmert_text_perturbation.py perturb            # the test per batch: current / grouped eager / graph replay
    python tools/probe_lxmert_text_perturbation.py kernels            # the builder launch alone against text_keep_batches
    python tools/probe_lxmert_text_perturbation.py evaluator          # examples/lxmert_perturbation_eval.py --text, child processes

``perturb``: ``perturbation_text`` (the current route: lengths read back, full padded width), ``perturbation_text_grouped`` eager with
2 and 3 groups, and ``GraphedTextPerturbation`` (2 groups; also 3) replayed, all fed the same cams; the text rows each route runs
through the body; the distance between the routes' scores.
``kernels``: ``ops.lxmert_perturb_text`` (one launch, device lengths) against ``text_keep_batches`` with host lengths (the torch
composition of the current route, without its ``tolist``), device events.
``evaluator``: ``examples/lxmert_perturbation_eval.py --num-samples 512 --text`` end to end as child processes, ``--text-groups 0``
and ``2`` alternated, three each, every child under its own ``timeout`` and nothing started after one that failed -> medians of
``samples_per_s_after_first_batch`` as the evaluator prints it (the first batch holds captures and library warm-up).

Each invocation is its own process (run each under its own ``timeout``).  A host clock around work that ends in a device synchronise
(host time is what the current route spends), device events for the builders; every variant warmed, variants alternated sample by
sample inside the process, medians of REPS = 20.  The A/A lines time the SAME variant twice in that interleaving: a difference between
two variants means something only beyond that spread.
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

from transformer_mm_explainability_amd import lxmert_model as lm  # noqa: E402
from transformer_mm_explainability_amd import lxmert_perturbation as lp  # noqa: E402
from transformer_mm_explainability_amd import ops  # noqa: E402

REPS = 20
B, T_PAD, REGIONS = 32, 20, 36


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
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def batch_of(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(8, 21, (B,), generator=g).tolist()
    ids, mask = torch.zeros(B, T_PAD, dtype=torch.long), torch.zeros(B, T_PAD)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, cfg.vocab_size, (n,), generator=g)
        mask[b, :n] = 1
    batch = dict(input_ids=ids.cuda(), attention_mask=mask.cuda(), token_type_ids=torch.zeros(B, T_PAD, dtype=torch.long).cuda(),
                 visual_feats=torch.randn(B, REGIONS, cfg.visual_feat_dim, generator=g).cuda(),
                 visual_pos=torch.rand(B, REGIONS, 4, generator=g).cuda())
    R_t_t = (torch.rand(B, T_PAD, T_PAD, generator=g) * mask[:, None, :]).cuda()
    R_t_i = torch.rand(B, T_PAD, REGIONS, generator=g).cuda()
    labels = torch.rand(B, cfg.num_qa_labels, generator=g).cuda()
    return batch, R_t_t, R_t_i, labels, lens


def report(name, stats, unit="ms"):
    for k, (med, lo, hi) in stats.items():
        print("%-10s %-44s median %8.3f %s (min %.3f max %.3f)" % (name, k, med, unit, lo, hi))


def part_perturb():
    cfg = lm.LxmertConfig()
    torch.manual_seed(0)
    model = lm.LxmertForQuestionAnswering(cfg).cuda().eval()
    pert = lp.LxmertPerturbation(model)
    batch, R_t_t, R_t_i, labels, lens = batch_of(cfg)
    _, cam_text = lp.normalize_cams_batch(R_t_t, R_t_i, batch["attention_mask"])
    S = len(pert.steps)
    print("shape: LXMERT-base, B=%d, T=%d (questions of %d..%d tokens, mean %.1f), %d regions, %d steps" %
          (B, T_PAD, min(lens), max(lens), sum(lens) / B, REGIONS, S))
    live = sum(2 + int((1 - step) * (n - 2)) for n in lens for step in pert.steps)
    print("text rows per batch: current route %d; two groups %d; three groups %d; live (kept tokens) %d" %
          (B * S * T_PAD, B * pert.text_step_groups(T_PAD, 2, "cuda").rows, B * pert.text_step_groups(T_PAD, 3, "cuda").rows, live))
    current = pert.perturbation_text(batch, cam_text)
    for groups in (1, 2, 3):
        got = pert.perturbation_text_grouped(batch, cam_text, max_groups=groups)
        print("max |scores(grouped, %d) - scores(current)| = %.3e (max |score| %.3f); arg-max equal: %s" %
              (groups, float((got - current).abs().max()), float(current.abs().max()), bool((got.argmax(-1) == current.argmax(-1)).all())))
    graphs = {g: lp.GraphedTextPerturbation(pert, batch, R_t_t, R_t_i, labels, max_groups=g) for g in (2, 3)}
    eager_acc = lp.LxmertPerturbation.accuracy(pert.perturbation_text_grouped(batch, cam_text), labels)
    print("graph replay (2 groups) accuracies bit-equal to the eager grouped route: %s" %
          torch.equal(graphs[2](batch, R_t_t, R_t_i, labels), eager_acc))

    def whole(run):           # the evaluator's step: cams from the relevancies, the test, the accuracies
        def f():
            _, cam = lp.normalize_cams_batch(R_t_t, R_t_i, batch["attention_mask"])
            return lp.LxmertPerturbation.accuracy(run(cam), labels)
        return f

    fns = {"current route (perturbation_text)": whole(lambda cam: pert.perturbation_text(batch, cam)),
           "current route, again (A/A)": whole(lambda cam: pert.perturbation_text(batch, cam)),
           "grouped eager, 2 groups": whole(lambda cam: pert.perturbation_text_grouped(batch, cam, max_groups=2)),
           "grouped eager, 3 groups": whole(lambda cam: pert.perturbation_text_grouped(batch, cam, max_groups=3)),
           "graph replay, 2 groups": lambda: graphs[2](batch, R_t_t, R_t_i, labels),
           "graph replay, 2 groups, again (A/A)": lambda: graphs[2](batch, R_t_t, R_t_i, labels),
           "graph replay, 3 groups": lambda: graphs[3](batch, R_t_t, R_t_i, labels)}
    stats = interleaved(fns, host_timed)
    report("perturb", stats)
    print("A/A spread: current %.2f %%, graph replay %.2f %%" %
          (spread(stats["current route (perturbation_text)"][0], stats["current route, again (A/A)"][0]),
           spread(stats["graph replay, 2 groups"][0], stats["graph replay, 2 groups, again (A/A)"][0])))


def part_kernels():
    cfg = lm.LxmertConfig()
    pert = lp.LxmertPerturbation(None)
    batch, R_t_t, R_t_i, _, lens = batch_of(cfg)
    _, cam = lp.normalize_cams_batch(R_t_t, R_t_i, batch["attention_mask"])
    cam = cam.contiguous()
    plan = pert.text_step_groups(T_PAD, 2, "cuda")
    place, elems = plan.layout(B).table, plan.layout(B).elems
    text_len = batch["attention_mask"].sum(dim=1).to(torch.int32)
    out = ops.lxmert_perturb_text(batch["input_ids"], batch["token_type_ids"], cam, text_len, plan.counts, place, elems)
    fns = {"ops.lxmert_perturb_text (2 groups, into out=)":
           lambda: ops.lxmert_perturb_text(batch["input_ids"], batch["token_type_ids"], cam, text_len, plan.counts, place, elems, out=out),
           "ops.lxmert_perturb_text, again (A/A)":
           lambda: ops.lxmert_perturb_text(batch["input_ids"], batch["token_type_ids"], cam, text_len, plan.counts, place, elems, out=out),
           "text_keep_batches (host lengths given)":
           lambda: lp.text_keep_batches(batch["input_ids"], batch["token_type_ids"], cam, pert.steps, False, n_tokens=lens),
           "text_keep_batches, again (A/A)":
           lambda: lp.text_keep_batches(batch["input_ids"], batch["token_type_ids"], cam, pert.steps, False, n_tokens=lens)}
    stats = interleaved(fns, event_timed)
    report("kernels", stats, "ms (device events, 10 calls each)")
    names = list(fns)
    print("A/A spread: builder %.2f %%, text_keep_batches %.2f %%" % (spread(stats[names[0]][0], stats[names[1]][0]),
                                                                      spread(stats[names[2]][0], stats[names[3]][0])))


def part_evaluator():
    results = {0: [], 2: []}
    for rnd in range(3):
        for groups in (0, 2):
            cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "examples", "lxmert_perturbation_eval.py"),
                   "--num-samples", "512", "--text", "--text-groups", str(groups)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:                   # a fault, an abort or a time limit: nothing more is started on the GPU
                print(r.stdout[-2000:], r.stderr[-2000:])
                sys.exit("evaluator --text-groups %d ended with status %d: stopping here" % (groups, r.returncode))
            line = json.loads(r.stdout.strip().splitlines()[-1])
            results[groups].append(line)
            print("evaluator --text --text-groups %d: %7.1f samples/s after the first batch, %7.1f overall, first batch %.2f s"
                  % (groups, line["samples_per_s_after_first_batch"], line["samples_per_s"], line["first_batch_s"]), flush=True)
    for groups, lines in sorted(results.items()):
        rates = [l["samples_per_s_after_first_batch"] for l in lines]
        print("evaluator --text-groups %d: median %.1f samples/s after the first batch (min %.1f max %.1f, spread %.2f %%), %d runs"
              % (groups, statistics.median(rates), min(rates), max(rates), spread(min(rates), max(rates)), len(rates)))
    accs = {groups: lines[0]["step_accuracy_percent"] for groups, lines in results.items()}
    print("step accuracies per route: %s" % json.dumps(accs, sort_keys=True))


if __name__ == "__main__":
    {"perturb": part_perturb, "kernels": part_kernels, "evaluator": part_evaluator}[sys.argv[1]]()
