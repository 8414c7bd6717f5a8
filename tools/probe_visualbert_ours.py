"""Probe (GPU box): the explain pass of ``generate_ours`` for a padded batch of ragged questions, at the shape of the evaluator
(``examples/visualbert_pert_eval.py``: BERT-base VisualBERT, B = 32 questions of 8..20 tokens padded to 24, 100 regions, N = 124).

    python tools/probe_visualbert_ours.py explain
    python tools/probe_visualbert_ours.py kernels
    python tools/probe_visualbert_ours.py evaluator

``explain``: the explain pass three ways -- a loop of 32 per-item ``generate_ours`` calls (the parent's route for ragged questions, the
baseline), ``SelfAttentionGenerator.generate_ours_padded_batch`` eager, and ``GraphedGenerateOursPadded`` replayed.
``kernels``: the two launches alone (``ops.selfattn_ours_row``) against a batched torch composition of the same row maths on the same
random slabs.
``evaluator``: ``examples/visualbert_pert_eval.py --method ours_no_lrp --perturb-batch 32 --num-samples 256`` end to end, as child
processes each under its own ``timeout``, with ``--explain-batch 32`` and ``--explain-batch 1``, alternated, ``samples_per_s`` as the
evaluator prints it (model construction is outside its clock).

Each invocation is its own process (run each under its own `timeout`).  A host clock around work that ends in a device synchronise
(the explain passes are bound by the host), device events for the kernels; every variant warmed, variants alternated sample by sample
inside the process, medians of REPS = 20.  The A/A lines time the SAME variant twice in that interleaving: a difference between two
variants means something only beyond that spread.

Not predicted here: the slabs of this shape are about 0.57 GB, a fraction of a millisecond of traffic next to a forward and a backward
of several milliseconds, so whatever the batched route gains should come from batching the body's passes, not from the kernel.  That is
an expectation, not a measurement, until ``explain`` and ``kernels`` have been run; read their figures, not this paragraph.
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

REPS = 20
DEV = "cuda"
B, T_PAD, REGIONS, FEAT = 32, 24, 100, 2048
KEYS = ("input_ids", "input_mask", "segment_ids", "image_feature_0")
CHILD_LIMIT = 240                   # seconds: the time limit of one evaluator child


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


def ragged_lengths(g):
    return torch.randint(8, 21, (B,), generator=g).tolist()          # the evaluator's synthetic questions: 8..20 tokens


def batch_and_lengths(cfg):
    g = torch.Generator().manual_seed(0)
    lens = ragged_lengths(g)
    ids, mask = torch.zeros(B, T_PAD, dtype=torch.long), torch.zeros(B, T_PAD, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, cfg.vocab_size, (n,), generator=g)
        mask[b, :n] = 1
    batch = {"input_ids": ids.to(DEV), "input_mask": mask.to(DEV), "segment_ids": torch.zeros(B, T_PAD, dtype=torch.long, device=DEV),
             "image_feature_0": torch.randn(B, REGIONS, FEAT, generator=g).to(DEV)}
    return batch, lens


def part_explain():
    cfg = vm.VisualBertConfig()
    torch.manual_seed(0)
    model = vm.VisualBERT(cfg).to(DEV).eval()
    batch, lens = batch_and_lengths(cfg)
    gen = vb.SelfAttentionGenerator(model)

    def per_item():                                     # (the wrapper trims its sample_list in place: a fresh dict per call)
        return [gen.generate_ours({k: batch[k][b:b + 1] for k in KEYS}).clone() for b in range(B)]

    def eager():
        return gen.generate_ours_padded_batch(batch)

    graphed = vb.GraphedGenerateOursPadded(model, batch)

    def replay():
        return graphed(batch)

    # results first: the batched routes against the per-item loop on the same items
    want, got_e, got_g = per_item(), eager().clone(), replay().clone()
    err = scale = 0.0
    for b, n in enumerate(lens):
        d = (vb.unpad_row(got_e, b, n, padded_text=T_PAD) - want[b]).abs()
        err, scale = max(err, float(d.max())), max(scale, float(want[b].abs().max()))
    print("== generate_ours, BERT-base VisualBERT, B = %d questions of %d..%d tokens padded to %d, %d regions"
          % (B, min(lens), max(lens), T_PAD, REGIONS))
    print("    max |batched - per item| over the rows = %.3g (largest entry %.3g); graphed == eager bit for bit: %s"
          % (err, scale, torch.equal(got_e, got_g)))
    m = interleaved({"item_a": per_item, "eager": eager, "graph_a": replay, "item_b": per_item, "graph_b": replay}, host_timed, warm=2)
    item = 0.5 * (m["item_a"] + m["item_b"])
    graph = 0.5 * (m["graph_a"] + m["graph_b"])
    print("    per-item loop (%d calls)   %9.2f ms per batch  %8.1f samples/s   A/A %9.2f / %9.2f ms, spread %.1f %%"
          % (B, item, B / item * 1e3, m["item_a"], m["item_b"], spread(m["item_a"], m["item_b"])))
    print("    batched, eager             %9.2f ms per batch  %8.1f samples/s   per-item / batched %.1fx" % (m["eager"], B / m["eager"] * 1e3, item / m["eager"]))
    print("    batched, graph replay      %9.2f ms per batch  %8.1f samples/s   per-item / graphed %.1fx   A/A %9.2f / %9.2f ms, spread %.1f %%"
          % (graph, B / graph * 1e3, item / graph, m["graph_a"], m["graph_b"], spread(m["graph_a"], m["graph_b"])))


def _live(t_len, v_len):
    j = torch.arange(T_PAD + REGIONS, device=DEV)[None, :]
    return ((j < t_len[:, None]) | ((j >= T_PAD) & (j < T_PAD + v_len[:, None]))).float()


def torch_ours_row(layers, grads, t_len, v_len):
    """The same ROW maths, batched: rule 5 per layer on the masked block, the row vector carried from the top layer down."""
    live = _live(t_len, v_len)
    m = live[:, :, None] * live[:, None, :]
    c = (t_len - 2).long()
    every = torch.arange(B, device=DEV)
    x = torch.zeros(B, T_PAD + REGIONS, device=DEV)
    x[every, c] = 1
    for P, G in zip(reversed(layers), reversed(grads)):
        A = (G * P).clamp(min=0).mean(dim=1) * m
        x = x + torch.bmm(x[:, None, :], A)[:, 0]
    x = x * live
    x[every, c] = 0
    return x


def part_kernels():
    H, L, N = 12, 12, T_PAD + REGIONS
    g = torch.Generator().manual_seed(1)
    t_len = torch.tensor(ragged_lengths(g), dtype=torch.int32).to(DEV)
    v_len = torch.full((B,), REGIONS, dtype=torch.int32, device=DEV)
    live = _live(t_len, v_len)

    def slab():
        x = torch.randn(B, H, N, N, generator=g).to(DEV)
        return torch.softmax(x.masked_fill(live[:, None, None, :] == 0, float("-inf")), dim=-1).contiguous()

    layers = [slab() for _ in range(L)]
    grads = [(torch.randn(B, H, N, N, generator=g) + 0.5).to(DEV) for _ in range(L)]
    slab_mb = layers[0].numel() * 4 / 2 ** 20
    print("== the two launches alone against a batched torch composition of the same row maths: B = %d, H = %d, T = %d, V = %d, 2 x %d "
          "slabs of %.1f MiB; samples of 10 calls between two events" % (B, H, T_PAD, REGIONS, L, slab_mb))
    new = lambda: ops.selfattn_ours_row(layers, grads, t_len, v_len, n_text=T_PAD)
    old = lambda: torch_ours_row(layers, grads, t_len, v_len)
    err, scale = float((new() - old()).abs().max()), float(old().abs().max())
    m = interleaved({"new_a": new, "torch": old, "new_b": new}, event_timed)
    hip = 0.5 * (m["new_a"] + m["new_b"])
    print("    ours (2 launches)            HIP %8.4f ms (A/A %8.4f / %8.4f, spread %.1f %%)   torch composition %8.4f ms   torch / HIP %.1fx   "
          "max |difference| %.2g (largest entry %.3g)" % (hip, m["new_a"], m["new_b"], spread(m["new_a"], m["new_b"]), m["torch"],
                                                          m["torch"] / hip, err, scale))
    need = ops.lib().mmx_selfattn_ours_row_workspace_bytes(L, B, T_PAD, REGIONS)
    read_mb = 2 * L * slab_mb
    print("    reads %.1f MiB of slabs once and writes + reads %.2f MiB of workspace: %.2f TB/s over the HIP time (part of a repeated "
          "call's slabs may still sit in the last-level cache; not separated here)"
          % (read_mb, need / 2 ** 20, (read_mb + 2 * need / 2 ** 20) * 2 ** 20 / (hip * 1e-3) / 1e12))


def part_evaluator(reps=3):
    script = os.path.join(ROOT, "examples", "visualbert_pert_eval.py")

    def run(explain):
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, script, "--method", "ours_no_lrp", "--num-samples", "256",
               "--perturb-batch", "32", "--explain-batch", str(explain)]
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_LIMIT + 30)
        if res.returncode != 0:                         # a child that failed or ran into its limit ends the probe: nothing after it
            raise SystemExit("evaluator child (--explain-batch %d) ended with %d:\n%s" % (explain, res.returncode, res.stderr[-2000:]))
        return json.loads(res.stdout.strip().splitlines()[-1])

    rows = {"item_a": [], "batch_a": [], "item_b": [], "batch_b": []}
    acc = {}
    for _ in range(reps):
        for key, explain in (("item_a", 1), ("batch_a", 32), ("item_b", 1), ("batch_b", 32)):
            out = run(explain)
            rows[key].append(out["samples_per_s"])
            acc[key] = out["step_accuracy_percent"]
    m = {k: statistics.median(v) for k, v in rows.items()}
    item, batch = 0.5 * (m["item_a"] + m["item_b"]), 0.5 * (m["batch_a"] + m["batch_b"])
    wider = max(spread(m["item_a"], m["item_b"]), spread(m["batch_a"], m["batch_b"]))
    print("== evaluator, --method ours_no_lrp --perturb-batch 32 --num-samples 256, image perturbation, medians of %d alternated child "
          "processes" % reps)
    print("    --explain-batch 1   %8.1f samples/s   A/A %8.1f / %8.1f, spread %.1f %%" % (item, m["item_a"], m["item_b"],
                                                                                         spread(m["item_a"], m["item_b"])))
    print("    --explain-batch 32  %8.1f samples/s   A/A %8.1f / %8.1f, spread %.1f %%" % (batch, m["batch_a"], m["batch_b"],
                                                                                         spread(m["batch_a"], m["batch_b"])))
    print("    batched / per-item %.2fx (%+.1f %%; the larger A/A spread is %.1f %%)   same step accuracies in every run: %s"
          % (batch / item, 100 * (batch / item - 1), wider, all(a == acc["item_a"] for a in acc.values())))


if __name__ == "__main__":
    if sys.argv[1:] not in (["explain"], ["kernels"], ["evaluator"]):
        raise SystemExit("usage: python tools/probe_visualbert_ours.py explain | kernels | evaluator")
    if sys.argv[1] == "evaluator":                      # (children only: this process never opens the GPU)
        part_evaluator()
    else:
        print("device: %s" % torch.cuda.get_device_name(0))
        part_kernels() if sys.argv[1] == "kernels" else part_explain()
