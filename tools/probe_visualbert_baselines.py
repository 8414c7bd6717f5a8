"""Probe (GPU box): the explain pass of the three attention-only VisualBERT baselines at the shape of the evaluator
(``examples/visualbert_pert_eval.py``: BERT-base VisualBERT, B = 32 questions of 8..20 tokens padded to 24, 100 regions, N = 124).

    python tools/probe_visualbert_baselines.py explain rollout        # | raw_attn | attn_gradcam
    python tools/probe_visualbert_baselines.py kernels
    python tools/probe_visualbert_baselines.py evaluator rollout      # | raw_attn | attn_gradcam

``explain``: one method's explain pass three ways -- a loop of 32 per-item calls of the existing generator (the parent's route, the
baseline), ``SelfAttentionGenerator.generate_*_batch`` eager, and ``GraphedBaselinesBatch`` replayed.
``kernels``: the new launches alone (``ops.selfattn_raw_row`` / ``ops.selfattn_gradcam_row`` / ``ops.selfattn_rollout_row``) against a
batched torch composition of the same maths on the same random slabs.
``evaluator``: ``examples/visualbert_pert_eval.py --num-samples 256`` end to end, as child processes, with ``--explain-batch 32`` and
without, alternated, ``samples_per_s`` as the evaluator prints it (model construction is outside its clock).

Each invocation is its own process (run each under its own `timeout`).  A host clock around work that ends in a device synchronise
(the explain passes are bound by the host), device events for the kernels; every variant warmed, variants alternated sample by sample
inside the process, medians of REPS = 20.  The A/A lines time the SAME variant twice in that interleaving: a difference between two
variants means something only beyond that spread.
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
METHODS = ("rollout", "raw_attn", "attn_gradcam")
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


def ragged_lengths(g):
    return torch.randint(8, 21, (B,), generator=g).tolist()          # the evaluator's synthetic questions: 8..20 tokens


def batch_and_items(cfg):
    g = torch.Generator().manual_seed(0)
    lens = ragged_lengths(g)
    ids, mask = torch.zeros(B, T_PAD, dtype=torch.long), torch.zeros(B, T_PAD, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, cfg.vocab_size, (n,), generator=g)
        mask[b, :n] = 1
    batch = {"input_ids": ids.to(DEV), "input_mask": mask.to(DEV), "segment_ids": torch.zeros(B, T_PAD, dtype=torch.long, device=DEV),
             "image_feature_0": torch.randn(B, REGIONS, FEAT, generator=g).to(DEV)}
    return batch, lens


def part_explain(method):
    cfg = vm.VisualBertConfig()
    torch.manual_seed(0)
    model = vm.VisualBERT(cfg).to(DEV).eval()
    batch, lens = batch_and_items(cfg)
    gen = vb.SelfAttentionGenerator(model)
    item_fn = {"rollout": gen.generate_rollout, "raw_attn": gen.generate_raw_attn, "attn_gradcam": gen.generate_attn_gradcam}[method]
    batch_fn = {"rollout": gen.generate_rollout_batch, "raw_attn": gen.generate_raw_attn_batch,
                "attn_gradcam": gen.generate_attn_gradcam_batch}[method]

    def per_item():                                     # (the wrapper trims its sample_list in place: a fresh dict per call)
        return [item_fn({k: batch[k][b:b + 1] for k in KEYS}).clone() for b in range(B)]

    def eager():
        return batch_fn(batch)

    graphed = vb.GraphedBaselinesBatch(model, batch, method)

    def replay():
        return graphed(batch)

    # results first: the batched routes against the per-item loop on the same items
    want, got_e, got_g = per_item(), eager().clone(), replay().clone()
    err = scale = 0.0
    for b, n in enumerate(lens):
        d = (vb.unpad_row(got_e, b, n, padded_text=T_PAD) - want[b]).abs()
        err, scale = max(err, float(torch.nan_to_num(d).max())), max(scale, float(torch.nan_to_num(want[b]).abs().max()))
    same = torch.equal(torch.nan_to_num(got_e, nan=-7.0), torch.nan_to_num(got_g, nan=-7.0))
    print("== %s, BERT-base VisualBERT, B = %d questions of %d..%d tokens padded to %d, %d regions"
          % (method, B, min(lens), max(lens), T_PAD, REGIONS))
    print("    max |batched - per item| over the rows = %.3g (largest entry %.3g); graphed == eager bit for bit: %s" % (err, scale, same))
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


def _row(maps, t_len, live):
    """Row c_b = t_b - 2 of ``[B, N, N]`` maps, zero at c_b and outside the live set."""
    c = (t_len - 2).long()
    rows = maps[torch.arange(B, device=DEV), c] * live
    rows[torch.arange(B, device=DEV), c] = 0
    return rows


def torch_raw(P, t_len, v_len):
    return _row(P.mean(dim=1), t_len, _live(t_len, v_len))


def torch_gradcam(P, G, t_len, v_len):
    live = _live(t_len, v_len)
    m = live[:, :, None] * live[:, None, :]
    n = (t_len + v_len).float()
    w = (G * m[:, None]).sum(dim=(2, 3), keepdim=True) / (n * n)[:, None, None, None]
    cam = (P * w).mean(dim=1).clamp(min=0)
    mn = cam.masked_fill(m == 0, float("inf")).amin(dim=(1, 2), keepdim=True)
    mx = cam.masked_fill(m == 0, float("-inf")).amax(dim=(1, 2), keepdim=True)
    return _row((cam - mn) / (mx - mn), t_len, live)


def torch_rollout(layers, t_len, v_len):
    """The full N x N product, as the per-item route forms it (batched, padded rows and columns masked away)."""
    live = _live(t_len, v_len)
    m = live[:, :, None] * live[:, None, :]
    eye = torch.eye(T_PAD + REGIONS, device=DEV)
    mats = [A.sum(dim=1) / A.shape[1] * m + eye for A in layers]
    joint = mats[0]
    for a in mats[1:]:
        joint = torch.bmm(a, joint)
    return _row(joint, t_len, live)


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
    G = (torch.randn(B, H, N, N, generator=g) + 0.5).to(DEV)
    slab_mb = layers[0].numel() * 4 / 2 ** 20
    print("== the new launches alone against a batched torch composition of the same maths: B = %d, H = %d, T = %d, V = %d, %d slabs of "
          "%.1f MiB; samples of 10 calls between two events" % (B, H, T_PAD, REGIONS, L, slab_mb))
    rows = [
        ("raw_attn (1 launch)", lambda: ops.selfattn_raw_row(layers[-1], t_len, v_len, n_text=T_PAD), lambda: torch_raw(layers[-1], t_len, v_len)),
        ("attn_gradcam (3 launches)", lambda: ops.selfattn_gradcam_row(layers[-1], G, t_len, v_len, n_text=T_PAD),
         lambda: torch_gradcam(layers[-1], G, t_len, v_len)),
        ("rollout (2 launches)", lambda: ops.selfattn_rollout_row(layers, t_len, v_len, n_text=T_PAD), lambda: torch_rollout(layers, t_len, v_len)),
    ]
    for name, new, old in rows:
        err = float((new() - old()).abs().max())
        m = interleaved({"new_a": new, "torch": old, "new_b": new}, event_timed)
        print("    %-28s HIP %8.4f ms (A/A %8.4f, spread %.1f %%)   torch composition %8.4f ms   torch / HIP %.1fx   max |difference| %.2g"
              % (name, m["new_a"], m["new_b"], spread(m["new_a"], m["new_b"]), m["torch"], m["torch"] / (0.5 * (m["new_a"] + m["new_b"])), err))
    need = ops.lib().mmx_selfattn_rollout_row_workspace_bytes(L, B, T_PAD, REGIONS)
    print("    rollout reads %.1f MiB of slabs once and writes + reads %.2f MiB of workspace; GradCAM reads 2 x %.1f MiB"
          % (L * slab_mb, need / 2 ** 20, slab_mb))


def part_evaluator(method, reps=3):
    script = os.path.join(ROOT, "examples", "visualbert_pert_eval.py")

    def run(explain):
        res = subprocess.run([sys.executable, script, "--method", method, "--num-samples", "256", "--explain-batch", str(explain)],
                             cwd=ROOT, capture_output=True, text=True, timeout=300, check=True)
        return json.loads(res.stdout.strip().splitlines()[-1])

    rows = {"item_a": [], "batch": [], "item_b": []}
    acc = {}
    for _ in range(reps):
        for key, explain in (("item_a", 1), ("batch", 32), ("item_b", 1)):
            out = run(explain)
            rows[key].append(out["samples_per_s"])
            acc[key] = out["step_accuracy_percent"]
    m = {k: statistics.median(v) for k, v in rows.items()}
    print("== evaluator, --method %s --num-samples 256, image perturbation, medians of %d alternated child processes" % (method, reps))
    print("    --explain-batch 1   %8.1f samples/s   A/A %8.1f / %8.1f, spread %.1f %%" % (0.5 * (m["item_a"] + m["item_b"]), m["item_a"], m["item_b"],
                                                                                         spread(m["item_a"], m["item_b"])))
    print("    --explain-batch 32  %8.1f samples/s   batched / per-item %.2fx   same step accuracies: %s"
          % (m["batch"], m["batch"] / (0.5 * (m["item_a"] + m["item_b"])), acc["batch"] == acc["item_a"] == acc["item_b"]))


if __name__ == "__main__":
    ok = (len(sys.argv) == 3 and sys.argv[1] in ("explain", "evaluator") and sys.argv[2] in METHODS) or sys.argv[1:] == ["kernels"]
    if not ok:
        raise SystemExit("usage: python tools/probe_visualbert_baselines.py explain|evaluator rollout|raw_attn|attn_gradcam  |  kernels")
    if sys.argv[1] == "evaluator":                      # (children only: this process never opens the GPU)
        part_evaluator(sys.argv[2])
    else:
        print("device: %s" % torch.cuda.get_device_name(0))
        if sys.argv[1] == "kernels":
            part_kernels()
        else:
            part_explain(sys.argv[2])
