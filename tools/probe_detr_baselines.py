"""Probe (GPU box): the explain pass of the three attention-only DETR baselines at the shape of bench leg cfg 3 (``detr_resnet50_head``,
25 x 38 = 950 image tokens, 100 queries, 8 heads, 6 + 6 layers) for K = 8 and K = 16 kept queries.

    python tools/probe_detr_baselines.py explain rollout 16        # | raw_attn | attn_gradcam, K
    python tools/probe_detr_baselines.py kernels 16

``explain``: one method's explain pass three ways -- the loop of K per-query calls of the existing generator (the parent's route),
``Generator.generate_*_multi`` eager, and ``GraphedBaselinesMulti`` replayed.
``kernels``: the new launches alone (``ops.detr_raw_rows`` / ``ops.detr_gradcam_rows`` / ``ops.detr_rollout_rows``) on the slabs of one
forward against a batched torch composition of the same maths on the same slabs (``mean(0)``, ``+ I``, normalise, K-row ``matmul``s);
for the rollout also ``Le H Ni^2 4`` bytes over its time as TB/s.

Each invocation is its own process (run each under its own `timeout`).  A host clock around work that ends in a device synchronise for
the explain passes, device events for the kernels; every variant warmed, variants alternated sample by sample inside the process,
medians of REPS = 20.  The A/A lines time the SAME variant twice in that interleaving: a difference between two variants means
something only beyond that spread.
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from transformer_mm_explainability_amd import detr_model, ops  # noqa: E402
from transformer_mm_explainability_amd import detr_explainability as de  # noqa: E402

REPS = 20
DEV = "cuda"
METHODS = ("rollout", "raw_attn", "attn_gradcam")


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


def body_and_targets(K):
    torch.manual_seed(0)
    model = detr_model.detr_resnet50_head().to(DEV).eval()
    g = torch.Generator(device=DEV).manual_seed(5000)
    feats = torch.randn(1, 2048, 25, 38, generator=g, device=DEV) * 0.5
    targets = (torch.arange(K, device=DEV) * 6 + 1) % 100
    return model, feats, targets


def part_explain(method, K):
    model, feats, targets = body_and_targets(K)
    gen = de.Generator(model)
    one = getattr(gen, "generate_" + method)
    multi = getattr(gen, "generate_%s_multi" % method)

    def per_query():                                    # DETR/mask_generator.py:90-110: one call per kept query
        return torch.cat([one(feats, targets[k:k + 1]).reshape(1, -1) for k in range(K)])

    def eager():
        return multi(feats, targets)

    graphed = de.GraphedBaselinesMulti(model, feats, method, K=K)

    def replay():
        return graphed(feats, targets)

    a, b = per_query(), eager()[0, 0]
    print("%s K=%d: max |multi - per query| = %.3e (max |map| %.3e), |replay - multi| = %.3e"
          % (method, K, float((a - b).abs().max()), float(a.abs().max()), float((replay()[0, 0] - b).abs().max())))
    fns = {"per-query loop": per_query, "per-query loop (A/A)": per_query, "multi eager": eager, "multi eager (A/A)": eager,
           "graph replay": replay, "graph replay (A/A)": replay}
    t = interleaved(fns, host_timed)
    for k in ("per-query loop", "multi eager", "graph replay"):
        print("%-14s %-16s K=%-3d %9.3f ms   A/A %9.3f ms (spread %.1f %%)" % (method, k, K, t[k], t[k + " (A/A)"], spread(t[k], t[k + " (A/A)"])))
    aa = max(spread(t[k], t[k + " (A/A)"]) for k in ("per-query loop", "multi eager", "graph replay"))
    print("%-14s K=%-3d per-query / multi eager = %.2fx, per-query / graph replay = %.2fx (largest A/A spread %.1f %%)"
          % (method, K, t["per-query loop"] / t["multi eager"], t["per-query loop"] / t["graph replay"], aa))


def part_kernels(K):
    model, feats, targets = body_and_targets(K)
    with torch.no_grad():
        logits, state = model.forward_shared(feats, K)
        one_hot = torch.zeros(K, logits.shape[1] * logits.shape[2], device=DEV)
        one_hot.scatter_(1, (targets * logits.shape[2]).reshape(K, 1), 1.0)
        model.backward_shared(state, one_hot.view(K, logits.shape[1], logits.shape[2]), stop_after_top_cross=True)
    tr = model.transformer
    enc = [b.self_attn.get_attn().detach().clone() for b in tr.encoder.layers]
    dec = [b.self_attn.get_attn().detach().clone() for b in tr.decoder.layers]
    last = tr.decoder.layers[-1].multihead_attn
    P, G = last.get_attn().detach().clone(), last.get_attn_gradients().detach().clone()
    H, Q, Ni = P.shape
    eye_i, eye_q = torch.eye(Ni, device=DEV), torch.eye(Q, device=DEV)
    onehot_q = torch.zeros(K, Q, device=DEV)
    onehot_q[torch.arange(K, device=DEV), targets] = 1.0

    def norm(m, eye):
        m = m.mean(0) + eye
        return m / m.sum(-1, keepdim=True)

    def torch_rollout():                                 # the same row maths on stock ops: one mean / + I / normalise per slab, K-row matmuls
        u = onehot_q
        for b in dec:
            u = u @ norm(b, eye_q).t()
        x = u @ P.mean(0)
        for a in reversed(enc):
            x = x @ norm(a, eye_i)
        return x

    def torch_raw():
        return P.mean(0).index_select(0, targets)

    def torch_gradcam():
        w = G.reshape(K, H, Q, Ni).mean(dim=[2, 3])                                     # [K, H]
        return (P.index_select(1, targets).permute(1, 0, 2) * w.unsqueeze(-1)).mean(1).clamp(min=0)

    pairs = {"rollout": (lambda: ops.detr_rollout_rows(enc, dec, P, targets), torch_rollout),
             "raw_attn": (lambda: ops.detr_raw_rows(P, targets), torch_raw),
             "attn_gradcam": (lambda: ops.detr_gradcam_rows(P, G, targets), torch_gradcam)}
    for method, (hip, ref) in pairs.items():
        a, b = hip(), ref()
        print("%s K=%d: max |kernels - torch composition| = %.3e (max |map| %.3e)" % (method, K, float((a - b).abs().max()), float(b.abs().max())))
        t = interleaved({"hip": hip, "hip (A/A)": hip, "torch": ref, "torch (A/A)": ref}, event_timed)
        line = "%-14s K=%-3d launches %8.4f ms (A/A %8.4f, spread %.1f %%)   torch composition %8.4f ms (A/A %8.4f, spread %.1f %%)   %.2fx" % (
            method, K, t["hip"], t["hip (A/A)"], spread(t["hip"], t["hip (A/A)"]), t["torch"], t["torch (A/A)"],
            spread(t["torch"], t["torch (A/A)"]), t["torch"] / t["hip"])
        if method == "rollout":
            nbytes = len(enc) * H * Ni * Ni * 4
            line += "   encoder slabs %.1f MB / %.4f ms = %.2f TB/s" % (nbytes / 1e6, t["hip"], nbytes / (t["hip"] * 1e-3) / 1e12)
        print(line)


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "explain" and sys.argv[2] in METHODS:
        part_explain(sys.argv[2], int(sys.argv[3]))
    elif len(sys.argv) >= 3 and sys.argv[1] == "kernels":
        part_kernels(int(sys.argv[2]))
    else:
        sys.exit(__doc__)
