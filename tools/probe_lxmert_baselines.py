"""Probe (GPU box): the explain pass of the three attention-only LXMERT baselines at the shape of BASELINE config 4 (LXMERT-base,
B = 32 questions of 6..20 tokens padded to 20, 36 regions).

    python tools/probe_lxmert_baselines.py explain rollout        # | raw_attn | attn_gradcam
    python tools/probe_lxmert_baselines.py kernels

``explain``: one method's explain pass three ways -- a loop of 32 per-item calls of the existing generator (one unpadded item per call:
the parent's route, the baseline), ``GeneratorBaselines.generate_*_batch`` eager, and ``GraphedBaselinesBatch`` replayed.
``kernels``: the new launches alone (``ops.head_mean_live`` / ``ops.attn_gradcam_live`` / ``ops.lxmert_rollout``) against a batched torch
composition of the same maths on the same random slabs.

Each invocation is its own process (run each under its own `timeout`).  A host clock around work that ends in a device synchronise
(the explain passes are bound by the host), device events for the kernels; every variant warmed, variants alternated sample by sample
inside the process, medians of REPS = 20.  The A/A lines time the SAME variant twice in that interleaving: a difference between two
variants means something only beyond that spread.
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from transformer_mm_explainability_amd import lxmert_explainability as le  # noqa: E402
from transformer_mm_explainability_amd import lxmert_model as lm  # noqa: E402
from transformer_mm_explainability_amd import ops  # noqa: E402

REPS = 20
DEV = "cuda"
B, T_PAD, REGIONS = 32, 20, 36
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


def batch_and_items(cfg):
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(6, T_PAD + 1, (B,), generator=g).tolist()
    ids, mask = torch.zeros(B, T_PAD, dtype=torch.long), torch.zeros(B, T_PAD)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, cfg.vocab_size, (n,), generator=g)
        mask[b, :n] = 1
    batch = dict(input_ids=ids.to(DEV), attention_mask=mask.to(DEV), token_type_ids=torch.zeros(B, T_PAD, dtype=torch.long, device=DEV),
                 visual_feats=torch.randn(B, REGIONS, cfg.visual_feat_dim, generator=g).to(DEV),
                 visual_pos=torch.rand(B, REGIONS, 4, generator=g).to(DEV))
    items = [{k: (v[b:b + 1, :n] if k in ("input_ids", "attention_mask", "token_type_ids") else v[b:b + 1]).contiguous()
              for k, v in batch.items()} for b, n in enumerate(lens)]
    return batch, items, lens


class ItemUsage:
    def __init__(self, model):
        self.model = model

    def forward(self, inputs):
        self.text_len, self.image_boxes_len = inputs["input_ids"].shape[1], inputs["visual_feats"].shape[1]
        return self.model(**inputs)


def part_explain(method):
    cfg = lm.LxmertConfig()
    torch.manual_seed(0)
    model = lm.LxmertForQuestionAnswering(cfg).to(DEV).eval()
    batch, items, lens = batch_and_items(cfg)
    base_item = le.GeneratorBaselines(ItemUsage(model))
    item_fn = {"rollout": base_item.generate_rollout, "raw_attn": base_item.generate_raw_attn,
               "attn_gradcam": base_item.generate_attn_gradcam}[method]
    gen = le.GeneratorBaselines(type("Usage", (), {"model": model})())
    batch_fn = {"rollout": gen.generate_rollout_batch, "raw_attn": gen.generate_raw_attn_batch,
                "attn_gradcam": gen.generate_attn_gradcam_batch}[method]

    def per_item():
        return [tuple(r.clone() for r in item_fn(it)) for it in items]

    def eager():
        return batch_fn(batch)

    graphed = le.GraphedBaselinesBatch(model, batch, method)

    def replay():
        return graphed(batch)

    # results first: the batched routes against the per-item loop on the same items
    want, got_e, got_g = per_item(), tuple(t.clone() for t in eager()), tuple(t.clone() for t in replay())
    err = 0.0
    for b, n in enumerate(lens):
        err = max(err, float((got_e[0][b, :n, :n] - want[b][0]).abs().max()), float((got_e[1][b, :n] - want[b][1]).abs().max()))
    print("== %s, LXMERT-base, B = %d questions of %d..%d tokens padded to %d, %d regions" % (method, B, min(lens), max(lens), T_PAD, REGIONS))
    print("    max |batched - per item| over the live blocks = %.3g; graphed == eager bit for bit: %s"
          % (err, all(torch.equal(a, b) for a, b in zip(got_e, got_g))))
    m = interleaved({"item_a": per_item, "eager": eager, "graph_a": replay, "item_b": per_item, "graph_b": replay}, host_timed, warm=2)
    item = 0.5 * (m["item_a"] + m["item_b"])
    graph = 0.5 * (m["graph_a"] + m["graph_b"])
    print("    per-item loop (%d calls)   %9.2f ms per batch  %8.1f samples/s   A/A %9.2f / %9.2f ms, spread %.1f %%"
          % (B, item, B / item * 1e3, m["item_a"], m["item_b"], spread(m["item_a"], m["item_b"])))
    print("    batched, eager             %9.2f ms per batch  %8.1f samples/s   per-item / batched %.1fx" % (m["eager"], B / m["eager"] * 1e3, item / m["eager"]))
    print("    batched, graph replay      %9.2f ms per batch  %8.1f samples/s   per-item / graphed %.1fx   A/A %9.2f / %9.2f ms, spread %.1f %%"
          % (graph, B / graph * 1e3, item / graph, m["graph_a"], m["graph_b"], spread(m["graph_a"], m["graph_b"])))


def _live_mask(lens, N):
    return (torch.arange(N, device=DEV)[None, :] < lens[:, None]).float()


def torch_head_mean(P, G, q_len, k_len, zero_cls):
    """The same maths as a batched torch composition (masks instead of per-sample loops)."""
    mq, mk = _live_mask(q_len, P.shape[2]), _live_mask(k_len, P.shape[3])
    m = mq[:, :, None] * mk[:, None, :]
    if G is None:
        out = P.mean(dim=1) * m
    else:
        w = (G * m[:, None]).sum(dim=(2, 3), keepdim=True) / (q_len * k_len).float()[:, None, None, None]
        out = (P * w).mean(dim=1).clamp(min=0) * m
    if zero_cls:
        out[:, 0, 0] = 0
    return out


def torch_rollout(text, img, cross, t_len):
    B_, H, T, I = cross.shape
    mt = _live_mask(t_len, T)
    m_tt = mt[:, :, None] * mt[:, None, :]
    eye_t, eye_i = torch.eye(T, device=DEV), torch.eye(I, device=DEV)

    def aug_text(A):
        a = A.mean(dim=1) * m_tt + eye_t            # padded rows keep the identity: no 0 / 0, and they never reach a live entry
        return a / a.sum(dim=-1, keepdim=True)

    def aug_img(A):
        a = A.mean(dim=1) + eye_i
        return a / a.sum(dim=-1, keepdim=True)

    mats = [aug_text(A) for A in text]
    r = mats[0]
    for a in mats[1:-1]:
        r = torch.bmm(a, r)
    r_ii = aug_img(img[0])
    for A in img[1:]:
        r_ii = torch.bmm(aug_img(A), r_ii)
    r_live = r * m_tt
    R_ti = torch.bmm(r_live.transpose(1, 2), torch.bmm(cross.mean(dim=1) * mt[:, :, None], r_ii))
    R_tt = torch.bmm(mats[-1], r) * m_tt
    R_tt[:, 0, 0] = 0
    return R_tt, R_ti, r_ii


def part_kernels():
    H, n_text, n_img = 12, 14, 9                    # LXMERT-base: 9 language + 5 x-layers | 5 vision + 4 x-layers
    g = torch.Generator().manual_seed(1)
    t_len = torch.randint(6, T_PAD + 1, (B,), generator=g).to(DEV)
    i_len = torch.full((B,), REGIONS, device=DEV)

    def slab(nq, nk, live_k):
        x = torch.randn(B, H, nq, nk, generator=g).to(DEV)
        x = x.masked_fill(_live_mask(live_k, nk)[:, None, None, :] == 0, float("-inf"))
        return torch.softmax(x, dim=-1).contiguous()

    text = [slab(T_PAD, T_PAD, t_len) for _ in range(n_text)]
    img = [slab(REGIONS, REGIONS, i_len) for _ in range(n_img)]
    cross = slab(T_PAD, REGIONS, i_len)
    g_tt, g_ti = torch.randn(B, H, T_PAD, T_PAD, generator=g).to(DEV), torch.randn(B, H, T_PAD, REGIONS, generator=g).to(DEV)
    slab_mb = sum(x.numel() for x in text + img + [cross]) * 4 / 2 ** 20
    print("== the new launches alone against a batched torch composition of the same maths: B = %d, H = %d, T = %d, I = %d, %d + %d + 1 "
          "slabs (%.1f MiB); samples of 10 calls between two events" % (B, H, T_PAD, REGIONS, n_text, n_img, slab_mb))
    rows = [
        ("raw_attn (two head means)", lambda: (ops.head_mean_live(text[-1], t_len, t_len, True), ops.head_mean_live(cross, t_len)),
         lambda: (torch_head_mean(text[-1], None, t_len, t_len, True), torch_head_mean(cross, None, t_len, i_len, False))),
        ("attn_gradcam (two GradCAMs)", lambda: (ops.attn_gradcam_live(text[-1], g_tt, t_len, t_len, True), ops.attn_gradcam_live(cross, g_ti, t_len)),
         lambda: (torch_head_mean(text[-1], g_tt, t_len, t_len, True), torch_head_mean(cross, g_ti, t_len, i_len, False))),
        ("rollout (mmx_lxmert_rollout)", lambda: ops.lxmert_rollout(text, img, cross, text_len=t_len),
         lambda: torch_rollout(text, img, cross, t_len)),
    ]
    for name, new, old in rows:
        err = max(float((a - b).abs().max()) for a, b in zip(new(), old()))
        m = interleaved({"new_a": new, "torch": old, "new_b": new}, event_timed)
        print("    %-30s HIP %8.4f ms (A/A %8.4f, spread %.1f %%)   torch composition %8.4f ms   torch / HIP %.1fx   max |difference| %.2g"
              % (name, m["new_a"], m["new_b"], spread(m["new_a"], m["new_b"]), m["torch"], m["torch"] / (0.5 * (m["new_a"] + m["new_b"])), err))
    need = ops.lib().mmx_lxmert_rollout_workspace_bytes(n_text, n_img, B, T_PAD, REGIONS)
    print("    rollout reads %.1f MiB of slabs once and writes + reads %.2f MiB of workspace" % (slab_mb, need / 2 ** 20))


if __name__ == "__main__":
    ok = (len(sys.argv) == 3 and sys.argv[1] == "explain" and sys.argv[2] in METHODS) or sys.argv[1:] == ["kernels"]
    if not ok:
        raise SystemExit("usage: python tools/probe_lxmert_baselines.py explain rollout|raw_attn|attn_gradcam  |  kernels")
    print("device: %s" % torch.cuda.get_device_name(0))
    if sys.argv[1] == "kernels":
        part_kernels()
    else:
        part_explain(sys.argv[2])
