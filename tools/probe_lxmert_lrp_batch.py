"""Probe (GPU box): the four LRP methods of LXMERT on a padded batch (``ours_with_lrp``, ``ours_with_lrp_no_normalization``,
``transformer_att``, ``partial_lrp``) at the shape of BASELINE config 4 (LXMERT-base, B = 32 questions of 8..20 tokens padded to 20,
36 regions).  Output kept in ``profiles/lxmert_lrp_batch_probe.txt``.

    python tools/probe_lxmert_lrp_batch.py errors
    python tools/probe_lxmert_lrp_batch.py explain ours_with_lrp     # | ours_with_lrp_no_normalization | transformer_att | partial_lrp
    python tools/probe_lxmert_lrp_batch.py kernels
    python tools/probe_lxmert_lrp_batch.py evaluator transformer_att [num_samples]
    python tools/probe_lxmert_lrp_batch.py conditioning f32          # | f64; no GPU

``errors``: the worst error / bound per output of ``mmx_lxmert_attr`` and ``mmx_head_minmax_live`` over the case table of
``tests/lxmert_lrp_batch_cases.py`` (the checks of ``tests/test_gpu_lxmert_lrp_batch_ops.py``, which assert while they measure), and
the distances of ``tests/test_gpu_lxmert_lrp_batch.py`` on the golden LXMERT: item 0 of the padded batch against the reference's
float64 pass, items 1 and 2 against the per-item methods.
``explain``: one method's explain pass two ways -- a loop of 32 per-item calls of the existing generator (one unpadded item per call: the
parent's route, the baseline) and the batched eager pass.
``kernels``: the two new launches alone against a batched torch composition of the same maths on the same random slabs.
``evaluator``: ``examples/lxmert_perturbation_eval.py --method M --batch-lrp 1`` against ``0``, three alternated child processes each.

Each invocation is its own process (run each under its own ``timeout``).  A host clock around work that ends in a device synchronise,
device events for the kernels; every variant warmed, variants alternated sample by sample inside the process, medians of REPS = 20.
The A/A lines time the SAME variant twice in that interleaving: a difference between two variants means something only beyond that
spread."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from transformer_mm_explainability_amd import lxmert_explainability as le  # noqa: E402
from transformer_mm_explainability_amd import lxmert_model as lm  # noqa: E402
from transformer_mm_explainability_amd import ops  # noqa: E402

REPS = 20
DEV = "cuda"
B, T_PAD, REGIONS = 32, 20, 36
METHODS = ("ours_with_lrp", "ours_with_lrp_no_normalization", "transformer_att", "partial_lrp")


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


# ------------------------------------------------------------------------------------------------ errors
def part_errors():
    import lxmert_lrp_batch_cases as cases
    import test_gpu_lxmert_lrp_batch as model_suite
    import test_gpu_lxmert_lrp_batch_ops as op_suite
    import test_gpu_lrp
    worst, where = {}, {}
    for case in cases.CASES:
        for name, ratio in list(op_suite.check_attr(case).items()) + [("min-max " + k, v) for k, v in op_suite.check_minmax(case).items()]:
            if ratio >= worst.get(name, -1.0):
                worst[name], where[name] = ratio, cases.case_id(case)
    print("== op level: worst |kernel - float64| / bound per output over the %d cases (every element inside its bound: asserted)" % len(cases.CASES))
    for name in worst:
        print("    %-28s %.3f   at %s" % (name, worst[name], where[name]))

    conftest_golden = lambda name: dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))  # noqa: E731
    from test_gpu_generators import _lxmert_from_golden
    gm, g = conftest_golden("lxmert_model"), conftest_golden("lxmert_model_lrp")
    model, _ = _lxmert_from_golden(gm)
    inputs = {k[4:]: torch.from_numpy(np.asarray(v)) for k, v in gm.items() if k.startswith("in__")}
    batch, items, index = model_suite.ragged_batch(inputs, int(g["index"]))
    batch = {k: v.to(DEV) for k, v in batch.items()}
    items = [{k: v.to(DEV) for k, v in it.items()} for it in items]
    print("== golden LXMERT, items of %s tokens padded to %d; factor allowed on item 0: %.1f, between the routes: 3.0"
          % (model_suite.TRUNCATIONS, batch["input_ids"].shape[1], test_gpu_lrp.LRP_FACTOR))
    for mode in ("argmax", "given"):
        given = mode == "given"
        batched = model_suite.run_batched(model, batch, torch.tensor(index, device=DEV) if given else None)
        per_item = {b: model_suite.run_per_item(model, items[b], index[b] if given else None) for b in (1, 2)}
        print("  index: %s" % ("given ids %s" % index if given else "None (arg-max per sample)"))
        for method in sorted(model_suite.KEYS):
            for key, _w in model_suite.KEYS[method]:
                r32, r64 = np.asarray(g[key], np.float64), np.asarray(g["f64__" + key], np.float64)
                top, noise = float(np.abs(r64).max()), float(np.abs(r32 - r64).max())
                got0 = model_suite.live(key, batched[method][key], 0, model_suite.TRUNCATIONS[0]).double().cpu().numpy()
                err0 = float(np.abs(got0 - r64).max())
                line = "    %-24s item 0: |batched - ref64| %.3e = %.3f x the reference's fp32 noise %.3e" % (key, err0, err0 / noise if noise else 0.0, noise)
                for b in (1, 2):
                    a, want = model_suite.live(key, batched[method][key], b, model_suite.TRUNCATIONS[b]), per_item[b][method][key]
                    scale = float(want.abs().max())
                    err = float((a - want).abs().max())
                    line += "   item %d: |batched - per item| %.3e = %.4f x (noise / top) max|b|" % (b, err, err / (noise / top * scale) if noise else 0.0)
                print(line)


# ------------------------------------------------------------------------------------------------ explain
def batch_and_items(cfg):
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(8, T_PAD + 1, (B,), generator=g).tolist()
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
    ours_item, base_item = le.GeneratorOurs(ItemUsage(model)), le.GeneratorBaselines(ItemUsage(model))
    usage = type("Usage", (), {"model": model})()
    ours, base = le.GeneratorOurs(usage), le.GeneratorBaselines(usage)
    item_fn = {"ours_with_lrp": lambda it: ours_item.generate_ours(it, use_lrp=True),
               "ours_with_lrp_no_normalization": lambda it: ours_item.generate_ours(it, normalize_self_attention=False),
               "transformer_att": base_item.generate_transformer_attr, "partial_lrp": base_item.generate_partial_lrp}[method]
    batch_fn = {"ours_with_lrp": lambda b: ours.generate_ours_batch(b, use_lrp=True),
                "ours_with_lrp_no_normalization": lambda b: ours.generate_ours_batch(b, use_lrp=True, normalize_self_attention=False),
                "transformer_att": base.generate_transformer_attr_batch, "partial_lrp": base.generate_partial_lrp_batch}[method]

    def per_item():
        return [tuple(r.clone() for r in item_fn(it)) for it in items]

    def eager():
        return batch_fn(batch)

    want, got = per_item(), tuple(t.clone() for t in eager())
    err = rel = 0.0
    for b, n in enumerate(lens):
        for a, w in ((got[0][b, :n, :n], want[b][0]), (got[1][b, :n], want[b][1])):
            d = float((a - w).abs().max())
            err, rel = max(err, d), max(rel, d / max(float(w.abs().max()), 1e-30))
    print("== %s, LXMERT-base, B = %d questions of %d..%d tokens padded to %d, %d regions" % (method, B, min(lens), max(lens), T_PAD, REGIONS))
    print("    max |batched - per item| over the live blocks = %.3g (%.3g of the map's largest entry)" % (err, rel))
    m = interleaved({"item_a": per_item, "eager_a": eager, "item_b": per_item, "eager_b": eager}, host_timed, warm=2)
    item, eag = 0.5 * (m["item_a"] + m["item_b"]), 0.5 * (m["eager_a"] + m["eager_b"])
    print("    per-item loop (%d calls)   %9.2f ms per batch  %8.1f samples/s   A/A %9.2f / %9.2f ms, spread %.1f %%"
          % (B, item, B / item * 1e3, m["item_a"], m["item_b"], spread(m["item_a"], m["item_b"])))
    print("    batched, eager             %9.2f ms per batch  %8.1f samples/s   A/A %9.2f / %9.2f ms, spread %.1f %%   per-item / batched %.1fx"
          % (eag, B / eag * 1e3, m["eager_a"], m["eager_b"], spread(m["eager_a"], m["eager_b"]), item / eag))


# ------------------------------------------------------------------------------------------------ kernels
def _live_mask(lens, N):
    return (torch.arange(N, device=DEV)[None, :] < lens[:, None]).float()


def torch_attr(text, img, cross, t_len):
    """The same maths as a batched torch composition (masks instead of per-sample loops; the slabs hold finite values everywhere)."""
    T, I = cross[0].shape[2:]
    mt = _live_mask(t_len, T)
    m_tt = mt[:, :, None] * mt[:, None, :]
    abar = lambda c, g: (g * c).clamp(min=0).mean(dim=1)  # noqa: E731
    r = torch.eye(T, device=DEV).expand(len(t_len), T, T) * m_tt
    for c, g in text:
        r = r + torch.bmm(abar(c, g) * m_tt, r)
    ri = torch.eye(I, device=DEV).expand(len(t_len), I, I)
    for c, g in img:
        ri = ri + torch.bmm(abar(c, g), ri)
    r = r.clone()
    r[:, 0, 0] = 0
    return r, abar(*cross) * mt[:, :, None], ri


def torch_minmax(cam, q_len, k_len, zero_cls):
    m = cam.mean(dim=1)
    live = (_live_mask(q_len, cam.shape[2])[:, :, None] * _live_mask(k_len, cam.shape[3])[:, None, :]) > 0
    lo = torch.where(live, m, torch.full_like(m, float("inf"))).amin(dim=(1, 2), keepdim=True)
    hi = torch.where(live, m, torch.full_like(m, float("-inf"))).amax(dim=(1, 2), keepdim=True)
    out = torch.where(live, (m - lo) / (hi - lo), torch.zeros_like(m))
    if zero_cls:
        out[:, 0, 0] = 0
    return out


def part_kernels():
    H, n_text, n_img = 12, 14, 9                    # LXMERT-base: 9 language + 5 x-layers | 5 vision + 4 x-layers
    g = torch.Generator().manual_seed(1)
    t_len = torch.randint(8, T_PAD + 1, (B,), generator=g).to(DEV)
    i_len = torch.full((B,), REGIONS, device=DEV)
    pair = lambda nq, nk: ((torch.randn(B, H, nq, nk, generator=g) * 1e-2).to(DEV), torch.randn(B, H, nq, nk, generator=g).to(DEV))  # noqa: E731
    text = [pair(T_PAD, T_PAD) for _ in range(n_text)]
    img = [pair(REGIONS, REGIONS) for _ in range(n_img)]
    cross = pair(T_PAD, REGIONS)
    slab_mb = sum(c.numel() + gr.numel() for c, gr in text + img + [cross]) * 4 / 2 ** 20
    print("== the new launches alone against a batched torch composition of the same maths: B = %d, H = %d, T = %d, I = %d, %d + %d + 1 "
          "pairs of slabs (%.1f MiB); samples of 10 calls between two events" % (B, H, T_PAD, REGIONS, n_text, n_img, slab_mb))
    rows = [
        ("transformer_att (mmx_lxmert_attr)", lambda: ops.lxmert_transformer_attr(text, img, cross, text_len=t_len),
         lambda: torch_attr(text, img, cross, t_len)),
        ("partial_lrp (two min-max maps)", lambda: (ops.head_minmax_live(text[-1][0], t_len, t_len, True), ops.head_minmax_live(cross[0], t_len)),
         lambda: (torch_minmax(text[-1][0], t_len, t_len, True), torch_minmax(cross[0], t_len, i_len, False))),
    ]
    for name, new, old in rows:
        err = max(float((a - b).abs().max()) for a, b in zip(new(), old()))
        m = interleaved({"new_a": new, "torch_a": old, "new_b": new, "torch_b": old}, event_timed)
        hip, tor = 0.5 * (m["new_a"] + m["new_b"]), 0.5 * (m["torch_a"] + m["torch_b"])
        print("    %-36s HIP %8.4f ms (A/A %8.4f / %8.4f, spread %.1f %%)   torch composition %8.4f ms (A/A spread %.1f %%)   torch / HIP %.1fx   "
              "max |difference| %.2g" % (name, hip, m["new_a"], m["new_b"], spread(m["new_a"], m["new_b"]), tor,
                                         spread(m["torch_a"], m["torch_b"]), tor / hip, err))
    need = ops.lib().mmx_lxmert_attr_workspace_bytes(n_text, n_img, B, T_PAD, REGIONS)
    print("    mmx_lxmert_attr reads %.1f MiB of slabs once and writes + reads %.2f MiB of workspace" % (slab_mb, need / 2 ** 20))


# ------------------------------------------------------------------------------------------------ conditioning (CPU)
def part_conditioning(precision):
    """No GPU: the randomly initialised LXMERT-base of the timing parts with the plain-torch capture stand-in and the oracle's
    attention core (the set-up of tests/test_bert_lrp_host.py), in fp32 or float64: every attention module's LRP cam of a padded
    batch against the same item run alone.  Items 0 and 3 are NOT padded: what they show is the conditioning of the pass itself."""
    from oracle import lrp_torch as lrp_oracle
    from test_bert_lrp_host import capture_stand_in, lxmert_cams
    from transformer_mm_explainability_amd import attention_modules
    dt = torch.float64 if precision == "f64" else torch.float32
    attention_modules.attention_capture = capture_stand_in
    attention_modules._SlabOwner._slabs = lambda self, B_, H, Nq, Nk, device: (torch.empty(B_, H, Nq, Nk, dtype=dt),
                                                                               torch.zeros(B_, H, Nq, Nk, dtype=dt))
    cfg = lm.LxmertConfig()
    torch.manual_seed(0)
    model = lm.LxmertForQuestionAnswering(cfg).eval().to(dt)
    g = torch.Generator().manual_seed(0)
    lens = [20, 13, 8, 20]
    ids, mask = torch.zeros(len(lens), T_PAD, dtype=torch.long), torch.zeros(len(lens), T_PAD, dtype=dt)
    for b, n in enumerate(lens):
        ids[b, :n] = torch.randint(1, cfg.vocab_size, (n,), generator=g)
        mask[b, :n] = 1
    batch = dict(input_ids=ids, attention_mask=mask, token_type_ids=torch.zeros(len(lens), T_PAD, dtype=torch.long),
                 visual_feats=torch.randn(len(lens), REGIONS, cfg.visual_feat_dim, generator=g).to(dt),
                 visual_pos=torch.rand(len(lens), REGIONS, 4, generator=g).to(dt))

    def run(inp, index):
        out = model(**inp).question_answering_score
        idx = out.argmax(-1) if index is None else torch.as_tensor(index)
        one_hot = torch.zeros_like(out).scatter_(1, idx.reshape(-1, 1), 1.0)
        model.zero_grad()
        torch.sum(one_hot * out).backward()
        model.relprop(one_hot.clone(), alpha=1, core=lrp_oracle.core)
        return idx, {n: m.get_attn_cam().detach().clone() for n, m in lxmert_cams(model).items()}, out.detach()

    idx, both, out_b = run(batch, None)
    print("== CPU, %s, LXMERT-base with random weights, stand-in capture op + oracle core: the LRP cams of a padded batch of %s tokens "
          "(padded to %d) against each item alone" % (precision, lens, T_PAD))
    for b, n in enumerate(lens):
        it = {k: (v[b:b + 1, :n] if k in ("input_ids", "attention_mask", "token_type_ids") else v[b:b + 1]) for k, v in batch.items()}
        _, alone, out_1 = run(it, [int(idx[b])])
        worst, at = 0.0, None
        for name, cam in alone.items():
            d = float((both[name][b:b + 1, :, :cam.shape[2], :cam.shape[3]] - cam).abs().max()) / max(float(cam.abs().max()), 1e-300)
            if d > worst:
                worst, at = d, name
        print("    item %d, %2d tokens: max |logits difference| %.2e   worst |cam difference| / max|cam| over the modules %.3e (%s)"
              % (b, n, float((out_b[b] - out_1[0]).abs().max()), worst, at))


# ------------------------------------------------------------------------------------------------ evaluator
def part_evaluator(method, num_samples):
    script = os.path.join(ROOT, "examples", "lxmert_perturbation_eval.py")
    rates = {0: [], 1: []}
    for rep in range(3):
        for flag in (0, 1):
            out = subprocess.run([sys.executable, script, "--method", method, "--num-samples", str(num_samples), "--batch-lrp", str(flag)],
                                 capture_output=True, text=True, timeout=600, check=True).stdout
            res = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            rates[flag].append((res["samples_per_s"], res.get("samples_per_s_after_first_batch"), res["step_accuracy_percent"]))
    print("== evaluator, --method %s --num-samples %d, three alternated child processes per setting (samples/s, whole run | after the first batch)"
          % (method, num_samples))
    for flag in (0, 1):
        whole, after = [r[0] for r in rates[flag]], [r[1] for r in rates[flag] if r[1] is not None]
        print("    --batch-lrp %d   median %8.1f (%s)   after the first batch: median %s (%s)"
              % (flag, statistics.median(whole), " ".join("%.1f" % x for x in whole),
                 "%.1f" % statistics.median(after) if after else "-", " ".join("%.1f" % x for x in after)))
        print("                     step accuracy %% of the last run: %s" % rates[flag][-1][2])
    print("    --batch-lrp 1 / 0: %.1fx on the whole run" % (statistics.median([r[0] for r in rates[1]]) / statistics.median([r[0] for r in rates[0]])))


if __name__ == "__main__":
    a = sys.argv[1:]
    ok = a in (["errors"], ["kernels"], ["conditioning", "f32"], ["conditioning", "f64"]) or \
        (len(a) == 2 and a[0] == "explain" and a[1] in METHODS) or \
        (len(a) in (2, 3) and a[0] == "evaluator" and a[1] in METHODS)
    if not ok:
        raise SystemExit("usage: python tools/probe_lxmert_lrp_batch.py errors | explain METHOD | kernels | evaluator METHOD [num_samples] | "
                         "conditioning f32|f64")
    if a[0] == "evaluator":                          # the children open the GPU, this process does not
        part_evaluator(a[1], int(a[2]) if len(a) == 3 else 128)
    elif a[0] == "conditioning":
        part_conditioning(a[1])
    else:
        print("device: %s" % torch.cuda.get_device_name(0))
        {"errors": part_errors, "kernels": part_kernels}.get(a[0], lambda: part_explain(a[1]))()
