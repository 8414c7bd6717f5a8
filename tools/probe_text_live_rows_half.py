"""Probe (GPU box): the fp16 row-list GEMM (csrc/gemm_rows_f16.hip) and the text tower of an fp16 body on the rows up to EOT (option
``text_live_rows_half``), ViT-B/32 with the 64 captions of bench.synthetic_inputs.

    python tools/probe_text_live_rows_half.py ops        # the four text-tower shapes: kernel vs library path vs the fp32 row-list kernel
    python tools/probe_text_live_rows_half.py step       # GraphedInterpret on the fp16 body, option 0 against option 1
    python tools/probe_text_live_rows_half.py special    # what the MFMA does with subnormal / overflowing fp16 inputs, beside torch.mm
    python tools/probe_text_live_rows_half.py accuracy   # max err / mag of the kernel and of the library product against float64

Each part is its own process (run each under its own `timeout`).  Device events around every timed call, every shape warmed, A and B
alternated call by call, medians.  The A/A line times the SAME call against itself in that interleaving: a difference between two
variants means something only beyond it.
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from transformer_mm_explainability_amd import clip_explainability as ce  # noqa: E402
from transformer_mm_explainability_amd import clip_model, ops  # noqa: E402

DEV = "cuda"
B, NT = 64, 77
SHAPES = ((512, 1536, "in_proj"), (512, 512, "out_proj"), (512, 2048, "c_fc"), (2048, 512, "c_proj"))      # K x N


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner * 1e3                                 # us per call


def interleaved(fns, reps=20, warm=3, inner=10):
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


def part_ops():
    _, texts = bench.synthetic_inputs(B, DEV, 0)
    eot = texts.argmax(dim=-1)
    lists = {"benchmark captions": ops.live_rows(eot, NT), "every row live": ops.live_rows(torch.full_like(eot, NT - 1), NT)}
    g = torch.Generator(device=DEV).manual_seed(0)
    for what, live in lists.items():
        print("== %s: %d live rows of %d; us per call, medians of 20 samples of 10 calls, alternated"
              % (what, int(live.count), live.cap))
        for K, N, name in SHAPES:
            x = torch.randn(B, NT, K, device=DEV, generator=g)
            w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
            bias = torch.randn(N, device=DEV, generator=g)
            out = torch.zeros(B, NT, N, device=DEV)
            fns = {"lib_a": lambda: ops.linear(x, w, bias, torch.float16),
                   "f16": lambda: ops.linear_rows(x, w, bias, live, out=out, dtype=torch.float16),
                   "f32": lambda: ops.linear_rows(x, w, bias, live, out=out),
                   "lib_b": lambda: ops.linear(x, w, bias, torch.float16)}
            m = interleaved(fns)
            line = "    %-8s K %4d N %4d: library fp16 path on all rows %7.1f (A/A %7.1f, spread %4.1f %%) | rows f16 %7.1f | rows f32 %7.1f" \
                % (name, K, N, m["lib_a"], m["lib_b"], spread(m["lib_a"], m["lib_b"]), m["f16"], m["f32"])
            for tn in (32, 64):
                ops.set_option("gemm_rows_tn", tn)
                line += " | f16 tn=%d %7.1f" % (tn, interleaved({"f16": fns["f16"]}, reps=10)["f16"])
            ops.set_option("gemm_rows_tn", 0)
            print(line)


def part_step():
    model = clip_model.random_init("ViT-B/32", seed=0).to(DEV)
    image, texts = bench.synthetic_inputs(B, DEV, 0)
    model.set_body_dtype(torch.float16)
    runs = {}
    for opt in (0, 1):
        ops.set_option("text_live_rows_half", opt)
        runs[opt] = ce.GraphedInterpret(model, image, texts, 0, 0)
        assert (runs[opt]._txt_pending is not None) == bool(opt)
    ops.set_option("text_live_rows_half", 0)
    a, b = [tuple(t.float().clone() for t in runs[o](image, texts)) for o in (0, 1)]
    print("== GraphedInterpret(model, image, texts, 0, 0), ViT-B/32, fp16 body, batch %d; ms per step" % B)
    print("    max |R_text(option 1) - R_text(option 0)| = %.3g, R_image: %.3g (largest entries %.3g / %.3g)"
          % (float((a[0] - b[0]).abs().max()), float((a[1] - b[1]).abs().max()), float(a[0].abs().max()), float(a[1].abs().max())))
    fns = {"opt0_a": lambda: runs[0](image, texts), "opt1": lambda: runs[1](image, texts), "opt0_b": lambda: runs[0](image, texts)}
    for rnd in range(5):
        m = interleaved(fns, reps=10, warm=2, inner=5)
        base = 0.5 * (m["opt0_a"] + m["opt0_b"])
        print("    round %d: option 0 %8.1f us (A/A %8.1f, spread %.2f %%) | option 1 %8.1f us | option 1 / option 0 = %.3f"
              % (rnd, m["opt0_a"], m["opt0_b"], spread(m["opt0_a"], m["opt0_b"]), m["opt1"], m["opt1"] / base))


def part_special():
    """One row, one 1 in the weight per column: C[0, n] = half(A[0, n]) * 1.  Not asserted anywhere: an observation."""
    vals = [1e-5, 6e-8, 2.0 ** -24, 2.0 ** -25, 3e-8, 65504.0, 65519.0, 65520.0, 7e4, -7e4, float("inf"), float("nan")]
    K = N = 16
    x = torch.zeros(1, 32, K, device=DEV)
    x[0, 0, :len(vals)] = torch.tensor(vals, device=DEV)
    w = torch.eye(N, K, device=DEV)
    live = ops.live_rows(torch.tensor([0], device=DEV), 32)
    got = ops.gemm_rows(x, w, live, out=torch.zeros(1, 32, N, device=DEV), dtype=torch.float16)[0, 0]
    lib = torch.mm(x[0, :1].half(), w.half().t(), out_dtype=torch.float32)[0]
    print("== subnormal / overflowing fp16 inputs through the MFMA (one exact product per output), beside torch.mm on the same operands")
    print("    %-12s %-14s %-14s %-14s" % ("fp32 input", "x.half()", "kernel", "torch.mm"))
    for i, v in enumerate(vals):
        print("    %-12.6g %-14.8g %-14.8g %-14.8g" % (v, float(x[0, 0, i].half()), float(got[i]), float(lib[i])))
    # a subnormal PRODUCT input pair: subnormal a times a large weight
    x2 = torch.zeros(1, 32, K, device=DEV)
    x2[0, 0, 0] = 3e-6
    w2 = torch.zeros(N, K, device=DEV)
    w2[0, 0] = 1024.0
    got2 = ops.gemm_rows(x2, w2.t().contiguous(), live, out=torch.zeros(1, 32, N, device=DEV), dtype=torch.float16)[0, 0, 0]
    lib2 = torch.mm(x2[0, :1].half(), w2.half().t(), out_dtype=torch.float32)[0, 0]
    print("    half(3e-6) * 1024: exact %.8g, kernel %.8g, torch.mm %.8g" % (float(x2[0, 0, 0].half()) * 1024, float(got2), float(lib2)))


def part_accuracy():
    _, texts = bench.synthetic_inputs(B, DEV, 0)
    live = ops.live_rows(texts.argmax(dim=-1), NT)
    listed = torch.zeros(B * NT, dtype=torch.bool, device=DEV)
    listed[live.rows[:int(live.count)].long()] = True
    g = torch.Generator(device=DEV).manual_seed(1)
    print("== max |C - ref| / (|A| |W|) on the live rows against float64 on the rounded operands; gamma_K = K u / (1 - K u), u = 2^-23")
    for K, N, name in SHAPES:
        x = torch.randn(B, NT, K, device=DEV, generator=g)
        w = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5
        xh, wh = x.view(-1, K).half(), w.half()
        ref = xh.double() @ wh.double().t()
        mag = (xh.double().abs() @ wh.double().abs().t()).clamp_min(1e-300)
        got = ops.gemm_rows(x, w.t().contiguous(), live, out=torch.zeros(B, NT, N, device=DEV), dtype=torch.float16).view(-1, N)
        lib = torch.mm(xh, wh.t(), out_dtype=torch.float32)
        u = 2.0 ** -23
        print("    %-8s K %4d N %4d: kernel %.3g   library %.3g   gamma_K %.3g"
              % (name, K, N, float(((got.double() - ref).abs() / mag)[listed].max()),
                 float(((lib.double() - ref).abs() / mag)[listed].max()), K * u / (1 - K * u)))


if __name__ == "__main__":
    parts = {"ops": part_ops, "step": part_step, "special": part_special, "accuracy": part_accuracy}
    if len(sys.argv) != 2 or sys.argv[1] not in parts:
        raise SystemExit("usage: python tools/probe_text_live_rows_half.py ops | step | special | accuracy")
    print("device: %s" % torch.cuda.get_device_name(0))
    parts[sys.argv[1]]()
