#!/usr/bin/env python3
"""Probe (GPU box): the depth of the register ring of ``gemm_rows_f32_kernel`` (option ``gemm_rows_pf``) at the launch shapes of the
headline step -- capacity 4928 rows, the 531-row list of the benchmark's captions (19 of 9 tokens, 45 of 8), (N, K) = (512, 512),
(512, 1536), (512, 2048), (1536, 512), (2048, 512) with the epilogues the step uses there.

    python tools/probe_gemm_rows_depth.py sweep [--parent PARENT_LIB] [--rounds 5] [--tiles 32x64,32x32,64x64] [--depths 3,4]
        op-level timing.  Per round one FRESH process per library (the tree's own, and PARENT_LIB through MMX_LIB_PATH: parent (A), tree,
        parent (B)); per configuration 200 launches captured in one linear graph, 2 warm-up replays, device events around 30 replays;
        us per launch, medians and max - min spreads over the rounds.  A child that fails ends the sweep.
    python tools/probe_gemm_rows_depth.py time [--tiles ...] [--depths ...]     one such process (what sweep starts); depth 0 only: a library
        without the option (the parent)
    python tools/probe_gemm_rows_depth.py sha [--depths ...]      sha256 of the raw bytes of every output: the cases of
        tests/test_gpu_gemm_rows_pipeline.py and the five launch shapes, every tile, plain / + bias / + bias and QuickGELU.  Run once per
        library (MMX_LIB_PATH) and compare the lines.
    python tools/probe_gemm_rows_depth.py launches N K PF [COUNT] [TN]   COUNT plain launches of one shape (for a counter or trace pass
        under rocprofv3; the program goes after its `--`)
"""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, NT = 64, 77
# (N, K, epilogues the step runs at that shape: 0 plain (backward), 1 + bias, 2 + bias + QuickGELU (forward))
SHAPES = ((512, 512, (0, 1)), (512, 1536, (0,)), (512, 2048, (0, 1)), (1536, 512, (1,)), (2048, 512, (0, 2)))
TILE_OPTIONS = {"32x64": (32, 64), "32x32": (32, 32), "64x64": (64, 0)}
CHILD_TIMEOUT = 240


def bench_list(ops, torch):
    eot = torch.tensor([8] * 19 + [7] * 45, device="cuda")
    live = ops.live_rows(eot, NT)
    assert int(live.count) == 531
    return live


def set_tile(ops, tile, pf):
    tm, tn = TILE_OPTIONS[tile]
    ops.set_option("gemm_rows_tm", tm)
    ops.set_option("gemm_rows_tn", tn)
    if pf:                                                   # (a library without the option is only ever asked for depth 0)
        ops.set_option("gemm_rows_pf", pf)


def operands(torch, N, K, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(B, NT, K, device="cuda", generator=g)
    w = torch.randn(K, N, device="cuda", generator=g) / K ** 0.5
    bias = torch.randn(N, device="cuda", generator=g)
    return x, w, w.t().contiguous(), bias


def entry(ops, epi, x, w, wt, bias, live, out, act):
    if epi == 0:
        return lambda: ops.gemm_rows(x, w, live, out=out)
    if epi == 1:
        return lambda: ops.linear_rows(x, wt, bias, live, out=out)
    return lambda: ops.linear_rows(x, wt, bias, live, out=out, gelu=True, act_out=act)


def graph_us(torch, fn, launches=200, warm=2, replays=30):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    for _ in range(warm):
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (replays * launches) * 1e3


def part_time(args):
    import torch
    from transformer_mm_explainability_amd import ops
    live = bench_list(ops, torch)
    for N, K, epis in SHAPES:
        x, w, wt, bias = operands(torch, N, K, N + K)
        out, act = torch.zeros(B, NT, N, device="cuda"), torch.zeros(B, NT, N, device="cuda")
        for tile in args.tiles:
            for pf in args.depths:
                set_tile(ops, tile, pf)
                for epi in epis:
                    us = graph_us(torch, entry(ops, epi, x, w, wt, bias, live, out, act))
                    print("T %s pf%d EPI%d N%d K%d %.3f" % (tile, pf, epi, N, K, us), flush=True)


def part_sha(args):
    import torch
    from transformer_mm_explainability_amd import ops

    def digest(*tensors):
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().cpu().contiguous().numpy().tobytes())
        return h.hexdigest()[:16]

    def three(x, w, bias, live):
        n = w.shape[1]
        fill = lambda: torch.full(x.shape[:-1] + (n,), 7.25, device="cuda")
        wt = w.t().contiguous()
        pre, act = ops.linear_rows(x, wt, bias, live, out=fill(), gelu=True, act_out=fill())
        return digest(ops.gemm_rows(x, w, live, out=fill()), ops.linear_rows(x, wt, bias, live, out=fill()), pre, act)

    def small(K, N, cap, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        return (torch.randn(1, cap, K, device="cuda", generator=g), torch.randn(K, N, device="cuda", generator=g) / K ** 0.5,
                torch.randn(N, device="cuda", generator=g))

    def hand(entries, cap, count=None):
        rows = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
        if entries:
            rows[:len(entries)] = torch.tensor(entries, dtype=torch.int32, device="cuda")
        return ops.LiveRows(rows, torch.tensor([len(entries) if count is None else count], dtype=torch.int32, device="cuda"), 1, cap)

    big = bench_list(ops, torch)
    caps = ops.live_rows(torch.tensor([2, 7, 0], device="cuda"), 8)
    perm = torch.randperm(70, generator=torch.Generator().manual_seed(5)).tolist()
    lists = {"count0": ([], None), "count1": ([41], None), "count_cap": (list(range(70)), None), "count33": (list(range(3, 36)), None),
             "count65": (list(range(2, 67)), None), "outside": ([5, -1, 17, 70, 64, 370, 33], None), "shuffled": (perm[:45], None),
             "count_above_cap": (list(range(70)), 79)}
    for tile in TILE_OPTIONS:
        for pf in args.depths:
            set_tile(ops, tile, pf)
            for K in (4, 20, 32, 36, 64, 68, 96, 128, 192, 200, 256, 2048):
                for N in ((16, 36, 64, 100) if K != 2048 else (64,)):
                    x, w, bias = small(K, N, 24, K * 1000 + N if K != 2048 else 11)
                    print("S %s pf%d edges K%d N%d %s" % (tile, pf, K, N, three(x.view(3, 8, K), w, bias, caps)))
            for K, N in ((36, 36), (200, 100)):
                x, w, bias = small(K, N, 70, K + N)
                for name, (entries, count) in lists.items():
                    print("S %s pf%d %s K%d N%d %s" % (tile, pf, name, K, N, three(x, w, bias, hand(entries, 70, count))))
            for N, K, _ in SHAPES:
                x, w, _, bias = operands(torch, N, K, N + K)
                print("S %s pf%d step N%d K%d %s" % (tile, pf, N, K, three(x, w, bias, big)), flush=True)


def part_launches(args):
    import torch
    from transformer_mm_explainability_amd import ops
    N, K, pf = (int(v) for v in args.rest[:3])
    count = int(args.rest[3]) if len(args.rest) > 3 else 50
    tile = "32x32" if len(args.rest) > 4 and args.rest[4] == "32" else "32x64"
    live = bench_list(ops, torch)
    x, w, wt, bias = operands(torch, N, K, N + K)
    out = torch.zeros(B, NT, N, device="cuda")
    set_tile(ops, tile, pf)
    for _ in range(count):
        ops.gemm_rows(x, w, live, out=out)
    torch.cuda.synchronize()


def child(lib_path, depths, tiles):
    env = dict(os.environ)
    env.pop("MMX_LIB_PATH", None)
    if lib_path:
        env["MMX_LIB_PATH"] = lib_path
    cmd = [sys.executable, os.path.abspath(__file__), "time", "--depths", ",".join(map(str, depths)), "--tiles", ",".join(tiles)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    if r.returncode != 0:
        sys.stdout.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("a timing process ended with status %d: the sweep stops here" % r.returncode)
    got = {}
    for line in r.stdout.splitlines():
        if line.startswith("T "):
            _, tile, pf, epi, n, k, us = line.split()
            got[(tile, int(pf[2:]), epi, n, k)] = float(us)
    return got


def part_sweep(args):
    series = (["parentA"] if args.parent else []) + ["tree"] + (["parentB"] if args.parent else [])
    runs = {s: [] for s in series}
    for rnd in range(args.rounds):
        for s in series:
            runs[s].append(child(args.parent, (0,), args.tiles) if s != "tree" else child(None, args.depths, args.tiles))
            print("round %d %s done" % (rnd, s), flush=True)
    med = lambda v: statistics.median(v)
    spr = lambda v: max(v) - min(v)
    fmt = lambda v: " ".join("%6.2f" % t for t in v) + "  med %6.2f spr %4.2f" % (med(v), spr(v))
    for N, K, epis in SHAPES:
        for tile in args.tiles:
            for epi in epis:
                key = lambda pf: (tile, pf, "EPI%d" % epi, "N%d" % N, "K%d" % K)
                base = None
                if args.parent:
                    pa, pb = [r[key(0)] for r in runs["parentA"]], [r[key(0)] for r in runs["parentB"]]
                    base = pa + pb
                    print("%s EPI%d N%d K%d parent A | %s" % (tile, epi, N, K, fmt(pa)))
                    print("%s EPI%d N%d K%d parent B | %s" % (tile, epi, N, K, fmt(pb)))
                for pf in args.depths:
                    t = [r[key(pf)] for r in runs["tree"]]
                    line = "%s EPI%d N%d K%d tree pf%d | %s" % (tile, epi, N, K, pf, fmt(t))
                    if base:
                        d = med(t) - med(base)
                        line += "  T-P %+5.2f %s" % (d, "FASTER" if -d > max(spr(t), spr(pa), spr(pb)) else
                                                     ("SLOWER" if d > max(spr(t), spr(pa), spr(pb)) else "same"))
                    print(line)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=("sweep", "time", "sha", "launches"))
    ap.add_argument("rest", nargs="*")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tiles", default="32x64,32x32,64x64")
    ap.add_argument("--depths", default="3,4")
    a = ap.parse_args()
    a.tiles = a.tiles.split(",")
    a.depths = [int(v) for v in a.depths.split(",")]
    {"sweep": part_sweep, "time": part_time, "sha": part_sha, "launches": part_launches}[a.part](a)
