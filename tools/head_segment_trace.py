"""The serial head segment of the CLIP headline step, out of a rocprofv3 kernel trace (CSV) of ``bench.py --headline-only``.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o step -- python bench.py --steps 20 --warmup 3 --no-cpu-baseline --headline-only
    python tools/head_segment_trace.py DIR [step index from the end, default 2] > segment.txt

One replayed step is what lies between two launches of the text tower's chain kernel (once per step, the last kernel of the main stream).
Inside it:
  A  the text forward's last row-list GEMM with a bias epilogue (``gemm_rows_f32_kernel<..., 1>``: the forward is the only user of EPI 1)
  B  the image backward's first dense library GEMM (the first ``Cijk_*`` dispatch after A whose workgroups x macro tile cover >= 2 M
     output elements: 3200 rows x 768; the 64-row products of the head cover <= 0.2 M)
  T  the text backward's first row-list GEMM without epilogue (``gemm_rows_f32_kernel<..., 0>``) after A
and the dispatches that START in [end of A, start of B) -- the stretch no tower can overlap -- are listed with queue, workgroups and
duration, then summed; the same for [end of A, start of T) on T's queue.  Totals per step: dispatches, kernel time, ATen / copy launches."""
import csv
import os
import re
import sys


def load(directory):
    for root, _, files in os.walk(directory):
        for name in files:
            if name.endswith("kernel_trace.csv"):
                with open(os.path.join(root, name)) as f:
                    return list(csv.DictReader(f))
    raise SystemExit("no *kernel_trace.csv under %s" % directory)


def _int(row, *keys):
    for k in keys:
        if row.get(k) not in (None, ""):
            return int(float(row[k]))
    return 1


def workgroups(r):
    n = 1
    for ax in "XYZ":
        g, w = _int(r, "Grid_Size_" + ax, "Grid_Size"), max(1, _int(r, "Workgroup_Size_" + ax, "Workgroup_Size"))
        n *= max(1, (g + w - 1) // w)
        if ("Grid_Size_" + ax) not in r:
            break
    return n


def covered_outputs(r):
    m = re.search(r"MT(\d+)x(\d+)x", r["Kernel_Name"])
    return workgroups(r) * int(m.group(1)) * int(m.group(2)) if m else 0


def is_aten(name):
    return "at::native" in name or "__amd_rocclr_copyBuffer" in name or "__amd_rocclr_fillBuffer" in name


def short(name):
    name = re.sub(r"\(.*", "", name.replace("void ", ""))
    return name if len(name) <= 110 else name[:107] + "..."


def listing(rows, t0):
    out, total = [], 0.0
    for r in rows:
        us = (r["e"] - r["s"]) / 1e3
        total += us
        out.append("  +%8.2f us  q%-3s %6d wg  %7.2f us  %s" % ((r["s"] - t0) / 1e3, r.get("Queue_Id", "?"), workgroups(r), us, short(r["Kernel_Name"])))
    return out, total


def main():
    directory = sys.argv[1]
    back = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    rows = load(directory)
    for r in rows:
        r["s"], r["e"] = float(r["Start_Timestamp"]), float(r["End_Timestamp"])
    rows.sort(key=lambda r: r["s"])
    ends = [i for i, r in enumerate(rows) if "self_chain_groups_kernel<5>" in r["Kernel_Name"]]
    if len(ends) < back + 1:
        raise SystemExit("only %d text-chain launches in the trace" % len(ends))
    step = rows[ends[-back - 1] + 1:ends[-back] + 1]
    print("trace: %d dispatches, %d text-chain launches; step taken: the %d. from the end" % (len(rows), len(ends), back))
    print("step: %d dispatches, kernel time %.1f us, wall %.1f us (first start to last end)"
          % (len(step), sum(r["e"] - r["s"] for r in step) / 1e3, (max(r["e"] for r in step) - step[0]["s"]) / 1e3))
    aten = [r for r in step if is_aten(r["Kernel_Name"])]
    print("at::native / __amd_rocclr_* dispatches in the step: %d, %.1f us of kernel time" % (len(aten), sum(r["e"] - r["s"] for r in aten) / 1e3))
    names = {}
    for r in aten:
        key = short(r["Kernel_Name"])
        names[key] = names.get(key, 0) + 1
    for key, n in sorted(names.items(), key=lambda kv: -kv[1]):
        print("  %3d x %s" % (n, key))
    fwd = [i for i, r in enumerate(step) if re.search(r"gemm_rows_f32_kernel<[^>]*, 1>", r["Kernel_Name"])]
    if not fwd:
        raise SystemExit("no gemm_rows_f32_kernel<..., 1> in the step (dense text forward?)")
    a = step[fwd[-1]]
    after = [r for r in step if r["s"] >= a["e"]]
    b = next((r for r in after if r["Kernel_Name"].startswith("Cijk_") and covered_outputs(r) >= 2000000), None)
    t = next((r for r in after if re.search(r"gemm_rows_f32_kernel<[^>]*, 0>", r["Kernel_Name"])), None)
    print("\nA  %s  (%d wg) ends at 0" % (short(a["Kernel_Name"]), workgroups(a)))
    if b is not None:
        seg = [r for r in after if r["s"] < b["s"]]
        lines, total = listing(seg, a["e"])
        print("B  %s  (%d wg, %.1f us) starts at +%.2f us" % (short(b["Kernel_Name"]), workgroups(b), (b["e"] - b["s"]) / 1e3, (b["s"] - a["e"]) / 1e3))
        print("stretch A -> B: %d dispatches (all queues), kernel time %.2f us, wall span %.2f us; %d of them at::native / copies"
              % (len(seg), total, (b["s"] - a["e"]) / 1e3, sum(is_aten(r["Kernel_Name"]) for r in seg)))
        print("\n".join(lines))
    if t is not None:
        seg = [r for r in after if r["s"] < t["s"] and r.get("Queue_Id") == t.get("Queue_Id")]
        lines, total = listing(seg, a["e"])
        print("\nT  %s  (%d wg) starts at +%.2f us" % (short(t["Kernel_Name"]), workgroups(t), (t["s"] - a["e"]) / 1e3))
        print("head of the text backward, A -> T on T's queue: %d dispatches, kernel time %.2f us, wall span %.2f us"
              % (len(seg), total, (t["s"] - a["e"]) / 1e3))
        print("\n".join(lines))


if __name__ == "__main__":
    main()
