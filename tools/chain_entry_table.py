#!/usr/bin/env python3
"""The host-side table of the self-attention relevancy chain's C entries and of ``mmx_set_option``: what the library answers WITHOUT a
device.  One line per call, ``section | case | rc or bytes | mmx_last_error()`` (the text only where rc != 0: a success leaves a stale one).

    workspace  ``mmx_self_chain_workspace_bytes`` over a grid of shapes under ``self_chain_algo`` x ``self_chain_groups`` (15 answers per
               line in ``ALGOS`` x ``GROUPS`` order, or ``all <bytes>`` when they agree): pins the cols rule, the group rule on the fixed
               256 compute units a process without a device assumes, and the N = 128 / 129 and LDS limits
    refusal    every refusal of the four entries alone, and pairs of faults for the order of the checks
    call       full calls on made-up addresses: rc -1100 and the first HIP call the route reached (which kernel a shape reaches on a
               device is held by ``check_route`` in ``tests/test_gpu_chain_bounds.py``)
    option     ``mmx_set_option`` for every key, two unknown keys and the null key at -1 .. 9, 32 and 2**31 - 1 (last: it leaves the
               options of the whole library changed)

``profiles/chain_entry_table.txt`` is this output for the library before the chain's dispatcher and option table were rebuilt;
``tests/test_abi_chain_entries.py`` holds the tree's library to it byte for byte.  No GPU: never run it where one is visible (the calls
of the third section would launch on the made-up addresses).  It changes global options: run it in a process of its own.
``python tools/chain_entry_table.py`` (``MMX_LIB_PATH``: another build of the library)"""
import ctypes as C
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32, F16, BF16 = 0, 1, 2
ENTRIES = {                                     # parameter names in the order of include/mmx_relevancy.h
    "mmx_relevancy_self_chain": ["attn", "grad", "L", "B", "H", "N", "dtype", "R_init", "R_out", "Rsq_init", "Rsq_out", "M",
                                 "workspace", "workspace_bytes", "stream"],
    "mmx_relevancy_self_chain_ex": ["attn", "grad", "L", "B", "H", "N", "dtype", "stride", "R_init", "R_out", "Rsq_init", "Rsq_out", "M",
                                    "workspace", "workspace_bytes", "stream"],
    "mmx_relevancy_self_chain_flags": ["attn", "grad", "L", "B", "H", "N", "dtype", "stride", "R_init", "R_out", "Rsq_init", "Rsq_out",
                                       "M", "flags", "workspace", "workspace_bytes", "stream"],
    "mmx_relevancy_self_chain_half": ["attn", "grad", "L", "B", "H", "N", "dtype", "stride", "R_out", "workspace", "workspace_bytes",
                                      "stream"],
}
HALF = "mmx_relevancy_self_chain_half"
OPTION_KEYS = ["self_chain_cols_c", "self_chain_cols_nb", "self_chain_algo", "self_chain_pipe", "self_chain_rows", "bmm_tiles",
               "text_live_rows", "text_live_rows_fwd", "gemm_rows_tm", "gemm_rows_tn", "gemm_rows_pf", "text_live_rows_half",
               "text_live_attn", "clip_head_fused", "self_chain_nt", "self_chain_groups", "attn_head_tile_skip", "attn_head",
               "attn_bf16_v3", "attn_bf16_v2", "attn_stream", "attn_fwd_split", "debug_flags"]
OPTION_VALUES = list(range(-1, 10)) + [32, 2**31 - 1]
CHAIN_DEFAULTS = {"self_chain_cols_c": 0, "self_chain_cols_nb": 0, "self_chain_algo": 0, "self_chain_pipe": 4, "self_chain_rows": 0,
                  "bmm_tiles": 1, "self_chain_nt": 1, "self_chain_groups": 0, "debug_flags": 0}
ALGOS, GROUPS = (0, 1, 5), (0, 1, 2, 4, 8)
BASE = 0x7f0000000000                           # made-up, 4096-byte aligned addresses


def addr(i):
    return BASE + 4096 * i


def layer_table(n, null_at=None):
    """HOST table of ``n`` made-up layer addresses (at least one slot, so that the pointer is never null)."""
    t = (C.c_void_p * max(n, 1))(*[addr(100 + i) for i in range(max(n, 1))])
    if null_at is not None:
        t[null_at] = None
    return t


def valid(entry):
    """A valid argument set: 2 layers, B 2, H 2, N 20, fp32 slabs, the full batch stride, no R_sq, a workspace of any size."""
    return dict(attn=layer_table(2), grad=layer_table(2), L=2, B=2, H=2, N=20, dtype=F32, stride=-1, R_init=None, R_out=addr(1),
                Rsq_init=None, Rsq_out=None, M=0, flags=0, workspace=addr(2), workspace_bytes=1 << 40, stream=None)


def call(handle, entry, over):
    vals = dict(valid(entry), **over)
    if "L" in over and "attn" not in over and 0 < over["L"] <= 48:
        vals.update(attn=layer_table(over["L"]), grad=layer_table(over["L"]))
    rc = getattr(handle, entry)(*[vals[n] for n in ENTRIES[entry]])
    return rc, (handle.mmx_last_error().decode("utf-8", "replace") if rc else "")


def set_options(handle, **kv):
    for k, v in kv.items():
        if handle.mmx_set_option(k.encode(), v) != 0:
            raise RuntimeError("mmx_set_option(%s, %d) refused" % (k, v))


def workspace_lines(handle):
    lines = []
    shapes = itertools.product((0, 1, 2, 3, 12, 48), (1, 16, 64, 129, 300), (1, 8), (1, 16, 39, 40, 77, 112, 113, 128, 129, 577), (0, 5))
    for L, B, H, N, M in shapes:
        got = []
        for algo in ALGOS:
            for groups in GROUPS:
                set_options(handle, self_chain_algo=algo, self_chain_groups=groups)
                got.append(handle.mmx_self_chain_workspace_bytes(L, B, H, N, M, F32))
        text = "all %d" % got[0] if len(set(got)) == 1 else " ".join(map(str, got))
        lines.append("workspace | L=%d B=%d H=%d N=%d M=%d | %s | " % (L, B, H, N, M, text))
    set_options(handle, **CHAIN_DEFAULTS)
    return lines


def refusal_cases(entry):
    """``(case name, options, overrides of the valid set)`` of one entry."""
    half, names = entry == HALF, ENTRIES[entry]
    out = [("null attn table", {}, {"attn": None}), ("null grad table", {}, {"grad": None}), ("null R_out", {}, {"R_out": None}),
           ("L=-1", {}, {"L": -1}), ("L=49", {}, {"L": 49}), ("B=0", {}, {"B": 0}), ("B=-1", {}, {"B": -1}), ("H=0", {}, {"H": 0}),
           ("N=0", {}, {"N": 0}), ("N=-1", {}, {"N": -1}), ("dtype 3", {}, {"dtype": 3}), ("dtype -1", {}, {"dtype": -1}),
           ("null attn layer 1", {}, {"attn": layer_table(2, 1)}), ("null grad layer 0", {}, {"grad": layer_table(2, 0)}),
           ("null R_out and L=49", {}, {"R_out": None, "L": 49}), ("L=49 and B=0", {}, {"L": 49, "B": 0}),
           ("B=0 and dtype 3", {}, {"B": 0, "dtype": 3}), ("dtype 3 and null attn layer 0", {}, {"dtype": 3, "attn": layer_table(2, 0)}),
           ("null attn layer 1 and null grad layer 0", {}, {"attn": layer_table(2, 1), "grad": layer_table(2, 0)}),
           ("N=129, no workspace", {}, {"N": 129, "workspace": None}), ("N=129, workspace short by 1", {}, {"N": 129, "workspace_bytes": None}),
           ("N=129, null grad layer 1 and no workspace", {}, {"N": 129, "grad": layer_table(2, 1), "workspace": None})]
    if "stride" in names:
        out += [("stride 5", {}, {"stride": 5}), ("stride 5 and null attn table", {}, {"stride": 5, "attn": None}),
                ("stride 5 and N=0", {}, {"stride": 5, "N": 0}), ("stride 0 and L=49", {}, {"stride": 0, "L": 49})]
    if half:
        out += [("bf16 slabs", {}, {"dtype": BF16}), ("bf16 slabs and B=0", {}, {"dtype": BF16, "B": 0})]
    else:
        out += [("M=-1", {}, {"M": -1}), ("M=5, no R_sq output", {}, {"M": 5}), ("M=0 with an R_sq output", {}, {"Rsq_out": addr(3)}),
                ("B=0 and M=5, no R_sq output", {}, {"B": 0, "M": 5}), ("M=5, no R_sq output and dtype 3", {}, {"M": 5, "dtype": 3}),
                ("M=5, no workspace", {}, {"M": 5, "Rsq_out": addr(3), "workspace": None}),
                ("M=5, workspace short by 1", {}, {"M": 5, "Rsq_out": addr(3), "workspace_bytes": None})]
        for algo in (0, 1):
            opts = {"self_chain_groups": 2, "self_chain_algo": algo}
            out += [("2 groups algo %d, no workspace" % algo, opts, {"workspace": None}),
                    ("2 groups algo %d, workspace short by 1" % algo, opts, {"workspace_bytes": None}),
                    ("2 groups algo %d, null grad layer 1 and no workspace" % algo, opts, {"grad": layer_table(2, 1), "workspace": None})]
    if "flags" in names:
        out += [("flags 2", {}, {"flags": 2}), ("flags 0x80000001", {}, {"flags": 0x80000001}), ("flags 2 and stride 5", {}, {"flags": 2, "stride": 5}),
                ("flags 2 and null R_out", {}, {"flags": 2, "R_out": None})]
    return out


def refusal_lines(handle):
    lines = []
    for entry in ENTRIES:
        for case, opts, over in refusal_cases(entry):
            set_options(handle, **opts)
            if "workspace_bytes" in over:           # short by 1: of what the query answers under these options
                v = dict(valid(entry), **over)
                over = dict(over, workspace_bytes=handle.mmx_self_chain_workspace_bytes(v["L"], v["B"], v["H"], v["N"], v["M"], v["dtype"]) - 1)
            rc, text = call(handle, entry, over)
            lines.append("refusal | %s: %s | %d | %s" % (entry, case, rc, text))
            set_options(handle, **CHAIN_DEFAULTS)
    return lines


CALLS = [       # (entry, case, options, overrides): one per route and per first HIP call of a route
    ("mmx_relevancy_self_chain", "N=20: fused kernel, static LDS limit", {}, {}),
    ("mmx_relevancy_self_chain", "N=20 L=0: fused kernel", {}, {"L": 0}),
    ("mmx_relevancy_self_chain_ex", "N=20 shared forward: fused kernel", {}, {"stride": 0}),
    ("mmx_relevancy_self_chain_flags", "N=128 algo 1: fused kernel above 48 KiB", {"self_chain_algo": 1}, {"N": 128}),
    ("mmx_relevancy_self_chain_flags", "N=20 fp16 slabs: fused kernel", {}, {"dtype": F16}),
    ("mmx_relevancy_self_chain_flags", "N=77 bf16 slabs L=12 B=16 H=8: fused kernel with groups", {}, {"N": 77, "dtype": BF16, "L": 12, "B": 16, "H": 8}),
    ("mmx_relevancy_self_chain_flags", "N=77 L=12 B=16 H=8 causal: groups kernel", {}, {"N": 77, "L": 12, "B": 16, "H": 8, "flags": 1}),
    ("mmx_relevancy_self_chain_flags", "N=77 L=12 B=16 H=8 algo 1: fused kernel with groups", {"self_chain_algo": 1}, {"N": 77, "L": 12, "B": 16, "H": 8}),
    ("mmx_relevancy_self_chain_flags", "N=128 L=48 2 groups: fused kernel with groups (the groups kernel's images do not fit)",
     {"self_chain_groups": 2}, {"N": 128, "L": 48}),
    ("mmx_relevancy_self_chain_flags", "N=112 L=6 2 groups: groups kernel (three images fit)", {"self_chain_groups": 2}, {"N": 112, "L": 6}),
    ("mmx_relevancy_self_chain_flags", "N=113 L=6 2 groups: fused kernel with groups (three images do not fit)", {"self_chain_groups": 2},
     {"N": 113, "L": 6}),
    ("mmx_relevancy_self_chain_flags", "N=40 L=1: cols kernel", {}, {"N": 40, "L": 1}),
    ("mmx_relevancy_self_chain_flags", "N=77 L=12 B=300 H=8: cols kernel above 48 KiB", {}, {"N": 77, "L": 12, "B": 300, "H": 8}),
    ("mmx_relevancy_self_chain_flags", "N=20 algo 5: cols kernel", {"self_chain_algo": 5}, {}),
    ("mmx_relevancy_self_chain_flags", "N=129: split path from the identity", {}, {"N": 129}),
    ("mmx_relevancy_self_chain_flags", "N=129 with R_init: split path", {}, {"N": 129, "R_init": addr(4)}),
    ("mmx_relevancy_self_chain_flags", "N=20 M=5: split path", {}, {"M": 5, "Rsq_out": addr(3)}),
    ("mmx_relevancy_self_chain_flags", "N=129 self_chain_rows: rows kernel", {"self_chain_rows": 1}, {"N": 129}),
    ("mmx_relevancy_self_chain_flags", "N=129 self_chain_rows L=0: identity", {"self_chain_rows": 1}, {"N": 129, "L": 0}),
    (HALF, "N=20: fused kernel", {}, {}),
    (HALF, "N=128 fp16 slabs: fused kernel above 48 KiB", {}, {"N": 128, "dtype": F16}),
    (HALF, "N=129: long path", {}, {"N": 129}),
]


def call_lines(handle):
    lines = []
    for entry, case, opts, over in CALLS:
        set_options(handle, **opts)
        rc, text = call(handle, entry, over)
        lines.append("call | %s: %s | %d | %s" % (entry, case, rc, text))
        set_options(handle, **CHAIN_DEFAULTS)
    return lines


def option_lines(handle):
    lines = []
    for key in OPTION_KEYS + ["no_such_option", "", None]:
        for value in OPTION_VALUES:
            rc = handle.mmx_set_option(None if key is None else key.encode(), value)
            lines.append("option | %s=%d | %d | %s" % ("(null key)" if key is None else key, value, rc,
                                                       handle.mmx_last_error().decode("utf-8", "replace") if rc else ""))
    return lines


def table(handle):
    return workspace_lines(handle) + refusal_lines(handle) + call_lines(handle) + option_lines(handle)


def load(path):
    from transformer_mm_explainability_amd import _lib
    handle = C.CDLL(path)
    for name, (res, args) in _lib._PROTOTYPES.items():
        if name in ENTRIES or name in ("mmx_self_chain_workspace_bytes", "mmx_set_option", "mmx_last_error"):
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
    return handle


def main():
    from transformer_mm_explainability_amd import _lib
    print("\n".join(table(load(os.environ.get("MMX_LIB_PATH") or _lib.LIB_PATH))))


if __name__ == "__main__":
    main()
