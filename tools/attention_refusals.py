#!/usr/bin/env python3
"""The refusal table of the 11 launching attention entries of ``csrc/attention_kernels.hip``: every entry called on made-up, aligned
addresses with one (or, for the order of the checks, two) arguments of a valid set spoiled, so that an argument check refuses the call
before any HIP call.  One line per call: ``entry | case | rc | mmx_last_error()``.  ``profiles/attention_entry_refusals.txt`` is this
output for the library before the entries were rebuilt on one fill and one run function; ``tests/test_abi_attention_entries.py``
holds the tree's library to it byte for byte.  No GPU: never run it where one is visible (a call that slipped past a dropped check
would launch on the made-up addresses; without a device it fails at the launch and shows up as a differing line).
``python tools/attention_refusals.py`` (``MMX_LIB_PATH``: another build of the library)"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32, F16, MMA_BF16 = 0, 1, 0x100
QKV = ["q", "k", "v"] + [t + s for t in "qkv" for s in ("_sb", "_sh", "_sn")]
MASK = ["mask", "mask_sb", "mask_sq"]
OUT = ["o", "o_sb", "o_sh", "o_sn"]
SIZES = ["B", "H", "Nq", "Nk", "D", "scale", "scale_mode"]
BWD_IN = ["do", "o_sb", "o_sh", "o_sn"]
FWD_O = ["fwd_o", "fo_sb", "fo_sh", "fo_sn"]
GRADS = ["dprobs", "dq", "dk", "dv"] + [t + s for t in ("dq", "dk", "dv") for s in ("_sb", "_sh", "_sn")]
WS = ["workspace", "workspace_bytes", "stream"]
REL = ["rel_in", "rel_out"]
_BWD_EX = QKV + ["probs", "probs_sb", "slab_dtype"] + BWD_IN + FWD_O + GRADS + SIZES + ["need_dqkv"]
ENTRIES = {                                     # parameter names in the order of include/mmx_relevancy.h
    "mmx_attn_capture_fwd": QKV + MASK + ["probs"] + OUT + SIZES + ["stream"],
    "mmx_attn_capture_fwd_ex": QKV + MASK + ["probs", "slab_dtype"] + OUT + SIZES + ["stream"],
    "mmx_attn_capture_fwd_live": QKV + MASK + ["probs", "slab_dtype"] + OUT + SIZES + ["eot", "stream"],
    "mmx_attn_fwd": QKV + MASK + OUT + SIZES + ["stream"],
    "mmx_attn_fwd_live": QKV + MASK + OUT + SIZES + ["eot", "stream"],
    "mmx_attn_capture_bwd": QKV + ["probs", "probs_sb"] + BWD_IN + GRADS + SIZES + ["need_dqkv"] + WS,
    "mmx_attn_capture_bwd_ex": _BWD_EX + WS,
    "mmx_attn_capture_bwd_live": QKV + ["probs", "probs_sb", "slab_dtype"] + BWD_IN + GRADS + SIZES + ["need_dqkv", "eot"] + WS,
    "mmx_attn_capture_bwd_rowrel": _BWD_EX + REL + WS,
    "mmx_attn_capture_bwd_rowrel_f32": _BWD_EX + REL + WS,
    "mmx_attn_capture_bwd_rowrel_f32_grouped": _BWD_EX + REL + ["n_images"] + WS,
}
ROW_WS = {"mmx_attn_capture_bwd_rowrel": "mmx_attn_capture_bwd_rowrel_workspace_bytes",
          "mmx_attn_capture_bwd_rowrel_f32": "mmx_attn_capture_bwd_rowrel_f32_workspace_bytes",
          "mmx_attn_capture_bwd_rowrel_f32_grouped": "mmx_attn_capture_bwd_rowrel_f32_grouped_workspace_bytes"}
GROUPED = "mmx_attn_capture_bwd_rowrel_f32_grouped"
POINTERS = ("q", "k", "v", "mask", "probs", "o", "do", "fwd_o", "dprobs", "dq", "dk", "dv", "rel_in", "rel_out", "eot", "workspace")


def valid(entry):
    """A valid argument set: B 2 (grouped: 6 targets over 3 images), H 4, N 50, D 64, bnhd strides, made-up 4096-byte aligned addresses."""
    H, N, D = 4, 50, 64
    vals = {name: 0x7f0000000000 + 4096 * i for i, name in enumerate(POINTERS)}
    for t in ("q", "k", "v", "o", "fo", "dq", "dk", "dv"):
        vals.update({t + "_sb": N * H * D, t + "_sh": D, t + "_sn": H * D})
    vals.update(mask_sb=0, mask_sq=N, probs_sb=H * N * N, B=6 if entry == GROUPED else 2, H=H, Nq=N, Nk=N, D=D, scale=0.125,
                scale_mode=1, need_dqkv=1, n_images=3, workspace_bytes=1 << 40, stream=None,
                slab_dtype=F32 | MMA_BF16 if entry == "mmx_attn_capture_bwd_rowrel" else F32)
    return vals


def cases(handle, entry):
    """``(case name, overrides of the valid set)`` of one entry."""
    names = ENTRIES[entry]
    row, bwd, live = entry in ROW_WS, "bwd" in entry, entry.endswith("_live")
    required = [p for p in POINTERS if p in names and p not in ("mask", "fwd_o", "workspace") and not (row and p == "dprobs")]
    out = [("null %s" % p, {p: None}) for p in required]
    out += [("%s=%d" % (s, n), {s: n}) for s in ("B", "H", "Nq", "Nk", "D") for n in (0, -1)]
    out += [("B=65536", {"B": 65536 * 3 if entry == GROUPED else 65536}), ("H=65536", {"H": 65536}), ("scale_mode=2", {"scale_mode": 2}),
            ("D=65", {"D": 65}), ("D=68", {"D": 68})]
    if "slab_dtype" in names:
        out.append(("slab dtype 3", {"slab_dtype": 3}))
    v = valid(entry)
    if bwd and not row:
        need = handle.mmx_attn_capture_bwd_workspace_bytes(v["B"], v["H"], v["Nq"])
        out += [("need_dqkv, no workspace", {"workspace": None}), ("need_dqkv, workspace short by 1", {"workspace_bytes": need - 1}),
                ("D=0 and need_dqkv workspace short by 1", {"D": 0, "workspace_bytes": need - 1}),
                ("D=65 and no workspace", {"D": 65, "workspace": None}), ("null v and B=0", {"v": None, "B": 0})]
    if row:
        need = getattr(handle, ROW_WS[entry])(v["B"], v["H"], v["Nq"], v["Nk"])
        out += [("row mode, no workspace", {"workspace": None}), ("row mode, workspace short by 1", {"workspace_bytes": need - 1}),
                ("row mode, Nq != Nk", {"Nq": 49}), ("row workspace short by 1 and D=0", {"workspace_bytes": need - 1, "D": 0}),
                ("row workspace short by 1 and scale_mode=2", {"workspace_bytes": need - 1, "scale_mode": 2}),
                ("row workspace short by 1 and D=65", {"workspace_bytes": need - 1, "D": 65}),
                ("null rel_out and slab dtype 3", {"rel_out": None, "slab_dtype": 3}),
                ("null probs and row workspace short by 1", {"probs": None, "workspace_bytes": need - 1})]
    if entry == "mmx_attn_capture_bwd_rowrel":
        out += [("no MMX_ATTN_MMA_BF16", {"slab_dtype": F32}), ("no MMX_ATTN_MMA_BF16 and Nk=0", {"slab_dtype": F32, "Nk": 0})]
    if entry in ("mmx_attn_capture_bwd_rowrel_f32", GROUPED):
        out += [("fp16 slab", {"slab_dtype": F16}), ("fp16 slab and row workspace short by 1", {"slab_dtype": F16, "workspace_bytes": need - 1}),
                ("N=300, need_dqkv, no dP slab", {"Nq": 300, "Nk": 300, "dprobs": None})]
    if entry == GROUPED:
        out += [("B=%d n_images=%d" % bn, {"B": bn[0], "n_images": bn[1]}) for bn in ((6, 0), (6, -1), (6, 4), (5, 2), (0, 1))]
    if live:
        out += [("null mask", {"mask": None})] if "mask" in names else []
        out += [("live N=300", {"Nq": 300, "Nk": 300}), ("live N=50", {}), ("null eot and D=0", {"eot": None, "D": 0})]
    if entry == "mmx_attn_fwd_live":
        out += [("Nq != Nk", {"Nq": 49}), ("Nq != Nk and null q", {"Nq": 49, "q": None})]
    if "slab_dtype" in names and not row:
        out += [("slab dtype 3 and Nk=0", {"slab_dtype": 3, "Nk": 0}), ("slab dtype 3 and H=65536", {"slab_dtype": 3, "H": 65536}),
                ("null probs and slab dtype 3", {"probs": None, "slab_dtype": 3})]
    if not bwd:
        out += [("null o and scale_mode=2", {"o": None, "scale_mode": 2}), ("null q and D=0", {"q": None, "D": 0})]
    return out


def table(handle):
    """The lines of the table for a loaded library (``_lib.lib()`` or ``load()``)."""
    lines = []
    for entry, names in ENTRIES.items():
        for case, over in cases(handle, entry):
            vals = dict(valid(entry), **over)
            rc = getattr(handle, entry)(*[vals[n] for n in names])
            lines.append("%s | %s | %d | %s" % (entry, case, rc, handle.mmx_last_error().decode("utf-8", "replace") if rc else ""))
    return lines


def load(path):
    from transformer_mm_explainability_amd import _lib
    handle = C.CDLL(path)
    for name, (res, args) in _lib._PROTOTYPES.items():
        if name in ENTRIES or name.endswith("_workspace_bytes") or name == "mmx_last_error":
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
    return handle


def main():
    from transformer_mm_explainability_amd import _lib
    print("\n".join(table(load(os.environ.get("MMX_LIB_PATH") or _lib.LIB_PATH))))


if __name__ == "__main__":
    main()
