"""ISA read of the exact-fp32 row-relevancy kernels against the same kernels without the row.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 --offload-device-only -S csrc/attention_head.hip -o head.s   (same for attention_stream)
    python tools/isa_rowrel.py head.s stream.s

Per kernel: VGPRs / AGPRs, scratch bytes, MFMAs, and the `s_waitcnt vmcnt` waits between the first and the last MFMA of the body
(the main loop's MFMA region).  The row must add neither scratch nor waits there.

    python tools/isa_rowrel.py --parent old_head.s old_stream.s -- head.s stream.s

compares every kernel of the parent build with the same instantiation here (a new trailing `false` template flag is the same
kernel), instruction by instruction: identical, or different only in the kernel-argument offsets behind a grown args struct.
"""
import re
import subprocess
import sys

# (template flags <DP, NTK, IOH, REL, GRP> / <DP, DT, MM, REL, IOH, GRP>; GRP = the grouped row mode)
WANT = [("attn_bwd_head_kernel<32, 4, false, ", "head, D<=32, N<=64 (CLIP B/32 N=50 at D=32)"),
        ("attn_bwd_head_kernel<64, 4, false, ", "head, D=64, N=50 (CLIP ViT-B/32)"),
        ("attn_bwd_head_kernel<64, 8, false, ", "head, D=64, N=128"),
        ("attn_bwd_q_stream_kernel<64, 0, false, ", "stream q-side, D=64, fp32 (N=197)")]


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\S+):(?:\s*;.*)?$", text, flags=re.M):
        name = m.group(1)
        end = text.find(".Lfunc_end", m.end())
        body = text[m.end():end]
        meta = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, flags=re.S)
        out[name] = (body, meta.group(1) if meta else "")
    return out


def field(meta, key):
    m = re.search(r"\." + key + r"\s+(\d+)", meta)
    return int(m.group(1)) if m else -1


def describe(body, meta):
    lines = [l.strip() for l in body.splitlines()]
    mf = [i for i, l in enumerate(lines) if l.startswith("v_mfma")]
    waits = sum(1 for l in lines[mf[0]:mf[-1] + 1] if l.startswith("s_waitcnt") and "vmcnt" in l) if mf else 0
    return dict(vgpr=field(meta, "amdhsa_next_free_vgpr"), agpr=field(meta, "amdhsa_accum_offset"),
                scratch=field(meta, "amdhsa_private_segment_fixed_size"), mfma=len(mf), vmcnt_in_mfma_body=waits)


def main(paths):
    ks = {}
    for p in paths:
        ks.update(kernels(p))
    names = {n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip() for n in ks}
    for pat, label in WANT:
        print("== %s" % label)
        for n, dn in sorted(names.items(), key=lambda x: x[1]):
            if pat in dn:
                rel = dn.rstrip(")").split("<", 1)[1].split(">")[0]
                d = describe(*ks[n])
                print("  <%s>  vgpr %d  accum_offset %d  scratch %d B  mfma %d  vmcnt waits between first/last mfma %d"
                      % (rel, d["vgpr"], d["agpr"], d["scratch"], d["mfma"], d["vmcnt_in_mfma_body"]))


def _normalised(body):
    body = re.sub(r";.*", "", body)
    body = re.sub(r"_Z\w+|\.LBB\d+_\d+|\.Ltmp\d+|\.Lfunc_end\d+|\.Lfunc_begin\d+", "L", body)
    return [l.strip() for l in body.splitlines() if l.strip()]


def _kernarg(line):
    """Kernel-argument loads / the implicit-argument pointer / the segment size: offsets masked."""
    if "s[0:1]" in line or line.startswith("s_add_u32 s4, s0,") or "kernarg_size" in line:
        return re.sub(r"0x[0-9a-f]+|\b\d+$", "X", line)
    return line


def compare(parent, here):
    def load(paths):
        ks = {}
        for p in paths:
            ks.update(kernels(p))
        dn = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True).stdout.split("\n")
        return {d: ks[n][0] for n, d in zip(ks, dn)}
    old, new = load(parent), load(here)
    same = moved = other = 0
    for name, body in sorted(old.items()):
        twin = name if name in new else next((n for n in new if n.replace(", false>(", ">(") == name), None)
        a, b = _normalised(body), _normalised(new[twin]) if twin else []
        if a == b:
            same += 1
        elif len(a) == len(b) and all(_kernarg(x) == _kernarg(y) for x, y in zip(a, b)):
            moved += 1
        else:
            other += 1
            print("  differs: %s" % name)
    print("parent kernels %d: identical %d, only kernel-argument offsets moved %d, other differences %d" % (len(old), same, moved, other))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--parent"]:
        cut = sys.argv.index("--")
        compare(sys.argv[2:cut], sys.argv[cut + 1:])
    else:
        main(sys.argv[1:])
