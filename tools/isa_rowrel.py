"""ISA read of the exact-fp32 row-relevancy kernels against the same kernels without the row.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 --offload-device-only -S csrc/attention_head.hip -o head.s   (same for attention_stream)
    python tools/isa_rowrel.py head.s stream.s

Per kernel: VGPRs / AGPRs, scratch bytes, MFMAs, and the `s_waitcnt vmcnt` waits between the first and the last MFMA of the body
(the main loop's MFMA region).  The row must add neither scratch nor waits there.
"""
import re
import subprocess
import sys

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


if __name__ == "__main__":
    main(sys.argv[1:])
