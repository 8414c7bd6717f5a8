#!/usr/bin/env python3
"""Host check of ``csrc/attention_align.h`` (``rows_aligned``): compiles ``tools/host/attention_align_main.cpp``, which includes nothing
but that header, with a plain host compiler (clang++, C++17) and runs it: the alignment expressions the attention kernel files held
before they shared one predicate, written out as they stood, against ``rows_aligned`` in the argument form of each call site, over
6 pointer offsets x 8 values of each of the three strides.  ``--cxxflag FLAG`` (repeatable) adds a compiler flag, e.g. the host
compiler's sanitizers for a run by hand.  No GPU.  Returns the program's exit status.
``python tools/check_attention_align.py [--cxx PATH] [--cxxflag FLAG ...]``"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxxflag", action="append", default=[])
    ap.add_argument("--cxx", default=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "attention_align_main")
        cmd = [args.cxx, "-std=c++17", "-O1", "-g", "-Wall", "-x", "c++", "-I", CSRC,
               os.path.join(ROOT, "tools", "host", "attention_align_main.cpp"), "-o", exe]
        cmd[1:1] = args.cxxflag
        subprocess.run(cmd, check=True)
        return subprocess.run([exe]).returncode


if __name__ == "__main__":
    sys.exit(main())
