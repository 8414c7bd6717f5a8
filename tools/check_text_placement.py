#!/usr/bin/env python3
"""Host check of ``csrc/text_placement.h`` (``check_text_placement``, the placement table of ``mmx_lxmert_perturb_text``): compiles
``tools/host/text_placement_main.cpp``, which includes nothing of the project but that header, with a plain host compiler (clang++,
C++17) and runs it: every small table of one or two steps (and a sample of three) against the sets of elements its sequences occupy,
and the edge cases by hand.
``--cxxflag FLAG`` (repeatable) adds a compiler flag, e.g. the host compiler's sanitizers for a run by hand.  No GPU.  Returns the
program's exit status.
``python tools/check_text_placement.py [--cxx PATH] [--cxxflag FLAG ...]``"""
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
        exe = os.path.join(tmp, "text_placement_main")
        cmd = [args.cxx, "-std=c++17", "-O1", "-g", "-Wall", "-x", "c++", "-I", CSRC,
               os.path.join(ROOT, "tools", "host", "text_placement_main.cpp"), "-o", exe]
        cmd[1:1] = args.cxxflag
        subprocess.run(cmd, check=True)
        return subprocess.run([exe]).returncode


if __name__ == "__main__":
    sys.exit(main())
