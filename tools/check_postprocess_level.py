#!/usr/bin/env python3
"""Host check of ``csrc/postprocess_level.h`` (``otsu_level``, the size limits of the two post-processing entries): compiles
``tools/host/postprocess_level_main.cpp``, which includes nothing but that header, with a plain host compiler (clang++, C++17) and runs
it: the level of a pixel against the bare cast it replaced wherever that cast is defined, and against the stated answer for NaN, infinite
and out-of-range values, where it is not.  ``--cxxflag FLAG`` (repeatable) adds a compiler flag, e.g. the host compiler's
undefined-behaviour sanitizer (``-fsanitize=float-cast-overflow``), under which the bare cast is reported and the helper is not.  No GPU.
Returns the program's exit status.
``python tools/check_postprocess_level.py [--cxx PATH] [--cxxflag FLAG ...]``"""
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
        exe = os.path.join(tmp, "postprocess_level_main")
        cmd = [args.cxx, "-std=c++17", "-O1", "-g", "-Wall", "-x", "c++", "-I", CSRC,
               os.path.join(ROOT, "tools", "host", "postprocess_level_main.cpp"), "-o", exe]
        cmd[1:1] = args.cxxflag
        subprocess.run(cmd, check=True)
        return subprocess.run([exe], timeout=60).returncode     # an undefined conversion may do anything, looping included


if __name__ == "__main__":
    sys.exit(main())
