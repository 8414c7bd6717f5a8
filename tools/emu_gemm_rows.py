#!/usr/bin/env python3
"""Host emulation of ``gemm_rows_f32_kernel`` and ``gemm_rows_f16_kernel``: compiles ``tools/host/gemm_rows_emu.cpp``, which includes
``csrc/gemm_rows_core.h`` and the two ``.hip`` files as they ship (``MMX_GEMM_ROWS_EMU`` leaves out their launches and C entries), for the
CPU (clang++, C++20) and runs the slab-count and row-list edge cases of ``tests/test_gpu_gemm_rows_pipeline.py`` (fp32: three tiles) and of
``tests/test_gpu_gemm_rows_half.py`` (fp16: both tiles) through all three epilogues.  ``--cxxflag FLAG`` (repeatable) adds a compiler
flag: with the host compiler's thread sanitizer switched on, the run reports any LDS access that no barrier of the kernels orders.  No GPU.
``python tools/emu_gemm_rows.py [--cxx PATH] [--cxxflag FLAG ...]``"""
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
        exe = os.path.join(tmp, "gemm_rows_emu")
        cmd = [args.cxx, "-std=c++20", "-O1", "-g", "-pthread", "-x", "c++", "-I", CSRC,
               os.path.join(ROOT, "tools", "host", "gemm_rows_emu.cpp"), "-o", exe]
        cmd[1:1] = args.cxxflag
        subprocess.run(cmd, check=True)
        return subprocess.run([exe]).returncode


if __name__ == "__main__":
    sys.exit(main())
