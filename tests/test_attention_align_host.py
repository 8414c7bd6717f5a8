"""CPU: ``csrc/attention_align.h`` -- ``rows_aligned``, the one alignment test of the attention kernels' eligibility rules -- compiled
alone for the host and compared by ``tools/host/attention_align_main.cpp`` with the expressions it replaced (the five spellings of the
kernel files and the two open-coded tests beside them, as they stood), in the argument form of every call site, over 3072 combinations of
pointer offset and strides per form."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rows_aligned_accepts_what_the_former_expressions_accepted():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_attention_align.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "12 forms x 3072 cases, 0 mismatches" in r.stdout, r.stdout
    assert "attention_align: ok" in r.stdout, r.stdout
