"""CPU: ``csrc/entry_checks.h`` -- ``align256``, ``ranges_overlap`` and ``spans_alias``, the alias test of every entry that takes a
workspace or a pointer table -- compiled alone for the host and checked exhaustively on small ranges by
``tools/host/entry_checks_main.cpp`` (every pair against the byte sets, every list of up to 3 outputs and 2 inputs against the pairwise
definition, the edge cases by hand)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_checks_header_on_the_host():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_entry_checks.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "entry_checks: ok" in r.stdout, r.stdout
