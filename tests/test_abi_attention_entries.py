"""CPU: the 11 launching attention entries refuse what they refused before they were rebuilt on one fill and one run function --
same rc, same text, same order of checks.  ``profiles/attention_entry_refusals.txt`` is the output of ``tools/attention_refusals.py``
for the library of the commit before that change; the tree's library must reproduce it byte for byte."""
import os
import subprocess

import pytest
import torch

from tools import attention_refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "attention_entry_refusals.txt")

# the addresses are made up: a call that slipped past a dropped check must never reach a device (without one it fails at the
# launch and shows up as a differing line)
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only where no GPU is visible")


@pytest.fixture(scope="module")
def lib():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib


def test_refusal_table_is_the_pinned_one(lib):
    with open(TABLE) as f:
        want = f.read()
    got = "\n".join(attention_refusals.table(lib.lib())) + "\n"
    assert got.splitlines() == want.splitlines()      # (the differing lines, readably)
    assert got == want


def test_pinned_table_holds_refusals_only():
    with open(TABLE) as f:
        rows = [line.split(" | ", 3) for line in f.read().splitlines()]
    assert len(rows) > 300 and {r[0] for r in rows} == set(attention_refusals.ENTRIES)
    assert all(len(r) == 4 and int(r[2]) in (-22, -95, -105) and r[3] for r in rows)     # MMX_EINVAL, MMX_ENOTSUP, MMX_EWORKSPACE
