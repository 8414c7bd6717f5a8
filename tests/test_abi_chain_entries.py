"""CPU: the relevancy chain's four entries, ``mmx_self_chain_workspace_bytes`` and ``mmx_set_option`` answer what they answered before
the chain's dispatcher, its entry checks and the option table were rebuilt -- same rc, same text, same order of checks, same bytes.
``profiles/chain_entry_table.txt`` is the output of ``tools/chain_entry_table.py`` for the library of the commit before that change;
the tree's library must reproduce it byte for byte.  The tool changes global options: it runs in a process of its own."""
import os
import subprocess
import sys

import pytest
import torch

from tools import chain_entry_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "profiles", "chain_entry_table.txt")

# the addresses are made up: the full calls of the table must never reach a device (without one they fail at their first HIP call)
pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only where no GPU is visible")


@pytest.fixture(scope="module")
def lib_path():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib.LIB_PATH


def test_chain_entry_table_is_the_pinned_one(lib_path):
    with open(TABLE) as f:
        want = f.read()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "chain_entry_table.py")], capture_output=True, text=True,
                       env=dict(os.environ, MMX_LIB_PATH=lib_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.splitlines() == want.splitlines()      # (the differing lines, readably)
    assert r.stdout == want


def test_pinned_table_covers_every_section():
    with open(TABLE) as f:
        rows = [line.split(" | ", 3) for line in f.read().splitlines()]
    assert all(len(r) == 4 for r in rows)
    by = {s: [r for r in rows if r[0] == s] for s in ("workspace", "refusal", "call", "option")}
    assert sum(map(len, by.values())) == len(rows)
    assert len(by["workspace"]) == 6 * 5 * 2 * 10 * 2
    assert {r[1].split(":")[0] for r in by["refusal"]} == set(chain_entry_table.ENTRIES)
    assert all(int(r[2]) in (-22, -105) and r[3] for r in by["refusal"])                       # MMX_EINVAL, MMX_EWORKSPACE
    assert len(by["call"]) == len(chain_entry_table.CALLS) and all(int(r[2]) == -1100 and r[3] for r in by["call"])
    assert len(by["option"]) == (len(chain_entry_table.OPTION_KEYS) + 3) * len(chain_entry_table.OPTION_VALUES)
    assert all((int(r[2]) == 0) == (r[3] == "") for r in by["option"])                          # a text only with a refusal
