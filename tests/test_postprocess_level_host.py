"""CPU: ``csrc/postprocess_level.h`` -- ``otsu_level``, the one float-to-level conversion of ``otsu_kernel`` -- compiled alone for the host
by ``tools/check_postprocess_level.py`` and run over every level boundary of six maps (the bits of the bare cast it replaced) and over NaN,
infinite and out-of-range values (the stated answers, where the bare cast has no defined one), plain and under the host compiler's
float-cast-overflow check."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["--cxxflag=-fsanitize=float-cast-overflow", "--cxxflag=-fno-sanitize-recover=all"]],
                         ids=["plain", "float-cast-overflow"])
def test_otsu_level_is_the_former_cast_where_that_was_defined_and_the_contract_elsewhere(flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_postprocess_level.py")] + flags, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout, r.stdout
    assert "postprocess_level: ok" in r.stdout, r.stdout
