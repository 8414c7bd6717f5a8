"""-m gpu: a plain ``bench.py`` run, the command every change is measured with -- one JSON line with the contract fields, none of
the ``--full`` measurements, ``--steps`` timed steps, and ``--dump-outputs`` writing the maps of the last timed step: those of
bench.py's seeded model and inputs (checked against an eager ``interpret`` of the same model and inputs in this process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "outputs"
    run = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["n_gpus"] == 1
    assert line["unit"] == "maps/s" and line["dtype"] == "f32" and line["higher_is_better"] is True
    assert abs(line["value"] - 64 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
    assert line["roofline"] is None and line["configs"] is None and line["config"]["variants"] is None
    assert "cpu_baseline" not in line
    assert sorted(os.listdir(out)) == ["R_image.npy", "R_text.npy"]
    R_text, R_image = np.load(out / "R_text.npy"), np.load(out / "R_image.npy")
    assert R_text.dtype == np.float32 and R_text.shape == (64, 77, 77)
    assert R_image.dtype == np.float32 and R_image.shape == (64, 49)

    from test_gpu_parity_fullsize import bench_inputs
    from transformer_mm_explainability_amd import clip_explainability as ce
    from transformer_mm_explainability_amd import clip_model
    model = clip_model.random_init("ViT-B/32", seed=0).cuda()
    image, texts = bench_inputs(64)
    want_text, want_img = ce.interpret(image.cuda(), texts.cuda(), model, "cuda", 0, 0)
    torch.cuda.synchronize()
    # both within 1e-5 of the oracle (test_gpu_parity_fullsize.py); the bench process uses the tuned GEMM selection
    np.testing.assert_allclose(R_text, want_text.cpu().numpy(), rtol=0, atol=2e-5)
    np.testing.assert_allclose(R_image, want_img.cpu().numpy(), rtol=0, atol=2e-5)
