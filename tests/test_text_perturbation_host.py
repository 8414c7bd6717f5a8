"""CPU: the host side of the caption perturbation test (``clip_text_perturbation.token_step_counts``) and the rule of
``mmx_perturb_tokens`` -- its plain-loop restatement (``text_perturbation_cases.restate``, what the GPU suite compares the kernel
with) equals the project's torch statement of the reference's text test, ``lxmert_perturbation.text_keep_batches``."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_perturbation_cases as cases  # noqa: E402


def test_token_step_counts_are_the_reference_arithmetic():
    from transformer_mm_explainability_amd.clip_text_perturbation import token_step_counts
    from transformer_mm_explainability_amd.lxmert_perturbation import PERT_STEPS
    table = token_step_counts(PERT_STEPS, 77)
    assert len(table) == len(PERT_STEPS) and all(len(row) == 76 for row in table)
    for s, step in enumerate(PERT_STEPS):
        for w in range(76):
            assert table[s][w] == int((1 - step) * w)
    assert token_step_counts((0,), 2) == [[0]]
    with pytest.raises(ValueError):
        token_step_counts(PERT_STEPS, 1)


@pytest.mark.parametrize("which", ["tiny", "ctx77"])
@pytest.mark.parametrize("positive", [False, True])
def test_restatement_equals_text_keep_batches(golden, which, positive):
    from transformer_mm_explainability_amd.clip_text_perturbation import token_step_counts
    from transformer_mm_explainability_amd.lxmert_perturbation import PERT_STEPS, text_keep_batches
    if which == "tiny":
        _, cam, texts = cases.evaluator_inputs(cases.tiny_cfg(golden), cases.TINY_LENGTHS, 23, 24)
    else:
        _, cam, texts = cases.evaluator_inputs(cases.CTX77_CFG, cases.CTX77_LENGTHS, 29, 30)
    B, N = texts.shape
    S = len(PERT_STEPS)
    eot = texts.argmax(dim=-1)
    ids, _, _ = text_keep_batches(texts, torch.zeros_like(texts), cam, PERT_STEPS, positive, n_tokens=(eot + 1).tolist())
    want = ids.view(B, S, N).transpose(0, 1)
    got, got_eot, _ = cases.restate(texts, -cam if positive else cam, token_step_counts(PERT_STEPS, N))
    assert torch.equal(got, want)
    assert torch.equal(got_eot, want.argmax(dim=-1))
    assert torch.equal(got[0], texts)                                    # step 0 removes nothing
    assert bool((got_eot[-1] == 1).all())                                # step 1 leaves [SOT, EOT]
