"""CPU: host logic of the image perturbation test (``vit_perturbation.py``): step counts, the area under a curve, argument
checks at construction, and the refusal of CPU tensors by the three ops."""
import pytest
import torch


class _Scorer:
    n_patches, patch_size = 196, 16


def test_step_counts_literal():
    from transformer_mm_explainability_amd import vit_perturbation as vp
    from transformer_mm_explainability_amd.lxmert_perturbation import PERT_STEPS
    assert vp.PERT_STEPS == PERT_STEPS == (0, 0.25, 0.5, 0.75, 0.8, 0.85, 0.9, 0.95, 1)
    # int((1 - step) * P) in double precision: 1 - 0.8 = 0.19999999999999996, 1 - 0.9 = 0.09999999999999998, ...
    assert vp.step_counts(PERT_STEPS, 49) == [49, 36, 24, 12, 9, 7, 4, 2, 0]
    assert vp.step_counts(PERT_STEPS, 196) == [196, 147, 98, 49, 39, 29, 19, 9, 0]
    assert vp.step_counts(PERT_STEPS, 576) == [576, 432, 288, 144, 115, 86, 57, 28, 0]


def test_auc_hand_computed():
    from transformer_mm_explainability_amd import vit_perturbation as vp
    steps = (0, 0.5, 1)
    values = torch.tensor([[1.0, 0.0], [0.5, 2.0], [0.0, 2.0]])          # [S, 2]
    # column 0: (1 + .5) / 2 * .5 + (.5 + 0) / 2 * .5 = .5;  column 1: (0 + 2) / 2 * .5 + (2 + 2) / 2 * .5 = 1.5;  span 1
    assert torch.allclose(vp.auc(values, steps), torch.tensor([0.5, 1.5]))
    # uneven steps and a span that is not 1: trapezoid / (steps[-1] - steps[0])
    v = torch.tensor([2.0, 4.0, 0.0])
    want = ((2 + 4) / 2 * 0.1 + (4 + 0) / 2 * 0.4) / 0.5
    assert torch.allclose(vp.auc(v, (0.25, 0.35, 0.75)), torch.tensor(want))
    with pytest.raises(ValueError):
        vp.auc(values, (0, 1))


def test_bad_mode_and_steps_are_refused_at_construction():
    from transformer_mm_explainability_amd import vit_perturbation as vp
    with pytest.raises(ValueError):
        vp.PatchPerturbation(_Scorer(), mode="blur")
    with pytest.raises(ValueError):
        vp.PatchPerturbation(_Scorer(), steps=(0, 0.5, 0.25, 1))
    with pytest.raises(ValueError):
        vp.PatchPerturbation(_Scorer(), steps=(0, 0.5, 0.5))
    with pytest.raises(ValueError):
        vp.PatchPerturbation(_Scorer(), steps=(0, 0.5, 1.5))
    with pytest.raises(ValueError):
        vp.PatchPerturbation(_Scorer(), steps=())
    p = vp.PatchPerturbation(_Scorer(), steps=(0.1, 0.2, 0.9), mode="drop")
    assert p.counts == [int((1 - s) * 196) for s in (0.1, 0.2, 0.9)]


def test_ops_refuse_cpu_tensors():
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    q = torch.randn(1, 17, 2, 32)
    with pytest.raises(MMXError):
        ops.attn_fwd(q, q, q, 32 ** -0.5)
    with pytest.raises(MMXError):
        ops.patch_ranks(torch.rand(2, 16))
    with pytest.raises(MMXError):
        ops.perturb_patches(torch.randn(2, 3, 32, 32), torch.zeros(2, 16, dtype=torch.int32), torch.tensor([16, 0], dtype=torch.int32),
                            torch.zeros(3))
