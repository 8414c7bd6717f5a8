"""CPU: the host arithmetic of the batched VisualBERT perturbation test (``visualbert_perturbation``): the keep counts of the
reference's step lists (``int((1 - step) * n)``, evaluation_loop.py:111 / :140), the groups of steps with one count, where the groups
start in the packed rows, the step -> group scatter, and the batched ``accuracy``."""
import pytest
import torch

from transformer_mm_explainability_amd import visualbert_perturbation as vp


def _counts(V):
    groups, step_group = vp.image_step_groups(vp.IMAGE_STEPS, V)
    return [groups[g] for g in step_group], groups, step_group


def test_image_counts_at_100_regions_are_all_distinct():
    per_step, groups, step_group = _counts(100)
    assert per_step == [100, 50, 25, 5, 4, 3, 2, 1, 0]
    assert groups == per_step and step_group == list(range(9))


def test_image_counts_at_36_regions_make_five_groups():
    per_step, groups, step_group = _counts(36)
    assert per_step == [36, 18, 9, 1, 1, 1, 0, 0, 0]
    assert groups == [36, 18, 9, 1, 0] and step_group == [0, 1, 2, 3, 3, 3, 4, 4, 4]


def test_image_counts_at_14_regions_make_four_groups():
    per_step, groups, step_group = _counts(14)
    assert per_step == [14, 7, 3, 0, 0, 0, 0, 0, 0]
    assert groups == [14, 7, 3, 0] and step_group == [0, 1, 2, 3, 3, 3, 3, 3, 3]


def test_image_counts_at_one_region():
    per_step, groups, step_group = _counts(1)
    assert per_step == [1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert groups == [1, 0] and step_group == [0] + [1] * 8


@pytest.mark.parametrize("V", [1, 2, 5, 14, 36, 100, 232, 253])
def test_groups_are_the_distinct_counts_in_descending_order(V):
    per_step, groups, step_group = _counts(V)
    assert per_step == [int((1 - step) * V) for step in vp.IMAGE_STEPS]
    assert groups == sorted(set(per_step), reverse=True) and all(0 <= c <= V for c in groups)
    assert len(step_group) == len(vp.IMAGE_STEPS) and set(step_group) == set(range(len(groups)))


def test_steps_in_any_order_map_to_their_group():
    groups, step_group = vp.image_step_groups((1, 0, 0.5, 0, 0.5), 10)
    assert groups == [10, 5, 0] and step_group == [2, 0, 1, 0, 1]


def test_group_offsets_pack_b_sequences_per_group():
    offsets, rows = vp.group_offsets([36, 18, 9, 1, 0], T=24, B=32)
    assert offsets == [0, 32 * 60, 32 * (60 + 42), 32 * (60 + 42 + 33), 32 * (60 + 42 + 33 + 25)]
    assert rows == 32 * (5 * 24 + 64)
    assert vp.group_offsets([0], T=3, B=1) == ([0], 3)
    groups, _ = vp.image_step_groups(vp.IMAGE_STEPS, 100)
    assert vp.group_offsets(groups, T=24, B=1)[1] == 9 * 24 + 190          # the rows that carry information


def test_step_to_group_scatter_repeats_the_group_that_computed_a_count():
    """What ``perturbation_image_batch`` does with the ``[G * B, L]`` scores of the packed pass."""
    B, L = 3, 4
    groups, step_group = vp.image_step_groups(vp.IMAGE_STEPS, 36)
    out = torch.arange(len(groups) * B * L, dtype=torch.float32).reshape(len(groups) * B, L)
    scores = out.view(len(groups), B, L).index_select(0, torch.tensor(step_group)).transpose(0, 1)
    assert scores.shape == (B, 9, L)
    for b in range(B):
        for s, g in enumerate(step_group):
            assert torch.equal(scores[b, s], out[g * B + b])
    assert torch.equal(scores[:, 3], scores[:, 5]) and torch.equal(scores[:, 6], scores[:, 8])


def test_text_count_table():
    table = vp.text_step_counts(vp.TEXT_STEPS, 24)
    assert len(table) == 9 and all(len(row) == 24 for row in table)
    assert table[0] == list(range(24)) and table[-1] == [0] * 24
    for s, step in enumerate(vp.TEXT_STEPS):
        assert table[s] == [int((1 - step) * w) for w in range(24)]
    assert [row[9] for row in table] == [9, 6, 4, 2, 1, 1, 0, 0, 0]


def test_accuracy_takes_batched_scores_and_keeps_the_per_item_form():
    g = torch.Generator().manual_seed(1)
    scores, targets = torch.rand(4, 9, 7, generator=g), torch.rand(4, 7, generator=g)
    acc = vp.VisualBertPerturbation.accuracy(scores, targets)
    assert acc.shape == (4, 9)
    for b in range(4):
        one = vp.VisualBertPerturbation.accuracy(scores[b], targets[b])
        assert one.shape == (9,) and torch.equal(one, targets[b][scores[b].argmax(dim=-1)]) and torch.equal(acc[b], one)
