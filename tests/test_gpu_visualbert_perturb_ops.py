"""-m gpu: ``mmx_selfattn_perturb_regions`` and ``mmx_selfattn_perturb_text`` at op level, on raw buffers between NaN-filled guard bands
(``tests/guard_arena.py``), against a torch restatement of the reference's loop (VisualBERT/mmf/trainers/core/evaluation_loop.py:100-159:
one ranking per item, ``topk`` of the stable descending order, physical gathers) computed on the host.  The outputs are copies and
integers: every comparison is ``torch.equal``.  Lengths outside 3 .. T give the result of the clamped length and touch no guard band;
``ranks`` equals ``ops.patch_ranks``; row b's outputs do not depend on the other rows of the batch."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guard_arena import Arena, ptr as _ptr  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 1, 4), (8, 5, 6), (16, 14, 96), (24, 100, 768), (24, 232, 8)]         # (T, V, E); E = 6: the one-float path
IMAGE_STEPS = (0, 0.5, 0.75, 0.95, 0.96, 0.97, 0.98, 0.99, 1)
TEXT_STEPS = (0, 0.25, 0.5, 0.75, 0.8, 0.85, 0.9, 0.95, 1)
STEP_LISTS = (IMAGE_STEPS, TEXT_STEPS, (0.5,))
SCORES = ("rand", "equal", "zeros", "nan")
LENGTHS = ("ragged", "min", "one_word", "full", "oob")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lens(kind, B, T):
    if kind == "oob":
        return [(0, 1, 2, T + 5, -7)[b % 5] for b in range(B)]
    if kind == "ragged":
        return [(T, 3, min(4, T), (T + 3) // 2, max(T - 1, 3))[b % 5] for b in range(B)]
    return [{"min": 3, "one_word": min(4, T), "full": T}[kind]] * B


def _clamped(lens, T):
    return [min(max(n, 3), T) for n in lens]


def _cam(kind, B, N, g):
    if kind == "equal":
        return torch.full((B, N), 0.5)
    cam = torch.randn(B, N, generator=g)
    if kind == "zeros":                                              # +0.0 == -0.0: ties, the lower index first
        cam = torch.where(torch.rand(B, N, generator=g) < 0.6, torch.zeros(B, N), cam)
        cam[:, ::2] = -cam[:, ::2]
    if kind == "nan":
        cam[:, N - 1] = float("nan")
        cam[:, 1] = float("nan")
    return cam


def _order(scores, positive):
    """evaluation_loop.py:102-103, :113 / :142 with the project's tie policy: ONE stable descending order, every step a prefix of it."""
    return torch.sort(-scores if positive else scores, dim=-1, descending=True, stable=True).indices


def _group_counts(steps, V):
    return sorted({int((1 - step) * V) for step in steps}, reverse=True)


# ---------------------------------------------------------------------------------------------------------------- regions
def regions_reference(emb, cam, lens, counts, T, positive):
    """-> (x [R, E], mask [R], pooled [G, B], ranks [B, V]) on the host (evaluation_loop.py:104-120, all items and groups)."""
    B, N, E = emb.shape
    V = N - T
    n = _clamped(lens, T)
    order = [_order(cam[b, T:], positive) for b in range(B)]
    xs, masks, pooled, row = [], [], torch.zeros(len(counts), B, dtype=torch.int64), 0
    for g, c in enumerate(counts):
        for b in range(B):
            xs.append(torch.cat((emb[b, :T], emb[b, T + order[b][:c]]), dim=0))
            m = torch.zeros(T + c)
            m[n[b]:T] = -10000.0
            masks.append(m)
            pooled[g, b] = row + n[b] - 2
            row += T + c
    ranks = torch.empty(B, V, dtype=torch.int32)
    for b in range(B):
        ranks[b, order[b]] = torch.arange(V, dtype=torch.int32)
    return torch.cat(xs, dim=0), torch.cat(masks), pooled, ranks


def run_regions(emb, cam, lens, counts, T, positive):
    """The C entry on its own output regions between guard bands -> (x, mask, pooled, ranks), copies."""
    from transformer_mm_explainability_amd import _lib
    B, N, E = emb.shape
    V, G = N - T, len(counts)
    R = B * sum(T + c for c in counts)
    arena = Arena([R * E, R, 2 * G * B, B * V])
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    counts_d = torch.tensor(counts, dtype=torch.int32, device="cuda")
    rc = _lib.lib().mmx_selfattn_perturb_regions(_ptr(emb), _ptr(cam), _ptr(lens_d), _ptr(counts_d), _ptr(arena.region(0)),
                                                 _ptr(arena.region(1)), _ptr(arena.region(2)), _ptr(arena.region(3)), B, T, V, E, G, R,
                                                 int(positive), _stream())
    _lib.check(rc, "mmx_selfattn_perturb_regions")
    torch.cuda.synchronize()
    arena.assert_guards_untouched([R * E, R, 2 * G * B, B * V])
    return (arena.region(0).reshape(R, E).clone(), arena.region(1).clone(), arena.region(2).view(torch.int64).reshape(G, B).clone(),
            arena.region(3).view(torch.int32).reshape(B, V).clone())


def _assert_all_equal(got, want, label):
    for name, a, b in zip(("x / ids", "mask / segments", "pooled / mask", "ranks / new_len"), got, want):
        assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), "%s: %s differs" % (label, name)


def _combos():
    out = [(score, "ragged", pos, steps) for score in SCORES for pos in (False, True) for steps in STEP_LISTS]
    return out + [("rand", lens, pos, IMAGE_STEPS) for lens in LENGTHS[1:] for pos in (False, True)]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T,V,E", SHAPES)
def test_perturb_regions_equals_the_restated_gather(T, V, E, B):
    from transformer_mm_explainability_amd import ops
    g = torch.Generator().manual_seed(1000 * T + 10 * V + B)
    emb = torch.randn(B, T + V, E, generator=g)
    emb_d = emb.cuda()
    for score, lens_kind, positive, steps in _combos():
        label = "T=%d V=%d E=%d B=%d %s %s positive=%s S=%d" % (T, V, E, B, score, lens_kind, positive, len(steps))
        cam, lens, counts = _cam(score, B, T + V, g), _lens(lens_kind, B, T), _group_counts(steps, V)
        cam_d = cam.cuda()
        got = run_regions(emb_d, cam_d, lens, counts, T, positive)
        _assert_all_equal(got, regions_reference(emb, cam, lens, counts, T, positive), label)
        region_scores = (-cam_d if positive else cam_d)[:, T:].contiguous()
        assert torch.equal(got[3], ops.patch_ranks(region_scores)), label + ": ranks != ops.patch_ranks"
        if lens_kind == "oob":                                       # == the clamped lengths, bit for bit
            _assert_all_equal(run_regions(emb_d, cam_d, _clamped(lens, T), counts, T, positive), got, label + " clamped")
    # the wrapper hands the same operands over: same bits, with and without the ranks
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    counts_d = torch.tensor(counts, dtype=torch.int32, device="cuda")
    rows = B * sum(T + c for c in counts)
    _assert_all_equal(ops.selfattn_perturb_regions(emb_d, cam_d, lens_d, counts_d, rows, T, positive, want_ranks=True), got, "ops")
    _assert_all_equal(ops.selfattn_perturb_regions(emb_d, cam_d, lens_d, counts_d, rows, T, positive), got[:3], "ops, no ranks")


@pytest.mark.parametrize("T,V,E", [(8, 5, 6), (24, 100, 768)])
def test_perturb_regions_row_does_not_depend_on_the_other_rows(T, V, E):
    B, g = 5, torch.Generator().manual_seed(7 * T + V)
    counts = _group_counts(IMAGE_STEPS, V)
    emb, cam, lens = torch.randn(B, T + V, E, generator=g), torch.randn(B, T + V, generator=g), _lens("ragged", B, T)
    first = run_regions(emb.cuda(), cam.cuda(), lens, counts, T, False)
    for b in (0, 3):
        emb2, cam2 = torch.randn(B, T + V, E, generator=g), torch.randn(B, T + V, generator=g)
        lens2 = [3] * B
        emb2[b], cam2[b], lens2[b] = emb[b], cam[b], lens[b]
        second = run_regions(emb2.cuda(), cam2.cuda(), lens2, counts, T, False)
        row = 0
        for gi, c in enumerate(counts):
            mine = slice(row + b * (T + c), row + (b + 1) * (T + c))
            assert torch.equal(first[0][mine], second[0][mine]) and torch.equal(first[1][mine], second[1][mine])
            row += B * (T + c)
        assert torch.equal(first[2][:, b], second[2][:, b]) and torch.equal(first[3][b], second[3][b])


# ---------------------------------------------------------------------------------------------------------------- text
def text_reference(ids, seg, cam, lens, steps, positive):
    """-> (ids, segments, mask [S, B, T], new_len [S, B]) on the host (evaluation_loop.py:129-159 for every item and step)."""
    B, T = ids.shape
    S, n = len(steps), _clamped(lens, T)
    out = [torch.zeros(S, B, T, dtype=torch.int64) for _ in range(3)]
    new_len = torch.zeros(S, B, dtype=torch.int64)
    for b in range(B):
        cls_index = n[b] - 2
        text_scores = cam[b, 1:cls_index]
        order = _order(text_scores, positive)
        for s, step in enumerate(steps):
            top = order[:int((1 - step) * text_scores.shape[0])].tolist()
            kept = sorted([0, cls_index, cls_index + 1] + [i + 1 for i in top])
            out[0][s, b, :len(kept)] = ids[b, kept]
            out[1][s, b, :len(kept)] = seg[b, kept]
            out[2][s, b, :len(kept)] = 1
            new_len[s, b] = len(kept)
    return out[0], out[1], out[2], new_len


def _text_counts(steps, T):
    return torch.tensor([[int((1 - step) * w) for w in range(T)] for step in steps], dtype=torch.int32, device="cuda")


def run_text(ids, seg, cam, lens, steps, positive):
    from transformer_mm_explainability_amd import _lib
    B, T = ids.shape
    V, S = cam.shape[1] - T, len(steps)
    sizes = [2 * S * B * T] * 3 + [2 * S * B]
    arena = Arena(sizes)
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    rc = _lib.lib().mmx_selfattn_perturb_text(_ptr(ids), _ptr(seg), _ptr(cam), _ptr(lens_d), _ptr(_text_counts(steps, T)),
                                              _ptr(arena.region(0)), _ptr(arena.region(1)), _ptr(arena.region(2)), _ptr(arena.region(3)),
                                              B, T, V, S, int(positive), _stream())
    _lib.check(rc, "mmx_selfattn_perturb_text")
    torch.cuda.synchronize()
    arena.assert_guards_untouched(sizes)
    return tuple(arena.region(i).view(torch.int64).reshape((S, B, T) if i < 3 else (S, B)).clone() for i in range(4))


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T,V,E", SHAPES)
def test_perturb_text_equals_the_restated_gather(T, V, E, B):
    from transformer_mm_explainability_amd import ops
    g = torch.Generator().manual_seed(2000 * T + 10 * V + B)
    ids = torch.randint(1, 30000, (B, T), generator=g)
    seg = torch.randint(0, 2, (B, T), generator=g)
    ids_d, seg_d = ids.cuda(), seg.cuda()
    for score, lens_kind, positive, steps in _combos():
        label = "T=%d V=%d B=%d %s %s positive=%s S=%d" % (T, V, B, score, lens_kind, positive, len(steps))
        cam, lens = _cam(score, B, T + V, g), _lens(lens_kind, B, T)
        cam_d = cam.cuda()
        got = run_text(ids_d, seg_d, cam_d, lens, steps, positive)
        _assert_all_equal(got, text_reference(ids, seg, cam, lens, steps, positive), label)
        assert torch.equal(got[3], got[2].sum(dim=-1)), label + ": new_len != number of kept positions"
        if lens_kind == "oob":
            _assert_all_equal(run_text(ids_d, seg_d, cam_d, _clamped(lens, T), steps, positive), got, label + " clamped")
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    _assert_all_equal(ops.selfattn_perturb_text(ids_d, seg_d, cam_d, lens_d, _text_counts(steps, T), positive), got, "ops")


def test_perturb_text_row_does_not_depend_on_the_other_rows():
    T, V, B, g = 24, 100, 5, torch.Generator().manual_seed(11)
    ids, seg = torch.randint(1, 30000, (B, T), generator=g), torch.randint(0, 2, (B, T), generator=g)
    cam, lens = torch.randn(B, T + V, generator=g), _lens("ragged", B, T)
    first = run_text(ids.cuda(), seg.cuda(), cam.cuda(), lens, TEXT_STEPS, True)
    for b in (1, 4):
        ids2, cam2, lens2 = torch.randint(1, 30000, (B, T), generator=g), torch.randn(B, T + V, generator=g), [T] * B
        ids2[b], cam2[b], lens2[b] = ids[b], cam[b], lens[b]
        seg2 = 1 - seg
        seg2[b] = seg[b]
        second = run_text(ids2.cuda(), seg2.cuda(), cam2.cuda(), lens2, TEXT_STEPS, True)
        for a, c in zip(first, second):
            assert torch.equal(a[:, b], c[:, b])
