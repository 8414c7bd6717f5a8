"""-m gpu: ``mmx_lxmert_perturb_text`` at op level, inputs and outputs on raw buffers between NaN-filled guard bands
(``tests/guard_arena.py``), against a plain-Python restatement of the reference's loop (lxmert/lxmert/perturbation.py:160-178: the scores
of the words 1 .. n - 2, ``topk`` of ONE stable descending order, [CLS] and [SEP] added back, sorted, gathered) computed per question on
the host.  The restatement ranks the words only, so a real ``-inf`` word score is a legal input (``text_keep_batches``, which pushes
every non-word to ``-inf``, is no referee for such rows).  The outputs are copies and integers: every comparison is bitwise, over EVERY
element of every buffer -- zeros behind the kept tokens, elements between the sequences (still NaN) and the guard bands included.
Lengths outside 2 .. T give the result of the clamped length; a width below a sequence's length truncates it and ``new_len`` still
reports the full length; row b's outputs do not depend on B or the other rows; two calls give the same bits."""
import ctypes as C
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guard_arena import Arena, ptr as _ptr  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS = [2, 3, 4, 12, 20, 63, 64, 65, 130, 256]
STANDARD = (0, 0.25, 0.5, 0.75, 0.8, 0.85, 0.9, 0.95, 1)
STEP_LISTS = (STANDARD, (0.5,), tuple(i / 63 for i in range(64)))
CAMS = ("rand", "three", "const", "special")
LENGTHS = ("ragged", "full", "two", "three", "oob")
PLACEMENTS = ("one", "two", "each")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lens(kind, B, T):
    if kind == "oob":
        return [(0, -5, T + 7, 1, T)[b % 5] for b in range(B)]
    if kind == "ragged":
        return [(T, 2, min(3, T), (T + 3) // 2, max(T - 1, 2))[b % 5] for b in range(B)]
    return [{"full": T, "two": 2, "three": min(3, T)}[kind]] * B


def _clamped(lens, T):
    return [min(max(n, 2), T) for n in lens]


def _cam(kind, B, T, g):
    if kind == "const":
        return torch.full((B, T), 0.25)
    if kind == "three":
        return torch.randint(0, 3, (B, T), generator=g).to(torch.float32) / 2
    cam = torch.randn(B, T, generator=g)
    if kind == "special":                                            # +-0, NaN, +-inf among ordinary scores, also outside the words
        pick = torch.randint(0, 8, (B, T), generator=g)
        for code, value in enumerate((0.0, -0.0, float("nan"), float("inf"), float("-inf"))):
            cam = torch.where(pick == code, torch.full_like(cam, value), cam)
    return cam


def _bounds(steps, T):
    return [2 + int((1 - step) * (T - 2)) for step in steps]


def _placement(kind, steps, B, T):
    """-> (rows of (base, stride, width), out_elems); no element is covered twice ("two" may leave a few uncovered between its blocks)."""
    S = len(steps)
    if kind == "one":                                                # one group at width T, the steps of a sample adjacent
        return [(s * T, S * T, T) for s in range(S)], B * S * T
    if kind == "two":                                                # the evaluator's two-group split
        from transformer_mm_explainability_amd import lxmert_perturbation as lp
        plan = lp.LxmertPerturbation(None, steps=steps).text_step_groups(T, 2)
        where = plan.layout(B)
        table = list(where.table)
        return [tuple(table[3 * s:3 * s + 3]) for s in range(S)], where.elems
    rows, at = [], 0                                                 # every step its own group at its own bound
    for width in _bounds(steps, T):
        rows.append((at, width, width))
        at += B * width
    return rows, at


def _descending(scores):
    """Indices in ONE stable descending order: NaN first, then by value (+0.0 == -0.0), lower index first among equals."""
    return sorted(range(len(scores)), key=lambda i: (0, 0.0) if math.isnan(scores[i]) else (1, -scores[i]))


def kept_positions(cam_row, n, steps, positive):
    """perturbation.py:160-178 for one question of n tokens -> the kept positions of every step."""
    pure = [-x if positive else x for x in cam_row[1:n - 1]]        # :163 (the reference hands over -cam for the positive test)
    order = _descending(pure)
    out = []
    for step in steps:
        top = order[:int((1 - step) * len(pure))]                    # :166-167
        out.append(sorted([0, n - 1] + [i + 1 for i in top]))        # :171-174
    return out


def reference(ids, types, cam, lens, steps, positive, place, blank):
    """-> (ids, types [out_elems] int64, mask [out_elems] fp32 as int32 bits, new_len [S, B], ranks [B, T]); ``blank``: what an element
    that no sequence covers holds (the arena's NaN fill)."""
    B, T = ids.shape
    S = len(steps)
    o_ids, o_types, o_mask = blank[0].clone(), blank[1].clone(), blank[2].clone()
    new_len = torch.zeros(S, B, dtype=torch.int64)
    ranks = torch.full((B, T), -1, dtype=torch.int32)
    ids_l, types_l, cam_l = ids.tolist(), types.tolist(), cam.tolist()
    differ = True
    for b, n in enumerate(_clamped(lens, T)):
        kept = kept_positions(cam_l[b], n, steps, positive)
        pure = [-x if positive else x for x in cam_l[b][1:n - 1]]
        for r, i in enumerate(_descending(pure)):
            ranks[b, i + 1] = r
        if n - 2 >= 2 and S > 1:
            differ = differ and len({tuple(k) for k in kept}) >= 2
        for s, (base, stride, width) in enumerate(place):
            at, k = base + b * stride, kept[s][:width]
            o_ids[at:at + width] = torch.tensor([ids_l[b][p] for p in k] + [0] * (width - len(k)), dtype=torch.int64)
            o_types[at:at + width] = torch.tensor([types_l[b][p] for p in k] + [0] * (width - len(k)), dtype=torch.int64)
            o_mask[at:at + width] = torch.tensor([1.0] * len(k) + [0.0] * (width - len(k))).view(torch.int32)
            new_len[s, b] = len(kept[s])
    assert differ, "a multi-word question whose steps all keep the same tokens: the case checks nothing"
    return o_ids, o_types, o_mask, new_len, ranks


class Call:
    """One shape's operands inside an input arena, and the C entry on an output arena of its own per call."""

    def __init__(self, ids, types, B, T):
        self.B, self.T = B, T
        self.in_sizes = [2 * B * T, 2 * B * T, B * T, B, 64 * max(T - 1, 1)]
        self.inputs = Arena(self.in_sizes)
        self.inputs.region(0).view(torch.int64).copy_(ids.reshape(-1))
        self.inputs.region(1).view(torch.int64).copy_(types.reshape(-1))

    def run(self, cam, lens, steps, positive, place, out_elems, want_ranks=True):
        from transformer_mm_explainability_amd import _lib
        B, T, S = self.B, self.T, len(steps)
        counts = torch.tensor([[int((1 - step) * w) for w in range(T - 1)] for step in steps], dtype=torch.int32).reshape(-1)
        self.inputs.region(2).copy_(cam.reshape(-1))
        self.inputs.region(3).view(torch.int32).copy_(torch.tensor(lens, dtype=torch.int32))
        self.inputs.region(4).view(torch.int32)[:counts.numel()].copy_(counts)
        before = self.inputs.buf.view(torch.int32).clone()
        sizes = [2 * out_elems, 2 * out_elems, out_elems, 2 * S * B, B * T]
        arena = Arena(sizes)
        blank = tuple(arena.region(i).view(dt).cpu() for i, dt in ((0, torch.int64), (1, torch.int64), (2, torch.int32)))
        table = (C.c_int64 * (3 * S))(*[int(v) for row in place for v in row])
        rc = _lib.lib().mmx_lxmert_perturb_text(
            *(_ptr(self.inputs.region(i)) for i in range(5)), table, *(_ptr(arena.region(i)) for i in range(4)),
            _ptr(arena.region(4)) if want_ranks else None, out_elems, B, T, S, int(positive), _stream())
        _lib.check(rc, "mmx_lxmert_perturb_text")
        torch.cuda.synchronize()
        arena.assert_guards_untouched(sizes if want_ranks else sizes[:4] + [0])
        assert torch.equal(self.inputs.buf.view(torch.int32), before), "an input was written"
        got = (arena.region(0).view(torch.int64).cpu(), arena.region(1).view(torch.int64).cpu(), arena.region(2).view(torch.int32).cpu(),
               arena.region(3).view(torch.int64).reshape(S, B).cpu(), arena.region(4).view(torch.int32).reshape(B, T).cpu())
        return got, blank


def _assert_all_equal(got, want, label):
    for name, a, b in zip(("ids", "types", "mask", "new_len", "ranks"), got, want):
        assert a.dtype == b.dtype and torch.equal(a, b), "%s: %s differs" % (label, name)


def _combos():
    out = [(cam, "ragged", pos, steps, PLACEMENTS[(ci + pi + si) % 3]) for ci, cam in enumerate(CAMS) for pi, pos in enumerate((False, True))
           for si, steps in enumerate(STEP_LISTS)]
    return out + [("rand", lens, pos, STANDARD, PLACEMENTS[(li + pi) % 3]) for li, lens in enumerate(LENGTHS[1:])
                  for pi, pos in enumerate((False, True))]


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("T", WIDTHS)
def test_perturb_text_equals_the_restated_loop(T, B):
    from transformer_mm_explainability_amd import ops
    g = torch.Generator().manual_seed(3000 * T + B)
    ids, types = torch.randint(1, 30000, (B, T), generator=g), torch.randint(0, 2, (B, T), generator=g)
    call = Call(ids, types, B, T)
    for n_case, (cam_kind, lens_kind, positive, steps, place_kind) in enumerate(_combos()):
        label = "T=%d B=%d %s %s positive=%s S=%d placement=%s" % (T, B, cam_kind, lens_kind, positive, len(steps), place_kind)
        cam, lens = _cam(cam_kind, B, T, g), _lens(lens_kind, B, T)
        place, out_elems = _placement(place_kind, steps, B, T)
        got, blank = call.run(cam, lens, steps, positive, place, out_elems)
        want = reference(ids, types, cam, lens, steps, positive, place, blank)
        _assert_all_equal(got, want, label)
        assert bool((got[3] <= torch.tensor([w for _, _, w in place]).unsqueeze(1)).all()), label + ": a width was too small"
        if lens_kind == "oob":                                       # == the clamped lengths, bit for bit
            _assert_all_equal(call.run(cam, _clamped(lens, T), steps, positive, place, out_elems)[0], got, label + " clamped")
        if n_case % 8 == 0:                                          # two calls give the same bits; ranks are optional
            again = call.run(cam, lens, steps, positive, place, out_elems, want_ranks=False)[0]
            _assert_all_equal(again[:4], got[:4], label + " second call")
    # the wrapper hands the same operands over: same bits, with and without the ranks
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    counts = torch.tensor([[int((1 - step) * w) for w in range(T - 1)] for step in steps], dtype=torch.int32, device="cuda")
    args = (ids.cuda(), types.cuda(), cam.cuda(), lens_d, counts, place, out_elems, positive)
    covered = torch.zeros(out_elems, dtype=torch.bool)               # (the wrapper's buffers are torch.empty: elements that no
    for base, stride, width in place:                                # sequence covers hold whatever was there)
        for b in range(B):
            covered[base + b * stride:base + b * stride + width] = True
    for want_ranks in (True, False):
        via = ops.lxmert_perturb_text(*args[:5], place if want_ranks else ops.text_placement(place), *args[6:], want_ranks=want_ranks)
        assert len(via) == (5 if want_ranks else 4) and via[2].dtype == torch.float32
        for k in range(3):
            mine = via[k].cpu() if k != 2 else via[k].view(torch.int32).cpu()
            assert mine.dtype == got[k].dtype and torch.equal(mine[covered], got[k][covered]), "ops: output %d differs" % k
        assert torch.equal(via[3].cpu(), got[3]) and (not want_ranks or torch.equal(via[4].cpu(), got[4]))


@pytest.mark.parametrize("T", [4, 20, 65])
def test_a_narrow_width_truncates_and_reports_the_full_length(T):
    """Widths BELOW the bound, sequences apart (stride > width, a base that is no multiple of anything): the sequence is cut at its
    width, ``new_len`` is the untruncated length, and the elements between the sequences are never written."""
    B, g = 5, torch.Generator().manual_seed(17 * T)
    ids, types = torch.randint(1, 30000, (B, T), generator=g), torch.randint(0, 2, (B, T), generator=g)
    cam, lens = torch.randn(B, T, generator=g), _lens("ragged", B, T)
    place, at = [], 5
    for s, bound in enumerate(_bounds(STANDARD, T)):
        width = max(1, bound - 1 - s % 3)
        place.append((at, width + 3, width))
        at += B * (width + 3) + s
    got, blank = Call(ids, types, B, T).run(cam, lens, STANDARD, True, place, at)
    want = reference(ids, types, cam, lens, STANDARD, True, place, blank)
    _assert_all_equal(got, want, "T=%d truncated" % T)
    widths = torch.tensor([w for _, _, w in place]).unsqueeze(1)
    assert bool((got[3] > widths).any()), "no sequence was truncated: the case checks nothing"
    assert torch.equal(got[3][:, 0], torch.tensor(_bounds(STANDARD, T)))          # row 0 is a question of T tokens: the bound itself


@pytest.mark.parametrize("T", [12, 130])
def test_a_row_does_not_depend_on_the_batch_around_it(T):
    g = torch.Generator().manual_seed(23 * T)
    B = 5
    ids, types = torch.randint(1, 30000, (B, T), generator=g), torch.randint(0, 2, (B, T), generator=g)
    cam, lens = _cam("three", B, T, g), _lens("ragged", B, T)
    place, out_elems = _placement("each", STANDARD, B, T)
    first = Call(ids, types, B, T).run(cam, lens, STANDARD, False, place, out_elems)[0]
    for b in (1, 3):
        # the same question among other rows, at another batch position
        ids2, types2 = torch.randint(1, 30000, (B, T), generator=g), 1 - types
        cam2, lens2 = torch.randn(B, T, generator=g), [T] * B
        ids2[4 - b], types2[4 - b], cam2[4 - b], lens2[4 - b] = ids[b], types[b], cam[b], lens[b]
        second = Call(ids2, types2, B, T).run(cam2, lens2, STANDARD, False, place, out_elems)[0]
        # ... and alone
        place1, elems1 = _placement("each", STANDARD, 1, T)
        alone = Call(ids[b:b + 1], types[b:b + 1], 1, T).run(cam[b:b + 1], lens[b:b + 1], STANDARD, False, place1, elems1)[0]
        for s, (base, stride, width) in enumerate(place):
            mine, theirs, single = base + b * stride, base + (4 - b) * stride, place1[s][0]
            for k in range(3):
                assert torch.equal(first[k][mine:mine + width], second[k][theirs:theirs + width])
                assert torch.equal(first[k][mine:mine + width], alone[k][single:single + width])
        assert torch.equal(first[3][:, b], second[3][:, 4 - b]) and torch.equal(first[3][:, b], alone[3][:, 0])
        assert torch.equal(first[4][b], second[4][4 - b]) and torch.equal(first[4][b], alone[4][0])
