"""CPU: the entry of the LXMERT text perturbation test on device-built step groups (``mmx_lxmert_perturb_text``) is declared, exported,
bound and reachable through ``ops`` and ``LxmertPerturbation``, and refuses bad arguments -- sizes, placement tables, aliases -- with
``MMX_EINVAL`` and a message before any HIP call.  Every call here runs on made-up device addresses and every one of them but the
placement header's own host program is a REFUSAL (the pattern of ``tests/test_abi_visualbert_perturbation.py``).  ``text_step_groups``
is host arithmetic: its row counts, and its widths against the lengths ``text_keep_batches`` produces, for every T = 2 .. 64."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mmx_lxmert_perturb_text"
PTR = 0x7f0000000000            # made-up device addresses: a launch on them would fail differently
STEP = 1 << 28                  # further apart than any operand of the shapes below is long
EINVAL = -22
B0, T0 = 2, 20
# the evaluator's two groups at T = 20 for B = 2: (20, 15, 11 | 6, 5, 4, 3, 2, 2), sample-major inside a group; the second block starts
# at a multiple of its stride (144, not 120): 216 elements, 2 * 96 of them covered
TWO_GROUPS = [(0, 60, 20), (20, 60, 20), (40, 60, 20)] + [(144 + 6 * j, 36, 6) for j in range(6)]


@pytest.fixture(scope="module")
def lib():
    from transformer_mm_explainability_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "transformer-mm-explainability_amd", "csrc"), "-j4"], check=True,
                       capture_output=True)
    return _lib


def _p(i):
    return C.c_void_p(PTR + STEP * i)


def _table(rows):
    return (C.c_int64 * (3 * len(rows)))(*[int(v) for row in rows for v in row])


def _args(place=TWO_GROUPS, out_elems=216, B=B0, T=T0, S=None):
    """ids, types, cam, text_len, counts, place (host), out_ids, out_types, out_mask, new_len, ranks, out_elems, B, T, S, positive, stream"""
    return [_p(0), _p(1), _p(2), _p(3), _p(4), _table(place), _p(6), _p(7), _p(8), _p(9), _p(10), out_elems, B, T,
            len(place) if S is None else S, 1, None]


def _refused(lib, args, word=None):
    handle = lib.lib()
    assert getattr(handle, NAME)(*args) == EINVAL
    msg = handle.mmx_last_error()
    assert msg and (word is None or word in msg), msg
    return msg


def test_symbol_is_declared_exported_bound_and_callable(lib):
    handle = lib.lib()
    assert NAME in lib.header_symbols()
    assert NAME in lib._PROTOTYPES
    assert hasattr(handle, NAME)
    assert handle.mmx_abi_version() == 2
    from transformer_mm_explainability_amd import lxmert_model as lm
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    from transformer_mm_explainability_amd import ops
    assert callable(ops.lxmert_perturb_text) and callable(ops.text_placement)
    for method in ("text_step_groups", "perturbation_text_grouped", "perturbation_text", "accuracy"):
        assert callable(getattr(lp.LxmertPerturbation, method))
    assert callable(lp.GraphedTextPerturbation) and callable(lp.GraphedImagePerturbation)
    assert callable(lm.LxmertForQuestionAnswering.encode_vision)


def test_citation_is_in_the_header():
    with open(os.path.join(ROOT, "include", "mmx_relevancy.h")) as f:
        assert "lxmert/lxmert/perturbation.py:160-178" in f.read()


@pytest.mark.parametrize("missing", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_null_pointers_are_refused(lib, missing):
    args = _args()
    args[missing] = None
    _refused(lib, args, b"null")


def test_the_accepted_table_gets_past_every_check_but_one(lib):
    """The table the other tests vary is itself legal: with it, only another argument's refusal is seen (here: the batch)."""
    msg = _refused(lib, _args(B=0), b"batch")
    assert b"overlap" not in msg and b"width" not in msg


@pytest.mark.parametrize("sizes", [dict(T=1), dict(T=0), dict(T=-3), dict(T=257), dict(S=0), dict(S=-1), dict(S=65), dict(B=0),
                                   dict(B=-2), dict(out_elems=0), dict(out_elems=-5), dict(out_elems=(1 << 40) + 1)])
def test_bad_sizes_are_refused_without_a_gpu(lib, sizes):
    _refused(lib, _args(**sizes))


@pytest.mark.parametrize("row,word", [((0, 60, 0), b"width"), ((0, 60, -1), b"width"), ((0, 60, 21), b"width"), ((0, 19, 20), b"stride"),
                                      ((0, 0, 1), b"stride"), ((0, -60, 20), b"stride"), ((-1, 60, 20), b"base")])
def test_a_bad_placement_row_is_refused(lib, row, word):
    place = list(TWO_GROUPS)
    place[0] = row
    _refused(lib, _args(place=place), word)


def test_a_table_that_overruns_by_one_element_is_refused(lib):
    _refused(lib, _args(out_elems=215), b"ends past")
    place = list(TWO_GROUPS)
    place[8] = (175, 36, 6)
    _refused(lib, _args(place=place), b"ends past")
    _refused(lib, _args(place=[(0, 20, 20)], out_elems=39, B=2), b"ends past")
    _refused(lib, _args(place=[(1 << 62, 1 << 62, 2)], out_elems=1 << 40, B=3), b"ends past")


@pytest.mark.parametrize("place", [
    [(0, 20, 20), (0, 20, 20)],                             # the same block twice
    [(0, 20, 20), (39, 20, 20)],                            # one element into the first step's second sequence
    [(0, 40, 20), (19, 40, 20)],                            # interleaved, windows one element into each other
    [(0, 40, 20), (30, 40, 20)],                            # interleaved, the second window wraps past the period
    [(0, 40, 10), (10, 30, 10)],                            # strides differ and the ranges are not apart
    TWO_GROUPS[:3] + [(119, 36, 6)] + TWO_GROUPS[4:],       # the second group one element into the first
    TWO_GROUPS[:3] + [(145, 36, 6)] + TWO_GROUPS[4:],       # a step one element into its neighbour's window
    TWO_GROUPS[:3] + [(121 + 6 * j, 36, 6) for j in range(6)],      # the second block off its period: disjoint, but a window wraps
])
def test_overlapping_placement_tables_are_refused(lib, place):
    _refused(lib, _args(place=place, out_elems=400), b"overlap")


@pytest.mark.parametrize("place,out_elems", [
    ([(0, 40, 20), (20, 40, 20)], 80),                      # two steps interleaved sample-major: rule (a)
    ([(0, 20, 20), (40, 20, 20)], 80),                      # one block per step: rule (b)
    ([(40, 20, 7), (0, 20, 20)], 80),                       # in any order
    (TWO_GROUPS, 216), (TWO_GROUPS, 217),
])
def test_legal_placement_tables_pass_the_placement_check(lib, place, out_elems):
    """A legal table is refused for ANOTHER reason only (here an aliased output, the last check before the launch)."""
    args = _args(place=place, out_elems=out_elems)
    args[7] = args[6]
    _refused(lib, args, b"alias")


@pytest.mark.parametrize("out", [6, 7, 8, 9, 10])
@pytest.mark.parametrize("inp", [0, 1, 2, 3, 4])
def test_output_aliasing_an_input_is_refused(lib, out, inp):
    args = _args()
    args[out] = args[inp]
    _refused(lib, args, b"alias")


def test_outputs_overlapping_each_other_or_an_input_tail_are_refused(lib):
    args = _args()
    args[7] = C.c_void_p(PTR + STEP * 6 + 8 * (216 - 1))            # out_types on out_ids' last element
    _refused(lib, args, b"alias")
    args = _args()
    args[8] = C.c_void_p(PTR + STEP * 2 + 4 * (B0 * T0 - 1))        # out_mask on cam's last float
    _refused(lib, args, b"alias")
    args = _args()
    args[10] = C.c_void_p(PTR + STEP * 9 + 8 * (9 * B0 - 1))        # ranks on new_len's last element
    _refused(lib, args, b"alias")
    args = _args()
    args[10] = None                                                 # ranks is optional: still the OTHER refusal only
    args[9] = args[6]
    _refused(lib, args, b"alias")


def test_ops_refuse_host_tensors_and_wrong_operands():
    import torch
    from transformer_mm_explainability_amd import ops
    from transformer_mm_explainability_amd._lib import MMXError
    B, T = 2, 6
    ids, cam = torch.ones(B, T, dtype=torch.int64), torch.rand(B, T)
    lens, counts = torch.full((B,), T, dtype=torch.int32), torch.zeros(9, T - 1, dtype=torch.int32)
    place = [(s * B * T, T, T) for s in range(9)]
    with pytest.raises(MMXError, match="no CPU path"):
        ops.lxmert_perturb_text(ids, ids, cam, lens, counts, place, 9 * B * T)
    with pytest.raises(MMXError, match="rows of"):
        ops.text_placement([(0, 1)])
    table = ops.text_placement(place)
    assert isinstance(table, C.Array) and list(table) == [v for row in place for v in row]


def test_text_step_groups_rows_and_widths():
    """T = 20, the standard steps: 180 rows at full width, 96 in two groups, 86 in three; and for every T = 2 .. 64 every step's group
    is at least as wide as the new length of EVERY question of n <= T tokens that ``text_keep_batches`` (the current route) builds."""
    import torch
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    pert = lp.LxmertPerturbation(None)
    S = len(lp.PERT_STEPS)
    plans = {g: pert.text_step_groups(20, g) for g in (1, 2, 3)}
    assert [plans[g].rows for g in (1, 2, 3)] == [180, 96, 86]
    assert plans[2].steps == [[0, 1, 2], [3, 4, 5, 6, 7, 8]] and plans[3].steps == [[0], [1, 2], [3, 4, 5, 6, 7, 8]]
    assert [w for _, _, w in plans[2].groups] == [20, 6] and [w for _, _, w in plans[3].groups] == [20, 15, 6]
    where = plans[2].layout(2)
    assert list(where.table) == [v for row in TWO_GROUPS for v in row] and where.offsets == [0, 144] and where.elems == 216
    assert pert.text_step_groups(20, 2) is plans[2] and plans[2].layout(2) is where                             # cached
    assert pert.text_step_groups(20, 64).rows == sum(plans[1].bounds) == 68                                    # every step its own group
    with pytest.raises(ValueError):
        pert.text_step_groups(1)
    g = torch.Generator().manual_seed(3)
    for T in range(2, 65):
        lens = list(range(2, T + 1))
        B = len(lens)
        ids, cam = torch.randint(1, 999, (B, T), generator=g), torch.rand(B, T, generator=g)
        _, _, mask = lp.text_keep_batches(ids, torch.zeros_like(ids), cam, lp.PERT_STEPS, n_tokens=lens)
        new_len = mask.sum(dim=1).reshape(B, S).to(torch.int64)                # [B, S]
        longest = new_len.max(dim=0).values.tolist()
        for max_groups in (1, 2, 3, 9):
            plan = pert.text_step_groups(T, max_groups)
            assert len(plan.groups) <= max_groups and plan.bounds == longest    # (the bound is reached by the question of T tokens)
            covered, rows, where = [], 0, plan.layout(3)
            table = list(where.table)
            for (steps_g, n, width), offset in zip(plan.groups, where.offsets):
                assert n == steps_g.numel() and offset % (n * width) == 0 and offset + 3 * n * width <= where.elems
                rows += n * width
                for j, s in enumerate(steps_g.tolist()):
                    covered.append(s)
                    assert width >= longest[s], (T, max_groups, s)
                    assert table[3 * s:3 * s + 3] == [offset + j * width, n * width, width]
            assert sorted(covered) == list(range(S)) and rows == plan.rows and where.elems < 3 * rows + len(plan.groups) * T * S


def test_image_constants_are_keyed_on_steps_and_grouping():
    from transformer_mm_explainability_amd import lxmert_perturbation as lp
    pert = lp.LxmertPerturbation(None)
    first = pert._image_constants(36, "cpu")
    assert len(first[4]) == 2
    pert.grouped = False
    assert len(pert._image_constants(36, "cpu")[4]) == 1
    pert.grouped, pert.steps = True, (0, 0.5)
    assert pert._image_constants(36, "cpu")[0].tolist() == [36, 18]
    pert.steps = tuple(lp.PERT_STEPS)
    assert pert._image_constants(36, "cpu") is first


def test_placement_header_on_the_host():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_text_placement.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "text_placement: ok" in r.stdout, r.stdout
