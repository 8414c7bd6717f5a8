"""The helpers every ``Graphed*`` wrapper shares (``graphed.py``), on CPU tensors: the checked copy of a new batch into the
captured buffers, the index variant and DETR's K-slot filling and chunk loop (the graph is a recorder here: ``replay_slots``
only ever calls ``graph.replay()``).  The capture itself needs a GPU: ``tests/test_gpu_graphed_call.py``."""
import pytest
import torch

from transformer_mm_explainability_amd import graphed


def _static():
    return {"input_ids": torch.zeros(2, 4, dtype=torch.long), "visual_feats": torch.zeros(2, 3, 5)}


def test_copy_inputs_copies_in_place():
    static = _static()
    ptrs = {k: v.data_ptr() for k, v in static.items()}
    new = {"input_ids": torch.arange(8).reshape(2, 4), "visual_feats": torch.randn(2, 3, 5, generator=torch.Generator().manual_seed(0))}
    graphed.copy_inputs(static, new)
    for k in new:
        assert torch.equal(static[k], new[k]) and static[k].data_ptr() == ptrs[k] and static[k] is not new[k]


@pytest.mark.parametrize("kw,want", [
    # the texts of the wrappers before they shared this helper, for key "input_ids", (2, 5) offered, (2, 4) captured
    (dict(hint=graphed.PAD_HINT), "input_ids: (2, 5), but the graph was captured for (2, 4) (pad the batch to the captured shape)"),
    (dict(), "input_ids: (2, 5), but the graph was captured for (2, 4)"),
    (dict(text="%s: %s, captured for %s"), "input_ids: (2, 5), captured for (2, 4)"),
])
def test_copy_inputs_refuses_another_shape_by_name(kw, want):
    static = _static()
    new = {"visual_feats": torch.ones(2, 3, 5), "input_ids": torch.ones(2, 5, dtype=torch.long)}
    with pytest.raises(ValueError) as err:
        graphed.copy_inputs(static, new, **kw)
    assert str(err.value) == want
    assert "input_ids" in want and "(2, 5)" in want and "(2, 4)" in want
    assert not static["input_ids"].any()


def test_copy_inputs_cams_text():
    """``GraphedVisualBertPerturbation``'s text for its cams (no hint)."""
    with pytest.raises(ValueError) as err:
        graphed.copy_inputs({"cams": torch.zeros(2, 7)}, {"cams": torch.zeros(3, 7)})
    assert str(err.value) == "cams: (3, 7), but the graph was captured for (2, 7)"


def test_copy_inputs_ignores_keys_outside_keys():
    static = _static()
    new = {"input_ids": torch.ones(2, 4, dtype=torch.long), "visual_feats": torch.ones(9, 9), "targets": torch.ones(1)}
    graphed.copy_inputs(static, new, keys=("input_ids",))              # another shape, a key never captured: neither is looked at
    assert static["input_ids"].all() and not static["visual_feats"].any()
    with pytest.raises(ValueError):
        graphed.copy_inputs(static, new, keys=("input_ids", "visual_feats"))


def test_copy_index():
    captured = torch.tensor([3, 7])
    ptr = captured.data_ptr()
    graphed.copy_index(captured, [1, 5])
    assert captured.tolist() == [1, 5] and captured.data_ptr() == ptr
    graphed.copy_index(captured, torch.tensor([2, 2]))
    assert captured.tolist() == [2, 2]
    graphed.copy_index(captured, None)                                  # nothing given: the captured index stays
    assert captured.tolist() == [2, 2]
    graphed.copy_index(None, None)
    with pytest.raises(ValueError) as err:
        graphed.copy_index(None, [1, 5])
    assert str(err.value) == "the graph was captured with index=None (arg-max answers)"
    with pytest.raises(ValueError) as err:
        graphed.copy_index(None, [1, 5], "this graph picks its classes itself (top_k mode)")
    assert str(err.value) == "this graph picks its classes itself (top_k mode)"


K = 4
CASES = [(1, 1, (1,)), (3, 1, (3,)), (4, 1, (4,)), (6, 2, (4, 2))]      # targets, chunks, kept widths


def _restated(targets, classes):
    """The slot rules as the issue states them: chunks of K; a chunk's targets and classes go to its first slots, spare slots repeat
    the chunk's last target and that slot's class; every class is -1 when none are given.  -> [(targets[K], classes[K], width)]"""
    chunks = []
    for i in range(0, len(targets), K):
        part = targets[i:i + K]
        cls = classes[i:i + K] if classes is not None else [-1] * len(part)
        spare = K - len(part)
        chunks.append((part + [part[-1]] * spare, cls + [cls[-1]] * spare, len(part)))
    return chunks


def _targets(n, with_classes):
    return [11 + 3 * i for i in range(n)], ([40 - i for i in range(n)] if with_classes else None)


@pytest.mark.parametrize("with_classes", [True, False])
@pytest.mark.parametrize("n,n_chunks,widths", CASES)
def test_fill_slots(n, n_chunks, widths, with_classes):
    targets, classes = _targets(n, with_classes)
    want = _restated(targets, classes)
    assert len(want) == n_chunks and tuple(w for _, _, w in want) == widths
    t_buf, i_buf = torch.full((K,), 99), torch.full((K,), 99)          # stale values of an earlier chunk
    for c, (want_t, want_i, width) in enumerate(want):
        part = torch.tensor(targets[c * K:(c + 1) * K])
        cls = None if classes is None else torch.tensor(classes[c * K:(c + 1) * K])
        assert graphed.fill_slots(t_buf, i_buf, part, cls) == width
        assert t_buf.tolist() == want_t and i_buf.tolist() == want_i
        if not with_classes:
            assert i_buf.tolist() == [-1] * K


class _Recorder:
    """Stands in for the captured pass: a replay writes one row per slot from what the slots hold."""

    def __init__(self, t_buf, i_buf, out):
        self.t_buf, self.i_buf, self.out, self.seen = t_buf, i_buf, out, []

    def replay(self):
        self.seen.append((self.t_buf.tolist(), self.i_buf.tolist()))
        self.out[0, 0, :, 0] = self.t_buf
        self.out[0, 0, :, 1] = self.i_buf


@pytest.mark.parametrize("with_classes", [True, False])
@pytest.mark.parametrize("n,n_chunks,widths", CASES)
def test_replay_slots(n, n_chunks, widths, with_classes):
    targets, classes = _targets(n, with_classes)
    want = _restated(targets, classes)
    t_buf, i_buf, out = torch.zeros(K, dtype=torch.long), torch.zeros(K, dtype=torch.long), torch.zeros(1, 1, K, 2, dtype=torch.long)
    graph = _Recorder(t_buf, i_buf, out)
    after = []
    got = graphed.replay_slots(graph, K, t_buf, i_buf, out, torch.tensor(targets), None if classes is None else torch.tensor(classes),
                               after_replay=lambda: after.append(len(graph.seen)))
    assert graph.seen == [(t, i) for t, i, _ in want] and len(graph.seen) == n_chunks
    assert after == list(range(1, n_chunks + 1))                        # once per chunk, after its replay
    assert got.shape == (1, 1, n, 2) and got.data_ptr() != out.data_ptr()
    assert got[0, 0, :, 0].tolist() == targets                          # the kept rows: every target once, in order
    assert got[0, 0, :, 1].tolist() == (classes if with_classes else [-1] * n)
    # and without the hook
    assert torch.equal(graphed.replay_slots(graph, K, t_buf, i_buf, out, torch.tensor(targets),
                                            None if classes is None else torch.tensor(classes)), got)
