"""What every ``Graphed*`` wrapper of this package does the same way, once: warm up and capture a call into a hipGraph
(``capture``), copy a new batch into the captured buffers (``copy_inputs`` / ``copy_index``) and DETR's K-slot replay loop
(``fill_slots`` / ``replay_slots``).  What a wrapper does on its own (its call, its refusals, its deferred checks) stays in
its class."""
import torch

from . import ops

MISMATCH = "%s: %s, but the graph was captured for %s"
PAD_HINT = " (pad the batch to the captured shape)"
NO_INDEX = "the graph was captured with index=None (arg-max answers)"


def capture(call, warmup, model=None, keep=()):
    """``warmup`` runs of ``call()`` on a fresh stream, then one captured into a hipGraph through ``ops.graph_capture``.
    Returns ``(graph, out, pinned)``: ``out`` is what the captured ``call()`` returned (the graph's output buffers) and
    ``pinned`` is everything the graph holds raw addresses of besides its own pool -- ``ops.pinned_state(model)`` plus the
    objects in ``keep`` (a callable: evaluated after the capture, for what the warm-up calls install).  The wrapper keeps
    ``pinned`` alive as long as ``graph``."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmup):
            call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        out = call()
    return graph, out, ops.pinned_state(model) + list(keep() if callable(keep) else keep)


def copy_inputs(static, new, keys=None, hint="", text=MISMATCH):
    """``static[k].copy_(new[k])`` for every key of ``keys`` (default: every key of ``new``), refusing a tensor of another
    shape than the captured one by name: ``text % (key, offered shape, captured shape) + hint``."""
    for k in (new if keys is None else keys):
        if new[k].shape != static[k].shape:
            raise ValueError(text % (k, tuple(new[k].shape), tuple(static[k].shape)) + hint)
        static[k].copy_(new[k])


def copy_index(static_index, index, refusal=NO_INDEX):
    """Overwrite the captured target indices with ``index`` (``None``: they stay).  A graph captured without indices picks
    its targets itself and refuses one with ``refusal``."""
    if index is not None:
        if static_index is None:
            raise ValueError(refusal)
        static_index.copy_(torch.as_tensor(index))


def fill_slots(targets_buf, index_buf, part, classes=None):
    """One chunk of at most K targets into the K slots: ``part`` (and its ``classes``; without them every slot's class is -1,
    "this pass's own arg-max") goes to the first slots, the spare ones repeat the chunk's last target and that slot's class.
    Returns the number of slots whose rows are kept."""
    n = part.numel()
    targets_buf[:n] = part
    index_buf.fill_(-1)
    if classes is not None:
        index_buf[:n] = classes
    if n < targets_buf.numel():
        targets_buf[n:] = part[-1]
        index_buf[n:] = index_buf[n - 1]
    return n


def replay_slots(graph, K, targets_buf, index_buf, out, targets, classes, after_replay=None):
    """``targets`` in chunks of ``K`` through the captured K-slot pass: fill the slots, replay, ``after_replay()`` (the
    wrapper's check of the pass, if it has one), keep the chunk's rows of ``out [1, 1, K, Ni]``.  Returns ``[1, 1, n, Ni]``."""
    chunks = []
    for i in range(0, targets.numel(), K):
        n = fill_slots(targets_buf, index_buf, targets[i:i + K], None if classes is None else classes[i:i + K])
        graph.replay()
        if after_replay is not None:
            after_replay()
        chunks.append(out[:, :, :n].clone())
    return torch.cat(chunks, dim=2) if len(chunks) != 1 else chunks[0]
