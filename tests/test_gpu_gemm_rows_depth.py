"""-m gpu: ``gemm_rows_f32_kernel`` at every depth of its register ring (``ops.set_option("gemm_rows_pf", 0 | 3 | 4)``: the
slabs of K requested ahead; 0 is the launcher's choice) on every tile reachable through ``gemm_rows_tm`` / ``gemm_rows_tn``, through both C
entries (plain, + bias, + bias + QuickGELU).  It follows ``tests/test_gpu_gemm_rows_pipeline.py``: 3 captions of 8 tokens (capacity 24
rows), the list built on the device.

K walks every slab count from 1 to 18 for both slab widths (32 on the 64-column tiles, 64 on the 32-column tile), each again
with a ragged + 4, so that every ring depth meets "fewer slabs than the ring", "exactly the ring", "one more" and "two rounds and a
remainder".  The row-list cases of that file run once per depth at (K, N) = (200, 100).

Bound, as there: for ANY order of an fp32 sum of K products, |err| <= gamma_K * sum |a_k| |w_k| with gamma_K = K u / (1 - K u), u = 2^-24
(Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), against a float64 product; gamma_{K+1} * (sum |a_k| |w_k| + |bias|)
with the bias.  Unlisted rows keep the bits of a sentinel.  And for a fixed tile the outputs are bit-equal across the depths: the depth
moves loads, the k order of every sum stays."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

B, NT = 3, 8                                   # cap = 24 rows
CAP = B * NT
SENTINEL = 7.25
U = 2.0 ** -24
TILES = ((32, 0), (32, 64), (32, 32), (64, 0))  # (tm, tn): tn = 0 is the launcher's own choice from the shape
DEPTHS = (0, 3, 4)
# slab counts 1 .. 18 of either slab width, each with a ragged + 4
KS_BY_SLAB = {w: tuple(k for j in range(1, 19) for k in (w * j, w * j + 4)) for w in (32, 64)}
NS = (16, 36, 64, 100)
EOT = (2, 7, 0)


@pytest.fixture
def options():
    """``options(tm, tn, pf)`` sets the tile and depth options; the defaults are restored afterwards."""
    from transformer_mm_explainability_amd import ops

    def choose(tm, tn, pf):
        ops.set_option("gemm_rows_tm", tm)
        ops.set_option("gemm_rows_tn", tn)
        ops.set_option("gemm_rows_pf", pf)
    yield choose
    choose(32, 0, 0)


@functools.lru_cache(maxsize=None)
def case(K, N, cap):
    """Operands of a (K, N) case over ``cap`` rows with their float64 product and magnitude: computed once, shared by every tile and
    depth, never written to."""
    g = torch.Generator(device="cuda").manual_seed(K * 1000 + N)
    x = torch.randn(1, cap, K, device="cuda", generator=g)
    w = torch.randn(K, N, device="cuda", generator=g) / K ** 0.5
    bias = torch.randn(N, device="cuda", generator=g)
    x2 = x.reshape(cap, K).double()
    return x, w, w.t().contiguous(), bias, x2 @ w.double(), x2.abs() @ w.double().abs()


def hand_list(entries, cap, count=None):
    """A ``LiveRows`` over ``cap`` rows (one sample of ``cap`` tokens) naming ``entries`` in that order; ``count`` overrides the length."""
    from transformer_mm_explainability_amd import ops
    rows = torch.full((cap,), -7, dtype=torch.int32, device="cuda")           # the slots past the count hold no row
    if entries:
        rows[:len(entries)] = torch.tensor(entries, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([len(entries) if count is None else count], dtype=torch.int32, device="cuda")
    return ops.LiveRows(rows, cnt, 1, cap)


def mask(entries, cap):
    listed = torch.zeros(cap, dtype=torch.bool, device="cuda")
    ok = [e for e in entries if 0 <= e < cap]
    if ok:
        listed[torch.tensor(ok, device="cuda")] = True
    return listed


def run_entries(x, w, wt, bias, live):
    """The three products of one case on sentinel-filled outputs: plain, + bias, (+ bias, QuickGELU of it)."""
    from transformer_mm_explainability_amd import ops
    cap, n = live.cap, w.shape[1]
    shape = x.shape[:-1] + (n,)
    fill = lambda: torch.full(shape, SENTINEL, device="cuda")
    plain = ops.gemm_rows(x, w, live, out=fill())
    lin = ops.linear_rows(x, wt, bias, live, out=fill())
    pre, act = ops.linear_rows(x, wt, bias, live, out=fill(), gelu=True, act_out=fill())
    return [t.view(cap, n) for t in (plain, lin, pre, act)]


def check_case(K, N, live, listed, what):
    """Runs the case twice (bit-equal), checks the bound on the listed rows and the sentinel on the others; returns the four outputs."""
    from transformer_mm_explainability_amd import ops
    x, w, wt, bias, ref, mag = case(K, N, live.cap)
    x = x.view(live.batch, live.n_tokens, K)
    first = run_entries(x, w, wt, bias, live)
    again = run_entries(x, w, wt, bias, live)
    for a, b in zip(first, again):
        assert torch.equal(a, b), ("two runs differ", what)
    plain, lin, pre, act = first
    for out in first:
        assert bool((out[~listed] == SENTINEL).all()), ("an unlisted row was written", what)
    if not bool(listed.any()):
        return first
    err = (plain.double() - ref).abs()[listed]
    bound = (K * U / (1 - K * U)) * mag[listed]
    assert bool((err <= bound).all()), (what, float(err.max()), float(bound.max()))
    errb = (lin.double() - (ref + bias.double())).abs()[listed]
    boundb = ((K + 1) * U / (1 - (K + 1) * U)) * (mag + bias.double().abs())[listed]
    assert bool((errb <= boundb).all()), (what, float(errb.max()), float(boundb.max()))
    assert torch.equal(pre[listed], lin[listed]), ("the pre-activation differs from the + bias product", what)
    assert torch.equal(act[listed], ops.quick_gelu_fwd(pre.contiguous())[listed]), ("QuickGELU bits", what)
    return first


def across_depths(options, tm, tn, cases):
    """``cases``: (K, N, live, listed, name).  Every case at every depth; per case the outputs of all depths are bit-equal."""
    for K, N, live, listed, name in cases:
        base = None
        for pf in DEPTHS:
            options(tm, tn, pf)
            what = "tm%d tn%d pf%d %s K%d N%d" % (tm, tn, pf, name, K, N)
            outs = check_case(K, N, live, listed, what)
            if base is None:
                base = outs
            for a, b in zip(base, outs):
                assert torch.equal(a, b), ("the outputs depend on the depth", what)


@pytest.mark.parametrize("slab", sorted(KS_BY_SLAB))
@pytest.mark.parametrize("tm,tn", TILES)
def test_depth_slab_counts(options, tm, tn, slab):
    """Slab counts 1 .. 18 of ``slab``-wide slabs, plain and ragged, against every N of ``NS``; the list built on the device."""
    from transformer_mm_explainability_amd import ops
    eot = torch.tensor(EOT, device="cuda")
    live = ops.live_rows(eot, NT)
    listed = mask([b * NT + p for b in range(B) for p in range(EOT[b] + 1)], CAP)
    across_depths(options, tm, tn, [(K, N, live, listed, "captions") for K in KS_BY_SLAB[slab] for N in NS])


@pytest.mark.parametrize("tm,tn", TILES)
def test_depth_row_list_edges(options, tm, tn):
    """Hand-made lists over 70 rows at (K, N) = (200, 100): none, one, all, 33 and 65 (a ragged last tile), entries outside ``[0, cap)``
    (skipped), a shuffled list, and a count above the capacity (clamped to it)."""
    cap = 70
    perm = torch.randperm(cap, generator=torch.Generator().manual_seed(5)).tolist()
    lists = {
        "count0": ([], None),
        "count1": ([41], None),
        "count_cap": (list(range(cap)), None),
        "count33": (list(range(3, 36)), None),
        "count65": (list(range(2, 67)), None),
        "outside": ([5, -1, 17, cap, 64, cap + 300, 33], None),
        "shuffled": (perm[:45], None),
        "count_above_cap": (list(range(cap)), cap + 9),
    }
    across_depths(options, tm, tn, [(200, 100, hand_list(entries, cap, count), mask(entries, cap), name)
                                    for name, (entries, count) in lists.items()])


def test_unknown_depth_is_refused():
    from transformer_mm_explainability_amd import ops
    for pf in (-1, 1, 2, 5, 6, 8, 16):
        with pytest.raises(ops.MMXError):
            ops.set_option("gemm_rows_pf", pf)
