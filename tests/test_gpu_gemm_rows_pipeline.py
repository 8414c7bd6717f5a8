"""-m gpu: the pipelined K loop of ``gemm_rows_f32_kernel`` at its edges -- slab counts around the depth of the prefetch ring, a ragged
last slab, one long K -- and the row list at its own: no row, one row, every row, a ragged last row tile, an entry outside the tensor,
a shuffled list.  Every case runs through both C entries (plain, + bias, + bias + QuickGELU) and every tile reachable through
``ops.set_option`` (``gemm_rows_tm`` 32 | 64, ``gemm_rows_tn`` 0 | 32 | 64).

Bound, as in ``test_live_rows_list_and_gemm_rows_kernel``: for ANY order of an fp32 sum of K products, |err| <= gamma_K * sum |a_k| |w_k|
with gamma_K = K u / (1 - K u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), against a float64
product.  The bias is one more rounded addition: gamma_{K+1} * (sum |a_k| |w_k| + |bias|) (same section, the bias as a K + 1-th term).
Unlisted rows keep the bits of a sentinel the outputs are pre-filled with."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, NT = 3, 8                                   # cap = 24 rows
CAP = B * NT
SENTINEL = 7.25
U = 2.0 ** -24
# (tm, tn) settings: tn = 0 is the launcher's own choice from the shape; tm = 64 has one tile width
TILES = ((32, 0), (32, 64), (32, 32), (64, 0))
# the slab is 32 wide on the 64-column tiles and 64 wide on the 32-column tile, the ring is 3 slabs deep on both:
#   4 | 20 | 32: one slab (20: a multiple of 4 that is no multiple of the slab)     36: slab + 4 on the 32-wide slab
#   64: 2 slabs / 1 slab (fewer than the ring)    68: slab + 4 on the 64-wide slab    96 | 128: exactly 3 / 4 slabs of 32
#   192 | 256: exactly 3 / 4 slabs of 64 (6 / 8 of 32: two rounds of the steady state)    200: a ragged seventh / fourth slab
KS = (4, 20, 32, 36, 64, 68, 96, 128, 192, 200, 256)
NS = (16, 36, 64, 100)


@pytest.fixture
def tiles():
    """``tiles(tm, tn)`` sets the two tile options; the defaults are restored afterwards."""
    from transformer_mm_explainability_amd import ops

    def choose(tm, tn):
        ops.set_option("gemm_rows_tm", tm)
        ops.set_option("gemm_rows_tn", tn)
    yield choose
    ops.set_option("gemm_rows_tm", 32)
    ops.set_option("gemm_rows_tn", 0)


def hand_list(entries, cap, count=None):
    """A ``LiveRows`` over ``cap`` rows (one sample of ``cap`` tokens) naming ``entries`` in that order; ``count`` overrides the length."""
    from transformer_mm_explainability_amd import ops
    rows = torch.full((cap,), -7, dtype=torch.int32, device="cuda")           # the slots past the count hold no row
    if entries:
        rows[:len(entries)] = torch.tensor(entries, dtype=torch.int32, device="cuda")
    cnt = torch.tensor([len(entries) if count is None else count], dtype=torch.int32, device="cuda")
    return ops.LiveRows(rows, cnt, 1, cap)


def run_entries(x, w, bias, live):
    """The three products of one case on sentinel-filled outputs: plain, + bias, (+ bias, QuickGELU of it)."""
    from transformer_mm_explainability_amd import ops
    cap, n = live.cap, w.shape[1]
    shape = x.shape[:-1] + (n,)
    fill = lambda: torch.full(shape, SENTINEL, device="cuda")
    plain = ops.gemm_rows(x, w, live, out=fill())
    wt = w.t().contiguous()                                                    # linear_rows takes the nn.Linear layout [out, in]
    lin = ops.linear_rows(x, wt, bias, live, out=fill())
    pre, act = ops.linear_rows(x, wt, bias, live, out=fill(), gelu=True, act_out=fill())
    return [t.view(cap, n) for t in (plain, lin, pre, act)]


def check_case(x, w, bias, live, listed, what):
    """Runs the case twice (bit-equal), checks the bound on the listed rows and the sentinel on the others."""
    from transformer_mm_explainability_amd import ops
    cap, K = live.cap, w.shape[0]
    first = run_entries(x, w, bias, live)
    again = run_entries(x, w, bias, live)
    for a, b in zip(first, again):
        assert torch.equal(a, b), ("two runs differ", what)
    plain, lin, pre, act = first
    x2 = x.reshape(cap, K).double()
    ref = x2 @ w.double()
    mag = x2.abs() @ w.double().abs()
    for out in first:
        assert bool((out[~listed] == SENTINEL).all()), ("an unlisted row was written", what)
    if not bool(listed.any()):
        return
    err = (plain.double() - ref).abs()[listed]
    bound = (K * U / (1 - K * U)) * mag[listed]
    print("%s: plain err %.3g bound %.3g" % (what, float(err.max()), float(bound.max())))
    assert bool((err <= bound).all()), (what, float(err.max()), float(bound.max()))
    errb = (lin.double() - (ref + bias.double())).abs()[listed]
    boundb = ((K + 1) * U / (1 - (K + 1) * U)) * (mag + bias.double().abs())[listed]
    print("%s: +bias err %.3g bound %.3g" % (what, float(errb.max()), float(boundb.max())))
    assert bool((errb <= boundb).all()), (what, float(errb.max()), float(boundb.max()))
    assert torch.equal(pre[listed], lin[listed]), ("the pre-activation differs from the + bias product", what)
    assert torch.equal(act[listed], ops.quick_gelu_fwd(pre.contiguous())[listed]), ("QuickGELU bits", what)


def operands(K, N, cap, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(1, cap, K, device="cuda", generator=g)
    w = torch.randn(K, N, device="cuda", generator=g) / K ** 0.5
    bias = torch.randn(N, device="cuda", generator=g)
    return x, w, bias


def mask(entries, cap):
    listed = torch.zeros(cap, dtype=torch.bool, device="cuda")
    ok = [e for e in entries if 0 <= e < cap]
    if ok:
        listed[torch.tensor(ok, device="cuda")] = True
    return listed


@pytest.mark.parametrize("tm,tn", TILES)
def test_pipeline_edges(tiles, tm, tn):
    """B = 3 captions of 8 tokens, the list built on the device, every K of ``KS`` against every N of ``NS``."""
    from transformer_mm_explainability_amd import ops
    tiles(tm, tn)
    eot = torch.tensor([2, 7, 0], device="cuda")
    live = ops.live_rows(eot, NT)
    entries = [b * NT + p for b in range(B) for p in range(int(eot[b]) + 1)]
    listed = mask(entries, CAP)
    for K in KS:
        for N in NS:
            x, w, bias = operands(K, N, CAP, seed=K * 1000 + N)
            check_case(x.view(B, NT, K), w, bias, live, listed, "tm%d tn%d K%d N%d" % (tm, tn, K, N))


@pytest.mark.parametrize("tm,tn", TILES)
def test_long_k_runs_the_steady_state(tiles, tm, tn):
    """K = 2048 at N = 64: 64 / 32 slabs, so the steady-state loop body runs many rounds of its ring."""
    from transformer_mm_explainability_amd import ops
    tiles(tm, tn)
    eot = torch.tensor([2, 7, 0], device="cuda")
    live = ops.live_rows(eot, NT)
    entries = [b * NT + p for b in range(B) for p in range(int(eot[b]) + 1)]
    x, w, bias = operands(2048, 64, CAP, seed=11)
    check_case(x.view(B, NT, 2048), w, bias, live, mask(entries, CAP), "tm%d tn%d K2048 N64" % (tm, tn))


@pytest.mark.parametrize("tm,tn", TILES)
def test_row_list_edges(tiles, tm, tn):
    """Hand-made lists over 70 rows (three row tiles of 32, two of 64): none, one, all, 33 and 65 (a ragged last tile), an entry
    outside ``[0, cap)`` (skipped), a shuffled list, and a count above the capacity (clamped to it)."""
    tiles(tm, tn)
    cap = 70
    perm = torch.randperm(cap, generator=torch.Generator().manual_seed(5)).tolist()
    cases = {
        "count0": ([], None),
        "count1": ([41], None),
        "count_cap": (list(range(cap)), None),
        "count33": (list(range(3, 36)), None),
        "count65": (list(range(2, 67)), None),
        "outside": ([5, -1, 17, cap, 64, cap + 300, 33], None),
        "shuffled": (perm[:45], None),
        "count_above_cap": (list(range(cap)), cap + 9),
    }
    for K, N in ((36, 36), (200, 100)):
        x, w, bias = operands(K, N, cap, seed=K + N)
        for name, (entries, count) in cases.items():
            live = hand_list(entries, cap, count)
            check_case(x, w, bias, live, mask(entries, cap), "tm%d tn%d %s K%d N%d" % (tm, tn, name, K, N))
