"""-m gpu: ``gemm_rows_f16_kernel`` at op level -- ``C[r] = half(A[r]) . W_h^T`` on the listed rows, fp32 accumulators and output,
through both C entries (plain, + bias, + bias + QuickGELU) and every tile the launcher can choose (``gemm_rows_tn`` 0 | 32 | 64).

Row lists over ``cap = 72`` rows (3 samples of 24 tokens): none, one row, 31 / 32 / 33 rows (around the 32-row tile), all 72, a shuffled
list, a list with entries outside the tensor, a count above ``cap``.  ``N``: 8, 40, 64, 104.  ``K`` from the kernel's own slab width
``BK`` and ring depth ``PF`` (64 / 3 on the 64-column tile, 128 / 2 on the 32-column one): 8 (less than a slab), one slab, one slab + 8
(ragged), ``PF - 1``, ``PF``, ``PF + 1`` and ``2 PF`` slabs, and ``(PF + 1) BK + 8``: a ragged last slab after a full round of the
steady state.  Every case runs twice and must be bit-equal; outputs are pre-filled with a sentinel whose bits unlisted rows keep.

Rounding (exact): with a weight that holds one 1 per output column every output is ONE exact product, so ``C`` must be
``A.half().float()`` permuted, bit for bit -- on values whose fp16 rounding is a tie or crosses a binade (a truncating conversion
fails on ``1 + 3 * 2^-11`` and on ``2047.5``).  Subnormal and overflowing fp16 values are kept out of it.

Accumulation: against float64 on the ROUNDED operands, ``|C - ref| <= gamma_K * sum |a_k| |w_k|`` with ``gamma_K = K u / (1 - K u)`` and
``u = 2^-23`` -- the bound of ``tests/test_gpu_gemm_rows_pipeline.py`` (Higham, Accuracy and Stability of Numerical Algorithms, section
3.1: any order of the sum) with the unit of a TRUNCATING fp32 addition, because the instruction's internal additions are not
documented as round-to-nearest; products of two fp16 numbers are exact in fp32.  With a bias: ``gamma_{K+1} * (mag + |bias|)``.  The
same figure of ``torch.mm(A.half(), W_h.t(), out_dtype=torch.float32)`` is printed beside the kernel's."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, NT = 3, 24
CAP = B * NT                                   # 72 rows: three 32-row tiles, the last one ragged
SENTINEL = 7.25
U = 2.0 ** -23
# gemm_rows_tn -> (BK, PF) of the kernel that setting launches at the N of this file (0: the launcher's choice, 32 columns for N <= 512)
TILES = {0: (128, 2), 32: (128, 2), 64: (64, 3)}
NS = (8, 40, 64, 104)


def ks_of(tn):
    bk, pf = TILES[tn]
    ks = (8, bk, bk + 8, (pf - 1) * bk, pf * bk, (pf + 1) * bk, 2 * pf * bk, (pf + 1) * bk + 8)
    assert max(ks) <= 512
    return tuple(sorted(set(ks)))


@pytest.fixture
def tiles():
    """``tiles(tn)`` sets the tile width option; the default is restored afterwards."""
    from transformer_mm_explainability_amd import ops
    yield lambda tn: ops.set_option("gemm_rows_tn", tn)
    ops.set_option("gemm_rows_tn", 0)


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


def operands(K, N, cap, seed):
    """``x [1, cap, K]`` fp32, ``w [N, K]`` fp32 (an nn.Linear weight, [out, in]; the kernel reads its fp16 copy), ``bias [N]``."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(1, cap, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) / K ** 0.5
    bias = torch.randn(N, device="cuda", generator=g)
    return x, w, bias


def run_entries(x, w, bias, live):
    """The three products of one case on sentinel-filled outputs: plain (``x @ weight`` with ``weight = w.t()``, [K, N]), + bias
    (``linear_rows`` with the nn.Linear layout ``w``), (+ bias, QuickGELU of it).  Both read the same fp16 values ``w.half()``."""
    from transformer_mm_explainability_amd import ops
    cap, n = live.cap, w.shape[0]
    shape = x.shape[:-1] + (n,)
    fill = lambda: torch.full(shape, SENTINEL, device="cuda")
    plain = ops.gemm_rows(x, w.t().contiguous(), live, out=fill(), dtype=torch.float16)
    lin = ops.linear_rows(x, w, bias, live, out=fill(), dtype=torch.float16)
    pre, act = ops.linear_rows(x, w, bias, live, out=fill(), gelu=True, act_out=fill(), dtype=torch.float16)
    return [t.view(cap, n) for t in (plain, lin, pre, act)]


def check_case(x, w, bias, live, listed, what):
    """Runs the case twice (bit-equal), checks the sentinel on the unlisted rows, the epilogues' bits and the bound on the listed rows.
    Returns ``max(err / mag)`` of the kernel and of the library product on the same operands (plain product)."""
    from transformer_mm_explainability_amd import ops
    cap, K = live.cap, w.shape[1]
    first = run_entries(x, w, bias, live)
    again = run_entries(x, w, bias, live)
    for a, b in zip(first, again):
        assert torch.equal(a, b), ("two runs differ", what)
    plain, lin, pre, act = first
    sentinel = torch.full((), SENTINEL, device="cuda")
    for out in first:
        assert torch.equal(out[~listed].view(torch.int32), sentinel.expand_as(out[~listed]).contiguous().view(torch.int32)), \
            ("an unlisted row was written", what)
    if not bool(listed.any()):
        return None
    xh, wh = x.reshape(cap, K).half(), w.half()
    ref = xh.double() @ wh.double().t()
    mag = xh.double().abs() @ wh.double().abs().t()
    lib_out = torch.mm(xh, wh.t(), out_dtype=torch.float32)
    err = (plain.double() - ref).abs()[listed]
    bound = (K * U / (1 - K * U)) * mag[listed]
    rel = float((err / mag[listed].clamp_min(1e-300)).max())
    rel_lib = float(((lib_out.double() - ref).abs()[listed] / mag[listed].clamp_min(1e-300)).max())
    print("%s: plain max err/mag kernel %.3g library %.3g gamma_K %.3g" % (what, rel, rel_lib, K * U / (1 - K * U)))
    assert bool((err <= bound).all()), (what, float(err.max()), float(bound.max()))
    errb = (lin.double() - (ref + bias.double())).abs()[listed]
    boundb = ((K + 1) * U / (1 - (K + 1) * U)) * (mag + bias.double().abs())[listed]
    print("%s: +bias err %.3g bound %.3g" % (what, float(errb.max()), float(boundb.max())))
    assert bool((errb <= boundb).all()), (what, float(errb.max()), float(boundb.max()))
    assert torch.equal(pre[listed], lin[listed]), ("the pre-activation differs from the + bias product", what)
    assert torch.equal(act[listed], ops.quick_gelu_fwd(pre.contiguous())[listed]), ("QuickGELU bits", what)
    return rel, rel_lib


@pytest.mark.parametrize("tn", sorted(TILES))
def test_pipeline_edges(tiles, tn):
    """3 captions of 24 tokens, the list built on the device (45 rows: a full and a ragged row tile), every K against every N."""
    from transformer_mm_explainability_amd import ops
    tiles(tn)
    eot = torch.tensor([20, 23, 0], device="cuda")
    live = ops.live_rows(eot, NT)
    entries = [b * NT + p for b in range(B) for p in range(int(eot[b]) + 1)]
    listed = mask(entries, CAP)
    for K in ks_of(tn):
        for N in NS:
            x, w, bias = operands(K, N, CAP, seed=K * 1000 + N)
            check_case(x.view(B, NT, K), w, bias, live, listed, "tn%d K%d N%d" % (tn, K, N))


@pytest.mark.parametrize("tn", sorted(TILES))
def test_row_list_edges(tiles, tn):
    """Hand-made lists over the 72 rows, at a one-slab-and-a-bit K and at the ragged slab after a round of the steady state."""
    tiles(tn)
    bk, pf = TILES[tn]
    perm = torch.randperm(CAP, generator=torch.Generator().manual_seed(5)).tolist()
    cases = {
        "count0": ([], None),
        "count1": ([41], None),
        "count31": (list(range(3, 34)), None),
        "count32": (list(range(5, 37)), None),
        "count33": (list(range(2, 35)), None),
        "count_cap": (list(range(CAP)), None),
        "shuffled": (perm[:45], None),
        "outside": ([5, -1, 17, CAP, 64, CAP + 300, 33], None),
        "count_above_cap": (list(range(CAP)), CAP + 9),
    }
    for K, N in ((bk + 8, 40), ((pf + 1) * bk + 8, 104)):
        x, w, bias = operands(K, N, CAP, seed=K + N)
        for name, (entries, count) in cases.items():
            live = hand_list(entries, CAP, count)
            check_case(x, w, bias, live, mask(entries, CAP), "tn%d %s K%d N%d" % (tn, name, K, N))


@pytest.mark.parametrize("tn", sorted(TILES))
def test_rounding_is_to_nearest_even_bit_for_bit(tiles, tn):
    """One 1 per output column: every output is one exact product (the other K - 1 terms are exact zeros), so ``C`` is ``A.half()``
    permuted, bit for bit, through all three epilogues (zero bias).  ``A`` holds the ties ``1 + 2^-11`` (-> 1) and ``1 + 3 * 2^-11``
    (-> ``1 + 2^-9``), ``2047.5`` (-> 2048, the next binade), their negatives, and random values of the normal fp16 range."""
    from transformer_mm_explainability_amd import ops
    tiles(tn)
    bk, pf = TILES[tn]
    live = hand_list(list(range(CAP)), CAP)
    for K, N in ((104, 104), ((pf + 1) * bk + 8, 104), (bk, 64)):
        g = torch.Generator(device="cuda").manual_seed(K + N)
        x = torch.randn(CAP, K, device="cuda", generator=g) * 8
        x = torch.where(x < 0, -1.0, 1.0) * x.abs().clamp(2.0 ** -10, 1000.0)       # normal fp16 range, no zero
        special = torch.tensor([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2047.5], device="cuda")
        special = torch.cat((special, -special))
        flat = x.view(-1)
        flat[::7] = special.repeat(flat[::7].numel() // 6 + 1)[:flat[::7].numel()]
        want_h = x.half()
        assert float(want_h[0, 0]) == 1.0 and float(want_h[0, 7]) == 1 + 2.0 ** -9 and float(want_h[0, 14]) == 2048.0
        assert bool(torch.isfinite(want_h).all()) and bool((want_h.abs() >= 2.0 ** -14).all())
        pick = torch.randperm(K, generator=torch.Generator().manual_seed(K))[:N].to("cuda")    # output column n reads input pick[n]
        w = torch.zeros(N, K, device="cuda")
        w[torch.arange(N, device="cuda"), pick] = 1.0
        want = want_h.float()[:, pick]
        outs = run_entries(x.view(1, CAP, K), w, torch.zeros(N, device="cuda"), live)
        for name, got in zip(("plain", "bias", "pre"), outs[:3]):
            assert torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32)), (name, tn, K, N)
        assert torch.equal(outs[3], ops.quick_gelu_fwd(outs[2].contiguous()))


def test_widths_outside_the_kernel_are_refused():
    from transformer_mm_explainability_amd import ops
    live = hand_list([0, 1], CAP)
    x = torch.zeros(1, CAP, 20, device="cuda")
    assert not ops.gemm_rows_eligible(torch.zeros(20, 16, device="cuda"), dtype=torch.float16)
    assert ops.gemm_rows_eligible(torch.zeros(20, 16, device="cuda"))
    assert not ops.gemm_rows_eligible(torch.zeros(16, 16, device="cuda"), dtype=torch.bfloat16)
    with pytest.raises(ops.MMXError):
        ops.gemm_rows(x, torch.zeros(20, 16, device="cuda"), live, dtype=torch.float16)
    with pytest.raises(ops.MMXError):
        ops.linear_rows(x, torch.zeros(16, 20, device="cuda"), torch.zeros(16, device="cuda"), live, dtype=torch.float16)


def test_poison_fills_the_new_outputs_too():
    """``LiveRows.poison``: the outputs the wrappers allocate start as NaN, so unlisted rows are NaN and listed rows are finite."""
    from transformer_mm_explainability_amd import ops
    entries = [3, 40, 41]
    live, listed = hand_list(entries, CAP), mask(entries, CAP)
    x, w, bias = operands(72, 40, CAP, seed=3)
    ops.LiveRows.poison = True
    try:
        plain = ops.gemm_rows(x, w.t().contiguous(), live, dtype=torch.float16).view(CAP, -1)
        pre, act = ops.linear_rows(x, w, bias, live, gelu=True, dtype=torch.float16)
    finally:
        ops.LiveRows.poison = False
    for out in (plain, pre.view(CAP, -1), act.view(CAP, -1)):
        assert bool(torch.isnan(out[~listed]).all()) and bool(torch.isfinite(out[listed]).all())
