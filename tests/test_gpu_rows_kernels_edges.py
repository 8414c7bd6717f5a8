"""-m gpu: the row-list forms of the elementwise kernels (``csrc/elementwise_kernels.hip``: ``ops.quick_gelu_bwd_rows``,
``ops.layernorm_bwd_add_rows``, ``ops.add_layernorm_rows``) at op level, on hand-made lists -- none, one, every row, shuffled, ids outside
the tensor, a count above the capacity, a negative count -- and on a device-built one, and the list builder (``ops.live_rows``,
``live_rows_kernel`` of ``csrc/gemm_rows_f32.hip``) against its definition beyond one chunk of 256 samples.

A row-list kernel is the dense kernel's template body with another row index, so a listed row has the dense op's bits on the same
full tensors; it also meets the float64 reference under the tolerance the dense op's own test has (``tests/test_gpu_ops.py``); an
unlisted row keeps the bits of the sentinel the output was filled with."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from parity import close  # noqa: E402
from test_gpu_gemm_rows_pipeline import hand_list, mask as listed_rows  # noqa: E402
from test_gpu_text_forward_live_rows import live_list  # noqa: E402

CAP = 70                                       # no multiple of the 4 rows a LayerNorm workgroup takes
SENTINEL = 7.25
WIDTHS = (4, 20, 256, 260, 772, 2048)


@pytest.fixture
def options():
    """The process-wide switches of the row-list route, back at their defaults afterwards (this suite sets none; a run that fails half
    way through another suite's test must not leak into the next one either)."""
    from transformer_mm_explainability_amd import ops
    yield ops
    for key, value in (("text_live_rows", 1), ("text_live_rows_fwd", 1), ("text_live_attn", 1), ("attn_head_tile_skip", 1),
                       ("gemm_rows_tm", 32), ("gemm_rows_tn", 0)):
        ops.set_option(key, value)
    ops.LiveRows.poison = False


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def hand_lists(names=None):
    """``name -> (LiveRows over CAP rows, listed [CAP] bool, leading shape of the tensors)``."""
    perm = torch.randperm(CAP, generator=torch.Generator().manual_seed(5)).tolist()
    cases = {
        "count0": ([], None),
        "count1": ([41], None),
        "count_cap": (list(range(CAP)), None),
        "shuffled": (perm[:45], None),
        "outside": ([5, -1, 17, CAP, 64, CAP + 300, 33], None),
        "count_above_cap": (list(range(CAP)), CAP + 9),
        "count_negative": (list(range(CAP)), -3),                       # nothing is written
    }
    out = {}
    for name, (entries, count) in cases.items():
        if names is None or name in names:
            listed = listed_rows(entries if count is None or count > 0 else [], CAP)
            out[name] = (hand_list(entries, CAP, count), listed, (1, CAP))
    return out


def all_lists(names=None):
    lists = hand_lists(names)
    B, N, live, listed = live_list()
    lists["device_built"] = (live, listed, (B, N))
    return lists


def ops_close(got, want, atol, what):
    """The comparator of ``tests/test_gpu_ops.py``: elementwise ``atol + 1e-5 |ref|``, the largest error below 1e-4 of the largest entry."""
    close(got, want.float().cpu().numpy(), atol=atol, rtol=1e-5, what=what, rel_always=True)


_OPERANDS = {}


def operands(rows, E):
    """``x dy d_res gamma beta`` over ``rows`` rows of width ``E``, once per shape (never modified).  ``x`` is standard normal, as in
    ``test_layernorm_bwd_add``; the QuickGELU test takes ``3 x`` as ``test_quick_gelu_fused`` does, the forward LayerNorm ``3 x + 1`` as
    ``test_add_layernorm_rows_equals_the_dense_kernel_bit_for_bit`` does."""
    if (rows, E) not in _OPERANDS:
        g = torch.Generator(device="cuda").manual_seed(rows * 10000 + E)
        x = torch.randn(rows, E, device="cuda", generator=g)
        dy, d_res = torch.randn(rows, E, device="cuda", generator=g), torch.randn(rows, E, device="cuda", generator=g)
        gamma, beta = torch.randn(E, device="cuda", generator=g), torch.randn(E, device="cuda", generator=g)
        _OPERANDS[(rows, E)] = (x, dy, d_res, gamma, beta)
    return _OPERANDS[(rows, E)]


@pytest.mark.parametrize("E", WIDTHS)
def test_quick_gelu_bwd_rows_equals_the_dense_kernel_bit_for_bit(options, E):
    ops = options
    for name, (live, listed, lead) in all_lists().items():
        rows = live.cap
        x, dy = (t.view(lead + (E,)) for t in operands(rows, E)[:2])
        x = x * 3
        dense = ops.quick_gelu_bwd(x, dy).view(rows, E)
        xr = x.double().requires_grad_(True)
        (xr * torch.sigmoid(1.702 * xr)).backward(dy.double())
        want = xr.grad.view(rows, E)
        out = torch.full(lead + (E,), SENTINEL, device="cuda")
        got = ops.quick_gelu_bwd_rows(x, dy, live, out=out)
        assert got is out
        got = got.view(rows, E)
        assert bool((got[~listed] == SENTINEL).all()), ("an unlisted row was written", name, E)
        assert same_bits(got[listed], dense[listed]), (name, E)
        if bool(listed.any()):
            ops_close(got[listed], want[listed], 2e-6, "quick_gelu_bwd_rows E%d %s" % (E, name))
        again = ops.quick_gelu_bwd_rows(x, dy, live, out=torch.full(lead + (E,), SENTINEL, device="cuda")).view(rows, E)
        assert same_bits(again, got), ("two runs differ", name, E)


def test_quick_gelu_bwd_rows_goes_round_its_grid(options):
    """520 rows of 8192 floats are 1 064 960 16-byte groups, the grid is capped at 4096 x 256 = 1 048 576 threads: the last 16 384
    groups run on a second trip of the grid-stride loop, list lookup included.  Every row, named in reverse order, then the last nine
    only (the second trip holds no work)."""
    ops = options
    rows, E = 520, 8192
    g = torch.Generator(device="cuda").manual_seed(52)
    x = torch.randn(1, rows, E, device="cuda", generator=g) * 3
    dy = torch.randn(1, rows, E, device="cuda", generator=g)
    dense = ops.quick_gelu_bwd(x, dy)
    out = torch.full((1, rows, E), SENTINEL, device="cuda")
    ops.quick_gelu_bwd_rows(x, dy, hand_list(list(range(rows - 1, -1, -1)), rows), out=out)
    assert same_bits(out, dense)
    out.fill_(SENTINEL)
    ops.quick_gelu_bwd_rows(x, dy, hand_list(list(range(rows - 9, rows)), rows), out=out)
    assert same_bits(out[0, rows - 9:], dense[0, rows - 9:])
    assert bool((out[0, :rows - 9] == SENTINEL).all())


@pytest.mark.parametrize("E", WIDTHS)
def test_layernorm_bwd_add_rows_equals_the_dense_kernel_bit_for_bit(options, E):
    ops = options
    for name, (live, listed, lead) in all_lists().items():
        rows = live.cap
        x, dy, d_res, gamma, beta = operands(rows, E)
        x, dy, d_res = (t.view(lead + (E,)) for t in (x, dy, d_res))
        _, _, mean, rstd = ops.add_layernorm(x, None, gamma, beta, 1e-5)
        xr = x.double().requires_grad_(True)
        torch.nn.functional.layer_norm(xr, (E,), gamma.double(), beta.double(), 1e-5).backward(dy.double())
        for res in (d_res, None):
            dense = ops.layernorm_bwd_add(dy, x, mean, rstd, gamma, res).view(rows, E)
            want = (xr.grad + res.double() if res is not None else xr.grad).view(rows, E)
            out = torch.full(lead + (E,), SENTINEL, device="cuda")
            got = ops.layernorm_bwd_add_rows(dy, x, mean, rstd, gamma, res, live, out=out)
            assert got is out
            got = got.view(rows, E)
            what = (name, E, "d_res" if res is not None else "no d_res")
            assert bool((got[~listed] == SENTINEL).all()), ("an unlisted row was written",) + what
            assert same_bits(got[listed], dense[listed]), what
            if bool(listed.any()):
                ops_close(got[listed], want[listed], 2e-5, "layernorm_bwd_add_rows E%d %s %s" % (E, name, what[2]))
            again = ops.layernorm_bwd_add_rows(dy, x, mean, rstd, gamma, res, live, out=torch.full(lead + (E,), SENTINEL, device="cuda"))
            assert same_bits(again.view(rows, E), got), ("two runs differ",) + what


def test_the_out_argument_is_checked(options):
    ops = options
    live, _, lead = hand_lists(("count1",))["count1"]
    x, dy, d_res, gamma, beta = (t.view(lead + (20,)) if t.dim() == 2 else t for t in operands(CAP, 20))
    _, _, mean, rstd = ops.add_layernorm(x, None, gamma, beta, 1e-5)
    for bad in (torch.empty(lead + (24,), device="cuda"), torch.empty(lead + (20,), device="cuda", dtype=torch.float64),
                torch.empty((1, CAP + 1, 20), device="cuda"), torch.empty(lead + (40,), device="cuda")[..., ::2]):
        with pytest.raises(ops.MMXError):
            ops.quick_gelu_bwd_rows(x, dy, live, out=bad)
        with pytest.raises(ops.MMXError):
            ops.layernorm_bwd_add_rows(dy, x, mean, rstd, gamma, d_res, live, out=bad)


@pytest.mark.parametrize("E", [1280, 2048, 2052, 4096])
def test_add_layernorm_rows_wide_instantiations_equal_the_dense_kernel_bit_for_bit(options, E):
    """Widths above 1024: 8 and 16 register chunks of 64 x 4 floats per row (1280 is a CLIP text width; 2048 and 4096 fill the last
    chunk, 2052 is the first width of the widest instantiation)."""
    ops = options
    fills = (7.25, -3.5, 1.5, 2.5)
    for name, (live, listed, lead) in all_lists(("outside", "shuffled", "count_above_cap")).items():
        rows = live.cap
        x, other, _, gamma, beta = operands(rows, E)
        x = x.view(lead + (E,)) * 3 + 1
        for y in (other.view(lead + (E,)), None):
            want = ops.add_layernorm(x, y, gamma, beta, 1e-5)
            out = (torch.full(lead + (E,), fills[0], device="cuda"), torch.full(lead + (E,), fills[1], device="cuda"),
                   torch.full((rows,), fills[2], device="cuda"), torch.full((rows,), fills[3], device="cuda"))
            got = ops.add_layernorm_rows(x, y, gamma, beta, 1e-5, live, out=out)
            if y is None:
                assert got[0] is x
            for i, (a, b, fill) in enumerate(zip(got, want, fills)):
                if i == 0 and y is None:
                    assert bool((out[0] == fills[0]).all())                  # no sum without a second operand
                    continue
                a2, b2 = a.reshape(rows, -1), b.reshape(rows, -1)
                assert same_bits(a2[listed], b2[listed]), (name, E, i)
                assert bool((a2[~listed] == fill).all()), (name, E, i)


def test_add_layernorm_rows_turns_down_a_row_wider_than_its_registers(options):
    ops = options
    live, _, lead = hand_lists(("count1",))["count1"]
    x = torch.randn(lead + (4100,), device="cuda")
    gamma = torch.ones(4100, device="cuda")
    with pytest.raises(ops.MMXError):
        ops.add_layernorm_rows(x, None, gamma, gamma, 1e-5, live)


# ---------------------------------------------------------------------------------------------------------- the list builder

def eot_for(B, N, seed):
    eot = torch.randint(-5, N + 5, (B,), generator=torch.Generator().manual_seed(seed))
    for index, value in ((0, -1), (255, N - 1), (256, 0), (B - 1, 2 ** 40)):
        if index < B:
            eot[index] = value
    return eot


def definition(eot, N):
    rows = []
    for b, e in enumerate(eot.tolist()):
        rows.extend(b * N + p for p in range(min(max(e, 0), N - 1) + 1))
    return torch.tensor(rows, dtype=torch.int32)


@pytest.mark.parametrize("B,N", [(1, 77), (255, 77), (256, 77), (257, 77), (600, 77), (300, 1), (300, 8)])
def test_live_rows_against_its_definition(options, B, N):
    """One workgroup walks the batch in chunks of 256 samples and reuses its two LDS arrays per chunk: 257 and 600 samples take a
    second and a third trip.  ``eot`` below 0 and above N - 1 is clamped.  600 samples: two calls back to back on one stream."""
    ops = options
    eot = eot_for(B, N, seed=B * 100 + N)
    want = definition(eot, N)
    on_device = eot.cuda()
    lists = [ops.live_rows(on_device, N) for _ in range(2 if B == 600 else 1)]
    for live in lists:
        assert live.cap == B * N and live.rows.dtype == torch.int32 and live.rows.numel() == B * N
        count = int(live.count.item())
        assert count == want.numel()
        assert torch.equal(live.rows[:count].cpu(), want)
