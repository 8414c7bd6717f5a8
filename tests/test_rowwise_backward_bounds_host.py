"""CPU: the bounds and the input set of ``tests/rowwise_backward_bounds.py`` are sound before a kernel is held to them.

* An fp32 numpy restatement of the LayerNorm backward kernels (their summation order, no FMA) and a plain fp32 torch-CPU evaluation of
  the formula meet the bound on every x family x dy family, with and without ``d_res``, fp32 and bf16 ``dy``, at every width.
* Every mutant (a deliberately wrong float64 reference) breaks the bound wherever ``required`` says it must.
* The restatement scales exactly with a power of two, and with the forward's statistics it is the gradient of ``layer_norm``.
* The bf16 interval check of the QuickGELU backward accepts the fp32 restatement rounded to nearest even and rejects each bf16 mutant.

The worst error / bound of every restatement and every mutant is printed (past pytest's capture)."""
import numpy as np
import pytest
import torch

import rowwise_backward_bounds as bb
import rowwise_bounds as rb

HOST_LAYOUTS = ((3, 3), (7, 2))             # grouped (x_rows neither 1 nor the row count) and a shared pair; the device test runs them all


def say(capsys, line):
    with capsys.disabled():
        print("\n  " + line, end="")


def torch_cpu_formula(dy, x, mean, rstd, gamma, d_res):
    """The definition in fp32 torch-CPU ops, torch's own reduction order."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    dy, x, mean, rstd, gamma, d_res = map(t, (dy, x, mean, rstd, gamma, d_res))
    m = torch.arange(dy.shape[0]) % x.shape[0]
    g = dy * gamma
    rs = rstd[m][:, None]
    xh = (x[m] - mean[m][:, None]) * rs
    o = (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True)) * rs
    return (o if d_res is None else o + d_res).numpy()


def cases(E, layouts=HOST_LAYOUTS, bf16=(False,)):
    for xf in rb.FAMILIES:
        for df in bb.DY_FAMILIES:
            for x_rows, K in layouts:
                for res in (False, True):
                    for h in bf16:
                        yield (xf, df, x_rows, K, res, h), bb.bwd_case(xf, df, x_rows, K, E, res, bf16=h)


@pytest.mark.parametrize("E", bb.BF16_WIDTHS)
def test_fp32_layernorm_backwards_meet_the_bound(E, capsys):
    top = {}
    for name, impl in (("restatement", bb.bwd_restatement), ("torch cpu formula", torch_cpu_formula)):
        for key, case in cases(E, bf16=(False, True)):
            ops = bb.operands(case)
            r = bb.bwd_ratio(impl(*ops), bb.bwd_ref(*ops), E)
            assert r <= 1.0, (name, E, key, r)
            top[name] = max(top.get(name, 0.0), r)
    say(capsys, "layernorm_bwd E=%-4d worst error / bound: %s" % (E, "  ".join("%s %.3f" % kv for kv in top.items())))


@pytest.mark.parametrize("mutant", sorted(bb.BWD_MUTANTS))
def test_every_layernorm_backward_mutant_is_killed_where_required(mutant, capsys):
    """Per width, x family and dy family: at least one case (layout (3, 3), with or without ``d_res``) that the mutant can differ on puts
    it outside the bound.  On ``std`` that is asked of every mutant at every width (``B_over_E_minus_1``: from E = 8 on)."""
    wrong, applies = bb.BWD_MUTANTS[mutant]
    for E in bb.WIDTHS:
        line = []
        for xf in rb.FAMILIES:
            if not any(applies(E, 3, 3, res, xf) for res in (False, True)):
                line.append("%s: same operation" % xf)
                continue
            low = None
            for df in bb.DY_FAMILIES:
                best = 0.0
                for res in (False, True):
                    if applies(E, 3, 3, res, xf):
                        ops = bb.operands(bb.bwd_case(xf, df, 3, 3, E, res))
                        best = max(best, bb.bwd_ratio(wrong(*ops), bb.bwd_ref(*ops), E))
                low = best if low is None else min(low, best)
                if bb.required(mutant, E, xf):
                    assert best > 1.0, "mutant %s survives at E=%d on x %s, dy %s (error / bound %.3g)" % (mutant, E, xf, df, best)
            line.append("%s %.3g%s" % (xf, low, "" if bb.required(mutant, E, xf) else " (not required)"))
        say(capsys, "layernorm_bwd mutant %-27s E=%-4d least error / bound over the dy families: %s" % (mutant, E, "  ".join(line)))


def test_std_is_required_of_every_mutant():
    for mutant in bb.BWD_MUTANTS:
        for E in bb.WIDTHS:
            assert bb.required(mutant, E, "std") or (mutant == "B_over_E_minus_1" and E < 8)


@pytest.mark.parametrize("E", bb.WIDTHS)
def test_the_restatement_scales_exactly_with_a_power_of_two(E):
    for df in ("randn", "poscode"):
        for x_rows, K in HOST_LAYOUTS:
            for res in (False, True):
                case = bb.bwd_case("std", df, x_rows, K, E, res)
                assert bb.scales_exactly(bb.bwd_restatement, case), (E, df, x_rows, K, res)


def test_the_scaling_check_sees_an_absolute_error():
    """What an absolute tolerance cannot see: 1e-9 added to every result passes atol = 2e-5 at any scale and breaks the identity."""
    case = bb.bwd_case("std", "randn", 3, 3, 260, True)
    off = lambda *ops: (bb.bwd_restatement(*ops) + np.float32(1e-9)).astype(np.float32)
    assert not bb.scales_exactly(off, case)


@pytest.mark.parametrize("E", bb.WIDTHS)
def test_with_the_forward_statistics_it_is_the_gradient_of_layer_norm(E, capsys):
    """The statistics of the forward restatement fed to the backward restatement, against float64 autograd of ``layer_norm`` on the
    same fp32 ``x``: within the backward bound plus what the forward's ``mean`` / ``rstd`` bounds carry through."""
    top = 0.0
    for xf in rb.FAMILIES:
        for df in bb.DY_FAMILIES:
            case = bb.bwd_case(xf, df, 3, 3, E, True)
            dy, x, mean, rstd, gamma, d_res = bb.operands(case)
            xr = torch.from_numpy(np.tile(x, (3, 1))).double().requires_grad_(True)
            torch.nn.functional.layer_norm(xr, (E,), torch.from_numpy(gamma).double(), torch.from_numpy(case["beta"]).double(),
                                           bb.EPS).backward(torch.from_numpy(dy).double())
            want = xr.grad.numpy() + d_res.astype(np.float64)
            f64 = rb.ln_ref(x, None, gamma, case["beta"], bb.EPS)
            ref = bb.bwd_ref(dy, x, f64["mean"], f64["rstd"], gamma, d_res)
            # two float64 routes to one gradient (ATen's and the definition): float64's unit roundoff is 2**-29 of fp32's and meets
            # the same cancellations, so the two agree three orders inside the fp32 bound (what is left is the reference's own error)
            assert (np.abs(ref["o"] - want) <= 1e-3 * bb.bwd_bound(ref, E)).all(), (E, xf, df)
            slack = bb.bwd_stats_slack(ref, x, gamma, case["beta"])
            r = bb.bwd_ratio(bb.bwd_restatement(dy, x, mean, rstd, gamma, d_res), ref, E, extra=slack)
            assert r <= 1.0, (E, xf, df, r)
            top = max(top, r)
    say(capsys, "layernorm_bwd E=%-4d forward statistics -> gradient of layer_norm, worst error / (bound + carried): %.3f" % (E, top))


# ---------------------------------------------------------------------------------------------------------------------
# bf16
# ---------------------------------------------------------------------------------------------------------------------
def test_rne_bf16_is_torchs_conversion_and_rounds_float64_once():
    rng = np.random.default_rng(2)
    a = np.concatenate([rng.standard_normal(100000) * 10.0 ** rng.integers(-30, 30, 100000), rb.SPECIALS, [3.4e38, -3.4e38, 1e-45]])
    a = a.astype(np.float32)
    want = torch.from_numpy(a).to(torch.bfloat16).float().numpy()
    got = bb.rne_bf16(a)
    assert np.array_equal(got.view(np.int32)[~np.isnan(a)], want.view(np.int32)[~np.isnan(a)]) and np.isnan(got[np.isnan(a)]).all()
    # 1 + 2**-8 is the tie between 1 and 1 + 2**-7: a float64 just above it goes up although its fp32 rounding is the tie itself
    assert bb.rne_bf16(np.array([1 + 2.0 ** -8]))[0] == 1.0 and bb.rne_bf16(np.array([1 + 2.0 ** -8 + 2.0 ** -40]))[0] == 1 + 2.0 ** -7
    assert bb.trunc_bf16(np.float32(1 + 2.0 ** -7 - 2.0 ** -20)) == 1.0


GELU_SHAPES = ((8, 1, 1), (24, 5, 1), (2040, 3, 1), (2056, 9, 1), (24, 4, 3), (2048, 5, 2))      # (x_n, K, x batch)


def test_the_bf16_interval_check_accepts_the_rounded_restatement(capsys):
    for x_n, K, xb in GELU_SHAPES:
        x, dy = bb.gelu_bf16_case(x_n, K, xb)
        full = x[rb.bcast_index(dy.size, x.size)]
        bad, why = bb.gelu_bf16_check(bb.gelu_bf16_restatement(full, dy), full, dy)
        assert bad == 0 and not why, (x_n, K, xb, bad, why)


@pytest.mark.parametrize("mutant", sorted(bb.GELU_BF16_MUTANTS))
def test_the_bf16_interval_check_rejects_every_mutant(mutant, capsys):
    wrong, applies = bb.GELU_BF16_MUTANTS[mutant]
    for x_n, K, xb in GELU_SHAPES:
        if not applies(xb, K):
            continue
        x, dy = bb.gelu_bf16_case(x_n, K, xb)
        full = x[rb.bcast_index(dy.size, x.size)]
        bad, why = bb.gelu_bf16_check(wrong(x, dy, x_n), full, dy)
        say(capsys, "quick_gelu_bwd bf16 mutant %-16s x_n=%-4d K=%d x batch %d: %d of %d elements outside their interval %s"
            % (mutant, x_n, K, xb, bad, dy.size, why))
        assert bad > 0 or why, (mutant, x_n, K, xb)
