"""CPU: the bounds and the input set of ``tests/rowwise_bounds.py`` are sound before a kernel is held to them.

* An fp32 numpy restatement of each kernel (its summation order, no FMA) and torch's own CPU fp32 ops meet the bounds on every input
  family at every width -- the bounds are no tighter than a correct fp32 implementation.
* Every mutant (a deliberately wrong float64 reference) exceeds a bound on at least one family at every width -- the bounds and the
  inputs together have teeth.

The worst error / bound of every restatement and every mutant is printed (past pytest's capture)."""
import math

import numpy as np
import pytest
import torch

import rowwise_bounds as rb

ROWS = 5


def worst(ratios, into):
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)


def say(capsys, line):
    with capsys.disabled():
        print("\n  " + line, end="")


def torch_cpu_layernorm(x, y, gamma, beta, eps):
    """``layer_norm`` returns ``h`` alone, and ``h`` alone is held to its bound: the statistics ATen keeps on the side come from a
    cascaded one-pass moment and are not the kernel's two-pass ones (at |mean| >> sigma its ``rstd`` is several bounds away)."""
    v = torch.from_numpy(rb.fp32_sum(x, y))
    h = torch.nn.functional.layer_norm(v, (v.shape[1],), torch.from_numpy(gamma), torch.from_numpy(beta), eps)
    return {"h": h.numpy()}


@pytest.mark.parametrize("E", rb.WIDTHS)
def test_fp32_layernorms_meet_the_bounds(E, capsys):
    for name, impl in (("restatement", rb.ln_restatement), ("torch cpu layer_norm", torch_cpu_layernorm)):
        top = {}
        for case, (x, y, gamma, beta), eps in rb.ln_cases(ROWS, E):
            ratios = rb.ln_ratios(impl(x, y, gamma, beta, eps), rb.ln_ref(x, y, gamma, beta, eps), E)
            assert max(ratios.values()) <= 1.0, (name, E, case, ratios)
            worst(ratios, top)
        say(capsys, "layernorm E=%-4d %-20s worst error / bound: %s" % (E, name, "  ".join(
            "%s %s" % (k, ("bits" if top[k] == 0 else "DIFFER") if k == "s" else "%.3f" % top[k]) for k in ("s", "mean", "rstd", "h") if k in top)))


@pytest.mark.parametrize("mutant", sorted(rb.LN_MUTANTS))
def test_every_layernorm_mutant_is_killed_at_every_width(mutant, capsys):
    wrong, applies = rb.LN_MUTANTS[mutant]
    for E in rb.WIDTHS:
        if not applies(E, ROWS, True):
            say(capsys, "layernorm mutant %-26s E=%-4d is the correct operation at this width (see LN_MUTANTS)" % (mutant, E))
            continue
        killed_by, top = [], 0.0
        for case, (x, y, gamma, beta), eps in rb.ln_cases(ROWS, E):
            if not applies(E, ROWS, case[1]):
                continue
            r = max(rb.ln_ratios(wrong(x, y, gamma, beta, eps), rb.ln_ref(x, y, gamma, beta, eps), E).values())
            top = max(top, r)
            if r > 1.0 and case[0] not in killed_by:
                killed_by.append(case[0])
        say(capsys, "layernorm mutant %-26s E=%-4d worst error / bound %9.3g  killed on: %s" % (mutant, E, top, " ".join(killed_by)))
        assert killed_by, "no input family rejects the mutant %s at E=%d (largest error / bound %.3g)" % (mutant, E, top)


def test_unbiased_variance_is_rejected_where_the_variance_counts():
    """On ``std`` / ``big`` / ``spike`` the variance dominates ``eps``: the E - 1 divisor must be far outside the bound at every width."""
    for E in rb.WIDTHS:
        for name in ("std", "big", "spike"):
            x, y, gamma, beta = rb.ln_case(name, ROWS, E, False)
            r = rb.ln_ratios(rb.LN_MUTANTS["unbiased_variance"][0](x, y, gamma, beta, 1e-5), rb.ln_ref(x, y, gamma, beta, 1e-5), E)
            assert r["rstd"] > 10.0, (E, name, r)


def gelu_sets():
    rng = np.random.default_rng(11)
    wide = np.concatenate([rng.uniform(-70.0, 70.0, 200000), rb.SPECIALS, rb.FAR]).astype(np.float32)
    return {"uniform[-70,70]": (wide, rng.standard_normal(wide.size).astype(np.float32)),
            "3 randn": ((3.0 * rng.standard_normal(200000)).astype(np.float32), rng.standard_normal(200000).astype(np.float32)),
            "grid + specials": rb.gelu_inputs(1 << 14)}


def torch_cpu_gelu(x, dy):
    xt = torch.from_numpy(x).clone().requires_grad_(True)
    y = xt * torch.sigmoid(1.702 * xt)
    y.backward(torch.from_numpy(dy))
    return y.detach().numpy(), xt.grad.numpy()


def test_fp32_quick_gelus_meet_the_bounds(capsys):
    for name, impl in (("restatement", rb.gelu_restatement), ("torch cpu x*sigmoid(1.702x)", torch_cpu_gelu)):
        for what, (x, dy) in gelu_sets().items():
            y, dx = impl(x, dy)
            rf, why_f = rb.gelu_fwd_check(y, x)
            rbk, why_b = rb.gelu_bwd_check(dx, x, dy)
            say(capsys, "quick_gelu %-28s %-16s worst error / bound: forward %.3f  backward %.3f" % (name, what, rf, rbk))
            if name == "restatement":
                assert rf <= 1.0 and rbk <= 1.0 and not why_f and not why_b, (name, what, rf, rbk, why_f, why_b)
            else:
                # autograd's backward is another formula (sigmoid', product rule): it is held to the forward rules and to the
                # backward bound inside the domain, not to the kernel's bit-exact identity outside of it
                assert rf <= 1.0 and rbk <= 1.0 and not why_f, (name, what, rf, rbk, why_f)


@pytest.mark.parametrize("mutant", sorted(rb.GELU_MUTANTS))
def test_every_quick_gelu_mutant_is_killed(mutant, capsys):
    rng = np.random.default_rng(3)
    sets = {"3 randn, n=1027": ((3.0 * rng.standard_normal(1027)).astype(np.float32), rng.standard_normal(1027).astype(np.float32)),
            "grid + specials, n=1027": rb.gelu_inputs(1027), "grid + specials, n=16384": rb.gelu_inputs(1 << 14)}
    for what, (x, dy) in sets.items():
        y, dx = rb.GELU_MUTANTS[mutant](x, dy)
        rf, why_f = rb.gelu_fwd_check(y.astype(np.float32), x)
        rbk, why_b = rb.gelu_bwd_check(dx.astype(np.float32), x, dy)
        say(capsys, "quick_gelu mutant %-18s %-25s error / bound: forward %9.3g %s backward %9.3g %s" % (mutant, what, rf, why_f, rbk, why_b))
        assert rf > 1.0 or why_f, (mutant, what, rf)
        assert rbk > 1.0 or why_b, (mutant, what, rbk)


def test_the_wrong_broadcast_index_is_killed(capsys):
    """``i // (n / x_n)`` instead of ``i % x_n``: x of batch 1 and of batch M = 3 against dy of batch 6 (K-major)."""
    rng = np.random.default_rng(5)
    for xb in (1, 3):
        x = (3.0 * rng.standard_normal((xb, 5, 12))).astype(np.float32)
        dy = rng.standard_normal((6, 5, 12)).astype(np.float32)
        right = x.reshape(-1)[rb.bcast_index(dy.size, x.size)]
        assert np.array_equal(right, np.tile(x, (6 // xb, 1, 1)).reshape(-1))
        wrong = x.reshape(-1)[rb.bcast_index(dy.size, x.size, wrong=True)]
        dx = rb.gelu_ref(wrong, dy.reshape(-1))["dx"].astype(np.float32)
        r, _ = rb.gelu_bwd_check(dx, right, dy.reshape(-1))
        say(capsys, "quick_gelu mutant wrong broadcast index, x batch %d: error / bound %.3g" % (xb, r))
        assert r > 1.0


def test_the_ratio_counts_a_one_sided_nan_as_a_failure():
    want = np.array([1.0, np.nan, np.inf])
    assert rb._ratio(np.array([1.0, np.nan, np.inf]), want, 1.0) == 0.0
    assert rb._ratio(np.array([1.0, 2.0, np.inf]), want, 1.0) == math.inf
    assert rb._ratio(np.array([np.nan, np.nan, np.inf]), want, 1.0) == math.inf
    assert rb._ratio(np.array([1.0, np.nan, -np.inf]), want, 1.0) == math.inf
    assert rb._ratio(np.array([1.5, np.nan, np.inf]), want, 0.0) == math.inf
