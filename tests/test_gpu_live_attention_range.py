"""-m gpu: the live-length instantiations of the whole-head attention kernels (``ops.attn_capture_fwd(live=...)`` /
``ops.attn_capture_bwd(live=...)``, ``csrc/attention_head.hip``) over the range they are compiled for -- 65 ... 80 tokens, either
head_dim padding, a padded head_dim, both scale modes, both layouts, the masked-tile skip on and off -- with live lengths on every
16-row strip boundary and ``eot`` values outside ``[0, N)``:

  (a) against the dense kernels on operands whose dead rows are zeros, bit for bit;
  (b) against ``torch_attention`` of ``tests/test_gpu_ops.py`` in float64 on the same zeroed operands (autograd for the gradients), under
      the comparator and tolerances ``test_attn_capture_fwd_bwd`` has for these kernels;
  (c) with the lengths handed over as int32 and as a non-contiguous view: the same bits.

Then what the route must turn down (an error, nothing launched), and towers of 65 and 80 tokens with head_dim 64 and 16."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

from parity import close  # noqa: E402
from test_gpu_ops import torch_attention  # noqa: E402
from test_gpu_text_attention_live_rows import captions, run_tower  # noqa: E402

H = 2
SENTINEL, SENTINEL_SLAB = 7.25, -3.5
NS, DS = (65, 72, 77, 80), (4, 20, 32, 36, 64)
VARIANT_SHAPES = ((77, 20), (80, 64), (65, 48))
# (N, D, scale_mode, layout, tile_skip): the full cross in the tower's own form, then one departure from it at a time
CASES = [(n, d, 0, "bnhd", 1) for n in NS for d in DS]
CASES += [(n, d, 1, "bnhd", 1) for n, d in VARIANT_SHAPES]
CASES += [(n, d, 0, "bhnd", 1) for n, d in VARIANT_SHAPES]
CASES += [(n, d, 0, "bnhd", 0) for n, d in VARIANT_SHAPES]


@pytest.fixture
def options():
    """``options(key=value, ...)`` sets process-wide switches; every one this suite touches is back at its default afterwards."""
    from transformer_mm_explainability_amd import ops

    def set_options(**kw):
        for key, value in kw.items():
            ops.set_option(key, value)
    yield set_options
    set_options(text_live_rows=1, text_live_rows_fwd=1, text_live_attn=1, attn_head_tile_skip=1, gemm_rows_tm=32, gemm_rows_tn=0)
    ops.LiveRows.poison = False


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def causal_mask(n):
    return torch.full((n, n), float("-inf"), device="cuda").triu_(1)


def eot_values(n):
    """Live lengths 1, one row either side of every strip boundary (16, 32, 48, 64), one that ends on the fifth tile's first row
    (eot 64), the last two rows, and values the kernels must clamp; a value that two entries share (65 tokens) is kept once."""
    out = []
    for e in [0, 15, 16, 31, 32, 47, 48, 63, 64, n - 2, n - 1, -3, n, n + 1000, 2 ** 40]:
        if e not in out:
            out.append(e)
    return out


def bhnd(t, layout):
    """``[B, H, N, D]`` view of an operand in its layout."""
    return t.permute(0, 2, 1, 3) if layout == "bnhd" else t


def by_head(name, t, layout):
    """A result with ``[B, H, N]`` in front: the slabs are that already, ``O dq dk dv`` come in the operands' layout."""
    return t if name in ("P", "dP") else bhnd(t, layout)


_CASES = {}


def case(N, D, mode, layout):
    """Operands and references of one shape, made once and never modified: ``q k v dO`` with zeros in the dead rows and with NaN there,
    the dense kernels' ``P O dP dq dk dv`` on the zeroed ones, and the float64 reference of the same zeroed problem (CPU)."""
    key = (N, D, mode, layout)
    if key in _CASES:
        return _CASES[key]
    from transformer_mm_explainability_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1000 * N + 10 * D + mode)
    eot_list = eot_values(N)
    B = len(eot_list)
    lengths = [min(max(e, 0), N - 1) + 1 for e in eot_list]                               # the definition: clamp(eot, 0, N - 1) + 1
    eot = torch.tensor(eot_list, device="cuda")
    dead = torch.arange(N, device="cuda")[None, :] >= torch.tensor(lengths, device="cuda")[:, None]      # [B, N]
    dead_bhn = dead[:, None, :].expand(B, H, N)
    qkv = torch.randn(B, N, 3, H, D, device="cuda", generator=g)
    d_o = torch.randn(B, N, H, D, device="cuda", generator=g)
    scale = D ** -0.5 if mode == 0 else D ** 0.5
    mask = causal_mask(N)

    def operands(fill):
        packed, grad = qkv.clone(), d_o.clone()
        packed[dead], grad[dead] = fill, fill
        if layout == "bnhd":                                                             # views of one packed tensor, as a tower has them
            return packed[:, :, 0], packed[:, :, 1], packed[:, :, 2], grad
        return tuple(t.permute(0, 2, 1, 3).contiguous() for t in (packed[:, :, 0], packed[:, :, 1], packed[:, :, 2], grad))

    zeroed, poisoned = operands(0.0), operands(float("nan"))
    q, k, v, go = zeroed
    assert ops.attn_live_shape(N, D) and ops.head_kernel_shape(N, N, D)
    probs = torch.full((B, H, N, N), SENTINEL, device="cuda")
    o = ops.attn_capture_fwd(q, k, v, probs, scale, mode, mask, layout=layout)
    dprobs = torch.full((B, H, N, N), SENTINEL, device="cuda")
    dqkv = ops.attn_capture_bwd(q, k, v, probs, go, dprobs, scale, mode, need_dqkv=True, layout=layout)
    # float64, CPU
    qr, kr, vr = (bhnd(t, layout).cpu().double().requires_grad_(True) for t in (q, k, v))
    p_ref, o_ref = torch_attention(qr, kr, vr, scale, mode, mask.cpu())
    p_ref.retain_grad()
    (o_ref * bhnd(go, layout).cpu().double()).sum().backward()
    ref = dict(P=p_ref.detach(), O=o_ref.detach(), dP=p_ref.grad, dq=qr.grad, dk=kr.grad, dv=vr.grad)
    o_poisoned = o.clone()
    bhnd(o_poisoned, layout)[dead_bhn] = float("nan")
    _CASES[key] = dict(N=N, D=D, B=B, mode=mode, layout=layout, scale=scale, mask=mask, eot=eot, eot_list=eot_list, lengths=lengths,
                       dead_bhn=dead_bhn, poisoned=poisoned, o_poisoned=o_poisoned, ref=ref,
                       dense=dict(P=probs, O=o, dP=dprobs, dq=dqkv[0], dk=dqkv[1], dv=dqkv[2]))
    return _CASES[key]


def run_live(c, live, need_dqkv=True):
    """Forward and backward with ``live=`` on the poisoned operands, every output pre-filled with a sentinel."""
    from transformer_mm_explainability_amd import ops
    B, N, D, layout = c["B"], c["N"], c["D"], c["layout"]
    q, k, v, go = c["poisoned"]
    probs = torch.full((B, H, N, N), SENTINEL_SLAB, device="cuda")
    out = torch.full(tuple(go.shape), SENTINEL, device="cuda")
    o = ops.attn_capture_fwd(q, k, v, probs, c["scale"], c["mode"], c["mask"], layout=layout, live=live, out=out)
    assert o is out
    dprobs = torch.full((B, H, N, N), SENTINEL_SLAB, device="cuda")
    if layout == "bnhd":                                                                 # views of one packed tensor, as a tower has them
        dqkv = torch.full((B, N, 3, H, D), SENTINEL, device="cuda")
        outs = (dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2])
    else:
        outs = tuple(torch.full((B, H, N, D), SENTINEL, device="cuda") for _ in range(3))
    res = ops.attn_capture_bwd(q, k, v, probs, go, dprobs, c["scale"], c["mode"], need_dqkv=need_dqkv, layout=layout,
                               out=outs if need_dqkv else None, o=c["o_poisoned"], live=live)
    if need_dqkv:
        assert all(a is b for a, b in zip(res, outs))
    else:
        assert res == (None, None, None)
    return dict(P=probs, O=o, dP=dprobs, dq=outs[0], dk=outs[1], dv=outs[2])


def check_bits(c, r, need_dqkv=True, what=""):
    """(a): the dense kernels' bits wherever the live kernels write, the sentinel wherever they do not, the filler of the dead rows."""
    N, layout, dead = c["N"], c["layout"], c["dead_bhn"]
    want = c["dense"]
    for name in ("P", "dP"):
        assert not bool(torch.isnan(r[name]).any()), (name, what)
        assert same_bits(r[name], want[name]), (name, what)
    assert bool((r["dP"][dead] == 0).all()), ("dead rows of dP", what)
    # dead rows of P: the softmax of zero scores under the mask, 1 / (i + 1) on j <= i and exact zeros beyond
    i = torch.arange(N, device="cuda")
    filler = (i[None, :] <= i[:, None]).float() / (i[:, None] + 1).float()
    got = r["P"][dead]
    row = i[None, None, :].expand_as(dead)[dead]
    assert got.shape[0] == sum(N - ln for ln in c["lengths"]) * H
    assert torch.allclose(got, filler[row], rtol=1e-6, atol=0), ("dead rows of P", what)
    assert bool((got[filler[row] == 0] == 0).all()), ("dead rows of P above the diagonal", what)
    for name in ("O", "dq", "dk", "dv"):
        got, ref = bhnd(r[name], layout), bhnd(want[name], layout)
        if name != "O" and not need_dqkv:
            assert bool((got == SENTINEL).all()), (name, what)
            continue
        assert not bool(torch.isnan(got).any()), (name, what)
        assert same_bits(got[~dead], ref[~dead]), (name, what)
        assert bool((got[dead] == SENTINEL).all()), (name + " dead rows", what)


def check_fp64(c, r, what):
    """(b): every value the live kernels write against float64, with ``test_attn_capture_fwd_bwd``'s comparator (elementwise
    ``atol + 1e-5 |ref|`` and the largest error below 1e-4 of the largest reference entry) and its tolerances."""
    layout, live = c["layout"], ~c["dead_bhn"].cpu()
    for name, atol in (("P", 2e-6), ("O", 1e-5), ("dP", 2e-5), ("dq", 2e-5), ("dk", 2e-5), ("dv", 2e-5)):
        got, ref = by_head(name, r[name], layout).cpu(), c["ref"][name].float()
        if name not in ("P", "dP"):
            got, ref = got[live], ref[live]
        close(got, ref.numpy(), atol=atol, rtol=1e-5, what="%s %s" % (name, what), rel_always=True)


def eot_forms(c):
    """(c): the lengths as int32 (2^40 does not fit: 2^31 - 1 clamps to the same length) and as a view with stride 2."""
    as_i32 = torch.tensor([min(e, 2 ** 31 - 1) for e in c["eot_list"]], dtype=torch.int32, device="cuda")
    strided = torch.stack([c["eot"], c["eot"] + 1], dim=1)[:, 0]
    assert not strided.is_contiguous()
    return (("int32", as_i32), ("strided", strided))


@pytest.mark.parametrize("N,D,mode,layout,tile_skip", CASES,
                         ids=["N%d-D%d-mode%d-%s-skip%d" % c for c in CASES])
def test_live_attention_over_the_instantiated_range(options, N, D, mode, layout, tile_skip):
    """One shape of the live kernels: (a), (b) and (c) of the module's docstring, forward and backward, ``need_dqkv`` True and False.
    ``tile_skip = 0``: the dense reference stays the one with the skip on, and the live run with the skip on is repeated next to it."""
    from transformer_mm_explainability_amd import ops
    c = case(N, D, mode, layout)
    what = "N%d D%d mode%d %s skip%d" % (N, D, mode, layout, tile_skip)
    live = ops.live_rows(c["eot"], N)
    # the list's own clamp against the lengths used here
    count = int(live.count.item())
    assert count == sum(c["lengths"])
    per_sample = torch.bincount(live.rows[:count].long() // N, minlength=c["B"])
    assert per_sample.tolist() == c["lengths"]
    assert live.eot.dtype == torch.long and live.eot.is_contiguous()

    options(attn_head_tile_skip=tile_skip)
    r = run_live(c, live)
    check_bits(c, r, what=what)
    check_fp64(c, r, what)
    lowest = run_live(c, live, need_dqkv=False)
    check_bits(c, lowest, need_dqkv=False, what=what + " dP only")
    assert same_bits(lowest["dP"], r["dP"])
    if not tile_skip:
        options(attn_head_tile_skip=1)
        skipping = run_live(c, live)
        for name in r:
            assert same_bits(by_head(name, r[name], layout), by_head(name, skipping[name], layout)), (name, what)
        options(attn_head_tile_skip=0)
    for form, eot in eot_forms(c):
        other = ops.live_rows(eot, N)
        assert other.eot.dtype == torch.long and other.eot.is_contiguous()
        assert int(other.count.item()) == count and torch.equal(other.rows[:count], live.rows[:count]), form
        again = run_live(c, other)
        for name in r:
            assert same_bits(by_head(name, r[name], layout), by_head(name, again[name], layout)), (name, form, what)


# ---------------------------------------------------------------------------------------------------------------- refusals

def plain_operands(B, N, D, seed=3):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(B, N, H, D, device="cuda", generator=g) for _ in range(4)]


def refused(q, k, v, d_o, live, N, D, match="live"):
    """Forward and backward with ``live=`` raise and launch nothing: the slabs and outputs keep their sentinel."""
    from transformer_mm_explainability_amd import ops
    B = q.shape[0]
    probs = torch.full((B, H, N, N), SENTINEL_SLAB, device="cuda")
    out = torch.full((B, N, H, D), SENTINEL, device="cuda")
    with pytest.raises(ops.MMXError, match=match):
        ops.attn_capture_fwd(q, k, v, probs, D ** -0.5, 0, causal_mask(N), live=live, out=out)
    torch.cuda.synchronize()
    assert bool((probs == SENTINEL_SLAB).all()) and bool((out == SENTINEL).all())
    given = torch.softmax(torch.randn(B, H, N, N, device="cuda") + causal_mask(N), dim=-1)
    dqkv = torch.full((B, N, 3, H, D), SENTINEL, device="cuda")
    with pytest.raises(ops.MMXError, match=match):
        ops.attn_capture_bwd(q, k, v, given, d_o, probs, D ** -0.5, 0, need_dqkv=True, out=(dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]),
                             live=live)
    torch.cuda.synchronize()
    assert bool((probs == SENTINEL_SLAB).all()) and bool((dqkv == SENTINEL).all())


def test_an_operand_off_a_16_byte_boundary_is_an_error_not_a_dense_run(options):
    """``q`` as a view that starts one float into a larger buffer: the whole-head kernels cannot load it 16 bytes at a time, and no
    other kernel knows the lengths."""
    from transformer_mm_explainability_amd import ops
    B, N, D = 3, 77, 64
    q, k, v, d_o = plain_operands(B, N, D)
    buf = torch.zeros(q.numel() + 4, device="cuda")
    off = buf[1:1 + q.numel()].view(B, N, H, D)
    off.copy_(q)
    assert off.data_ptr() % 16 == 4
    live = ops.live_rows(torch.tensor([5, 76, 40], device="cuda"), N)
    refused(off, k, v, d_o, live, N, D)
    # the same call on the aligned tensor is served
    probs = torch.empty(B, H, N, N, device="cuda")
    ops.attn_capture_fwd(q, k, v, probs, D ** -0.5, 0, causal_mask(N), live=live)


@pytest.mark.parametrize("N,D", [(64, 64), (81, 64), (77, 6)])
def test_a_shape_outside_the_instantiated_range_is_an_error(options, N, D):
    from transformer_mm_explainability_amd import ops
    assert not ops.attn_live_shape(N, D)
    q, k, v, d_o = plain_operands(2, N, D)
    live = ops.live_rows(torch.tensor([5, N - 1], device="cuda"), N)
    refused(q, k, v, d_o, live, N, D)


def test_the_wrappers_turn_down_what_the_live_kernels_do_not_do(options):
    """``mma_bf16``, no mask, a bf16 ``d_o``, ``rel_row=`` and a shared forward (``batch=`` other than B) next to ``live=``."""
    from transformer_mm_explainability_amd import ops
    B, N, D = 2, 77, 32
    q, k, v, d_o = plain_operands(B, N, D)
    live = ops.live_rows(torch.tensor([5, 60], device="cuda"), N)
    mask, scale = causal_mask(N), D ** -0.5
    probs = torch.full((B, H, N, N), SENTINEL_SLAB, device="cuda")
    with pytest.raises(ops.MMXError, match="live"):
        ops.attn_capture_fwd(q, k, v, probs, scale, 0, mask, mma_bf16=True, live=live)
    with pytest.raises(ops.MMXError, match="live"):
        ops.attn_capture_fwd(q, k, v, probs, scale, 0, None, live=live)
    assert bool((probs == SENTINEL_SLAB).all())
    ops.attn_capture_fwd(q, k, v, probs, scale, 0, mask, live=live)
    dprobs = torch.full((B, H, N, N), SENTINEL_SLAB, device="cuda")
    for kw in (dict(mma_bf16=True), dict(rel_row=torch.ones(B, N, device="cuda")), dict(batch=B + 1)):
        with pytest.raises(ops.MMXError, match="live"):
            ops.attn_capture_bwd(q, k, v, probs, d_o, dprobs, scale, 0, live=live, **kw)
    with pytest.raises(ops.MMXError, match="live"):
        ops.attn_capture_bwd(q, k, v, probs, d_o.bfloat16(), dprobs, scale, 0, live=live)
    torch.cuda.synchronize()
    assert bool((dprobs == SENTINEL_SLAB).all())
    ops.attn_capture_bwd(q, k, v, probs, d_o, dprobs, scale, 0, live=live, batch=B)     # the batch itself is no shared forward


# ---------------------------------------------------------------------------------------------------------------- tower level

_TOWER = {}


def small_clip(golden, context, heads):
    """The golden tiny configuration at another context length and head count (width 64: head_dim 64 with one head, 16 with four),
    random weights, captions whose lengths sit on and around the 16-row strips, and the CPU oracle's maps.  Once per pair."""
    if (context, heads) not in _TOWER:
        from oracle import clip_torch
        from transformer_mm_explainability_amd import clip_model
        g = golden("clip_tiny")
        cfg = dict(json.loads(str(g["cfg_json"])), context_length=context, transformer_heads=heads)
        torch.manual_seed(41)
        model = clip_model.CLIP(**cfg).float().eval()
        image = torch.from_numpy(g["image"])
        lengths = [n for n in (2, 16, 17, 32, 33, 48, 49, 64, 65, context) if n <= context]
        texts = captions(lengths, context, cfg["vocab_size"], seed=42)
        sd = clip_torch.prepare_state_dict(model.state_dict(), heads)
        _TOWER[(context, heads)] = (cfg, model.cuda(), image.cuda(), texts.cuda(), clip_torch.interpret(sd, image, texts, 0, 0))
    return _TOWER[(context, heads)]


@pytest.mark.parametrize("heads", [1, 4], ids=["head_dim64", "head_dim16"])
@pytest.mark.parametrize("context", [65, 80])
def test_tower_at_the_ends_of_the_range_equals_the_zero_filled_dense_attention(golden, options, context, heads):
    """Default options against ``text_live_attn = 0`` (dense attention over a zero-filled ``qkv``): maps and raw slabs bit for bit; both
    against the CPU oracle under the 1e-5 contract of ``parity.close``."""
    from transformer_mm_explainability_amd import ops
    cfg, model, image, texts, (want_text, want_image) = small_clip(golden, context, heads)
    assert ops.attn_live_shape(context, cfg["transformer_width"] // heads)
    options(text_live_attn=0)
    filled = run_tower(model, image, texts)
    options(text_live_attn=1)
    live = run_tower(model, image, texts)
    assert filled["pending"] and live["pending"]
    for key in ("R_text", "R_image", "raw_probs", "raw_grads"):
        assert not bool(torch.isnan(live[key]).any()), key
        assert torch.equal(live[key], filled[key]), key
    for name, run in (("live", live), ("zero-filled dense", filled)):
        close(run["R_text"], want_text.numpy(), what="R_text %s attention" % name)
        close(run["R_image"], want_image.numpy(), what="R_image %s attention" % name)
