"""-m gpu: the fused CLIP similarity head (``ops.clip_head_grads`` / ``mmx_clip_head_f32``) at op level.

The kernel gives the gradients of ``sum_b logits_per_image[b, b]`` (CLIP_explainability.ipynb cell 6:6-10) with respect to both
un-normalised features in closed form: ``d_img[b] = s (t^ - c i^) / |i|``, ``d_txt[b] = s (i^ - c t^) / |t|``.

Reference: float64 autograd over ``CLIP.logits`` on the same fp32 inputs with ``eye`` as the upstream gradient.
Bound per element: ``2 (D + 16) 2^-24 s / |i|`` (``|t_b|`` for ``d_txt``): ``c`` is a D-term dot product of unit vectors (gamma_D), plus
the three normalisations and the final combine; every element of the result is at most ``2 s / |i|`` in magnitude.  The fp32
autograd path and an fp32 closed form stay below 0.02 of this bound on the CPU for every case here, so the reference alone is far
inside it and a wrong term is ten thousand times outside."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

LOGIT_SCALE = math.log(100.0)
# (B, Bi, img_group, D, feature scale)
CASES = [(1, 1, 1, 4, 1.0), (2, 1, 1, 20, 1e3), (3, 3, 1, 64, 1e-3), (6, 3, 2, 36, 1.0), (65, 65, 1, 100, 7.0), (64, 1, 1, 512, 1.0),
         (5, 1, 1, 1028, 30.0)]
GUARD = 64


@pytest.fixture(scope="module")
def ops():
    from transformer_mm_explainability_amd import ops as _ops
    return _ops


def _features(B, Bi, D, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Bi, D, generator=g) * scale, torch.randn(B, D, generator=g) * scale


def _pair_rows(img, B, Bi, img_group):
    """Image row of every pair: row 0 when there is one image, else ``b // img_group``."""
    idx = torch.zeros(B, dtype=torch.long) if Bi == 1 else torch.arange(B) // img_group
    return img[idx]


def _reference(img, txt, B, Bi, img_group, logit_scale):
    """float64 autograd over ``CLIP.logits`` (CLIP/clip/model.py:369-378), upstream gradient ``eye`` -> (d_img, d_txt, diag), float64."""
    from transformer_mm_explainability_amd import clip_model

    class _Scale:
        pass
    holder = _Scale()
    holder.logit_scale = torch.tensor(logit_scale, dtype=torch.float64)
    i = _pair_rows(img, B, Bi, img_group).double().requires_grad_(True)
    t = txt.double().requires_grad_(True)
    logits_per_image, _ = clip_model.CLIP.logits(holder, i, t)
    torch.autograd.backward(logits_per_image, grad_tensors=torch.eye(B, dtype=torch.float64), inputs=[i, t])
    return i.grad, t.grad, logits_per_image.detach().diagonal()


@pytest.fixture(scope="module")
def references():
    """The float64 references, computed once and shared."""
    out = {}
    for n, (B, Bi, group, D, scale) in enumerate(CASES):
        img, txt = _features(B, Bi, D, scale, 100 + n)
        out[(B, Bi, group, D, scale)] = (img, txt) + _reference(img, txt, B, Bi, group, LOGIT_SCALE)
    return out


def _ratios(got_img, got_txt, ref_img, ref_txt, img, txt, B, Bi, group, D, s):
    unit = 2.0 * (D + 16) * 2.0 ** -24 * s
    bound_img = unit / _pair_rows(img, B, Bi, group).double().norm(dim=-1, keepdim=True)
    bound_txt = unit / txt.double().norm(dim=-1, keepdim=True)
    r_img = ((got_img.double().cpu() - ref_img).abs() / bound_img).max().item()
    r_txt = ((got_txt.double().cpu() - ref_txt).abs() / bound_txt).max().item()
    return r_img, r_txt


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d_Bi%d_g%d_D%d_x%g" % c)
def test_gradients_against_float64_autograd(ops, references, case):
    B, Bi, group, D, scale = case
    img, txt, ref_img, ref_txt, ref_diag = references[case]
    ls = torch.tensor(LOGIT_SCALE, dtype=torch.float32).cuda()
    d_img, d_txt, diag = ops.clip_head_grads(img.cuda(), txt.cuda(), ls, group, want_diag=True)
    assert d_img.shape == (B, D) and d_txt.shape == (B, D) and diag.shape == (B,)
    r_img, r_txt = _ratios(d_img, d_txt, ref_img, ref_txt, img, txt, B, Bi, group, D, math.exp(LOGIT_SCALE))
    print("clip_head %s: error / bound  d_img %.4f  d_txt %.4f" % (case, r_img, r_txt))
    assert r_img <= 1.0 and r_txt <= 1.0, (case, r_img, r_txt)
    # the diagonal logit: |s c| <= s, the same D-term dot product
    assert ((diag.double().cpu() - ref_diag).abs().max().item()) <= 2.0 * (D + 16) * 2.0 ** -24 * math.exp(LOGIT_SCALE)


def test_exact_case_bit_for_bit(ops):
    """``logit_scale = 0``, one shared image ``2 e_0``, ``txt[b] = 4 e_(b mod D)``: every operation is exact."""
    B, D = 10, 8
    img = torch.zeros(1, D)
    img[0, 0] = 2.0
    txt = torch.zeros(B, D)
    want_img, want_txt = torch.zeros(B, D), torch.zeros(B, D)
    for b in range(B):
        j = b % D
        txt[b, j] = 4.0
        if j != 0:
            want_img[b, j] = 0.5
            want_txt[b, 0] = 0.25
    d_img, d_txt, diag = ops.clip_head_grads(img.cuda(), txt.cuda(), torch.zeros((), dtype=torch.float32).cuda(), want_diag=True)
    assert torch.equal(d_img.cpu(), want_img)
    assert torch.equal(d_txt.cpu(), want_txt)
    assert torch.equal(diag.cpu(), (torch.arange(B) % D == 0).float())


def test_null_outputs_and_the_diagonal(ops, references):
    case = CASES[3]
    img, txt = references[case][:2]
    ic, tc, ls = img.cuda(), txt.cuda(), torch.tensor(LOGIT_SCALE, dtype=torch.float32).cuda()
    d_img, d_txt, diag = ops.clip_head_grads(ic, tc, ls, case[2], want_diag=True)
    only_img = ops.clip_head_grads(ic, tc, ls, case[2], want_txt=False)
    only_txt = ops.clip_head_grads(ic, tc, ls, case[2], want_img=False)
    only_diag = ops.clip_head_grads(ic, tc, ls, case[2], want_img=False, want_txt=False, want_diag=True)
    assert only_img[1] is None and only_img[2] is None and torch.equal(only_img[0], d_img)
    assert only_txt[0] is None and only_txt[2] is None and torch.equal(only_txt[1], d_txt)
    assert only_diag[0] is None and only_diag[1] is None and torch.equal(only_diag[2], diag)


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[4], CASES[6]], ids=lambda c: "B%d_Bi%d_g%d_D%d_x%g" % c)
def test_nothing_is_written_outside_the_outputs(ops, references, case):
    """Sentinel-filled outputs with a guard band behind each: the band keeps the sentinel, the outputs are fully written."""
    import ctypes as C
    from transformer_mm_explainability_amd import _lib
    B, Bi, group, D, _ = case
    img, txt = references[case][:2]
    ic, tc, ls = img.cuda(), txt.cuda(), torch.tensor(LOGIT_SCALE, dtype=torch.float32).cuda()
    sentinel = -12345.0
    bufs = [torch.full((n + GUARD,), sentinel, dtype=torch.float32, device="cuda") for n in (B * D, B * D, B)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib().mmx_clip_head_f32(*[C.c_void_p(t.data_ptr()) for t in (ic, tc, ls)], *[C.c_void_p(t.data_ptr()) for t in bufs],
                                      B, D, Bi, group, stream)
    assert rc == 0
    torch.cuda.synchronize()
    want = ops.clip_head_grads(ic, tc, ls, group, want_diag=True)
    for buf, n, ref in zip(bufs, (B * D, B * D, B), want):
        assert torch.equal(buf[n:], torch.full((GUARD,), sentinel, device="cuda"))
        assert torch.equal(buf[:n], ref.reshape(-1))
        assert not (buf[:n] == sentinel).any()


def test_two_runs_are_bit_equal(ops, references):
    for case in (CASES[4], CASES[5], CASES[6]):
        img, txt = references[case][:2]
        ic, tc, ls = img.cuda(), txt.cuda(), torch.tensor(LOGIT_SCALE, dtype=torch.float32).cuda()
        a = ops.clip_head_grads(ic, tc, ls, case[2], want_diag=True)
        b = ops.clip_head_grads(ic, tc, ls, case[2], want_diag=True)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_a_captured_graph_replayed_with_new_features_equals_eager(ops):
    B, D = 6, 36
    g = torch.Generator().manual_seed(7)
    img, txt = torch.randn(3, D, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()
    ls = torch.tensor(LOGIT_SCALE, dtype=torch.float32).cuda()
    ops.clip_head_grads(img, txt, ls, 2, want_diag=True)                  # warm-up: the library is loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with ops.graph_capture(graph):
        outs = ops.clip_head_grads(img, txt, ls, 2, want_diag=True)
    for seed in (8, 9):
        g = torch.Generator().manual_seed(seed)
        img.copy_(torch.randn(3, D, generator=g) * 3)
        txt.copy_(torch.randn(B, D, generator=g) * 0.5)
        ls.fill_(LOGIT_SCALE - 0.25 * seed)                                # the scale is read on the device at every replay
        graph.replay()
        eager = ops.clip_head_grads(img, txt, ls, 2, want_diag=True)
        torch.cuda.synchronize()
        for x, y in zip(outs, eager):
            assert torch.equal(x, y)
