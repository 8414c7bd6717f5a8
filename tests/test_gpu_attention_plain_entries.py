"""-m gpu: ``mmx_attn_capture_fwd`` and ``mmx_attn_capture_bwd``, the two attention entries ``ops.py`` never calls (it uses the
``_ex`` forms), through ctypes with data: P, O, dP, dq, dk and dv must be bit-equal to the ``_ex`` entries with ``MMX_F32`` and no
forward-output hint -- the header's definition of the two.  (The ``_ex`` values themselves are pinned by
``tests/test_gpu_attention_f32.py``.)  B = 2, H = 2 at the smallest shape of each dispatch route."""
import pytest
import torch

pytestmark = pytest.mark.gpu

ROUTES = [("whole-head", 5, 8),         # short sequence
          ("streaming", 130, 8),        # long sequence
          ("tiled", 130, 6)]            # D % 4 != 0 is declined by both the whole-head and the streaming kernels


def same_bits(a, b):
    return a.shape == b.shape and bool((a.reshape(-1).view(torch.int32) == b.reshape(-1).view(torch.int32)).all())


@pytest.mark.parametrize("route,N,D", ROUTES, ids=[r[0] for r in ROUTES])
def test_plain_entries_are_the_ex_entries_with_f32(route, N, D):
    from transformer_mm_explainability_amd import _lib, ops
    lib, p, B, H = _lib.lib(), ops._p, 2, 2
    gen = torch.Generator().manual_seed(N * 64 + D)
    q, k, v, d_o = (torch.randn(B, N, H, D, generator=gen).cuda() for _ in range(4))
    strides = (N * H * D, D, H * D)                                 # bnhd: batch, head, token
    qkv = (p(q), p(k), p(v)) + strides * 3
    dims = (B, H, N, N, D, float(D) ** -0.5, _lib.SCALE_Q_FIRST)
    stream = ops._stream()

    def nan(*shape):
        return torch.full(shape, float("nan"), device="cuda")
    P, O, P_ex, O_ex = nan(B, H, N, N), nan(B, N, H, D), nan(B, H, N, N), nan(B, N, H, D)
    _lib.check(lib.mmx_attn_capture_fwd(*qkv, None, 0, 0, p(P), p(O), *strides, *dims, stream), "mmx_attn_capture_fwd")
    _lib.check(lib.mmx_attn_capture_fwd_ex(*qkv, None, 0, 0, p(P_ex), _lib.MMX_F32, p(O_ex), *strides, *dims, stream),
               "mmx_attn_capture_fwd_ex")
    assert not torch.isnan(P_ex).any() and not torch.isnan(O_ex).any()
    assert same_bits(P, P_ex) and same_bits(O, O_ex)

    need = lib.mmx_attn_capture_bwd_workspace_bytes(B, H, N)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    got, want = ([nan(B, H, N, N)] + [nan(B, N, H, D) for _ in range(3)] for _ in range(2))
    grads = lambda t: tuple(p(x) for x in t) + strides * 3          # noqa: E731
    _lib.check(lib.mmx_attn_capture_bwd(*qkv, p(P_ex), H * N * N, p(d_o), *strides, *grads(got), *dims, 1, p(ws), need, stream),
               "mmx_attn_capture_bwd")
    _lib.check(lib.mmx_attn_capture_bwd_ex(*qkv, p(P_ex), H * N * N, _lib.MMX_F32, p(d_o), *strides, None, 0, 0, 0, *grads(want), *dims,
                                           1, p(ws), need, stream), "mmx_attn_capture_bwd_ex")
    torch.cuda.synchronize()
    for name, a, b in zip(("dP", "dq", "dk", "dv"), got, want):
        assert not torch.isnan(b).any(), name
        assert same_bits(a, b), name
