// Relevancy-propagation kernels for gfx950 (MI355X): rule 5 head reduction, exact-fp32 MFMA batched matmul, eq. 8-9 normalisation,
// the chain on vectors, the bimodal rules 10 / 11, rollout.  (The self-attention chain, rules 5 + 6: relevancy_chain.hip.)
//
// Reference sites replaced by each kernel are cited in include/mmx_relevancy.h; DESIGN.md has the
// layouts, the algorithmic-byte model and the roofline each kernel is bound by.
#include "mmx_common.h"

#include <type_traits>

namespace mmx {

// =====================================================================================================
// K_avg_heads: A_bar[b] = (1/H) sum_h clamp(G[b,h] * A[b,h], 0).   Pure HBM stream: A and G read once.
// grid = (ceil(NN/4 / 256), B), block 256; thread owns 4 consecutive positions and walks the heads in
// order (deterministic, same summation order as a sequential mean over dim h).
// =====================================================================================================
// R16: the reference's half-precision chain (notebook cell 6:20,43 with an fp16 model): the product grad * attn and the head mean
// are each rounded to fp16 (round_f16).
template <int DT, bool R16 = false>
__global__ __launch_bounds__(256) void avg_heads_kernel(const void* __restrict__ attn,
                                                        const void* __restrict__ grad,
                                                        float* __restrict__ out, int H, int64_t NN,
                                                        int64_t attn_bstride) {
    const int b = blockIdx.y;
    const int64_t p = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 4;
    if (p >= NN) return;
    const int64_t base = static_cast<int64_t>(b) * H * NN + p;
    const int64_t base_a = static_cast<int64_t>(b) * attn_bstride + p;   // attn_bstride = 0: one forward shared by the batch
    const float fH = static_cast<float>(H);
    // fast path: one aligned load per (head, array).  16-bit slabs of odd N^2 start every second head on a 2-byte
    // boundary; load4_stream fetches the three aligned dwords around the chunk instead of four 2-byte loads (it
    // over-reads two elements, hence p + 5 < NN; the last chunk of a slab takes the element-wise path)
    if (p + 5 < NN) {
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int h = 0; h < H; ++h) {
            const f32x4 a = load4_stream<DT>(attn, base_a + h * NN);
            const f32x4 g = load4_stream<DT>(grad, base + h * NN);
            const f32x4 x = R16 ? round_f16(g * a) : g * a;
            s[0] += relu_nan(x[0]); s[1] += relu_nan(x[1]);
            s[2] += relu_nan(x[2]); s[3] += relu_nan(x[3]);
        }
        float* o = out + static_cast<int64_t>(b) * NN + p;
        const f32x4 m = R16 ? round_f16(s / fH) : s / fH;
        o[0] = m[0]; o[1] = m[1]; o[2] = m[2]; o[3] = m[3];
    } else {
        for (int e = 0; p + e < NN; ++e) {
            float s = 0.f;
            for (int h = 0; h < H; ++h) {
                const float x = load1_as_f32<DT>(grad, base + h * NN + e) * load1_as_f32<DT>(attn, base_a + h * NN + e);
                s += relu_nan(R16 ? round_f16(x) : x);
            }
            out[static_cast<int64_t>(b) * NN + p + e] = R16 ? round_f16(s / fH) : s / fH;
        }
    }
}

// =====================================================================================================
// K_bmm_f32: C[b] = (Cin ? Cin[b] : 0) + op(A[b]) . B[b] on v_mfma_f32_16x16x4_f32 (exact fp32).
// 64x64 output tile per 256-thread workgroup (4 waves as 2x2, 32x32 each = 2x2 MFMA tiles), BK = 32.
// The next K-slab's global loads are issued into registers before the MFMAs of the current one (the problems here
// are small -- rule 10 at DETR size is [100 x 950] . [950 x 950] = 30 workgroups -- so the loop is latency-, not
// bandwidth-bound, and a workgroup has to cover its own load latency).  LDS tiles are k-major with row stride 80
// floats: a wave's ds_read_b32 of [k = lane>>4][m = lane&15] hits 32 distinct banks per half-wave.  Guarded scalar
// global loads: any M, N, K, any alignment.
// =====================================================================================================
constexpr int kBmmBK = 32;

// T x T output tile per 256-thread workgroup, 4 waves as 2 x 2, each (T/2) x (T/2) = (T/32)^2 MFMA tiles.
// T = 64 for large problems; T = 32 when 64 x 64 tiles would leave most CUs with at most one workgroup (nothing to
// hide the global-load latency behind): 4x the workgroups for the same work.
template <int T>
__global__ __launch_bounds__(256) void bmm_f32_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                      const float* Cin, float* C, int M, int N, int K,
                                                      int trans_a, int64_t sa, int64_t sb, int64_t sc,
                                                      int nan_to_zero, int cin_is_row) {
    constexpr int W = T / 32;              // MFMA tiles per wave and dimension
    constexpr int E = kBmmBK * T / 256;    // elements of each operand per thread and slab
    constexpr int LA = T + 17, LB = T + 16;   // odd A stride: the k-fastest stores of a row-major A spread over the banks
    __shared__ float As[kBmmBK][LA];
    __shared__ float Bs[kBmmBK][LB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    // 1-D grid, XCD-aware: workgroups are dealt round-robin to the 8 XCDs, so in dispatch order the tiles of ONE batch entry
    // would land on all eight L2s and every one of them would fetch that entry's A and B (measured at N = 577: FETCH_SIZE
    // 2.8x the operands, profiles/r02_chain_split_roofline.txt).  xcd_contiguous_id gives each XCD one contiguous range of
    // (batch, m tile, n tile) triples: an entry's operands live in one L2.
    const int tiles_n = (N + T - 1) / T, tiles_m = (M + T - 1) / T;
    const int wg = xcd_contiguous_id(blockIdx.x, gridDim.x);
    const int bx = wg % tiles_n, by = (wg / tiles_n) % tiles_m, bz = wg / (tiles_n * tiles_m);
    const int m0 = by * T, n0 = bx * T;
    const float* Ab = A + static_cast<int64_t>(bz) * sa;
    const float* Bb = B + static_cast<int64_t>(bz) * sb;
    f32x4 acc[W][W];
#pragma unroll
    for (int i = 0; i < W; ++i)
#pragma unroll
        for (int j = 0; j < W; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    float ra[E], rb[E];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int idx = tid + e * 256;
            int m, k;
            if (trans_a) { k = idx / T; m = idx % T; } else { m = idx / kBmmBK; k = idx % kBmmBK; }
            const int gm = m0 + m, gk = k0 + k;
            const bool ok = gm < M && gk < K;
            const int64_t off = trans_a ? static_cast<int64_t>(gk) * M + gm : static_cast<int64_t>(gm) * K + gk;
            const float va = Ab[ok ? off : 0];            // unconditional (clamped) load: no per-element vmcnt(0)
            ra[e] = ok ? va : 0.f;
            const int kb = idx / T, nb = idx % T;
            const int gkb = k0 + kb, gn = n0 + nb;
            const bool okb = gkb < K && gn < N;
            const float vb = Bb[okb ? static_cast<int64_t>(gkb) * N + gn : 0];
            rb[e] = okb ? vb : 0.f;
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += kBmmBK) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int idx = tid + e * 256;
            if (trans_a) As[idx / T][idx % T] = ra[e]; else As[idx % kBmmBK][idx / kBmmBK] = ra[e];
            Bs[idx / T][idx % T] = rb[e];
        }
        lds_barrier();
        if (k0 + kBmmBK < K) fetch(k0 + kBmmBK);          // in flight across the MFMAs and the next (LDS-only) barrier
#pragma unroll
        for (int ks = 0; ks < kBmmBK / 4; ++ks) {
            const int kk = ks * 4 + (lane >> 4);
            float av[W], bv[W];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                av[i] = As[kk][wr * (T / 2) + 16 * i + (lane & 15)];
                bv[i] = Bs[kk][wc * (T / 2) + 16 * i + (lane & 15)];
            }
#pragma unroll
            for (int i = 0; i < W; ++i)
#pragma unroll
                for (int j = 0; j < W; ++j) acc[i][j] = mfma16x16x4(av[i], bv[j], acc[i][j]);
        }
        lds_barrier();
    }
    const int64_t cbase = static_cast<int64_t>(bz) * sc;
#pragma unroll
    for (int i = 0; i < W; ++i)
#pragma unroll
        for (int j = 0; j < W; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gm = m0 + wr * (T / 2) + i * 16 + (lane >> 4) * 4 + r;
                const int gn = n0 + wc * (T / 2) + j * 16 + (lane & 15);
                if (gm < M && gn < N) {
                    const int64_t off = cbase + static_cast<int64_t>(gm) * N + gn;
                    float v = acc[i][j][r];
                    if (Cin) v = (cin_is_row ? Cin[gn] : Cin[off]) + v;      // cin_is_row: a bias row shared by every row
                    if (nan_to_zero && v != v) v = 0.f;
                    C[off] = v;
                }
            }
}

static int g_bmm_tiles = 1;   // option "bmm_tiles": 1 (default) large plain products on bmm_f32_tiles.hip | 0: always the general kernel below
bool bmm_option(const char* key, int value) {
    if (strcmp(key, "bmm_tiles") == 0 && value >= 0 && value <= 1) { g_bmm_tiles = value; return true; }
    return false;
}

static void launch_bmm(const float* A, const float* B, const float* Cin, float* C, int batch, int M, int N, int K,
                       int trans_a, int64_t sa, int64_t sb, int64_t sc, int nan_to_zero, hipStream_t s, int cin_is_row = 0) {
    if (g_bmm_tiles && bmm_f32_tiles_try(A, B, Cin, C, batch, M, N, K, trans_a, sa, sb, sc, nan_to_zero, cin_is_row, s)) return;
    const int64_t wgs64 = static_cast<int64_t>((N + 63) / 64) * ((M + 63) / 64) * batch;
    // (a 128 x 128 tiling was measured SLOWER at the long-sequence chain shapes -- profiles/r02_bmm_probe.txt: 384 vs 281 us at
    // [32 x 577 x 577]^2 -- and removed in round 5)
    if (wgs64 >= 1024) {
        bmm_f32_kernel<64><<<dim3(static_cast<unsigned>(wgs64)), 256, 0, s>>>(A, B, Cin, C, M, N, K, trans_a, sa,
                                                                                    sb, sc, nan_to_zero, cin_is_row);
    } else {
        bmm_f32_kernel<32><<<dim3(static_cast<unsigned>(static_cast<int64_t>((N + 31) / 32) * ((M + 31) / 32) * batch)), 256, 0, s>>>(A, B, Cin, C, M, N, K, trans_a, sa,
                                                                                    sb, sc, nan_to_zero, cin_is_row);
    }
}

// =====================================================================================================
// Row kernels: one wave per row.
//   mode 0  handle_residual (eq. 8-9): out = (R - I)/rowsum(R - I) + I ; also min_i(R[i,i] - 1)
//   mode 1  rollout prep, normalised : out = (A + I)/rowsum(A + I)
//   mode 2  rollout prep, plain      : out = A + I
// =====================================================================================================
// A NaN must stick (the reference's ``assert diag.min() >= 0`` fails on a NaN diagonal): it is published as 0xffc00000, which the
// unsigned max keeps above every negative float and the signed min keeps below every non-negative one, whatever arrives later (a NaN
// with the sign bit clear, 0x7fc00000, would be replaced by the next non-negative value's signed min).
__device__ __forceinline__ void atomic_min_float(float* addr, float v) {
    if (v != v) atomicMax(reinterpret_cast<unsigned int*>(addr), 0xffc00000u);
    else if (v >= 0.f) atomicMin(reinterpret_cast<int*>(addr), __float_as_int(v));
    else atomicMax(reinterpret_cast<unsigned int*>(addr), __float_as_uint(v));
}

__global__ void fill_scalar_kernel(float* p, float v) { *p = v; }

__global__ __launch_bounds__(256) void row_normalise_kernel(const float* __restrict__ R, float* __restrict__ out,
                                                            int rows_total, int N, int mode, float* diag_min) {
    const int row_g = blockIdx.x * 4 + (threadIdx.x >> 6);  // global row over batch*N
    const int lane = threadIdx.x & 63;
    if (row_g >= rows_total) return;
    const int i = row_g % N;
    const float* r = R + static_cast<int64_t>(row_g) * N;
    float* o = out + static_cast<int64_t>(row_g) * N;
    const float dsub = (mode == 0) ? -1.f : 1.f;
    float s = 0.f;
    for (int j = lane; j < N; j += 64) s += r[j] + (j == i ? dsub : 0.f);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (mode == 0 && diag_min && lane == 0) atomic_min_float(diag_min, r[i] - 1.f);
    for (int j = lane; j < N; j += 64) {
        float v = r[j] + (j == i ? dsub : 0.f);
        if (mode != 2) v = v / s;
        if (mode == 0 && j == i) v += 1.f;
        o[j] = v;
    }
}

}  // namespace mmx

// =====================================================================================================
// C-ABI entry points (see include/mmx_relevancy.h)
// =====================================================================================================
using namespace mmx;

// r16: the head mean of the fp16-mode chain (mmx_relevancy_self_chain_half's long path: fp32 or fp16 slabs)
int mmx::avg_heads_launch(const void* attn_dev, const void* grad_dev, void* out_dev, int B, int H, int Nq, int Nk, int dtype,
                          int64_t attn_bstride, void* stream, bool r16) {
    MMX_CHECK_ARG(attn_dev && grad_dev && out_dev, "mmx_avg_heads: null pointer");
    MMX_CHECK_ARG(B > 0 && H > 0 && Nq > 0 && Nk > 0, "mmx_avg_heads: non-positive size B=%d H=%d Nq=%d Nk=%d", B, H, Nq, Nk);
    const int64_t NN = static_cast<int64_t>(Nq) * Nk;
    dim3 grid(static_cast<unsigned>((((NN + 3) >> 2) + 255) / 256), B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* out = static_cast<float*>(out_dev);
    void (*kern)(const void*, const void*, float*, int, int64_t, int64_t) = nullptr;
    switch (dtype) {
        case MMX_F32: kern = r16 ? avg_heads_kernel<MMX_F32, true> : avg_heads_kernel<MMX_F32>; break;
        case MMX_F16: kern = r16 ? avg_heads_kernel<MMX_F16, true> : avg_heads_kernel<MMX_F16>; break;
        case MMX_BF16: if (!r16) { kern = avg_heads_kernel<MMX_BF16>; break; }
            [[fallthrough]];
        default: set_error("mmx_avg_heads: unsupported dtype %d", dtype); return MMX_EINVAL;
    }
    kern<<<grid, 256, 0, s>>>(attn_dev, grad_dev, out, H, NN, attn_bstride);
    MMX_LAUNCH_CHECK(r16 ? "avg_heads_kernel (fp16 chain)" : "avg_heads_kernel");
    return MMX_OK;
}

extern "C" int mmx_avg_heads(const void* attn_dev, const void* grad_dev, void* out_dev, int B, int H, int Nq,
                             int Nk, int dtype, void* stream) {
    return avg_heads_launch(attn_dev, grad_dev, out_dev, B, H, Nq, Nk, dtype, static_cast<int64_t>(H) * Nq * Nk, stream);
}

extern "C" int mmx_avg_heads_ex(const void* attn_dev, const void* grad_dev, void* out_dev, int B, int H, int Nq,
                                int Nk, int dtype, int64_t attn_batch_stride, void* stream) {
    const int64_t full = static_cast<int64_t>(H) * Nq * Nk;
    if (attn_batch_stride < 0) attn_batch_stride = full;
    MMX_CHECK_ARG(attn_batch_stride == 0 || attn_batch_stride == full,
                  "mmx_avg_heads_ex: attn_batch_stride must be 0 (shared forward) or H*Nq*Nk");
    return avg_heads_launch(attn_dev, grad_dev, out_dev, B, H, Nq, Nk, dtype, attn_batch_stride, stream);
}

extern "C" int mmx_bmm_f32(const void* A_dev, const void* B_dev, const void* Cin_dev, void* C_dev, int batch, int M,
                           int N, int K, int trans_a, int64_t stride_a, int64_t stride_b, int64_t stride_c,
                           int nan_to_zero, void* stream) {
    MMX_CHECK_ARG(A_dev && B_dev && C_dev, "mmx_bmm_f32: null pointer");
    MMX_CHECK_ARG(batch > 0 && M > 0 && N > 0 && K > 0, "mmx_bmm_f32: non-positive size");
    MMX_CHECK_ARG(batch <= 65535, "mmx_bmm_f32: batch %d > 65535", batch);
    launch_bmm(static_cast<const float*>(A_dev), static_cast<const float*>(B_dev), static_cast<const float*>(Cin_dev),
               static_cast<float*>(C_dev), batch, M, N, K, trans_a, stride_a, stride_b, stride_c, nan_to_zero,
               static_cast<hipStream_t>(stream));
    MMX_LAUNCH_CHECK("bmm_f32_kernel");
    return MMX_OK;
}

extern "C" int mmx_linear_f32(const void* x_dev, const void* wt_dev, const void* bias_dev, void* out_dev, int M, int N, int K,
                              void* stream) {
    MMX_CHECK_ARG(x_dev && wt_dev && out_dev, "mmx_linear_f32: null pointer");
    MMX_CHECK_ARG(M > 0 && N > 0 && K > 0, "mmx_linear_f32: non-positive size");
    launch_bmm(static_cast<const float*>(x_dev), static_cast<const float*>(wt_dev), static_cast<const float*>(bias_dev),
               static_cast<float*>(out_dev), 1, M, N, K, 0, 0, 0, 0, 0, static_cast<hipStream_t>(stream), 1);
    MMX_LAUNCH_CHECK("bmm_f32_kernel (linear)");
    return MMX_OK;
}

static int launch_rows(const void* R, void* out, int batch, int N, int mode, float* diag_min, hipStream_t s) {
    const int rows = batch * N;
    if (diag_min) fill_scalar_kernel<<<1, 1, 0, s>>>(diag_min, __builtin_inff());
    row_normalise_kernel<<<(rows + 3) / 4, 256, 0, s>>>(static_cast<const float*>(R), static_cast<float*>(out), rows,
                                                        N, mode, diag_min);
    MMX_LAUNCH_CHECK("row_normalise_kernel");
    return MMX_OK;
}

extern "C" int mmx_handle_residual(const void* R_dev, void* out_dev, int batch, int N, void* diag_min_dev,
                                   void* stream) {
    MMX_CHECK_ARG(R_dev && out_dev, "mmx_handle_residual: null pointer");
    MMX_CHECK_ARG(batch > 0 && N > 0, "mmx_handle_residual: non-positive size");
    return launch_rows(R_dev, out_dev, batch, N, 0, static_cast<float*>(diag_min_dev),
                       static_cast<hipStream_t>(stream));
}

// ----------------------------------------------------------------------------------------- chain on vectors
// One ROW / COLUMN of the chain instead of the matrix (DETR rows-only rules, detr_explainability._rows_only_rules):
//   matvec:  out[b] = base[b] + A[b] . y[b]       (R 1 carried bottom-up: the row sums eq. 8-9 divides by)
//   vecmat:  out[b] = base[b] + x[b] . A[b]       (a row of R carried top-down)
// `base` is separate from the multiplied vector so that a caller can carry the DEVIATION from the start vector
// (e <- e + A (1 + e) for R 1 - 1, d <- d + (v + d) A for v R - v): subtracting the start vector at the end instead would
// cancel 2-3 digits, because R - I is small against I.
// A: [B, N, N] fp32 (the head-averaged map of a layer).  Both read A once: N^2 bytes instead of the 2 N^3 flops of
// R <- R + A.R.  matvec: one wave per row.  vecmat: a workgroup reduces a 32-row chunk for all columns into a partial
// row, a second pass adds the chunks in a fixed order (deterministic; no atomics).
namespace mmx {

__global__ __launch_bounds__(256) void chain_matvec_kernel(const float* __restrict__ A, const float* __restrict__ y,
                                                           const float* __restrict__ base, float* __restrict__ out,
                                                           int rows_total, int N) {
    const int row_g = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row_g >= rows_total) return;
    const int b = row_g / N;
    const float* a = A + static_cast<int64_t>(row_g) * N;
    const float* yb = y + static_cast<int64_t>(b) * N;
    float s = 0.f;
    const int n4 = N >> 2;
    for (int j = lane; j < n4; j += 64) {
        const f32x4 av = ldg4_u(a + 4 * j), yv = ldg4_u(yb + 4 * j);
        s += av[0] * yv[0] + av[1] * yv[1] + av[2] * yv[2] + av[3] * yv[3];
    }
    for (int j = 4 * n4 + lane; j < N; j += 64) s += a[j] * yb[j];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[row_g] = base[row_g] + s;
}

constexpr int kVecmatRows = 32;

__global__ __launch_bounds__(256) void chain_vecmat_partial_kernel(const float* __restrict__ A, const float* __restrict__ x,
                                                                   float* __restrict__ part, int N, int chunks) {
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int r0 = chunk * kVecmatRows, r1 = min(N, r0 + kVecmatRows);
    const float* xb = x + static_cast<int64_t>(b) * N;
    const float* Ab = A + static_cast<int64_t>(b) * N * N;
    float* pb = part + (static_cast<int64_t>(b) * chunks + chunk) * N;
    for (int c = threadIdx.x * 4; c < N; c += 256 * 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (c + 3 < N) {
            for (int r = r0; r < r1; ++r) acc += ldg4_u(Ab + static_cast<int64_t>(r) * N + c) * xb[r];
            pb[c] = acc[0]; pb[c + 1] = acc[1]; pb[c + 2] = acc[2]; pb[c + 3] = acc[3];
        } else {
            for (int e = 0; c + e < N; ++e) {
                float sacc = 0.f;
                for (int r = r0; r < r1; ++r) sacc += Ab[static_cast<int64_t>(r) * N + c + e] * xb[r];
                pb[c + e] = sacc;
            }
        }
    }
}

__global__ __launch_bounds__(256) void chain_vecmat_reduce_kernel(const float* __restrict__ part, const float* __restrict__ base,
                                                                  float* __restrict__ out, int N, int chunks) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= N) return;
    const float* pb = part + static_cast<int64_t>(b) * chunks * N + c;
    float s = 0.f;
    for (int k = 0; k < chunks; ++k) s += pb[static_cast<int64_t>(k) * N];
    out[static_cast<int64_t>(b) * N + c] = base[static_cast<int64_t>(b) * N + c] + s;
}

// One row of the chain through one layer WITHOUT materialising A_bar:  out[b] = base[b] + x[b] . mean_h clamp(G[b, h] * A[b, h], 0).
// A workgroup owns 4 rows of the slabs (wave w: row 4 chunk + w; lane: 4 consecutive columns, all heads' 2 x 16-byte loads in flight
// at once), scales its head mean by x[b, row] and the four rows meet in LDS: one [N] partial per workgroup, summed over the N / 4
// workgroups by a second small launch (in workgroup order: deterministic).  Replaces avg_heads + the two chain_vecmat launches of
// the row-vector chain (ViT-B/16 at one image: 10.7 + 17.4 + 4.9 us per layer, latency-bound at 7 workgroups).
constexpr int kAhvRows = 4;

template <int DT>
__global__ __launch_bounds__(256) void avg_heads_vecmat_partial_kernel(const void* __restrict__ attn, const void* __restrict__ grad,
                                                                       const float* __restrict__ x, float* __restrict__ part, int H,
                                                                       int N, int64_t attn_bstride, int chunks) {
    __shared__ f32x4 red[kAhvRows][64];
    const int chunk = blockIdx.x, b = blockIdx.y;
    const int rl = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = chunk * kAhvRows + rl;
    const int64_t NN = static_cast<int64_t>(N) * N;
    const int n4 = (N + 3) >> 2;
    const float fH = static_cast<float>(H);
    const float xr = row < N ? x[static_cast<int64_t>(b) * N + row] : 0.f;
    for (int cg0 = 0; cg0 < n4; cg0 += 64) {
        const int cg = cg0 + lane, c = cg * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row < N && cg < n4) {
            const int64_t p = static_cast<int64_t>(row) * N + c;
            const int64_t base_g = static_cast<int64_t>(b) * H * NN + p, base_a = static_cast<int64_t>(b) * attn_bstride + p;
            f32x4 s = {0.f, 0.f, 0.f, 0.f};
            if (c + 3 < N && p + 5 < NN) {          // a whole chunk (p + 5: the 16-bit loads over-read two elements)
#pragma unroll 4
                for (int h = 0; h < H; ++h) {
                    const f32x4 a = load4_stream<DT>(attn, base_a + h * NN);
                    const f32x4 g = load4_stream<DT>(grad, base_g + h * NN);
                    const f32x4 t = g * a;
                    s[0] += relu_nan(t[0]); s[1] += relu_nan(t[1]); s[2] += relu_nan(t[2]); s[3] += relu_nan(t[3]);
                }
            } else {
                for (int e = 0; e < 4 && c + e < N; ++e)
                    for (int h = 0; h < H; ++h)
                        s[e] += relu_nan(load1_as_f32<DT>(grad, base_g + h * NN + e) * load1_as_f32<DT>(attn, base_a + h * NN + e));
            }
            v = f32x4{s[0] / fH * xr, s[1] / fH * xr, s[2] / fH * xr, s[3] / fH * xr};
        }
        red[rl][lane] = v;
        __syncthreads();
        if (rl == 0 && cg < n4) {
            const f32x4 t = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
            *reinterpret_cast<f32x4*>(part + (static_cast<int64_t>(b) * chunks + chunk) * (n4 * 4) + c) = t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void avg_heads_vecmat_reduce_kernel(const float* __restrict__ part, const float* __restrict__ base,
                                                                      float* __restrict__ out, int N, int ld, int chunks) {
    const int c = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (c >= N) return;
    const float* pb = part + static_cast<int64_t>(b) * chunks * ld + c;
    float s = 0.f;
    for (int k = 0; k < chunks; ++k) s += pb[static_cast<int64_t>(k) * ld];
    out[static_cast<int64_t>(b) * N + c] = base[static_cast<int64_t>(b) * N + c] + s;
}

}  // namespace mmx

extern "C" size_t mmx_avg_heads_vecmat_workspace_bytes(int B, int N) {
    const size_t chunks = (static_cast<size_t>(N) + mmx::kAhvRows - 1) / mmx::kAhvRows;
    return sizeof(float) * static_cast<size_t>(B) * chunks * (((static_cast<size_t>(N) + 3) >> 2) * 4);
}

extern "C" int mmx_avg_heads_vecmat(const void* attn_dev, const void* grad_dev, const void* x_dev, const void* base_dev, void* out_dev,
                                    int B, int H, int N, int dtype, int64_t attn_batch_stride, void* workspace_dev,
                                    size_t workspace_bytes, void* stream) {
    MMX_CHECK_ARG(attn_dev && grad_dev && x_dev && base_dev && out_dev && B > 0 && H > 0 && N > 0 && B <= 65535,
                  "mmx_avg_heads_vecmat: bad argument");
    const int64_t full = static_cast<int64_t>(H) * N * N;
    if (attn_batch_stride < 0) attn_batch_stride = full;
    MMX_CHECK_ARG(attn_batch_stride == 0 || attn_batch_stride == full,
                  "mmx_avg_heads_vecmat: attn_batch_stride must be 0 (shared forward) or H*N*N");
    MMX_CHECK_ARG(x_dev != out_dev, "mmx_avg_heads_vecmat: out may not alias x");
    if (!workspace_dev || workspace_bytes < mmx_avg_heads_vecmat_workspace_bytes(B, N) ||
        (reinterpret_cast<uintptr_t>(workspace_dev) & 15u)) {
        mmx::set_error("mmx_avg_heads_vecmat: workspace %zu < %zu (or not 16-byte aligned)", workspace_bytes,
                       mmx_avg_heads_vecmat_workspace_bytes(B, N));
        return MMX_EWORKSPACE;
    }
    const int chunks = (N + mmx::kAhvRows - 1) / mmx::kAhvRows, ld = ((N + 3) >> 2) * 4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace_dev);
    const float* x = static_cast<const float*>(x_dev);
    dim3 grid(chunks, B);
    switch (dtype) {
        case MMX_F32: mmx::avg_heads_vecmat_partial_kernel<MMX_F32><<<grid, 256, 0, s>>>(attn_dev, grad_dev, x, part, H, N, attn_batch_stride, chunks); break;
        case MMX_F16: mmx::avg_heads_vecmat_partial_kernel<MMX_F16><<<grid, 256, 0, s>>>(attn_dev, grad_dev, x, part, H, N, attn_batch_stride, chunks); break;
        case MMX_BF16: mmx::avg_heads_vecmat_partial_kernel<MMX_BF16><<<grid, 256, 0, s>>>(attn_dev, grad_dev, x, part, H, N, attn_batch_stride, chunks); break;
        default: mmx::set_error("mmx_avg_heads_vecmat: unsupported dtype %d", dtype); return MMX_EINVAL;
    }
    MMX_LAUNCH_CHECK("avg_heads_vecmat_partial_kernel");
    mmx::avg_heads_vecmat_reduce_kernel<<<dim3((N + 255) / 256, B), 256, 0, s>>>(part, static_cast<const float*>(base_dev),
                                                                                 static_cast<float*>(out_dev), N, ld, chunks);
    MMX_LAUNCH_CHECK("avg_heads_vecmat_reduce_kernel");
    return MMX_OK;
}

extern "C" int mmx_chain_matvec(const void* A_dev, const void* y_dev, const void* base_dev, void* out_dev, int B, int N,
                                void* stream) {
    MMX_CHECK_ARG(A_dev && y_dev && base_dev && out_dev && B > 0 && N > 0 && y_dev != out_dev, "mmx_chain_matvec: bad argument");
    const int rows = B * N;
    mmx::chain_matvec_kernel<<<(rows + 3) / 4, 256, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const float*>(A_dev), static_cast<const float*>(y_dev), static_cast<const float*>(base_dev),
        static_cast<float*>(out_dev), rows, N);
    MMX_LAUNCH_CHECK("chain_matvec_kernel");
    return MMX_OK;
}

extern "C" size_t mmx_chain_vecmat_workspace_bytes(int B, int N) {
    const size_t chunks = (static_cast<size_t>(N) + mmx::kVecmatRows - 1) / mmx::kVecmatRows;
    return sizeof(float) * static_cast<size_t>(B) * chunks * N;
}

extern "C" int mmx_chain_vecmat(const void* A_dev, const void* x_dev, const void* base_dev, void* out_dev, int B, int N,
                                void* workspace_dev, size_t workspace_bytes, void* stream) {
    MMX_CHECK_ARG(A_dev && x_dev && base_dev && out_dev && B > 0 && N > 0, "mmx_chain_vecmat: bad argument");
    if (!workspace_dev || workspace_bytes < mmx_chain_vecmat_workspace_bytes(B, N)) {
        mmx::set_error("mmx_chain_vecmat: workspace %zu < %zu", workspace_bytes, mmx_chain_vecmat_workspace_bytes(B, N));
        return MMX_EWORKSPACE;
    }
    const int chunks = (N + mmx::kVecmatRows - 1) / mmx::kVecmatRows;
    hipStream_t s = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(workspace_dev);
    mmx::chain_vecmat_partial_kernel<<<dim3(chunks, B), 256, 0, s>>>(static_cast<const float*>(A_dev),
                                                                    static_cast<const float*>(x_dev), part, N, chunks);
    MMX_LAUNCH_CHECK("chain_vecmat_partial_kernel");
    mmx::chain_vecmat_reduce_kernel<<<dim3((N + 255) / 256, B), 256, 0, s>>>(part, static_cast<const float*>(base_dev),
                                                                             static_cast<float*>(out_dev), N, chunks);
    MMX_LAUNCH_CHECK("chain_vecmat_reduce_kernel");
    return MMX_OK;
}

// ----------------------------------------------------------------------------------------- rules 10/11
__global__ void copy_scrub_kernel(const float* __restrict__ in, float* __restrict__ out, long n, int nan_to_zero) {
    const long i = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) {
        const float v = in[i];
        out[i] = (nan_to_zero && v != v) ? 0.0f : v;
    }
}


extern "C" size_t mmx_mm_rules_workspace_bytes(int Ns, int Nq) {
    // Rn_ss [Ns,Ns] + Rn_qq [Nq,Nq] + tmp [Ns,Nq]
    return align256(sizeof(float) * Ns * Ns) + align256(sizeof(float) * Nq * Nq) + align256(sizeof(float) * Ns * Nq);
}

extern "C" int mmx_mm_attention_rules(const void* R_ss_dev, const void* R_qq_dev, const void* R_qs_dev,
                                      const void* cam_sq_dev, void* R_sq_add_dev, void* R_ss_add_dev, int Ns, int Nq,
                                      unsigned flags, void* diag_min_dev, void* workspace_dev,
                                      size_t workspace_bytes, void* stream) {
    MMX_CHECK_ARG(R_ss_dev && R_qq_dev && cam_sq_dev && R_sq_add_dev, "mmx_mm_attention_rules: null pointer");
    MMX_CHECK_ARG(Ns > 0 && Nq > 0, "mmx_mm_attention_rules: non-positive size");
    MMX_CHECK_ARG((R_qs_dev == nullptr) == (R_ss_add_dev == nullptr),
                  "mmx_mm_attention_rules: R_qs and R_ss_add must be given together (rule 11)");
    if (workspace_bytes < mmx_mm_rules_workspace_bytes(Ns, Nq) || !workspace_dev) {
        set_error("mmx_mm_attention_rules: workspace %zu < %zu", workspace_bytes, mmx_mm_rules_workspace_bytes(Ns, Nq));
        return MMX_EWORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace_dev);
    float* Rn_ss = reinterpret_cast<float*>(ws);
    float* Rn_qq = reinterpret_cast<float*>(ws + align256(sizeof(float) * Ns * Ns));
    float* tmp = reinterpret_cast<float*>(ws + align256(sizeof(float) * Ns * Ns) + align256(sizeof(float) * Nq * Nq));
    const int nan0 = (flags & MMX_MM_NAN_TO_ZERO) ? 1 : 0;
    int rc;
    const float* ss = static_cast<const float*>(R_ss_dev);
    const float* qq = static_cast<const float*>(R_qq_dev);
    if (flags & MMX_MM_NORMALIZE) {
        // The reference normalises (and asserts diag >= 0) BEFORE it looks at apply_self_in_rule_10
        // (DETR/modules/ExplanationGenerator.py:36-38, lxmert/.../ExplanationGenerator.py:35-37), so the check word is
        // produced in both branches.  Both residual normalisations share diag_min (min over both diagonals).
        float* dm = static_cast<float*>(diag_min_dev);
        if (dm) fill_scalar_kernel<<<1, 1, 0, s>>>(dm, __builtin_inff());
        if ((flags & MMX_MM_SELF_IN_RULE10) || dm) {
            row_normalise_kernel<<<(Ns + 3) / 4, 256, 0, s>>>(ss, Rn_ss, Ns, Ns, 0, dm);
            row_normalise_kernel<<<(Nq + 3) / 4, 256, 0, s>>>(qq, Rn_qq, Nq, Nq, 0, dm);
            MMX_LAUNCH_CHECK("row_normalise_kernel");
        }
        ss = Rn_ss;
        qq = Rn_qq;
    }
    if (flags & MMX_MM_SELF_IN_RULE10) {
        // tmp = cam_sq . Rn_qq ; R_sq_add = Rn_ss^T . tmp
        rc = mmx_bmm_f32(cam_sq_dev, qq, nullptr, tmp, 1, Ns, Nq, Nq, 0, 0, 0, 0, 0, stream);
        if (rc) return rc;
        rc = mmx_bmm_f32(ss, tmp, nullptr, R_sq_add_dev, 1, Ns, Nq, Ns, 1, 0, 0, 0, nan0, stream);
        if (rc) return rc;
    } else {
        // the reference returns cam_sq itself; the DETR flavour scrubs its NaNs too (:40-42)
        const long n = static_cast<long>(Ns) * Nq;
        copy_scrub_kernel<<<static_cast<unsigned>((n + 255) / 256), 256, 0, s>>>(
            static_cast<const float*>(cam_sq_dev), static_cast<float*>(R_sq_add_dev), n, nan0);
        MMX_LAUNCH_CHECK("copy_scrub_kernel");
    }
    if (R_qs_dev) {
        rc = mmx_bmm_f32(cam_sq_dev, R_qs_dev, nullptr, R_ss_add_dev, 1, Ns, Ns, Nq, 0, 0, 0, 0, 0, stream);
        if (rc) return rc;
    }
    return MMX_OK;
}

// ----------------------------------------------------------------------------------------- rollout
extern "C" size_t mmx_rollout_workspace_bytes(int B, int N) {
    return 2 * align256(sizeof(float) * static_cast<size_t>(B) * N * N);
}

extern "C" int mmx_rollout_chain(const void* const* layers, int n_layers, int B, int N, int normalize, void* out_dev,
                                 void* workspace_dev, size_t workspace_bytes, void* stream) {
    MMX_CHECK_ARG(layers && out_dev, "mmx_rollout_chain: null pointer");
    MMX_CHECK_ARG(n_layers > 0 && B > 0 && N > 0, "mmx_rollout_chain: non-positive size");
    if (workspace_bytes < mmx_rollout_workspace_bytes(B, N) || !workspace_dev) {
        set_error("mmx_rollout_chain: workspace %zu < %zu", workspace_bytes, mmx_rollout_workspace_bytes(B, N));
        return MMX_EWORKSPACE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t mat = align256(sizeof(float) * static_cast<size_t>(B) * N * N);
    float* aug = static_cast<float*>(workspace_dev);
    float* pong = reinterpret_cast<float*>(static_cast<char*>(workspace_dev) + mat);
    float* out = static_cast<float*>(out_dev);
    const int mode = normalize ? 1 : 2;
    const int64_t nn = static_cast<int64_t>(N) * N;
    // joint = aug_0; joint = aug_i . joint.  Ping-pong so that the last product lands in `out`.
    float* cur = ((n_layers - 1) % 2 == 0) ? out : pong;
    int rc = launch_rows(layers[0], cur, B, N, mode, nullptr, s);
    if (rc) return rc;
    for (int i = 1; i < n_layers; ++i) {
        float* nxt = (cur == out) ? pong : out;
        rc = launch_rows(layers[i], aug, B, N, mode, nullptr, s);
        if (rc) return rc;
        rc = mmx_bmm_f32(aug, cur, nullptr, nxt, B, N, N, N, 0, nn, nn, nn, 0, stream);
        if (rc) return rc;
        cur = nxt;
    }
    return MMX_OK;
}

