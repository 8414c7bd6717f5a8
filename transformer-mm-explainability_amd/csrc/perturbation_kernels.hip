// Kernels of the patch perturbation test for image models (vit_perturbation.py): rank the patches of every image by their
// relevancy and build, in one launch, the S perturbed copies of the batch that keep the first counts[s] patches of that order.
//
//   * mmx_patch_ranks: ranks[b][i] = position of patch i in ONE stable descending order of row b (torch.sort(descending=True,
//     stable=True): among equal scores the lower index first, +0.0 == -0.0, NaN before +inf).  One workgroup per image; the
//     scores are turned into order-preserving 32-bit keys staged in LDS and every thread COUNTS the patches that precede its
//     own: rank = #{j : key_j > key_i} + #{j < i : key_j == key_i}.  P <= 4096 patches, so the P^2 comparisons of an image
//     (38 k at 196 patches) are cheaper than the launches of a device-wide sort, the result does not depend on any
//     scheduling order, and the inner loop reads LDS at one address per wave (broadcast, conflict-free), four keys per read.
//   * mmx_perturb_patches: out[s][b][c][y][x] = ranks[b][patch of (y, x)] < counts[s] ? images[b][c][y][x] : fill[c].  A thread
//     owns four consecutive pixels of one image row: it reads them and their patch ranks ONCE and writes the S copies as
//     16-byte stores (rows that are not a multiple of 4 pixels wide, or unaligned tensors, take the one-pixel form).  A pure
//     streaming kernel: S * B * C * R^2 * 4 bytes written, B * C * R^2 * 4 read.  counts lives on the device so that a
//     captured pass builds nothing from host lists.
//
// Token perturbation test for CLIP captions (clip_text_perturbation.py; the text half of the reference's bi-modal test,
// lxmert/lxmert/perturbation.py:158-176, on the EOT convention of CLIP/clip/model.py:360):
//   * mmx_perturb_tokens: the S perturbed copies of B captions in ONE launch.  One wave per caption: the ids are read once into LDS, the
//     wave finds e = the first maximum of the row (text.argmax: the EOT token), turns the scores of the words 1 <= p < e into the keys
//     of mmx_patch_ranks (every other position: key 0, below every real key, so the counting loop needs no second predicate), ranks them
//     by counting (W <= 254 words: at most 64 k comparisons), and for every step compacts [SOT, kept words, EOT] with one ballot and a
//     popcount prefix per 64 positions.  The compacted row is assembled in LDS and leaves as contiguous 8-byte stores, zeros behind
//     it.  counts [S][N - 1] (device, host-built once: int((1 - step) * w) for every word count w) is indexed with the caption's own
//     W: no float arithmetic on steps here, nothing read back.  No atomics, no workspace.
#include "mmx_common.h"

namespace mmx {
namespace {

constexpr int kMaxPatches = 4096;     // a 64 x 64 grid

// monotone key: a > b as floats (torch order: NaN greatest, -0 == +0)  <=>  key(a) > key(b) as unsigned; every key is > 0
__device__ __forceinline__ unsigned order_key(float x) {
    if (x != x) return 0xFFFFFFFFu;
    unsigned u = __float_as_uint(x);
    if ((u << 1) == 0u) u = 0u;                              // -0.0 -> +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(1024) void patch_ranks_kernel(const float* __restrict__ scores, int* __restrict__ ranks, int P) {
    __shared__ __attribute__((aligned(16))) unsigned keys[kMaxPatches];
    const int b = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    const int P4 = (P + 3) & ~3;
    const float* row = scores + static_cast<int64_t>(b) * P;
    for (int j = tid; j < P4; j += nthreads) keys[j] = j < P ? order_key(row[j]) : 0u;    // padding: below every real key
    __syncthreads();
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    for (int i = tid; i < P; i += nthreads) {
        const unsigned ki = keys[i];
        int before = 0;
        for (int j = 0; j < P4; j += 4) {
            const u32x4_t kj = *reinterpret_cast<const u32x4_t*>(keys + j);
#pragma unroll
            for (int e = 0; e < 4; ++e) before += (kj[e] > ki || (kj[e] == ki && j + e < i)) ? 1 : 0;
        }
        ranks[static_cast<int64_t>(b) * P + i] = before;
    }
}

// VEC = 4: R % 4 == 0 and 16-byte aligned images / out; UNI: patch % 4 == 0, the four pixels share one patch
template <int VEC, bool UNI>
__global__ __launch_bounds__(256) void perturb_patches_kernel(const float* __restrict__ images, const int* __restrict__ ranks,
                                                              const int* __restrict__ counts, const float* __restrict__ fill,
                                                              float* __restrict__ out, int B, int C, int R, int patch, int S) {
    // grid (pixel groups of one plane, C, B)
    const int RV = R / VEC;
    const int64_t plane = static_cast<int64_t>(R) * R;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= R * RV) return;
    const int xv = idx % RV, y = idx / RV, c = blockIdx.y, b = blockIdx.z;
    const int G = R / patch, x0 = xv * VEC;
    const int* rrow = ranks + static_cast<int64_t>(b) * G * G + (y / patch) * G;
    const int64_t off = (static_cast<int64_t>(b) * C + c) * plane + static_cast<int64_t>(y) * R + x0;
    const int64_t step = static_cast<int64_t>(B) * C * plane;
    const float f = fill[c];
    if constexpr (VEC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(images + off);
        int rk[4];
        if constexpr (UNI) {
            rk[0] = rk[1] = rk[2] = rk[3] = rrow[x0 / patch];
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) rk[e] = rrow[(x0 + e) / patch];
        }
        for (int s = 0; s < S; ++s) {
            const int n = counts[s];
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = rk[e] < n ? v[e] : f;
            *reinterpret_cast<f32x4*>(out + s * step + off) = o;
        }
    } else {
        const float v = images[off];
        const int rk = rrow[x0 / patch];
        for (int s = 0; s < S; ++s) out[s * step + off] = rk < counts[s] ? v : f;
    }
}

constexpr int kMaxPositions = 256, kMaxTokenSteps = 64;

// grid B, one wave: caption b -> out_ids[s][b][.], out_eot[s][b] for every step s, ranks[b][.] (optional)
__global__ __launch_bounds__(64) void perturb_tokens_kernel(const long long* __restrict__ ids, const float* __restrict__ scores,
                                                            const int* __restrict__ counts, long long* __restrict__ out_ids,
                                                            long long* __restrict__ out_eot, int* __restrict__ ranks, int B, int N,
                                                            int S) {
    __shared__ __attribute__((aligned(16))) unsigned keys[kMaxPositions];
    __shared__ long long idrow[kMaxPositions];
    __shared__ long long outrow[kMaxPositions];
    __shared__ int rk[kMaxPositions];
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long* irow = ids + static_cast<int64_t>(b) * N;
    const float* srow = scores + static_cast<int64_t>(b) * N;
    const int chunks = (N + 63) >> 6;

    // e: index of the FIRST maximum of the row (a lane walks its positions in ascending order: strictly greater only)
    long long best = 0;
    int e = N;                                              // (a lane without a position: loses every tie)
    for (int c = 0; c < chunks; ++c) {
        const int p = c * 64 + lane;
        if (p < N) {
            const long long v = irow[p];
            idrow[p] = v;
            if (e == N || v > best) { best = v; e = p; }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long ob = __shfl_xor(best, off);
        const int oe = __shfl_xor(e, off);
        if (oe < N && (e == N || ob > best || (ob == best && oe < e))) { best = ob; e = oe; }
    }
    const int W = e > 1 ? e - 1 : 0;                        // the words are the positions 1 .. e - 1

    const int N4 = (N + 3) & ~3;
    for (int c = 0; c < (N4 + 63) >> 6; ++c) {
        const int p = c * 64 + lane;
        if (p < N4) keys[p] = (p >= 1 && p < e) ? order_key(srow[p]) : 0u;       // scores outside the words are never read
    }
    __syncthreads();
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    const int E4 = (e + 3) & ~3;                            // <= N4: keys at and past e are 0
    for (int c = 0; c < chunks; ++c) {
        const int p = c * 64 + lane;
        if (p < N) {
            int before = -1;
            if (p >= 1 && p < e) {
                const unsigned kp = keys[p];
                before = 0;
                for (int j = 0; j < E4; j += 4) {
                    const u32x4_t kj = *reinterpret_cast<const u32x4_t*>(keys + j);
#pragma unroll
                    for (int r = 0; r < 4; ++r) before += (kj[r] > kp || (kj[r] == kp && j + r < p)) ? 1 : 0;
                }
            }
            rk[p] = before;
            if (ranks) ranks[static_cast<int64_t>(b) * N + p] = before;
        }
    }
    __syncthreads();

    for (int s = 0; s < S; ++s) {
        const int keep_n = counts[static_cast<int64_t>(s) * (N - 1) + W];        // W <= N - 2
        int total = 0;
        for (int c = 0; c < chunks; ++c) {
            const int p = c * 64 + lane;
            const bool keep = p < N && (p == 0 || p == e || (p < e && rk[p] < keep_n));
            const unsigned long long m = __ballot(keep);
            if (keep) outrow[total + __popcll(m & ((1ull << lane) - 1ull))] = idrow[p];
            total += __popcll(m);
        }
        __syncthreads();
        long long* orow = out_ids + (static_cast<int64_t>(s) * B + b) * N;
        for (int c = 0; c < chunks; ++c) {
            const int p = c * 64 + lane;
            if (p < N) orow[p] = p < total ? outrow[p] : 0ll;
        }
        if (lane == 0) out_eot[static_cast<int64_t>(s) * B + b] = total - 1;
        __syncthreads();                                    // the next step rewrites outrow
    }
}

}  // namespace
}  // namespace mmx

using namespace mmx;

extern "C" int mmx_patch_ranks(const void* scores_dev, void* ranks_dev, int B, int P, void* stream) {
    MMX_CHECK_ARG(scores_dev && ranks_dev, "mmx_patch_ranks: null pointer");
    MMX_CHECK_ARG(B >= 1, "mmx_patch_ranks: batch %d < 1", B);
    MMX_CHECK_ARG(P >= 1 && P <= kMaxPatches, "mmx_patch_ranks: %d patches outside 1 .. %d (a 64 x 64 grid)", P, kMaxPatches);
    const int threads = P >= 1024 ? 1024 : (P + 63) / 64 * 64;
    patch_ranks_kernel<<<dim3(B), threads, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const float*>(scores_dev),
                                                                                 static_cast<int*>(ranks_dev), P);
    MMX_LAUNCH_CHECK("patch_ranks_kernel");
    return MMX_OK;
}

extern "C" int mmx_perturb_patches(const void* images_dev, const void* ranks_dev, const void* counts_dev, const void* fill_dev,
                                   void* out_dev, int B, int C, int R, int patch, int S, void* stream) {
    MMX_CHECK_ARG(images_dev && ranks_dev && counts_dev && fill_dev && out_dev, "mmx_perturb_patches: null pointer");
    MMX_CHECK_ARG(B >= 1 && C >= 1 && S >= 1, "mmx_perturb_patches: batch %d, channels %d, steps %d: all must be >= 1", B, C, S);
    MMX_CHECK_ARG(R >= 1 && patch >= 1 && R % patch == 0, "mmx_perturb_patches: patch size %d does not divide the resolution %d",
                  patch, R);
    MMX_CHECK_ARG(B <= 65535 && C <= 65535 && R <= 16384, "mmx_perturb_patches: B / C exceed the grid limit 65535 or R > 16384");
    const bool vec = R % 4 == 0 && ((reinterpret_cast<uintptr_t>(images_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15u) == 0;
    const int per_plane = vec ? R * (R / 4) : R * R;
    const dim3 grid((per_plane + 255) / 256, C, B);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float* img = static_cast<const float*>(images_dev);
    const int* rk = static_cast<const int*>(ranks_dev);
    const int* cn = static_cast<const int*>(counts_dev);
    const float* fl = static_cast<const float*>(fill_dev);
    float* out = static_cast<float*>(out_dev);
    if (vec && patch % 4 == 0) perturb_patches_kernel<4, true><<<grid, 256, 0, s>>>(img, rk, cn, fl, out, B, C, R, patch, S);
    else if (vec) perturb_patches_kernel<4, false><<<grid, 256, 0, s>>>(img, rk, cn, fl, out, B, C, R, patch, S);
    else perturb_patches_kernel<1, false><<<grid, 256, 0, s>>>(img, rk, cn, fl, out, B, C, R, patch, S);
    MMX_LAUNCH_CHECK("perturb_patches_kernel");
    return MMX_OK;
}

extern "C" int mmx_perturb_tokens(const void* ids_dev, const void* scores_dev, const void* counts_dev, void* out_ids_dev,
                                  void* out_eot_dev, void* ranks_dev, int B, int N, int S, void* stream) {
    MMX_CHECK_ARG(ids_dev && scores_dev && counts_dev && out_ids_dev && out_eot_dev, "mmx_perturb_tokens: null pointer");
    MMX_CHECK_ARG(B >= 1, "mmx_perturb_tokens: batch %d < 1", B);
    MMX_CHECK_ARG(N >= 2 && N <= kMaxPositions, "mmx_perturb_tokens: %d positions outside 2 .. %d", N, kMaxPositions);
    MMX_CHECK_ARG(S >= 1 && S <= kMaxTokenSteps, "mmx_perturb_tokens: %d steps outside 1 .. %d", S, kMaxTokenSteps);
    perturb_tokens_kernel<<<dim3(B), 64, 0, static_cast<hipStream_t>(stream)>>>(
        static_cast<const long long*>(ids_dev), static_cast<const float*>(scores_dev), static_cast<const int*>(counts_dev),
        static_cast<long long*>(out_ids_dev), static_cast<long long*>(out_eot_dev), static_cast<int*>(ranks_dev), B, N, S);
    MMX_LAUNCH_CHECK("perturb_tokens_kernel");
    return MMX_OK;
}
