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
//     popcount prefix per 64 positions.  The kept positions are assembled in LDS and the row leaves as contiguous 8-byte stores, zeros behind
//     it.  counts [S][N - 1] (device, host-built once: int((1 - step) * w) for every word count w) is indexed with the caption's own
//     W: no float arithmetic on steps here, nothing read back.  No atomics, no workspace.
//
// Perturbation test of VisualBERT on a padded batch (visualbert_perturbation.py; VisualBERT/mmf/trainers/core/evaluation_loop.py:100-159),
// sequence = [T text positions | V regions], lengths from a device array, clamped to 3 .. T:
//   * mmx_selfattn_perturb_regions: one workgroup per (item, group of steps with one keep count c): it ranks the item's V <= 253 region
//     scores in LDS the way mmx_patch_ranks does, then copies the item's T embedded text rows and its c best regions, in rank order,
//     into the group's packed rows (16-byte loads / stores when E % 4 == 0), with the additive key mask and the pooled row index.
//   * mmx_selfattn_perturb_text: mmx_perturb_tokens on the '?'-pooler convention (positions 0, n - 2, n - 1 stay, the words are
//     1 .. n - 3) for ids and segments at once; the three wave-level steps are shared with perturb_tokens_kernel.
//
// Text perturbation test of LXMERT on a padded batch (lxmert_perturbation.py; lxmert/lxmert/perturbation.py:160-178):
//   * mmx_lxmert_perturb_text: the same three wave-level steps on the [CLS] ... [SEP] convention (positions 0 and n - 1 stay, the words
//     are 1 .. n - 2, lengths from a device array clamped to 2 .. T) for ids and token types at once, with a float mask.  Every step's
//     sequences are written where a host placement table (base, stride, width per step, passed by value) puts them, so that groups of
//     steps leave the kernel at their own width: [B * n_g, Q_g] blocks the body embeds as they are.  A sequence writes exactly its
//     width -- the kept positions, zeros behind them, truncated at the width -- and nothing else.
#include "mmx_common.h"
#include "text_placement.h"

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

// The whole workgroup stages the keys of one row of P scores (NEGATE: of their negations) in LDS, padded with 0 -- below every real
// key -- to the next multiple of 4, and meets at a barrier: keys is complete on return.
template <bool NEGATE>
__device__ __forceinline__ void block_stage_keys(const float* __restrict__ row, int P, unsigned* keys) {
    const int P4 = (P + 3) & ~3;
    for (int j = threadIdx.x; j < P4; j += blockDim.x) keys[j] = j < P ? order_key(NEGATE ? -row[j] : row[j]) : 0u;
    __syncthreads();
}

// Position of element i in ONE stable descending order of keys[0 .. n4) (n4 % 4 == 0, 16-byte aligned LDS): the keys above its own plus
// the equal ones in front of it.  One LDS address per wave and read (broadcast, conflict-free), four keys per read.  The one counting
// loop of this file: patch_ranks_kernel, selfattn_perturb_regions_kernel and wave_word_ranks call it.
__device__ __forceinline__ int keys_before(const unsigned* keys, int n4, int i) {
    typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
    const unsigned ki = keys[i];
    int before = 0;
    for (int j = 0; j < n4; j += 4) {
        const u32x4_t kj = *reinterpret_cast<const u32x4_t*>(keys + j);
#pragma unroll
        for (int e = 0; e < 4; ++e) before += (kj[e] > ki || (kj[e] == ki && j + e < i)) ? 1 : 0;
    }
    return before;
}

__global__ __launch_bounds__(1024) void patch_ranks_kernel(const float* __restrict__ scores, int* __restrict__ ranks, int P) {
    __shared__ __attribute__((aligned(16))) unsigned keys[kMaxPatches];
    const int b = blockIdx.x;
    block_stage_keys<false>(scores + static_cast<int64_t>(b) * P, P, keys);
    const int P4 = (P + 3) & ~3;
    for (int i = threadIdx.x; i < P; i += blockDim.x) ranks[static_cast<int64_t>(b) * P + i] = keys_before(keys, P4, i);
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

// ---- one wave, one row of N <= 256 positions: the three steps the token kernels share (perturb_tokens_kernel, selfattn_perturb_text_kernel)
// keys[p] = order_key(score of word p) for the words lo <= p < hi (NEGATE: of its negation), 0 -- below every real key -- at every other
// position up to the next multiple of 4: the counting loop needs no second predicate.  Scores outside the words are never read.
template <bool NEGATE>
__device__ __forceinline__ void wave_word_keys(const float* __restrict__ srow, int lo, int hi, int N, int lane, unsigned* keys) {
    const int N4 = (N + 3) & ~3;
    for (int c = 0; c < (N4 + 63) >> 6; ++c) {
        const int p = c * 64 + lane;
        if (p < N4) keys[p] = (p >= lo && p < hi) ? order_key(NEGATE ? -srow[p] : srow[p]) : 0u;
    }
}

// rk[p] = position of word p in ONE stable descending order of the words (the counting of patch_ranks_kernel), -1 outside the words;
// ranks_row (optional, global) receives the same.  keys must be complete (a barrier after wave_word_keys).
__device__ __forceinline__ void wave_word_ranks(const unsigned* keys, int lo, int hi, int N, int lane, int* rk, int* ranks_row) {
    const int E4 = (hi + 3) & ~3;                           // <= (N + 3) & ~3: keys at and past hi are 0
    for (int c = 0; c < (N + 63) >> 6; ++c) {
        const int p = c * 64 + lane;
        if (p < N) {
            const int before = (p >= lo && p < hi) ? keys_before(keys, E4, p) : -1;
            rk[p] = before;
            if (ranks_row) ranks_row[p] = before;
        }
    }
}

// src[j] = the j-th position p < N (ascending) with keep(p): one ballot and a popcount prefix per 64 positions.  Returns their number.
template <class Keep>
__device__ __forceinline__ int wave_compact(int N, int lane, Keep keep, int* src) {
    int total = 0;
    for (int c = 0; c < (N + 63) >> 6; ++c) {
        const int p = c * 64 + lane;
        const bool k = p < N && keep(p);
        const unsigned long long m = __ballot(k);
        if (k) src[total + __popcll(m & ((1ull << lane) - 1ull))] = p;
        total += __popcll(m);
    }
    return total;
}

// grid B, one wave: caption b -> out_ids[s][b][.], out_eot[s][b] for every step s, ranks[b][.] (optional)
__global__ __launch_bounds__(64) void perturb_tokens_kernel(const long long* __restrict__ ids, const float* __restrict__ scores,
                                                            const int* __restrict__ counts, long long* __restrict__ out_ids,
                                                            long long* __restrict__ out_eot, int* __restrict__ ranks, int B, int N,
                                                            int S) {
    __shared__ __attribute__((aligned(16))) unsigned keys[kMaxPositions];
    __shared__ long long idrow[kMaxPositions];
    __shared__ int src[kMaxPositions];
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

    wave_word_keys<false>(srow, 1, e, N, lane, keys);
    __syncthreads();
    wave_word_ranks(keys, 1, e, N, lane, rk, ranks ? ranks + static_cast<int64_t>(b) * N : nullptr);
    __syncthreads();

    for (int s = 0; s < S; ++s) {
        const int keep_n = counts[static_cast<int64_t>(s) * (N - 1) + W];        // W <= N - 2
        const int total = wave_compact(N, lane, [&](int p) { return p == 0 || p == e || (p < e && rk[p] < keep_n); }, src);
        __syncthreads();
        long long* orow = out_ids + (static_cast<int64_t>(s) * B + b) * N;
        for (int c = 0; c < chunks; ++c) {
            const int p = c * 64 + lane;
            if (p < N) orow[p] = p < total ? idrow[src[p]] : 0ll;
        }
        if (lane == 0) out_eot[static_cast<int64_t>(s) * B + b] = total - 1;
        __syncthreads();                                    // the next step rewrites src
    }
}

// ---- VisualBERT (single-stream) perturbation test on a PADDED batch: sequence = [T text positions | V regions], relevancy rows [B, T + V]
__device__ __forceinline__ int clamp_text_len(const int* __restrict__ text_len, int b, int T) {
    const int n = text_len[b];
    return n < 3 ? 3 : (n > T ? T : n);
}

constexpr int kRegionThreads = 256;
constexpr int kMaxRowFloats = 1 << 20;                      // E: the floats of a sequence, (T + c) * E <= 2^28, index as int

// grid B * G (workgroup w: item w % B of group w / B), 256 threads.  VEC = 4: E % 4 == 0 and 16-byte aligned emb / x
template <int VEC, bool NEGATE>
__global__ __launch_bounds__(kRegionThreads) void selfattn_perturb_regions_kernel(
    const float* __restrict__ emb, const float* __restrict__ cam, const int* __restrict__ text_len, const int* __restrict__ counts,
    float* __restrict__ x, float* __restrict__ mask, long long* __restrict__ pooled, int* __restrict__ ranks, int B, int T, int V, int E,
    int G, long long R) {
    __shared__ __attribute__((aligned(16))) unsigned keys[kMaxPositions];
    __shared__ int order[kMaxPositions];                    // order[r] = the region ranked r
    const int b = blockIdx.x % B, g = blockIdx.x / B, tid = threadIdx.x;
    const int N = T + V, V4 = (V + 3) & ~3;
    block_stage_keys<NEGATE>(cam + static_cast<int64_t>(b) * N + T, V, keys);
    if (tid < V) {                                          // V <= 253 < blockDim.x
        const int before = keys_before(keys, V4, tid);
        order[before] = tid;                                // a permutation of 0 .. V - 1: every slot written once
        if (ranks && g == 0) ranks[static_cast<int64_t>(b) * V + tid] = before;
    }
    // where the sequence (g, b) starts: off_g + b * (T + c_g); counts clamped to 0 .. V, and nothing is written past R rows
    long long row0 = 0;
    for (int h = 0; h < g; ++h) {
        const int ch = counts[h];
        row0 += static_cast<long long>(B) * (T + (ch < 0 ? 0 : (ch > V ? V : ch)));
    }
    int c = counts[g];
    c = c < 0 ? 0 : (c > V ? V : c);
    const int L = T + c;
    row0 += static_cast<long long>(b) * L;
    if (row0 + L > R) return;                               // (uniform over the workgroup)
    __syncthreads();
    const int n = clamp_text_len(text_len, b, T);
    for (int p = tid; p < L; p += kRegionThreads) mask[row0 + p] = (p < T && p >= n) ? -10000.0f : 0.0f;
    if (tid == 0) pooled[static_cast<int64_t>(g) * B + b] = row0 + n - 2;
    const float* ebase = emb + static_cast<int64_t>(b) * N * E;
    float* xbase = x + row0 * E;
    const int EV = E / VEC;
    for (int i = tid; i < L * EV; i += kRegionThreads) {
        const int p = i / EV, col = (i - p * EV) * VEC;
        const int q = p < T ? p : T + order[p - T];
        const float* sp = ebase + static_cast<int64_t>(q) * E + col;
        float* dp = xbase + static_cast<int64_t>(p) * E + col;
        if constexpr (VEC == 4) *reinterpret_cast<f32x4*>(dp) = *reinterpret_cast<const f32x4*>(sp);
        else *dp = *sp;
    }
}

// grid B, one wave: question b -> out_ids / out_seg / out_mask [s][b][.] and new_len[s][b] for every step s (perturb_tokens_kernel's
// structure; the length comes from text_len, the words are 1 .. c - 1 with c = n - 2, and 0, c, c + 1 always stay)
template <bool NEGATE>
__global__ __launch_bounds__(64) void selfattn_perturb_text_kernel(const long long* __restrict__ ids, const long long* __restrict__ seg,
                                                                   const float* __restrict__ cam, const int* __restrict__ text_len,
                                                                   const int* __restrict__ counts, long long* __restrict__ out_ids,
                                                                   long long* __restrict__ out_seg, long long* __restrict__ out_mask,
                                                                   long long* __restrict__ new_len, int B, int T, int V, int S) {
    __shared__ __attribute__((aligned(16))) unsigned keys[kMaxPositions];
    __shared__ long long idrow[kMaxPositions];
    __shared__ long long segrow[kMaxPositions];
    __shared__ int src[kMaxPositions];
    __shared__ int rk[kMaxPositions];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int chunks = (T + 63) >> 6;
    const int n = clamp_text_len(text_len, b, T), c = n - 2, W = n - 3;
    for (int k = 0; k < chunks; ++k) {
        const int p = k * 64 + lane;
        if (p < T) {
            idrow[p] = ids[static_cast<int64_t>(b) * T + p];
            segrow[p] = seg[static_cast<int64_t>(b) * T + p];
        }
    }
    wave_word_keys<NEGATE>(cam + static_cast<int64_t>(b) * (T + V), 1, c, T, lane, keys);
    __syncthreads();
    wave_word_ranks(keys, 1, c, T, lane, rk, nullptr);
    __syncthreads();

    for (int s = 0; s < S; ++s) {
        const int keep_n = counts[static_cast<int64_t>(s) * T + W];              // W <= T - 3
        const int total = wave_compact(T, lane, [&](int p) { return p == 0 || p == c || p == c + 1 || (p < c && rk[p] < keep_n); }, src);
        __syncthreads();
        const int64_t o = (static_cast<int64_t>(s) * B + b) * T;
        for (int k = 0; k < chunks; ++k) {
            const int p = k * 64 + lane;
            if (p < T) {
                const bool live = p < total;
                out_ids[o + p] = live ? idrow[src[p]] : 0ll;
                out_seg[o + p] = live ? segrow[src[p]] : 0ll;
                out_mask[o + p] = live ? 1ll : 0ll;
            }
        }
        if (lane == 0) new_len[static_cast<int64_t>(s) * B + b] = total;
        __syncthreads();                                    // the next step rewrites src
    }
}

// place.v[s] = {base, stride, width} of step s (text_placement.h; validated by the entry): 64 x 3 x 8 bytes of kernel arguments
struct TextPlacement {
    long long v[kMaxTokenSteps][3];
};

// grid B, one wave: question b -> for every step s the width_s elements at base_s + b * stride_s of out_ids / out_types / out_mask,
// new_len[s][b] (untruncated) and ranks[b][.] (optional).  The length comes from text_len clamped to 2 .. T; the words are 1 .. n - 2.
template <bool NEGATE>
__global__ __launch_bounds__(64) void lxmert_perturb_text_kernel(const long long* __restrict__ ids, const long long* __restrict__ types,
                                                                 const float* __restrict__ cam, const int* __restrict__ text_len,
                                                                 const int* __restrict__ counts, long long* __restrict__ out_ids,
                                                                 long long* __restrict__ out_types, float* __restrict__ out_mask,
                                                                 long long* __restrict__ new_len, int* __restrict__ ranks,
                                                                 const TextPlacement place, int B, int T, int S) {
    __shared__ __attribute__((aligned(16))) unsigned keys[kMaxPositions];
    __shared__ long long idrow[kMaxPositions];
    __shared__ long long typerow[kMaxPositions];
    __shared__ int src[kMaxPositions];
    __shared__ int rk[kMaxPositions];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int chunks = (T + 63) >> 6;
    int n = text_len[b];
    n = n < 2 ? 2 : (n > T ? T : n);
    const int e = n - 1, W = n - 2;                         // [SEP] sits at e; the words are 1 .. e - 1
    for (int k = 0; k < chunks; ++k) {
        const int p = k * 64 + lane;
        if (p < T) {
            idrow[p] = ids[static_cast<int64_t>(b) * T + p];
            typerow[p] = types[static_cast<int64_t>(b) * T + p];
        }
    }
    wave_word_keys<NEGATE>(cam + static_cast<int64_t>(b) * T, 1, e, T, lane, keys);
    __syncthreads();
    wave_word_ranks(keys, 1, e, T, lane, rk, ranks ? ranks + static_cast<int64_t>(b) * T : nullptr);
    __syncthreads();

    for (int s = 0; s < S; ++s) {
        const int keep_n = counts[static_cast<int64_t>(s) * (T - 1) + W];        // W <= T - 2
        const int total = wave_compact(T, lane, [&](int p) { return p == 0 || p == e || (p < e && rk[p] < keep_n); }, src);
        __syncthreads();
        const int64_t o = place.v[s][0] + static_cast<int64_t>(b) * place.v[s][1];
        const int width = static_cast<int>(place.v[s][2]);                      // 1 .. T: the entry refuses anything else
        for (int k = 0; k < chunks; ++k) {
            const int p = k * 64 + lane;
            if (p < width) {
                const bool live = p < total;
                out_ids[o + p] = live ? idrow[src[p]] : 0ll;
                out_types[o + p] = live ? typerow[src[p]] : 0ll;
                out_mask[o + p] = live ? 1.0f : 0.0f;
            }
        }
        if (lane == 0) new_len[static_cast<int64_t>(s) * B + b] = total;
        __syncthreads();                                    // the next step rewrites src
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

extern "C" int mmx_selfattn_perturb_regions(const void* emb_dev, const void* cam_dev, const void* text_len_dev, const void* counts_dev,
                                            void* x_dev, void* mask_dev, void* pooled_dev, void* ranks_dev, int B, int T, int V, int E,
                                            int G, int64_t R, int positive, void* stream) {
    const char* me = "mmx_selfattn_perturb_regions";
    MMX_CHECK_ARG(emb_dev && cam_dev && text_len_dev && counts_dev && x_dev && mask_dev && pooled_dev, "%s: null pointer", me);
    MMX_CHECK_ARG(B >= 1 && E >= 1 && E <= kMaxRowFloats, "%s: B=%d < 1 or E=%d outside 1 .. %d", me, B, E, kMaxRowFloats);
    MMX_CHECK_ARG(T >= 3 && V >= 1 && T <= kMaxPositions && V <= kMaxPositions && T + V <= kMaxPositions,
                  "%s: T=%d V=%d outside T >= 3, V >= 1, T + V <= %d", me, T, V, kMaxPositions);
    MMX_CHECK_ARG(G >= 1 && G <= kMaxTokenSteps, "%s: %d groups outside 1 .. %d", me, G, kMaxTokenSteps);
    const int64_t bg = static_cast<int64_t>(B) * G;
    MMX_CHECK_ARG(bg <= 0x7FFFFFFF, "%s: B * G = %lld workgroups exceed the grid limit 2^31 - 1", me, static_cast<long long>(bg));
    MMX_CHECK_ARG(R >= bg * T && R <= bg * (T + V), "%s: %lld packed rows outside B * G * T .. B * G * (T + V) = %lld .. %lld", me,
                  static_cast<long long>(R), static_cast<long long>(bg * T), static_cast<long long>(bg * (T + V)));
    const size_t f = sizeof(float), N = static_cast<size_t>(T + V), nb = static_cast<size_t>(B), rows = static_cast<size_t>(R);
    const Span ins[4] = {{emb_dev, f * nb * N * E}, {cam_dev, f * nb * N}, {text_len_dev, sizeof(int) * nb}, {counts_dev, sizeof(int) * G}};
    const Span outs[4] = {{x_dev, f * rows * E}, {mask_dev, f * rows}, {pooled_dev, sizeof(long long) * static_cast<size_t>(bg)},
                          {ranks_dev, sizeof(int) * nb * V}};
    MMX_CHECK_ARG(!spans_alias(outs, 4, ins, 4), "%s: an output may not alias an input or another output", me);
    const bool vec = E % 4 == 0 && ((reinterpret_cast<uintptr_t>(emb_dev) | reinterpret_cast<uintptr_t>(x_dev)) & 15u) == 0;
    const dim3 grid(static_cast<unsigned>(bg));
    hipStream_t s = static_cast<hipStream_t>(stream);
#define MMX_REGIONS_LAUNCH(VEC, NEG)                                                                                                 \
    selfattn_perturb_regions_kernel<VEC, NEG><<<grid, kRegionThreads, 0, s>>>(                                                       \
        static_cast<const float*>(emb_dev), static_cast<const float*>(cam_dev), static_cast<const int*>(text_len_dev),               \
        static_cast<const int*>(counts_dev), static_cast<float*>(x_dev), static_cast<float*>(mask_dev),                              \
        static_cast<long long*>(pooled_dev), static_cast<int*>(ranks_dev), B, T, V, E, G, static_cast<long long>(R))
    if (vec && positive) MMX_REGIONS_LAUNCH(4, true);
    else if (vec) MMX_REGIONS_LAUNCH(4, false);
    else if (positive) MMX_REGIONS_LAUNCH(1, true);
    else MMX_REGIONS_LAUNCH(1, false);
#undef MMX_REGIONS_LAUNCH
    MMX_LAUNCH_CHECK("selfattn_perturb_regions_kernel");
    return MMX_OK;
}

extern "C" int mmx_selfattn_perturb_text(const void* ids_dev, const void* segments_dev, const void* cam_dev, const void* text_len_dev,
                                         const void* counts_dev, void* out_ids_dev, void* out_segments_dev, void* out_mask_dev,
                                         void* new_len_dev, int B, int T, int V, int S, int positive, void* stream) {
    const char* me = "mmx_selfattn_perturb_text";
    MMX_CHECK_ARG(ids_dev && segments_dev && cam_dev && text_len_dev && counts_dev && out_ids_dev && out_segments_dev && out_mask_dev &&
                      new_len_dev, "%s: null pointer", me);
    MMX_CHECK_ARG(B >= 1, "%s: batch %d < 1", me, B);
    MMX_CHECK_ARG(T >= 3 && V >= 1 && T <= kMaxPositions && V <= kMaxPositions && T + V <= kMaxPositions,
                  "%s: T=%d V=%d outside T >= 3, V >= 1, T + V <= %d", me, T, V, kMaxPositions);
    MMX_CHECK_ARG(S >= 1 && S <= kMaxTokenSteps, "%s: %d steps outside 1 .. %d", me, S, kMaxTokenSteps);
    const size_t ll = sizeof(long long), nb = static_cast<size_t>(B), nt = static_cast<size_t>(T), ns = static_cast<size_t>(S);
    const Span ins[5] = {{ids_dev, ll * nb * nt}, {segments_dev, ll * nb * nt}, {cam_dev, sizeof(float) * nb * (T + V)},
                         {text_len_dev, sizeof(int) * nb}, {counts_dev, sizeof(int) * ns * nt}};
    const Span outs[4] = {{out_ids_dev, ll * ns * nb * nt}, {out_segments_dev, ll * ns * nb * nt}, {out_mask_dev, ll * ns * nb * nt},
                          {new_len_dev, ll * ns * nb}};
    MMX_CHECK_ARG(!spans_alias(outs, 4, ins, 5), "%s: an output may not alias an input or another output", me);
    hipStream_t s = static_cast<hipStream_t>(stream);
#define MMX_TEXT_LAUNCH(NEG)                                                                                                         \
    selfattn_perturb_text_kernel<NEG><<<dim3(B), 64, 0, s>>>(                                                                        \
        static_cast<const long long*>(ids_dev), static_cast<const long long*>(segments_dev), static_cast<const float*>(cam_dev),     \
        static_cast<const int*>(text_len_dev), static_cast<const int*>(counts_dev), static_cast<long long*>(out_ids_dev),            \
        static_cast<long long*>(out_segments_dev), static_cast<long long*>(out_mask_dev), static_cast<long long*>(new_len_dev), B, T, V, S)
    if (positive) MMX_TEXT_LAUNCH(true);
    else MMX_TEXT_LAUNCH(false);
#undef MMX_TEXT_LAUNCH
    MMX_LAUNCH_CHECK("selfattn_perturb_text_kernel");
    return MMX_OK;
}

extern "C" int mmx_lxmert_perturb_text(const void* ids_dev, const void* types_dev, const void* cam_dev, const void* text_len_dev,
                                       const void* counts_dev, const int64_t* place_host, void* out_ids_dev, void* out_types_dev,
                                       void* out_mask_dev, void* new_len_dev, void* ranks_dev, int64_t out_elems, int B, int T, int S,
                                       int positive, void* stream) {
    const char* me = "mmx_lxmert_perturb_text";
    MMX_CHECK_ARG(ids_dev && types_dev && cam_dev && text_len_dev && counts_dev && place_host && out_ids_dev && out_types_dev &&
                      out_mask_dev && new_len_dev, "%s: null pointer", me);
    MMX_CHECK_ARG(B >= 1, "%s: batch %d < 1", me, B);
    MMX_CHECK_ARG(T >= 2 && T <= kMaxPositions, "%s: %d positions outside 2 .. %d", me, T, kMaxPositions);
    MMX_CHECK_ARG(S >= 1 && S <= kMaxTokenSteps, "%s: %d steps outside 1 .. %d", me, S, kMaxTokenSteps);
    MMX_CHECK_ARG(out_elems >= 1 && out_elems <= (static_cast<int64_t>(1) << 40), "%s: %lld output elements outside 1 .. 2^40", me,
                  static_cast<long long>(out_elems));
    int s0 = -1, s1 = -1;
    switch (check_text_placement(place_host, S, B, T, out_elems, &s0, &s1)) {
        case TEXT_PLACE_OK: break;
        case TEXT_PLACE_WIDTH:
            MMX_CHECK_ARG(false, "%s: step %d: width %lld outside 1 .. T = %d", me, s0, static_cast<long long>(place_host[3 * s0 + 2]), T);
        case TEXT_PLACE_STRIDE:
            MMX_CHECK_ARG(false, "%s: step %d: stride %lld < width %lld", me, s0, static_cast<long long>(place_host[3 * s0 + 1]),
                          static_cast<long long>(place_host[3 * s0 + 2]));
        case TEXT_PLACE_BASE: MMX_CHECK_ARG(false, "%s: step %d: base %lld < 0", me, s0, static_cast<long long>(place_host[3 * s0]));
        case TEXT_PLACE_OVERRUN:
            MMX_CHECK_ARG(false, "%s: step %d: its last sequence ends past the %lld output elements", me, s0,
                          static_cast<long long>(out_elems));
        case TEXT_PLACE_OVERLAP: MMX_CHECK_ARG(false, "%s: the sequences of steps %d and %d overlap", me, s0, s1);
    }
    const size_t ll = sizeof(long long), nb = static_cast<size_t>(B), nt = static_cast<size_t>(T), ns = static_cast<size_t>(S),
                 ne = static_cast<size_t>(out_elems);
    const Span ins[5] = {{ids_dev, ll * nb * nt}, {types_dev, ll * nb * nt}, {cam_dev, sizeof(float) * nb * nt},
                         {text_len_dev, sizeof(int) * nb}, {counts_dev, sizeof(int) * ns * (nt - 1)}};
    const Span outs[5] = {{out_ids_dev, ll * ne}, {out_types_dev, ll * ne}, {out_mask_dev, sizeof(float) * ne}, {new_len_dev, ll * ns * nb},
                          {ranks_dev, sizeof(int) * nb * nt}};
    MMX_CHECK_ARG(!spans_alias(outs, 5, ins, 5), "%s: an output may not alias an input or another output", me);
    TextPlacement place = {};
    for (int s = 0; s < S; ++s)
        for (int k = 0; k < 3; ++k) place.v[s][k] = place_host[3 * s + k];
    hipStream_t st = static_cast<hipStream_t>(stream);
#define MMX_LXMERT_TEXT_LAUNCH(NEG)                                                                                                  \
    lxmert_perturb_text_kernel<NEG><<<dim3(B), 64, 0, st>>>(                                                                         \
        static_cast<const long long*>(ids_dev), static_cast<const long long*>(types_dev), static_cast<const float*>(cam_dev),        \
        static_cast<const int*>(text_len_dev), static_cast<const int*>(counts_dev), static_cast<long long*>(out_ids_dev),            \
        static_cast<long long*>(out_types_dev), static_cast<float*>(out_mask_dev), static_cast<long long*>(new_len_dev),             \
        static_cast<int*>(ranks_dev), place, B, T, S)
    if (positive) MMX_LXMERT_TEXT_LAUNCH(true);
    else MMX_LXMERT_TEXT_LAUNCH(false);
#undef MMX_LXMERT_TEXT_LAUNCH
    MMX_LAUNCH_CHECK("lxmert_perturb_text_kernel");
    return MMX_OK;
}
