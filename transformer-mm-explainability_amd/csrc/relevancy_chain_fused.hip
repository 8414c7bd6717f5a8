// K1  self_chain_fused_kernel: the self-attention relevancy chain (rules 5 + 6), all layers in ONE launch, stream and matrix waves
// meeting at one s_barrier per layer.  What runs for 16-bit slabs, for the fp16-mode chain, under option self_chain_algo = 1, and for
// fp32 slabs where relevancy_chain_groups.hip's LDS images do not fit (N = 113 .. 128 with layer groups) or relevancy_chain_cols.hip
// does not apply (N < 40); relevancy_chain.hip decides.
//
// Reference sites: CLIP_explainability.ipynb cell 6:22-32 / 45-55, CLIP/example.py:22-30, ViT notebook cell 7:28-33,
// VisualBERT/.../ExplanationGenerator.py:86-93 (include/mmx_relevancy.h, mmx_relevancy_self_chain).
#include "chain_launch.h"
#include "chain_matrix.h"

namespace mmx {

// =====================================================================================================
// K_self_chain_fused: one workgroup (16 waves) per sample runs the WHOLE chain
//     R <- I;  for every layer l:  A_bar_l = mean_h clamp(G_l*A_l, 0);  R <- R + A_bar_l . R
// in one launch.  Roles (wave-uniform):
//   waves [NT, 16)  "stream" waves: read A_l / G_l head slabs with 16-B loads, reduce over heads in
//                    registers, write A_bar_l into one of two LDS buffers (row stride NP+4 floats).
//   waves [0, NT)   "matrix" waves: wave w owns the 16-column slab w of R in registers (chain_matrix.h).
// One s_barrier per layer: stream waves publish A_bar_l, then immediately start streaming layer l+1
// into the other buffer while the matrix waves multiply.  HBM traffic = A and G once + R out.
// NT = ceil(N/16) <= 8 (N <= 128); larger N takes the split path (avg_heads + bmm).
// =====================================================================================================
struct ChainArgs {
    const void* attn[MMX_MAX_LAYERS];
    const void* grad[MMX_MAX_LAYERS];
    int n_layers, B, H, N;
    const float* R_init;
    float* R_out;
    // layer-group split (G > 1): workgroup (b, g) multiplies only its contiguous layer group; the partial products
    // P_g go to `parts` [B][G][N*N] and the last arriver of a sample (ticket on counters[b]) combines them.
    int G;
    float* parts;
    unsigned* counters;
    int debug;  // profiling only: bit0 = return before the hand-off/combine, bit2 = matrix waves skip the MFMAs
    int64_t attn_bstride;  // batch stride of the attention slabs in elements (H*N*N, or 0: one forward shared by the batch)
    int pipe;  // option "self_chain_pipe": software-pipelined stream waves (fp32 slabs)
    int nt;    // option "self_chain_nt": cache policy of the pipelined slab loads (0 default policy, 1 = nt on the read-once slabs)
};

// 1024 threads: NT matrix waves + (16 - NT) stream waves, the head reduction 4 heads per load batch; the matrix waves only reduce
// the chunks left over after the stream waves' full passes.  Measured on MI355X (profiles/r01_chain_probe.txt): narrower workgroups
// (768 / 512 threads, whose larger VGPR budget per lane keeps 8 .. 12 heads in flight) and an equal share of the reduction for every
// wave are all SLOWER (text tower 75.7 us vs 77.8 .. 90.4 us) -- a CU already streams at ~8 of its ~10 B/cycle HBM ceiling, more bytes
// in flight per lane do not raise it and fewer waves lose issue overlap; 6 or 8 heads per batch spill at 128 VGPRs per lane.
constexpr int kChainThreads = 1024;

//   R16 = true: the half-precision chain of the reference's fp16 mode (round_f16): grad * attn, the head mean, A_bar . R and
//        R + A_bar . R are each rounded to fp16, sums run in fp32 -- R is carried as fp32 registers holding fp16 values.  One
//        workgroup per sample (the layer-group split re-associates the products), the plain (not software-pipelined) stream loop.
template <int NT, int DT, bool R16>
__global__ __launch_bounds__(kChainThreads) void self_chain_fused_kernel(const ChainArgs a) {
    constexpr int NP = kChainNP<NT>;
    constexpr int S = kChainS<NT>;
    extern __shared__ __attribute__((aligned(16))) float smem[];  // 2 * NP * S floats

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int G = a.G;
    const int b = blockIdx.x / G, g = blockIdx.x - b * G;
    const int N = a.N, H = a.H;
    const int per = (a.n_layers + G - 1) / G;
    const int l0 = min(a.n_layers, g * per), l1 = min(a.n_layers, l0 + per);
    const int L = l1 - l0;
    const int64_t NN = static_cast<int64_t>(N) * N;

    for (int i = tid; i < 2 * NP * S; i += kChainThreads) smem[i] = 0.f;  // pads must read as 0 (dword stores: the code of rounds 1-6,
    __syncthreads();                                                      // kept so that this kernel's registers stay as measured)

    const ChainLane q = chain_lane(wave, lane);
    f32x4 Rold[NT], Rnew[NT];

    // ---- head reduction of one 4-element chunk of A_bar_l (used by the stream waves and, for the remainder pass, by
    // the otherwise idle matrix waves)
    constexpr int LT = kChainThreads - NT * 64;   // stream lanes
    constexpr int ML = NT * 64;                   // matrix lanes
    const float fH = static_cast<float>(H);
    const int64_t sample = static_cast<int64_t>(b) * H * NN;
    const int64_t sampleA = static_cast<int64_t>(b) * a.attn_bstride;
    const int nchunks = static_cast<int>((NN + 3) >> 2);
    // Work split: a chunk costs one batch of global round trips whatever the number of busy lanes, so the pass count
    // of the stream waves is what matters.  When the chunks left over after the stream waves' full passes fit the
    // matrix lanes (text tower: 1483 = 2 x 704 + 75), the matrix waves reduce them between their MFMAs and the stream
    // waves save a whole, almost empty, pass per layer.
    const int full = nchunks / LT;
    const bool split = full >= 1 && nchunks - full * LT <= ML;
    const int stream_end = split ? full * LT : nchunks;
    auto reduce_chunk = [&](int c, const void* A, const void* Gr, float* Ab) {
        const int64_t p = static_cast<int64_t>(c) * 4;
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        if (p + 3 < NN) {
#pragma unroll 4
            for (int h = 0; h < H; ++h) {
                const f32x4 av = load4_as_f32<DT>(A, sampleA + h * NN + p);
                const f32x4 gv = load4_as_f32<DT>(Gr, sample + h * NN + p);
                const f32x4 x = R16 ? round_f16(gv * av) : gv * av;
                s[0] += relu_nan(x[0]); s[1] += relu_nan(x[1]);
                s[2] += relu_nan(x[2]); s[3] += relu_nan(x[3]);
            }
        } else {
            for (int e = 0; p + e < NN; ++e)
                for (int h = 0; h < H; ++h) {
                    const float x = load1_as_f32<DT>(Gr, sample + h * NN + p + e) * load1_as_f32<DT>(A, sampleA + h * NN + p + e);
                    s[e] += relu_nan(R16 ? round_f16(x) : x);
                }
        }
        int row = static_cast<int>(p / N);
        int cc = static_cast<int>(p - static_cast<int64_t>(row) * N);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (p + e < NN) Ab[row * S + cc] = R16 ? round_f16(s[e] / fH) : s[e] / fH;
            if (++cc == N) { cc = 0; ++row; }
        }
    };

    if (wave < NT) {
        // ------------------------------------------------------------------ matrix waves
        auto remainder_pass = [&](int l) {   // this lane's share of A_bar_l: the remainder chunks
            if (l >= L) return;
            const int c = stream_end + tid;
            if (split && c < nchunks) reduce_chunk(c, a.attn[l0 + l], a.grad[l0 + l], smem + (l & 1) * NP * S);
        };
        remainder_pass(0);
        chain_slab_load<int64_t>(Rold, a.R_init && g == 0, a.R_init, b * NN, N, q);
        for (int l = 0; l < L; ++l) {
            __syncthreads();  // A_bar_l is in buffer l&1
            if (a.debug & 4) { remainder_pass(l + 1); continue; }
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                const f32x4 acc = chain_tile_product(smem + (l & 1) * NP * S, ti, Rold, lane, q, std::false_type{}, wave);
                Rnew[ti] = R16 ? round_f16(Rold[ti] + round_f16(acc))   // torch.bmm rounds its result, the sum is rounded again
                               : Rold[ti] + acc;                        // R + (A_bar . R): same association as the reference
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) Rold[t] = Rnew[t];
            remainder_pass(l + 1);   // into the other buffer; published by the next barrier
        }
        float* dst = (G == 1) ? a.R_out + b * NN : a.parts + (static_cast<int64_t>(b) * G + g) * NN;
        chain_slab_store<int64_t>(dst, 0, Rold, N, q, G != 1, false);
    } else {
        // ------------------------------------------------------------------ stream waves
        const int lt = tid - NT * 64;
        if (!R16 && DT == MMX_F32 && a.pipe && static_cast<int64_t>(stream_end) * 4 <= NN && stream_end > 0 &&
            static_cast<int64_t>(H) * NN * 4 < (1ll << 31)) {
            // Software-pipelined form (fp32 slabs, option "self_chain_pipe"): the pass is a flat sequence of load batches
            // (layer, chunk of this lane, 4 heads x 2 arrays); batch i + 1 is ISSUED before batch i is reduced, so 8 16-byte
            // loads per lane are always in flight -- also across the chunk's LDS write and across the per-layer barrier (the
            // plain loop below drains its loads at every chunk and restarts cold after every barrier).  Raw buffer loads: one
            // wave-uniform resource per (layer, array), a scalar head offset, ONE lane offset register for all 16 loads of two
            // batches, which is what lets two batches fit the 128-VGPR budget of the 1024-thread workgroup.
            // Chunk-to-lane mapping: a stream wave owns blocks of 64 * CPL consecutive chunks and a batch is 4 / CPL heads x CPL
            // chunks x 2 arrays, so that one batch reads CPL KB CONTIGUOUS per (head, array) instead of 1 KB from each of 8
            // streams (CPL = 1).  CPL is as large as still leaves every stream wave a block (text tower, 77 tokens: 1408 chunks
            // = 11 waves x 128 -> CPL = 2).  Heads are summed in ascending order whatever CPL: bit-identical results.
            auto run = [&](auto cpl_tag, auto aux_tag) {
                constexpr int CPL = decltype(cpl_tag)::value, HPB = 4 / CPL;
                // cache policy of the slab loads (buffer aux bits: 2 = nt).  The gradient slab is read exactly once per launch;
                // the probability slab as well unless the batch shares one forward (attn_bstride == 0: every sample re-reads it
                // from L2, so it keeps the default policy).
                constexpr int AUXG = decltype(aux_tag)::value, AUXA = decltype(aux_tag)::value & 1 ? 0 : decltype(aux_tag)::value;
                constexpr int NW = LT / 64;
                const int ws = wave - NT;                                   // this stream wave
                const int nk = (stream_end + LT * CPL - 1) / (LT * CPL);   // rounds (lanes past the end redo the last chunk)
                const int HB = (H + HPB - 1) / HPB;
                const int total = L * nk * HB;
                const int hstride = static_cast<int>(NN) * 4;
                auto issue = [&](int it, u32x4 (&av)[4], u32x4 (&gv)[4]) {
                    const int hb = it % HB, k = (it / HB) % nk, l = it / (HB * nk);
                    const int base = (ws + k * NW) * (64 * CPL) + lane;
                    const auto rA = __builtin_amdgcn_make_buffer_rsrc(
                        const_cast<char*>(sgpr_ptr(reinterpret_cast<const char*>(a.attn[l0 + l]) + sampleA * 4)), 0, 0x7fffffff,
                        kRawBufferFlags);
                    const auto rG = __builtin_amdgcn_make_buffer_rsrc(
                        const_cast<char*>(sgpr_ptr(reinterpret_cast<const char*>(a.grad[l0 + l]) + sample * 4)), 0, 0x7fffffff,
                        kRawBufferFlags);
#pragma unroll
                    for (int u = 0; u < HPB; ++u) {
                        const int hoff = min(hb * HPB + u, H - 1) * hstride;        // clamped: no conditional load
#pragma unroll
                        for (int jj = 0; jj < CPL; ++jj) {
                            const unsigned voff = static_cast<unsigned>(min(base + jj * 64, stream_end - 1)) * 16u;
                            av[u * CPL + jj] = __builtin_amdgcn_raw_buffer_load_b128(rA, voff, hoff, AUXA & ~1);
                            gv[u * CPL + jj] = __builtin_amdgcn_raw_buffer_load_b128(rG, voff, hoff, AUXG & ~1);
                        }
                    }
                };
                f32x4 s[CPL];
#pragma unroll
                for (int jj = 0; jj < CPL; ++jj) s[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
                auto consume = [&](int it, bool valid, const u32x4 (&av)[4], const u32x4 (&gv)[4]) {
                    const int hb = it % HB, k = (it / HB) % nk, l = it / (HB * nk);
#pragma unroll
                    for (int u = 0; u < HPB; ++u) {
                        // heads in order: the same sum as the plain loop.  Every loaded register is USED unconditionally (a
                        // head beyond H is a clamped duplicate of head H - 1): behind a branch the compiler would have to assume
                        // the skipped loads still pending and drain vmcnt before the next batch may overwrite their registers.
                        // The duplicate is SELECTED away, not multiplied by 0 (inf * 0 would plant a NaN where the reference has
                        // +inf), as in chain_stream.h; on finite values the bits are those of the weighted form.
                        const bool on = valid && hb * HPB + u < H;
#pragma unroll
                        for (int jj = 0; jj < CPL; ++jj) {
                            const f32x4 x = __builtin_bit_cast(f32x4, gv[u * CPL + jj]) * __builtin_bit_cast(f32x4, av[u * CPL + jj]);
                            s[jj][0] += on ? relu_nan(x[0]) : 0.f; s[jj][1] += on ? relu_nan(x[1]) : 0.f;
                            s[jj][2] += on ? relu_nan(x[2]) : 0.f; s[jj][3] += on ? relu_nan(x[3]) : 0.f;
                        }
                    }
                    if (valid && hb == HB - 1) {
                        float* Ab = smem + (l & 1) * NP * S;
#pragma unroll
                        for (int jj = 0; jj < CPL; ++jj) {
                            const int c = (ws + k * NW) * (64 * CPL) + jj * 64 + lane;
                            if (c < stream_end) {
                                const int p = c * 4;
                                int row = p / N, cc = p - row * N;
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    Ab[row * S + cc] = s[jj][e] / fH;
                                    if (++cc == N) { cc = 0; ++row; }
                                }
                            }
                            s[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
                        }
                        if (k == nk - 1) __syncthreads();  // publish A_bar_l (pairs with the matrix waves' barrier of layer l)
                    }
                };
                // Two register sets; every issue is UNCONDITIONAL (past the end: the last batch again, consumed with nothing selected)
                // so that the number of loads in flight is the same on every path -- with a conditional issue the compiler
                // merges the two paths' wait counts and drains everything before each reduction.
                u32x4 a0[4], g0[4], a1[4], g1[4];
                if (total > 0) issue(0, a0, g0);
                for (int it = 0; it < total; it += 2) {
                    issue(min(it + 1, total - 1), a1, g1);
                    consume(it, true, a0, g0);
                    issue(min(it + 2, total - 1), a0, g0);
                    consume(min(it + 1, total - 1), it + 1 < total, a1, g1);
                }
            };
            constexpr int NWs = LT / 64;
            // aux tag: 0 default policy | 2 nt on both slabs | 3 nt on the gradient slab only (bit 0 = "probabilities are shared")
            auto run_cpl = [&](auto aux_tag) {
                if (a.pipe >= 4 && stream_end >= NWs * 256) run(std::integral_constant<int, 4>{}, aux_tag);
                else if (a.pipe >= 2 && stream_end >= NWs * 128) run(std::integral_constant<int, 2>{}, aux_tag);
                else run(std::integral_constant<int, 1>{}, aux_tag);
            };
            if (!a.nt) run_cpl(std::integral_constant<int, 0>{});
            else if (a.attn_bstride == 0) run_cpl(std::integral_constant<int, 3>{});
            else run_cpl(std::integral_constant<int, 2>{});
        } else
        for (int l = 0; l < L; ++l) {
            float* Ab = smem + (l & 1) * NP * S;
            const void* A = a.attn[l0 + l];
            const void* Gr = a.grad[l0 + l];
            for (int c = lt; c < stream_end; c += LT) reduce_chunk(c, A, Gr, Ab);
            __syncthreads();  // publish A_bar_l (pairs with the matrix waves' barrier of layer l)
        }
    }
    if (G == 1 || (a.debug & 1)) return;

    // ------------------------------------------------------------------ hand-off + combine (G > 1)
    // R = P_{G-1} . ... . P_1 . P_0 (P_0 already includes R_init).  Mathematically the sequential chain; the
    // products are re-associated at the group boundaries (rounding-level difference, tests bound it at 1e-5).
    unsigned* ticket_lds = reinterpret_cast<unsigned*>(smem + 2 * NP * S - 4);  // inside the (zero) row padding
    const unsigned ticket = chain_handoff_ticket(a.counters + b, ticket_lds, tid);
    if (ticket != static_cast<unsigned>(G - 1)) return;
    if (tid == 0) {
        *ticket_lds = 0u;  // restore the zero padding
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    const float* part = a.parts + static_cast<int64_t>(b) * G * NN;
    if (wave < NT) chain_slab_load<int64_t>(Rold, true, part, 0, N, q);
    constexpr int CE = (NP * NP + kChainThreads - 1) / kChainThreads;  // elements of a partial product per thread
    float pre[CE];
    auto prefetch = [&](int gg) {
        const float* P = part + gg * NN;
#pragma unroll
        for (int i = 0; i < CE; ++i) {
            const int idx = tid + i * kChainThreads;
            pre[i] = (idx < N * N) ? P[idx] : 0.f;
        }
    };
    prefetch(1);
    for (int gg = 1; gg < G; ++gg) {
#pragma unroll
        for (int i = 0; i < CE; ++i) {
            const int idx = tid + i * kChainThreads;
            if (idx < N * N) {
                const int row = idx / N, cc = idx - row * N;
                smem[row * S + cc] = pre[i];
            }
        }
        lds_barrier();
        if (gg + 1 < G) prefetch(gg + 1);  // in flight while the MFMAs run
        if (wave < NT) {
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) Rnew[ti] = chain_tile_product(smem, ti, Rold, lane, q, std::false_type{}, wave);
#pragma unroll
            for (int t = 0; t < NT; ++t) Rold[t] = Rnew[t];
        }
        lds_barrier();
    }
    if (wave < NT) chain_slab_store<int64_t>(a.R_out, b * NN, Rold, N, q, false, false);
}

// ------------------------------------------------------------------------------------------------------------ host side
// half_chain: the fp16-mode chain (R16), one group.  grp.G > 1: the partial products and tickets of the layer groups.
int self_chain_fused_launch(const ChainCall& c, int dtype, const ChainGroups& grp, int pipe, bool half_chain, hipStream_t s) {
    ChainArgs args;
    chain_fill_args(args, c);
    args.G = grp.G;
    args.counters = grp.counters;
    args.parts = grp.parts;
    args.pipe = pipe;
    return dispatch_nt((c.N + 15) / 16, [&](auto nt_tag) -> int {
        constexpr int NT = decltype(nt_tag)::value;
        const size_t lds = sizeof(float) * 2 * kChainNP<NT> * kChainS<NT>;
        void (*kern)(const ChainArgs) = nullptr;
        switch (dtype) {
            case MMX_F32: kern = half_chain ? self_chain_fused_kernel<NT, MMX_F32, true> : self_chain_fused_kernel<NT, MMX_F32, false>; break;
            case MMX_F16: kern = half_chain ? self_chain_fused_kernel<NT, MMX_F16, true> : self_chain_fused_kernel<NT, MMX_F16, false>; break;
            case MMX_BF16: if (!half_chain) { kern = self_chain_fused_kernel<NT, MMX_BF16, false>; break; }
                [[fallthrough]];
            default: set_error("self_chain: unsupported dtype %d%s", dtype, half_chain ? " for the fp16 chain" : ""); return MMX_EINVAL;
        }
        if (int rc = set_dynamic_lds(kern, lds)) return rc;
        if (args.G > 1) {
            int zrc = zero_async(args.counters, sizeof(unsigned) * args.B, s);
            if (zrc) return zrc;
        }
        kern<<<args.B * args.G, kChainThreads, lds, s>>>(args);
        MMX_LAUNCH_CHECK("self_chain_fused_kernel");
        return MMX_OK;
    });
}

}  // namespace mmx
