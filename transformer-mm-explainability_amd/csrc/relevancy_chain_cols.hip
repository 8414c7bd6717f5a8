// K1c  self_chain_cols_kernel: the self-attention relevancy chain (rules 5 + 6, all layers in one launch) in strict layer order, one
// workgroup per sample by default -- what runs for fp32 slabs when the batch alone fills the chip (no layer groups), and the
// experiment VERDICT r04 asked for (split by COLUMNS of R over several workgroups of a sample).
//
//     R <- R + A_bar_l . R   (l = 0 .. L-1, strict order),   A_bar_l = mean_h clamp(G_l * A_l, 0)
//
// is independent per column of R.  A sample's C workgroups each own every C-th 16-column slab of R over ALL layers (MFMA accumulators
// of one wave per slab: the K1 trick), and each of them reduces the FULL A_bar_l of every layer itself.  With C > 1 the workgroups
// of a sample are placed on one XCD (ids congruent mod 8), so a slab line is fetched from HBM by whichever of them asks first and
// re-served from that XCD's L2 to the others; workgroup c starts every layer at block c * NBLK / C so that each of them is the first
// to ask for a different part.  There are no partial products, no hand-off, no counters in global memory, no scratch: the result is
// the sequential chain, bit-identical to self_chain_fused_kernel with one group, at any batch size.
//
// Measured (profiles/r05_chain_cols_probe.txt): C = 2..4 at B = 64 takes 107-137 us against 73-74 us of the layer-group kernel -- a CU
// ingests ~43 GB/s at most, from L2 as from HBM, and every workgroup has to ingest the sample's whole 4.58 MB.  C = 1 however beats
// the fused kernel's single-group form at every batch (B = 64 118 vs 145 us, B = 160 139 vs 162 us, B = 256 202 vs 207 us at CLIP's
// text shape) because its stream waves never meet a barrier: it is the default for fp32 slabs whenever one group is chosen.
//
// Reference sites: CLIP_explainability.ipynb cell 6:22-32 / 45-55, CLIP/example.py:22-30, ViT notebook cell 7:28-33,
// VisualBERT/.../ExplanationGenerator.py:86-93 (include/mmx_relevancy.h, mmx_relevancy_self_chain).
//
// Inside a workgroup (1024 threads): `nown` matrix waves (one per owned slab) + 16 - nown stream waves.  Stream waves are the
// barrier-free register pipelines of relevancy_chain_groups.hip (64-chunk blocks of (layer, block) items in layer order, heads
// summed in ascending order), scattering into a ring of NB LDS images of A_bar (slot l % NB) and counting arrivals per 16-row tile;
// a matrix wave follows tile by tile.  Back-pressure on the ring: a stream wave about to write layer l waits until every matrix wave
// has finished layer l - NB (progress words in LDS) -- the matrix waves need 1.3 us per layer against ~5 us of streaming, so it
// does not wait in practice.
#include "chain_launch.h"
#include "chain_matrix.h"
#include "chain_stream.h"

namespace mmx {

struct ColsArgs {
    const void* attn[MMX_MAX_LAYERS];
    const void* grad[MMX_MAX_LAYERS];
    int n_layers, B, H, N;
    int C;               // workgroups per sample (<= NT)
    int NB;              // LDS images of A_bar (ring)
    int nchunks;         // ceil(N*N / 4)
    unsigned row_magic;  // ceil(2^32 / N): row = (p * magic) >> 32, exact for p < N*N + 8
    const float* R_init;
    float* R_out;
    int64_t attn_bstride;
    int nt;
    int causal;          // MMX_CHAIN_CAUSAL: chunks entirely above the diagonal are not requested (chain_stream.h)
    int debug;           // profiling only: bit0 = matrix waves skip the MFMAs, bit1 = no block rotation
};

constexpr int kColsThreads = 1024;
constexpr int kColsWaves = kColsThreads / 64;

template <int NT>
__global__ __launch_bounds__(kColsThreads) void self_chain_cols_kernel(const ColsArgs a) {
    constexpr int NP = kChainNP<NT>;
    constexpr int S = kChainS<NT>;
    extern __shared__ __attribute__((aligned(16))) float smem[];   // NB images (NP x S floats) + NB x NT arrival counters + 16 progress words

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int C = a.C, NB = a.NB;
    int b, c;       // the C workgroups of a sample on one XCD
    chain_xcd_placement(blockIdx.x, a.B, C, b, c);
    const int N = a.N, H = a.H, L = a.n_layers;
    const int NN = N * N;
    const int nown = (NT - c + C - 1) / C;                                     // slabs c, c + C, ... < NT
    unsigned* lds_cnt = reinterpret_cast<unsigned*>(smem + NB * NP * S);       // [NB][NT] elements landed per (slot, 16-row tile), cumulative
    unsigned* prog = lds_cnt + NB * NT;                                        // [16] layers finished per matrix wave

    // pads must read as 0; counters = 0  (rounded up: the allocation has the slack)
    chain_lds_zero(smem, (NB * NP * S + NB * NT + 16 + 3) >> 2, tid, kColsThreads);
    __syncthreads();

    const int NBLK = (a.nchunks + 63) >> 6;            // 64-chunk blocks per layer
    const int rot = (a.debug & 2) ? 0 : (c * NBLK) / C;

    if (wave >= nown) {
        // =============================================================================================== stream waves (chain_stream.h)
        const ChainStreamGeom gm{a.attn, a.grad, 0, NBLK, rot, a.nchunks, H, NN, b, a.B, a.attn_bstride, (a.nt && C == 1) ? 1 : 0, a.causal, N, a.row_magic};
        // (with several workgroups per sample the partners re-read every line from L2: default cache policy)
        chain_stream_wave(gm, wave - nown, kColsWaves - nown, L * NBLK, lane, [&](int l, int cidx, f32x4 mean) {
            const int slot = l % NB;
            if (l >= NB) {
                // ring back-pressure: every matrix wave must have left layer l - NB (bounded like every wait here)
                const unsigned need = static_cast<unsigned>(l - NB + 1);
                int turns = 0;
                while (!__all(lane >= nown ||
                              __hip_atomic_load(prog + (lane & 15), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >= need) &&
                       ++turns < (1 << 24))
                    __builtin_amdgcn_s_sleep(1);
                if (turns >= (1 << 24) && lane == 0) prog[15] = 1u;        // (word 15 is no wave's progress: "a wait gave up")
            }
            // arrival counts are cumulative over the uses of the slot
            chain_stream_deliver(smem + slot * NP * S, S, lds_cnt + slot * NT, cidx, lane, a.nchunks, N, NN, a.row_magic, mean);
        });
    } else {
        // =============================================================================================== matrix waves
        const int slab = c + wave * C;
        const ChainLane q = chain_lane(slab, lane);
        f32x4 Rold[NT], Rnew[NT];
        chain_slab_load<int>(Rold, a.R_init != nullptr, a.R_init, static_cast<int64_t>(b) * NN, N, q);
        bool poisoned = false;
        for (int l = 0; l < L; ++l) {
            const int slot = l % NB;
            const unsigned uses = static_cast<unsigned>(l / NB + 1);    // arrival counts are cumulative over the uses of the slot
#pragma unroll
            for (int ti = 0; ti < NT; ++ti) {
                if (chain_tile_wait(lds_cnt + slot * NT + ti, N, ti, uses)) poisoned = true;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                if (!(a.debug & 1)) acc = chain_tile_product(smem + slot * NP * S, ti, Rold, lane, q, std::false_type{}, slab);
                Rnew[ti] = Rold[ti] + acc;                  // R + (A_bar . R): same association as the reference
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) Rold[t] = Rnew[t];
            // this wave's reads of the slot are done (its MFMAs have their operands): release it to the stream waves
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) __hip_atomic_store(prog + wave, static_cast<unsigned>(l + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        if (__hip_atomic_load(prog + 15, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) poisoned = true;
        chain_slab_store<int>(a.R_out + static_cast<int64_t>(b) * NN, 0, Rold, N, q, false, poisoned);
    }
}

// ------------------------------------------------------------------------------------------------------------ host side
static size_t cols_lds_bytes(int nt, int nb) {
    return sizeof(float) * (static_cast<size_t>(nb) * nt * 16 * (nt * 16 + 4) + static_cast<size_t>(nb) * nt + 20);
}

static int g_cols_c = 0, g_cols_nb = 0;    // 0 = auto
void chain_cols_options(int c, int nb) {
    if (c >= 0) g_cols_c = c;
    if (nb >= 0) g_cols_nb = nb;
}

// workgroups per sample / ring depth
static void cols_plan(int n_layers, int B, int N, int* C, int* NB) {
    const int nt = (N + 15) / 16;
    // One workgroup per sample unless asked: a CU ingests at most ~43 GB/s whether the lines come from HBM or from its XCD's L2
    // (profiles/r05_chain_cols_probe.txt: 4.58 MB per sample = 107-137 us with C = 2..4 at B = 64), so several workgroups that each
    // reduce the whole sample never beat the layer-group kernel; C > 1 stays as the measured experiment.
    (void)B;
    int c = g_cols_c ? g_cols_c : 1;
    if (c > nt) c = nt;
    int nb = g_cols_nb ? g_cols_nb : 6;
    while (nb > 1 && cols_lds_bytes(nt, nb) > 160 * 1024) --nb;
    if (nb > n_layers && n_layers > 0) nb = n_layers;
    *C = c;
    *NB = nb;
}

bool self_chain_cols_applies(int n_layers, int B, int H, int N) {
    const int nt = (N + 15) / 16;
    return n_layers >= 1 && nt <= 8 && cols_lds_bytes(nt, 1) <= 160 * 1024 && static_cast<size_t>(H) * N * N * 4 < (1ull << 31);
}

int self_chain_cols_launch(const ChainCall& c, hipStream_t s) {
    ColsArgs r;
    chain_fill_stream_args(r, c);
    cols_plan(r.n_layers, r.B, r.N, &r.C, &r.NB);
    r.debug = ((c.debug & 4) ? 1 : 0) | ((c.debug & 16) ? 2 : 0);      // option "debug_flags" -> this kernel's own bits
    return dispatch_nt((r.N + 15) / 16, [&](auto nt_tag) -> int {
        constexpr int NT = decltype(nt_tag)::value;
        const size_t lds = cols_lds_bytes(NT, r.NB);
        if (int rc = set_dynamic_lds(self_chain_cols_kernel<NT>, lds)) return rc;
        self_chain_cols_kernel<NT><<<r.B * r.C, kColsThreads, lds, s>>>(r);
        MMX_LAUNCH_CHECK("self_chain_cols_kernel");
        return MMX_OK;
    });
}

}  // namespace mmx
