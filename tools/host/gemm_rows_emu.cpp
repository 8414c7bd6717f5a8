// Host emulation of gemm_rows_f32_kernel and gemm_rows_f16_kernel: csrc/gemm_rows_core.h, csrc/gemm_rows_f32.hip and csrc/gemm_rows_f16.hip
// themselves (MMX_GEMM_ROWS_EMU leaves their launches and C entries out) compiled for the host, one std::thread per work-item, std::barrier
// for s_barrier, each MFMA as a wave-collective fmaf chain in the lane / k layout the kernels' comments state.  It checks the index
// arithmetic of the staging ring, the LDS stages and the epilogues against a float64 product (the bounds of the GPU tests) with a sentinel
// in unlisted rows; built with the host compiler's thread sanitizer it also checks that the kernels' barriers order every LDS access (every
// __shared__ access is a plain memory access here).  It says nothing about the real instructions' internal order, wait counts or speed.
#include <barrier>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <memory>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
struct Dim { int x; };
static thread_local Dim threadIdx, blockIdx;
static std::barrier<>* g_wg_barrier;
static std::barrier<>* g_wave_barrier[4];
static float g_ma[4][64], g_mb[4][64];
static f16x8 g_ha[4][64], g_hb[4][64];
#define __global__
#define __device__
#define __forceinline__ inline
#define __shared__ static
#define __restrict__
#define __launch_bounds__(...)
#define __builtin_amdgcn_sched_barrier(mask) ((void)0)
using std::min;
static f32x4 ldg4_u(const float* p) { f32x4 v; std::memcpy(&v, p, sizeof v); return v; }
static void lds_barrier() { g_wg_barrier->arrive_and_wait(); }
static void __syncthreads() { g_wg_barrier->arrive_and_wait(); }
static float quick_gelu_f(float v) { return v / (1.f + std::exp(-1.702f * v)); }
static void set_error(const char*, ...) {}
// v_mfma_f32_32x32x2_f32: lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][col l & 31]; D: col = l & 31, row = (v & 3) + 8 (v >> 2) + 4 (l >> 5)
static f32x16 emu_mfma(float a, float b, f32x16 acc, int, int, int) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lg = lane >> 5;
    g_ma[wave][lane] = a; g_mb[wave][lane] = b;
    g_wave_barrier[wave]->arrive_and_wait();
    for (int v = 0; v < 16; ++v) {
        const int row = (v >> 2) * 8 + lg * 4 + (v & 3);
        float d = acc[v];
        for (int k = 0; k < 2; ++k) d = std::fmaf(g_ma[wave][row + 32 * k], g_mb[wave][li + 32 * k], d);
        acc[v] = d;
    }
    g_wave_barrier[wave]->arrive_and_wait();
    return acc;
}
// v_mfma_f32_32x32x16_f16: lane l holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31], j = 0..7; D as above
static f32x16 emu_mfma_f16(f16x8 a, f16x8 b, f32x16 acc, int, int, int) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lg = lane >> 5;
    g_ha[wave][lane] = a; g_hb[wave][lane] = b;
    g_wave_barrier[wave]->arrive_and_wait();
    for (int v = 0; v < 16; ++v) {
        const int row = (v >> 2) * 8 + lg * 4 + (v & 3);
        float d = acc[v];
        for (int k = 0; k < 16; ++k)
            d = std::fmaf(static_cast<float>(g_ha[wave][row + 32 * (k >> 3)][k & 7]), static_cast<float>(g_hb[wave][li + 32 * (k >> 3)][k & 7]), d);
        acc[v] = d;
    }
    g_wave_barrier[wave]->arrive_and_wait();
    return acc;
}
#define __builtin_amdgcn_mfma_f32_32x32x2f32 emu_mfma
#define __builtin_amdgcn_mfma_f32_32x32x16_f16 emu_mfma_f16
#define MMX_GEMM_ROWS_EMU
#include "gemm_rows_f32.hip"
#include "gemm_rows_f16.hip"

// One workgroup after the other, 256 threads each.  A thread that returns early must drop out of the barriers: the kernels return only
// workgroup-uniformly before the first barrier, or after the last one.
template <class Body>
static void launch(int grid, Body body) {
    for (int b = 0; b < grid; ++b) {
        std::barrier<> wg(256); g_wg_barrier = &wg;
        std::unique_ptr<std::barrier<>> wb[4];
        for (int w = 0; w < 4; ++w) { wb[w].reset(new std::barrier<>(64)); g_wave_barrier[w] = wb[w].get(); }
        std::vector<std::thread> th;
        for (int t = 0; t < 256; ++t) th.emplace_back([=] { threadIdx.x = t; blockIdx.x = b; body(); });
        for (auto& x : th) x.join();
    }
}
// The two kernels as the cases see them: the weight's element type and layout ([K][N] fp32 | [N][K] fp16), the rounding of A, the unit
// of the bound, and a launch per epilogue.
template <int TM_, int TN_, int BK_, int PF_>
struct F32 {
    static constexpr int TM = TM_, TN = TN_, BK = BK_, PF = PF_;
    static constexpr const char* name = "f32";
    typedef float W;
    static size_t w_at(int k, int n, int N, int K) { return (size_t)k * N + n; }
    static double a_val(float a) { return a; }
    static double unit() { return std::ldexp(1.0, -24); }
    static int terms(int K, int) { return K + 1; }      // (gamma_(K+1) for every epilogue: tests/test_gpu_gemm_rows_pipeline.py)
    template <int EPI, class... Args> static void run(Args... args) { mmx::gemm_rows_f32_kernel<TM, TN, BK, PF, EPI>(args...); }
};
template <int TM_, int TN_, int BK_, int PF_>
struct F16 {
    static constexpr int TM = TM_, TN = TN_, BK = BK_, PF = PF_;
    static constexpr const char* name = "f16";
    typedef _Float16 W;
    static size_t w_at(int k, int n, int N, int K) { return (size_t)n * K + k; }
    static double a_val(float a) { return static_cast<double>(static_cast<_Float16>(a)); }   // the reference reads the ROUNDED operand
    static double unit() { return std::ldexp(1.0, -23); }
    static int terms(int K, int epi) { return K + (epi ? 1 : 0); }   // (gamma_K, with a bias gamma_(K+1): tests/test_gpu_gemm_rows_half.py)
    template <int EPI, class... Args> static void run(Args... args) { mmx::gemm_rows_f16_kernel<TM, TN, BK, PF, EPI>(args...); }
};
template <class Kn>
static int run_case(int cap, int N, int K, const std::vector<int>& list, int count_override) {
    typedef typename Kn::W W;
    std::vector<float> A((size_t)cap * K), bias(N);
    std::vector<W> Wt((size_t)K * N);
    for (auto& v : A) v = (rand() % 2001 - 1000) / 1000.f;
    for (auto& v : Wt) v = static_cast<W>((rand() % 2001 - 1000) / 1000.f);
    for (auto& v : bias) v = (rand() % 2001 - 1000) / 1000.f;
    std::vector<int> rows(cap, -7);
    for (size_t i = 0; i < list.size(); ++i) rows[i] = list[i];
    int count = count_override >= 0 ? count_override : (int)list.size();
    std::vector<char> listed(cap, 0);
    for (int i = 0; i < std::min(count, cap); ++i) if (rows[i] >= 0 && rows[i] < cap) listed[rows[i]] = 1;
    const int grid = ((N + Kn::TN - 1) / Kn::TN) * ((cap + Kn::TM - 1) / Kn::TM);
    std::vector<double> ref((size_t)cap * N, 0.0), mag((size_t)cap * N, 0.0);
    for (int r = 0; r < cap; ++r)
        for (int n = 0; n < N; ++n)
            for (int k = 0; listed[r] && k < K; ++k) {
                const double p = Kn::a_val(A[(size_t)r * K + k]) * static_cast<double>(Wt[Kn::w_at(k, n, N, K)]);
                ref[(size_t)r * N + n] += p;
                mag[(size_t)r * N + n] += std::fabs(p);
            }
    int bad = 0;
    for (int epi = 0; epi < 3; ++epi) {
        std::vector<float> C((size_t)cap * N, 7.25f), C2((size_t)cap * N, 7.25f);
        const float* a = A.data(); const W* w = Wt.data(); float *c = C.data(), *c2 = C2.data(); const float* bs = bias.data();
        const int *rw = rows.data(), *cn = &count;
        if (epi == 0) launch(grid, [=] { Kn::template run<0>(a, w, c, rw, cn, cap, N, K, (const float*)nullptr, (float*)nullptr); });
        if (epi == 1) launch(grid, [=] { Kn::template run<1>(a, w, c, rw, cn, cap, N, K, bs, (float*)nullptr); });
        if (epi == 2) launch(grid, [=] { Kn::template run<2>(a, w, c, rw, cn, cap, N, K, bs, c2); });
        const int terms = Kn::terms(K, epi);
        const double g = terms * Kn::unit() / (1 - terms * Kn::unit());
        for (int r = 0; r < cap; ++r)
            for (int n = 0; n < N; ++n) {
                const float got = C[(size_t)r * N + n], got2 = C2[(size_t)r * N + n];
                if (!listed[r]) { if (got != 7.25f || got2 != 7.25f) ++bad; continue; }
                const double want = ref[(size_t)r * N + n] + (epi ? bias[n] : 0.f), m = mag[(size_t)r * N + n] + (epi ? std::fabs(bias[n]) : 0.f);
                if (!(std::fabs(got - want) <= g * m)) ++bad;
                if (epi == 2 && got2 != quick_gelu_f(got)) ++bad;
                if (epi != 2 && got2 != 7.25f) ++bad;
            }
    }
    printf("%s TM%d TN%d BK%d PF%d cap %d N %d K %d count %d: %s (%d bad)\n", Kn::name, Kn::TM, Kn::TN, Kn::BK, Kn::PF, cap, N, K, count,
           bad ? "FAIL" : "ok", bad);
    fflush(stdout);
    return bad;
}
static std::vector<int> range(int a, int b) { std::vector<int> v; for (int i = a; i < b; ++i) v.push_back(i); return v; }
static std::vector<int> shuffled(int cap, int keep) {
    std::vector<int> v = range(0, cap);
    for (int i = cap - 1; i > 0; --i) std::swap(v[i], v[rand() % (i + 1)]);
    v.resize(keep);
    return v;
}
// fp32 at another depth of the register ring (option "gemm_rows_pf"): slab counts around the ring -- one fewer, exactly the ring, one more
// and ragged, two rounds and a ragged remainder -- and the shuffled row list (tests/test_gpu_gemm_rows_depth.py walks every count on the GPU)
template <int TM, int TN, int BK, int PF>
static int run_depth_f32() {
    typedef F32<TM, TN, BK, PF> Kn;
    int bad = 0;
    std::vector<int> some = {0, 1, 2, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    for (int K : {(PF - 1) * BK, PF * BK, (PF + 1) * BK + 4, (2 * PF + 1) * BK + 4}) bad += run_case<Kn>(24, 100, K, some, -1);
    bad += run_case<Kn>(70, 100, 200, shuffled(70, 45), -1);
    return bad;
}
// fp32: the slab-count and row-list cases of tests/test_gpu_gemm_rows_pipeline.py at depth 3, then the other depth the library ships
template <int TM, int TN, int BK>
static int run_all_f32() {
    typedef F32<TM, TN, BK, 3> Kn;
    int bad = run_depth_f32<TM, TN, BK, 4>();
    std::vector<int> some = {0, 1, 2, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    for (int K : {4, 20, 32, 36, 64, 68, 96, 128, 192, 200, 256})
        for (int N : {36, 100}) bad += run_case<Kn>(24, N, K, some, -1);
    bad += run_case<Kn>(24, 64, 2048, some, -1);
    bad += run_case<Kn>(70, 36, 36, {}, -1);
    bad += run_case<Kn>(70, 36, 36, {41}, -1);
    bad += run_case<Kn>(70, 100, 200, range(0, 70), -1);
    bad += run_case<Kn>(70, 100, 200, range(0, 70), 79);
    bad += run_case<Kn>(70, 100, 200, range(3, 36), -1);
    bad += run_case<Kn>(70, 100, 200, {5, -1, 17, 70, 64, 370, 33}, -1);
    bad += run_case<Kn>(70, 100, 200, shuffled(70, 45), -1);
    return bad;
}
// fp16: the K and N lists and the row lists of tests/test_gpu_gemm_rows_half.py (72 rows: three 32-row tiles, the last one ragged)
template <int TN, int BK, int PF>
static int run_all_f16() {
    typedef F16<32, TN, BK, PF> Kn;
    const int cap = 72;
    int bad = 0;
    std::vector<int> captions = range(0, 21), second = range(24, 48);   // 3 captions of 24 tokens, EOT at 20, 23, 0: 45 rows
    captions.insert(captions.end(), second.begin(), second.end());
    captions.push_back(48);
    std::vector<int> ks = {8, BK, BK + 8, (PF - 1) * BK, PF * BK, (PF + 1) * BK, 2 * PF * BK, (PF + 1) * BK + 8};
    std::sort(ks.begin(), ks.end());
    ks.erase(std::unique(ks.begin(), ks.end()), ks.end());
    for (int K : ks)
        for (int N : {8, 40, 64, 104}) bad += run_case<Kn>(cap, N, K, captions, -1);
    const int shapes[2][2] = {{BK + 8, 40}, {(PF + 1) * BK + 8, 104}};
    for (auto& kn : shapes) {
        const int K = kn[0], N = kn[1];
        bad += run_case<Kn>(cap, N, K, {}, -1);
        bad += run_case<Kn>(cap, N, K, {41}, -1);
        bad += run_case<Kn>(cap, N, K, range(3, 34), -1);
        bad += run_case<Kn>(cap, N, K, range(5, 37), -1);
        bad += run_case<Kn>(cap, N, K, range(2, 35), -1);
        bad += run_case<Kn>(cap, N, K, range(0, cap), -1);
        bad += run_case<Kn>(cap, N, K, shuffled(cap, 45), -1);
        bad += run_case<Kn>(cap, N, K, {5, -1, 17, cap, 64, cap + 300, 33}, -1);
        bad += run_case<Kn>(cap, N, K, range(0, cap), cap + 9);
    }
    return bad;
}
int main() {
    int bad = run_all_f32<32, 64, 32>() + run_all_f32<64, 64, 32>() + run_all_f32<32, 32, 64>();
    bad += run_all_f16<32, 128, 2>() + run_all_f16<64, 64, 3>();
    printf("TOTAL bad %d\n", bad);
    return bad != 0;
}
