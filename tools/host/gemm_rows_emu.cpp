// Host emulation of gemm_rows_f32_kernel (csrc/gemm_rows_f32.hip): the kernel's own text (gemm_rows_kernel.inc, cut out of the .hip by
// tools/emu_gemm_rows.py) compiled for the host, one std::thread per work-item, std::barrier for s_barrier, the MFMA as a wave-collective
// fmaf chain.  It checks the index arithmetic of the staging ring, the LDS stages and the epilogues against a float64 product (the bound of
// the GPU tests) with a sentinel in unlisted rows; built with the host compiler's thread sanitizer it also checks that the kernel's barriers order every LDS
// access (every __shared__ access is a plain memory access here).  It says nothing about wait counts or speed.
#include <barrier>
#include <thread>
#include <vector>
#include <cstdio>
#include <cstdint>
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <memory>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
struct Dim { int x; };
static thread_local Dim threadIdx, blockIdx;
static std::barrier<>* g_wg_barrier;
static std::barrier<>* g_wave_barrier[4];
static float g_ma[4][64], g_mb[4][64];
#define __global__
#define __shared__ static
#define __restrict__
#define __launch_bounds__(...)
using std::min;
static f32x4 ldg4_u(const float* p) { f32x4 v = {p[0], p[1], p[2], p[3]}; return v; }
static void lds_barrier() { g_wg_barrier->arrive_and_wait(); }
static float quick_gelu_f(float v) { return v / (1.f + std::exp(-1.702f * v)); }
static int __builtin_amdgcn_readfirstlane(int x) { return x; }
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
#define __builtin_amdgcn_mfma_f32_32x32x2f32 emu_mfma
namespace mmx {
#include "gemm_rows_kernel.inc"
}
// NOTE: a thread that returns early must drop out of the barriers; the kernel returns only workgroup-uniformly before barriers, or after the last one
template <int TM, int TN, int BK, int EPI>
static void launch(int grid, const float* A, const float* W, float* C, const int* rows, const int* count, int cap, int N, int K, const float* bias, float* C2) {
    for (int b = 0; b < grid; ++b) {
        std::barrier<> wg(256); g_wg_barrier = &wg;
        std::unique_ptr<std::barrier<>> wb[4];
        for (int w = 0; w < 4; ++w) { wb[w].reset(new std::barrier<>(64)); g_wave_barrier[w] = wb[w].get(); }
        std::vector<std::thread> th;
        for (int t = 0; t < 256; ++t)
            th.emplace_back([=] { threadIdx.x = t; blockIdx.x = b; mmx::gemm_rows_f32_kernel<TM, TN, BK, 3, EPI>(A, W, C, rows, count, cap, N, K, bias, C2); });
        for (auto& x : th) x.join();
    }
}
template <int TM, int TN, int BK>
static int run_case(int cap, int N, int K, const std::vector<int>& list, int count_override) {
    std::vector<float> A((size_t)cap * K), W((size_t)K * N), bias(N);
    for (auto& v : A) v = (rand() % 2001 - 1000) / 1000.f;
    for (auto& v : W) v = (rand() % 2001 - 1000) / 1000.f;
    for (auto& v : bias) v = (rand() % 2001 - 1000) / 1000.f;
    std::vector<int> rows(cap, -7);
    for (size_t i = 0; i < list.size(); ++i) rows[i] = list[i];
    int count = count_override >= 0 ? count_override : (int)list.size();
    std::vector<char> listed(cap, 0);
    for (int i = 0; i < std::min(count, cap); ++i) if (rows[i] >= 0 && rows[i] < cap) listed[rows[i]] = 1;
    const int grid = ((N + TN - 1) / TN) * ((cap + TM - 1) / TM);
    int bad = 0;
    for (int epi = 0; epi < 3; ++epi) {
        std::vector<float> C((size_t)cap * N, 7.25f), C2((size_t)cap * N, 7.25f);
        if (epi == 0) launch<TM, TN, BK, 0>(grid, A.data(), W.data(), C.data(), rows.data(), &count, cap, N, K, nullptr, nullptr);
        if (epi == 1) launch<TM, TN, BK, 1>(grid, A.data(), W.data(), C.data(), rows.data(), &count, cap, N, K, bias.data(), nullptr);
        if (epi == 2) launch<TM, TN, BK, 2>(grid, A.data(), W.data(), C.data(), rows.data(), &count, cap, N, K, bias.data(), C2.data());
        for (int r = 0; r < cap; ++r)
            for (int n = 0; n < N; ++n) {
                const float got = C[(size_t)r * N + n], got2 = C2[(size_t)r * N + n];
                if (!listed[r]) { if (got != 7.25f || got2 != 7.25f) ++bad; continue; }
                double ref = 0, mag = 0;
                for (int k = 0; k < K; ++k) { ref += (double)A[(size_t)r * K + k] * W[(size_t)k * N + n]; mag += std::fabs((double)A[(size_t)r * K + k] * W[(size_t)k * N + n]); }
                if (epi) { ref += bias[n]; mag += std::fabs(bias[n]); }
                const double u = std::ldexp(1.0, -24), g = (K + 1) * u / (1 - (K + 1) * u);
                if (!(std::fabs(got - ref) <= g * mag)) ++bad;
                if (epi == 2 && got2 != quick_gelu_f(got)) ++bad;
                if (epi != 2 && got2 != 7.25f) ++bad;
            }
    }
    printf("TM%d TN%d BK%d cap %d N %d K %d count %d: %s (%d bad)\n", TM, TN, BK, cap, N, K, count, bad ? "FAIL" : "ok", bad);
    fflush(stdout);
    return bad;
}
template <int TM, int TN, int BK>
static int run_all() {
    int bad = 0;
    std::vector<int> some = {0, 1, 2, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    for (int K : {4, 20, 32, 36, 64, 68, 96, 128, 192, 200, 256})
        for (int N : {36, 100}) bad += run_case<TM, TN, BK>(24, N, K, some, -1);
    bad += run_case<TM, TN, BK>(24, 64, 2048, some, -1);
    std::vector<int> all70, r33, shuffled, outside = {5, -1, 17, 70, 64, 370, 33};
    for (int i = 0; i < 70; ++i) all70.push_back(i);
    for (int i = 3; i < 36; ++i) r33.push_back(i);
    shuffled = all70; std::random_shuffle(shuffled.begin(), shuffled.end()); shuffled.resize(45);
    bad += run_case<TM, TN, BK>(70, 36, 36, {}, -1);
    bad += run_case<TM, TN, BK>(70, 36, 36, {41}, -1);
    bad += run_case<TM, TN, BK>(70, 100, 200, all70, -1);
    bad += run_case<TM, TN, BK>(70, 100, 200, all70, 79);
    bad += run_case<TM, TN, BK>(70, 100, 200, r33, -1);
    bad += run_case<TM, TN, BK>(70, 100, 200, outside, -1);
    bad += run_case<TM, TN, BK>(70, 100, 200, shuffled, -1);
    return bad;
}
int main() {
    int bad = run_all<32, 64, 32>() + run_all<64, 64, 32>() + run_all<32, 32, 64>();
    printf("TOTAL bad %d\n", bad);
    return bad != 0;
}
