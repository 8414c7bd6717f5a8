// Device helpers the attention kernels share for bf16 data held as raw words (attention_head.hip, attention_stream.hip,
// attention_bf16.hip, attention_bf16_v3.hip): the word types, fp32 <-> packed bf16, the fast exponential, and the LDS tile layouts
// of the second and third bf16-MFMA generations.
#pragma once
#include "mmx_common.h"

namespace mmx {

typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
typedef unsigned short bf16_t;

__device__ __forceinline__ unsigned pack2_bf16(float lo, float hi) {      // two fp32 -> packed bf16 pair, round to nearest even
    typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
    bf2 r;
    r[0] = static_cast<__bf16>(lo);
    r[1] = static_cast<__bf16>(hi);
    return __builtin_bit_cast(unsigned, r);
}
__device__ __forceinline__ bf16x8 as_bf16x8(u32x4v v) { return __builtin_bit_cast(bf16x8, v); }
__device__ __forceinline__ bf16x8 pack8(f32x4 lo, f32x4 hi) {
    return as_bf16x8(u32x4v{pack2_bf16(lo[0], lo[1]), pack2_bf16(lo[2], lo[3]), pack2_bf16(hi[0], hi[1]), pack2_bf16(hi[2], hi[3])});
}
// packed bf16 -> fp32, exact: the low / high half of a word, and four elements (two words).  (The delta sums of the bf16-MFMA query
// sides take the halves one by one, in the order of their fma chain: with the vector form in front the third generation's kernel
// comes out with another instruction order.)
__device__ __forceinline__ float bflo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bfhi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ f32x4 widen_bf16x4(u32x2v r) { return f32x4{bflo(r[0]), bfhi(r[0]), bflo(r[1]), bfhi(r[1])}; }

// exp(x) = 2^(x log2 e) on the hardware v_exp_f32 (1 ulp).  The rounding of x * log2(e) adds |x| * 6e-8 of relative
// error; the ABSOLUTE error of a probability p = exp(x) is then at most max_x |x| e^x * 6e-8 = 2.2e-8, and its relative
// error stays below the 1e-5 parity bar for every x that does not underflow.  Two instructions instead of libm expf's
// ~15: PMC showed these kernels issue-bound on VALU work around the MFMAs, not HBM-bound.
__device__ __forceinline__ float exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// ---- LDS tiles of the bf16-MFMA generations (attention_bf16.hip, attention_bf16_v3.hip): 64 rows x head dim 64 (padded), bf16.
// Bank-conflict free for every access of those files under the lane-group rules of MI355X_MICROARCH.md (searched by brute force
// over row strides / swizzles; the first version -- 72-element rows, no swizzle -- spent 22 % of its wave cycles in
// SQ_LDS_BANK_CONFLICT: the transposed ds_write_b64 of 16 lanes hit 2 bank positions):
//   row-major tile  [row][d]:  80-element (160 B) rows, no swizzle   (ds_write_b64 by (row, 4 d), ds_read_b128 by (row i, 8 g))
//   transposed tile [d][row]:  80-element rows; the 4-row group index of a row is XOR-ed with (d / 4) & 15
//                              (ds_write_b64 of 4 consecutive rows by 16 lanes of different d; ds_read_b64 by (d = i, group g))
// (Unpadded 64-element rows with XOR swizzles are conflict-free too and would let THREE workgroups fit a CU, but the second
//  generation needs 162-184 VGPRs: under __launch_bounds__(256, 3) it spills 60-128 registers and runs 4 x slower.)
constexpr int kLR = 64 + 16;
constexpr int kLT = 64 + 16;
// where rows 4 grp .. 4 grp + 3 (one 8-byte word) of column d sit in row d of a transposed tile: element offset from tile + d * kLT.
// d4 = d / 4, in whatever form the caller has it (a staging thread's st & 15, a lane's 4 dt + (i >> 2)): taken from d itself the
// compiler no longer sees which bits are lane bits and which are constants, and the kernels' address code changes.
__device__ __forceinline__ int transposed_slot(int d4, int grp) { return 4 * (grp ^ (d4 & 15)); }

// A staging thread st (0 .. 255) owns the 4 x 4 block rows 4 (st / 16) .. + 3, columns 4 (st % 16) .. + 3 of a 64 x 64 tile.
// rows[e] = columns c, c+1 | c+2, c+3 of row e -> column dd as 4 consecutive rows (8 bytes)
__device__ __forceinline__ u32x2v column_of(const u32x2v (&rows)[4], int dd) {
    const int w = dd >> 1;
    const unsigned sel = (dd & 1) ? 0x07060302u : 0x05040100u;     // high / low halves of (row e+1, row e)
    return u32x2v{__builtin_amdgcn_perm(rows[1][w], rows[0][w], sel), __builtin_amdgcn_perm(rows[3][w], rows[2][w], sel)};
}
__device__ __forceinline__ void store_row_major(bf16_t* tile, const u32x2v (&rows)[4], int st) {
    const int r4 = 4 * (st >> 4), c = 4 * (st & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e) *reinterpret_cast<u32x2v*>(tile + (r4 + e) * kLR + c) = rows[e];
}
// column dd of the block (col = column_of(rows, dd)) -> tile[c + dd][r4 .. r4 + 3]: one 8-byte store
__device__ __forceinline__ void store_transposed_col(bf16_t* tile, u32x2v col, int dd, int st) {
    *reinterpret_cast<u32x2v*>(tile + (4 * (st & 15) + dd) * kLT + transposed_slot(st & 15, st >> 4)) = col;
}

}  // namespace mmx
