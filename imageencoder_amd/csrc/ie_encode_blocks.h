// imageencoder_amd/csrc/ie_encode_blocks.h -- what encode_kernel (ie_encode.hip) and encode4p_kernel
// (ie_encode4p.hip) share: zig-zag tables, tile geometry, pixel loads, the FP64 reference-order
// evaluations, rounding, sizing and the emission of records into the LDS bit image.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "ie_common.hpp"
#include "ie_dct.h"
#include "ie_device.h"

namespace ie {

template <int N> struct ZigZag;
template <> struct ZigZag<4> {
    static constexpr int idx[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
};
template <> struct ZigZag<8> {
    static constexpr int idx[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                    12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                    58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
};

// pos[k] = zig-zag position of natural index k (inverse of ZigZag<N>::idx)
template <int N> struct ZigZagInv;
template <> struct ZigZagInv<4> {
    static constexpr int pos[16] = {0, 1, 5, 6, 2, 4, 7, 12, 3, 8, 11, 13, 9, 10, 14, 15};
};
template <> struct ZigZagInv<8> {
    static constexpr int pos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                    3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                    21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
};

#ifndef IE_PROFILE
#define IE_PROFILE 0
#endif
#ifndef IE_BPT4
#define IE_BPT4 4
#endif
#ifndef IE_WAVES4
#define IE_WAVES4 5
#endif
#ifndef IE_WAVES8
#define IE_WAVES8 4
#endif
// Threads per tile (= per workgroup).  256 (four waves, 1024 4x4 blocks); 64 makes every wave an
// independent tile (no workgroup barriers, 16 tiles per CU) but quadruples the look-backs, which
// measured slower.
#ifndef IE_TPB
#define IE_TPB 256
#endif
constexpr int kEncTPB = IE_TPB;
template <int N> struct Geo;
template <> struct Geo<4> {  // IE_BPT4 blocks side by side: 4 * IE_BPT4 bytes per pixel row per lane
    static constexpr int BPT = IE_BPT4;
    static constexpr int WAVES = IE_WAVES4;  // __launch_bounds__ occupancy hint (waves per SIMD)
};
template <> struct Geo<8> {  // one block: 8 bytes per pixel row per lane
    static constexpr int BPT = 1;
    static constexpr int WAVES = IE_WAVES8;  // 4: <= 128 registers
};

#ifndef IE_FIX_UNROLL
#define IE_FIX_UNROLL 16  // exact_coef_row's unroll: terms of a row per step
#endif

template <int WPR>
__device__ __forceinline__ uint32_t pix(const uint32_t (&row)[WPR], int byte) {
    return (row[byte >> 2] >> (8 * (byte & 3))) & 0xFFu;
}

// The pixel bytes of one block, packed four to a word (row-major): the argument of the
// out-of-line FP64 path, passed in registers.
template <int N> struct BlockPx {
    uint32_t w[N * N / 4];
};

// Exact coefficient in the reference's FP64 order (algo.cpp:314-325, Block.cpp:149-152):
//   acc = 0; for i, j: acc = acc + P[uv][ij] * x[ij];  D = acc * (C(u)C(v));  round(D / q)
// with x[ij] = double(p) - 128 (Block.cpp:141-143).  This file is compiled with
// -ffp-contract=off, so every product and sum is rounded separately as in the reference; the
// division is IEEE (a multiply by the exact reciprocal when q is a power of two); the rounding is
// half away from zero (std::round).  Out of line: it runs only for the few coefficients whose
// FP32 quotient lies near a rounding tie, and must not inflate the hot path's registers.
template <int N>
__device__ __forceinline__ int exact_coef_inl(const EncTables* __restrict__ tab, int k, BlockPx<N> px) {
    constexpr int NN = N * N;
    const double* P = &tab->P[k * NN];
    double acc = 0.0;
#pragma unroll
    for (int ij = 0; ij < NN; ij++) {
        const double x = double(int((px.w[ij >> 2] >> (8 * (ij & 3))) & 0xFFu) - 128);  // == double(p) + (-128.0), exactly
        acc = acc + P[ij] * x;
    }
    const double D = acc * tab->S[k];
    const double rq = tab->rq[k];
    const double t = (rq != 0.0) ? D * rq : D / tab->qd[k];
    double r = trunc(t);
    if (fabs(t - r) >= 0.5) r += copysign(1.0, t);
    return int(r);
}

// The same evaluation with the coefficient's row of P and its scalars taken from an LDS copy.
// (The row is walked four terms at a time so the compiler does not hoist all NN LDS loads and
// conversions at once: the caller's packed coefficients stay live around it.)
template <int N>
__device__ __forceinline__ int exact_coef_row(const double* P, double S, double rq, double qd, const BlockPx<N>& px) {
    constexpr int NN = N * N;
    double acc = 0.0;
#pragma unroll IE_FIX_UNROLL
    for (int ij = 0; ij < NN; ij++) {
        const double x = double(int((px.w[ij >> 2] >> (8 * (ij & 3))) & 0xFFu) - 128);  // == double(p) + (-128.0), exactly
        acc = acc + P[ij] * x;
    }
    const double D = acc * S;
    const double t = (rq != 0.0) ? D * rq : D / qd;
    double r = trunc(t);
    if (fabs(t - r) >= 0.5) r += copysign(1.0, t);
    return int(r);
}

// exact_coef_row for a fix-up task: the block's pixel words are read from their LDS slot pw
// (4 pixels per word) and the row through a generic pointer P (the LDS copy of a structural row or
// the table in global memory), one pixel word per step of a loop the compiler need not unroll --
// a register copy of the pixels indexed by a loop counter would live in scratch memory.
template <int N>
__device__ __forceinline__ int exact_coef_task(const double* P, double S, double rq, double qd, const uint32_t* pw) {
    constexpr int NN = N * N;
    double acc = 0.0;
    for (int w = 0; w < NN / 4; w++) {
        const uint32_t px4 = pw[w];
        double pr[4];
#pragma unroll
        for (int e = 0; e < 4; e++) pr[e] = P[4 * w + e];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const double x = double(int((px4 >> (8 * e)) & 0xFFu) - 128);
            acc = acc + pr[e] * x;
        }
    }
    const double D = acc * S;
    const double t = (rq != 0.0) ? D * rq : D / qd;
    double r = trunc(t);
    if (fabs(t - r) >= 0.5) r += copysign(1.0, t);
    return int(r);
}

// exact_coef_task for a 4x4 block whose pixel rows are 256 words apart (encode4p_kernel's LDS
// layout), one row per step of a loop left rolled: few registers live beside the caller's.
__device__ __forceinline__ int exact_coef_rows4(const double* P, double S, double rq, double qd, const uint32_t* pw) {
    double acc = 0.0;
#pragma unroll 1
    for (int w = 0; w < 4; w++) {
        const uint32_t px4 = pw[w * 256];
        double pr[4];
#pragma unroll
        for (int e = 0; e < 4; e++) pr[e] = P[4 * w + e];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const double x = double(int((px4 >> (8 * e)) & 0xFFu) - 128);  // == double(p) + (-128.0), exactly
            acc = acc + pr[e] * x;
        }
    }
    const double D = acc * S;
    const double t = (rq != 0.0) ? D * rq : D / qd;
    double r = trunc(t);
    if (fabs(t - r) >= 0.5) r += copysign(1.0, t);
    return int(r);
}

// exact_coef_task for an 8x8 block in encode_kernel<8>'s LDS pixel layout (row r = words
// r*128, r*128 + 1 from pw): the pixel words come from LDS one at a time (a register copy of the
// block indexed by the loop counter would live in scratch memory).
__device__ __forceinline__ int exact_coef_rows8(const double* P, double S, double rq, double qd, const uint32_t* pw) {
    double acc = 0.0;
#pragma unroll 2
    for (int w = 0; w < 16; w++) {
        const uint32_t px4 = pw[(w >> 1) * 128 + (w & 1)];
        double pr[4];
#pragma unroll
        for (int e = 0; e < 4; e++) pr[e] = P[4 * w + e];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const double x = double(int((px4 >> (8 * e)) & 0xFFu) - 128);  // == double(p) + (-128.0), exactly
            acc = acc + pr[e] * x;
        }
    }
    const double D = acc * S;
    const double t = (rq != 0.0) ? D * rq : D / qd;
    double r = trunc(t);
    if (fabs(t - r) >= 0.5) r += copysign(1.0, t);
    return int(r);
}

// Out-of-line copy for the EXACT mode's per-coefficient loop.
template <int N>
__device__ __noinline__ int exact_coef(const EncTables* __restrict__ tab, int k, BlockPx<N> px) {
    return exact_coef_inl<N>(tab, k, px);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// Load the pixel rows of one group: seg[r][m] = bytes [4m, 4m+4) of the group's row r.
template <int N, int WPR, int BPT = Geo<N>::BPT>
__device__ __forceinline__ void load_group(const EncArgs& a, const uint8_t* base, int nblk, uint32_t (&seg)[N][WPR]) {
    if (a.vec_ok && nblk == BPT) {
#pragma unroll
        for (int r = 0; r < N; r++) {
            const uint8_t* p = base + size_t(r) * a.stride;
            if constexpr (WPR == 4) {
                const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
                seg[r][0] = v.x; seg[r][1] = v.y; seg[r][2] = v.z; seg[r][3] = v.w;
            } else if constexpr (WPR == 2) {
                const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
                seg[r][0] = v.x; seg[r][1] = v.y;
            } else {
                seg[r][0] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < N; r++) {
            const uint8_t* p = base + size_t(r) * a.stride;
#pragma unroll
            for (int m = 0; m < WPR; m++) {
                uint32_t wv = 0;
                if (m * 4 < nblk * N) {
#pragma unroll
                    for (int e = 0; e < 4; e++) wv |= uint32_t(p[m * 4 + e]) << (8 * e);
                }
                seg[r][m] = wv;
            }
        }
    }
}

template <int N> struct Packed {
    uint32_t w[N * N / 2];  // zig-zag order, two int16 per word: z[2j] in the low half
};

constexpr float kMagic = 12582912.0f;  // 1.5 * 2^23: t + kMagic rounds t (|t| < 2^22) to an integer

// The "structural" coefficients (0,N/2), (N/2,0), (N/2,N/2): their reference value is, up to
// FP64 rounding, a rational multiple of an integer pixel sum (every c[u][i]c[v][j] is +-1/2 or
// +-sqrt(1/2)), so their quotients land EXACTLY on rounding ties for 1/(4q) of all blocks, where
// only the reference's own FP64 rounding decides.  They are flagged per coefficient and
// re-evaluated alone; the other coefficients reach a tie only within the FP32 error bound.
template <int N> struct Structural {
    static constexpr int k[3] = {N / 2, (N / 2) * N, (N / 2) * N + N / 2};
    static constexpr int zpos(int s) { return ZigZagInv<N>::pos[k[s]]; }
};

// Round the FP32 quotients t[] to int16 (zig-zag packed).  y = t + 1.5*2^23 leaves
// int16(rint(t)) in y's low 16 bits and |t - (y - 1.5*2^23)| is the rounding residual.  Returns
// the largest residual of the ordinary (non-structural, non-exact) coefficients -- >= lim_ord means
// the block may hold a tie within the error bound -- and in *sflags bit s a possible tie of
// structural coefficient s.
template <int N>
__device__ __forceinline__ float round_block(const EncTables* __restrict__ tab, const float (&t)[N * N],
                                             uint32_t (&zp)[N * N / 2], uint32_t* sflags) {
    constexpr int NN = N * N;
    uint32_t yb[NN];
    float e[NN];
#pragma unroll
    for (int k = 0; k < NN; k++) {
        const float y = t[k] + kMagic;
        e[k] = fabsf(t[k] - (y - kMagic));
        yb[k] = __float_as_uint(y);
    }
    // t[0] exact (q[0] a power of two): std::round's half-away-from-zero directly
    const uint32_t dc = uint32_t(int(truncf(t[0] + copysignf(0.5f, t[0]))));
    const bool dcx = tab->dc_exact != 0;
    yb[0] = dcx ? dc : yb[0];
    float emax = dcx ? 0.0f : e[0];
#pragma unroll
    for (int k = 1; k < NN; k++) {
        if (k == Structural<N>::k[0] || k == Structural<N>::k[1] || k == Structural<N>::k[2]) continue;
        emax = fmaxf(emax, e[k]);
    }
    uint32_t sf = 0;
#pragma unroll
    for (int s = 0; s < 3; s++) sf |= (e[Structural<N>::k[s]] >= tab->lim[Structural<N>::k[s]]) ? (1u << s) : 0u;
    *sflags = sf;
#pragma unroll
    for (int j = 0; j < NN / 2; j++)
        zp[j] = __builtin_amdgcn_perm(yb[ZigZag<N>::idx[2 * j + 1]], yb[ZigZag<N>::idx[2 * j]], 0x05040100u);
    return emax;
}

// 8x8: round as above, but flag every coefficient on its own (bit k of the returned mask: its
// residual reaches lim[k]).  The fix-up then re-evaluates single coefficients and never
// recomputes a whole 8x8 block, whose 64 live quotients would spill next to the 32 packed words.
template <int N>
__device__ __forceinline__ uint64_t round_block_mask(const EncTables* __restrict__ tab, const float (&t)[N * N],
                                                     uint32_t (&zp)[N * N / 2]) {
    constexpr int NN = N * N;
    static_assert(NN <= 64, "one mask bit per coefficient");
    uint32_t yb[NN];
    uint64_t near = 0;
#pragma unroll
    for (int k = 0; k < NN; k++) {
        const float y = t[k] + kMagic;
        const float e = fabsf(t[k] - (y - kMagic));
        yb[k] = __float_as_uint(y);
        near |= uint64_t(e >= tab->lim[k]) << k;
    }
    if (tab->dc_exact) {
        yb[0] = uint32_t(int(truncf(t[0] + copysignf(0.5f, t[0]))));
        near &= ~1ull;
    }
#pragma unroll
    for (int j = 0; j < NN / 2; j++)
        zp[j] = __builtin_amdgcn_perm(yb[ZigZag<N>::idx[2 * j + 1]], yb[ZigZag<N>::idx[2 * j]], 0x05040100u);
    return near;
}

// round_block_mask for 8x8 with each zig-zag pair rounded and packed (and pinned) in turn: never
// 64 magic-added quotients live beside the 64 quotients.  Same results bit for bit.
__device__ __forceinline__ uint64_t round_block_mask_lean8(const EncTables* __restrict__ tab, const float (&t)[64],
                                                         uint32_t (&zp)[32]) {
    uint64_t near = 0;
    const bool dcx = tab->dc_exact != 0;
#pragma unroll
    for (int j = 0; j < 32; j++) {
        uint32_t yb[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int k = ZigZag<8>::idx[2 * j + h];
            const float y = t[k] + kMagic;
            const float e = fabsf(t[k] - (y - kMagic));
            yb[h] = __float_as_uint(y);
            if (k == 0) {
                yb[h] = dcx ? uint32_t(int(truncf(t[0] + copysignf(0.5f, t[0])))) : yb[h];
                near |= (!dcx && e >= tab->lim[0]) ? 1ull : 0ull;
            } else {
                near |= uint64_t(e >= tab->lim[k]) << k;
            }
        }
        zp[j] = __builtin_amdgcn_perm(yb[1], yb[0], 0x05040100u);
        asm volatile("" : "+v"(zp[j]));
    }
    return near;
}

template <int N, int WPR>
__device__ __forceinline__ void block_pixels(const uint32_t (&seg)[N][WPR], int b, float (&x)[N * N]) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) x[i * N + j] = float(pix<WPR>(seg[i], b * N + j));
}

template <int N>
__device__ __forceinline__ void quotients(const EncTables* __restrict__ tab, float (&x)[N * N]) {
    if constexpr (N == 4) quot4(x, tab->plan4, FloatOp());
    else quot8(x, tab->dct, tab->g, FloatOp());
}

// The FP64 fix-up of one flagged block, all in line (a call would make the caller spill its
// live coefficient registers around it): the same FP32 quotients rounded into the task's LDS
// result slot, then every coefficient whose residual reaches its own lim[k] re-evaluated in the
// reference's FP64 order and patched in place (a runtime position: LDS, not a register array).
template <int N>
__device__ __forceinline__ void fix_block(const EncTables* __restrict__ tab, const BlockPx<N>& px, uint32_t* res) {
    constexpr int NN = N * N;
    float x[NN];
#pragma unroll
    for (int k = 0; k < NN; k++) x[k] = float((px.w[k >> 2] >> (8 * (k & 3))) & 0xFFu);
    quotients<N>(tab, x);
    uint32_t yb[NN];
    uint64_t near = 0;
#pragma unroll
    for (int k = 0; k < NN; k++) {
        const float y = x[k] + kMagic;
        const float e = fabsf(x[k] - (y - kMagic));
        yb[k] = __float_as_uint(y);
        if (k == 0 && tab->dc_exact) yb[0] = uint32_t(int(truncf(x[0] + copysignf(0.5f, x[0]))));
        else near |= uint64_t(e >= tab->lim[k]) << k;
    }
#pragma unroll
    for (int j = 0; j < NN / 2; j++)
        res[j] = __builtin_amdgcn_perm(yb[ZigZag<N>::idx[2 * j + 1]], yb[ZigZag<N>::idx[2 * j]], 0x05040100u);
    while (near) {
        const int k = __ffsll((unsigned long long)near) - 1;
        near &= near - 1;
        const int kz = ZigZagInv<N>::pos[k];
        const uint32_t v = uint32_t(exact_coef_inl<N>(tab, k, px)) & 0xFFFFu;
        const uint32_t w = res[kz >> 1];  // same-type read-modify-write (no uint16 aliasing)
        res[kz >> 1] = (kz & 1) ? ((w & 0xFFFFu) | (v << 16)) : ((w & 0xFFFF0000u) | v);
    }
}

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// Packed int16 helpers (the compiler otherwise splits them into per-half compares).
// (Constants go in a register: an inline constant of a packed op feeds the low half only.)
__device__ __forceinline__ uint32_t pk_min1_u16(uint32_t w) {  // per half: min(h, 1) = (h != 0)
    uint32_t r;
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(w), "s"(0x00010001u));
    return r;
}
__device__ __forceinline__ uint32_t pk_sign_i16(uint32_t w) {  // per half: h >> 15 (arithmetic)
    uint32_t r;
    asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(r) : "s"(0x000F000Fu), "v"(w));
    return r;
}

// Zig-zag RLE sizing of one packed block (Block.cpp:186-232, :383-397), two coefficients per
// packed-int16 instruction.  Returns bl | Lw << 8 and the record length in bits.  In the RLE
// truncation case (L == N*N, z[N*N-2] == 0: the reference drops the last coefficient,
// Block.cpp:388-390) z[N*N-1] is cleared, so every coefficient at or past Lw is zero.
// 4x4 form with 32-bit masks throughout (the 64-bit nz mask cost 64-bit compares and moves), the
// pair masks merged by shift-or and the widest value by one three-input op per word.
__device__ __forceinline__ uint32_t size_block4(uint32_t (&zp)[8], int rle, uint32_t* bits) {
    uint32_t M = 0, mo = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t w = zp[j];
        M = (pk_min1_u16(w) << (2 * j)) | M;  // v_lshl_or_b32
        mo = (w ^ pk_sign_i16(w)) | mo;  // one v_bitop3 (the compiler's table: a hand-written one had the operands swapped)
    }
    const uint32_t nz = (M & 0x5555u) | ((M >> 15) & 0xAAAAu);  // bit kz: z[kz] != 0
    mo = (mo | (mo >> 16)) & 0xFFFFu;
    const int maxb = 33 - __clz(mo);
    const int L = 32 - __clz(nz);                       // 0 for nz == 0
    const int ffsL = L ? 32 - __clz(uint32_t(L)) : 1;  // utils.hpp:210-216, with ffs(0) == 1
    const int bl = max(maxb, ffsL);
    int lw;
    if (!rle) {
        lw = 16;
    } else if (L == 16 && !((nz >> 14) & 1u)) {
        lw = 32 - __clz(nz & 0x7FFFu);  // drop the last element (Block.cpp:388-390)
        zp[7] &= 0xFFFFu;
    } else {
        lw = L;
    }
    *bits = __umul24(uint32_t(bl), uint32_t(lw + rle)) + 4u;
    return uint32_t(bl) | (uint32_t(lw) << 8);
}

template <int N>
__device__ __forceinline__ uint32_t size_block(uint32_t (&zp)[N * N / 2], int rle, uint32_t* bits) {
    constexpr int NN = N * N;
    constexpr int NP = NN / 2;
    uint64_t nz = 0;  // bit kz set iff z[kz] != 0
    uint32_t mo = 0;  // OR of v ^ (v >> 15) per half: its bit length + 1 is the widest bits_needed
#pragma unroll
    for (int g = 0; g < NP / 8; g++) {
        uint32_t M = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t w = zp[g * 8 + j];
            M |= pk_min1_u16(w) << (2 * j);
            mo |= w ^ pk_sign_i16(w);  // one v_bitop3
        }
        const uint32_t nz16 = (M & 0x5555u) | ((M >> 15) & 0xAAAAu);
        nz |= uint64_t(nz16) << (16 * g);
    }
    mo = (mo | (mo >> 16)) & 0xFFFFu;
    const int maxb = 33 - __clz(mo);  // bits_needed (utils.hpp:226-243) of the widest value
    const int L = nz ? 64 - __clzll((long long)nz) : 0;
    const int ffsL = L ? 32 - __clz(L) : 1;  // utils.hpp:210-216, with ffs(0) == 1
    const int bl = max(maxb, ffsL);
    int lw;
    if (!rle) {
        lw = NN;
    } else if (L == NN && !((nz >> (NN - 2)) & 1ull)) {
        const uint64_t m = nz & ((1ull << (NN - 1)) - 1);  // drop the last element (Block.cpp:388-390)
        lw = m ? 64 - __clzll((long long)m) : 0;
        zp[NP - 1] &= 0xFFFFu;
    } else {
        lw = L;
    }
    *bits = __umul24(uint32_t(bl), uint32_t(lw + rle)) + 4u;  // (a 64-bit v_mad otherwise)
    return uint32_t(bl) | (uint32_t(lw) << 8);
}

// OR the low `len` bits of v (MSB first) into the LDS bit image at bit p (len + p%32 <= 64).
__device__ __forceinline__ void scatter_bits(uint32_t* img, uint32_t p, uint32_t v, uint32_t len) {
    // The image is the dynamic LDS area at LDS byte address 0 (the encode kernels allocate no static
    // LDS; tools/asmcheck.py checks their group_segment_fixed_size): the word pair's byte address
    // straight from p, the second word through the instruction's offset field.  The field is
    // left-aligned once, then funnel-shifted into the pair (-2.7 % against a 64-bit shift).
    (void)img;
    const uint32_t a = (p >> 3) & ~3u;
    const uint32_t s = p & 31u;
    const uint32_t u = v << (32u - len);  // the field left-aligned (len <= 32)
    const uint32_t hi = u >> s;
    const uint32_t lo = __builtin_amdgcn_alignbit(u, 0u, s);  // u << (32 - s), 0 for s = 0
    // (two ds_or_b32, never one ds_or_b64: the address is only 4-byte aligned, and a 64-bit LDS
    // atomic there raises a memory violation -- tools/asmcheck.py rejects 64-bit DS atomics)
    asm volatile("ds_or_b32 %0, %1\n\tds_or_b32 %0, %2 offset:4" ::"v"(a), "v"(hi), "v"(lo) : "memory");
}

// Branch-free variant: every pair is written (past Lw the packed coefficients are zero, so
// those ORs are no-ops) and the wave leaves the loop once no lane has a pair left: no per-lane
// exec-mask juggling per pair.  The zero pairs may land up to 2 * 16 * N*N/2 bits past the
// record: the image keeps that much slack.
template <int N>
__device__ __forceinline__ void emit_block2(uint32_t* img, uint32_t p, const uint32_t (&zp)[N * N / 2], uint32_t blw,
                                            int rle) {
    const uint32_t bl = blw & 0xFFu, lw = blw >> 8;
    if (rle) {
        scatter_bits(img, p, ((bl & 0xFu) << bl) | lw, 4u + bl);
        p += 4u + bl;
    } else {
        scatter_bits(img, p, bl & 0xFu, 4u);
        p += 4u;
    }
    const uint32_t m = (1u << bl) - 1u;
#pragma unroll
    for (int j = 0; j < N * N / 2; j++) {
        if (j > 0 && !__ballot(uint32_t(2 * j) < lw)) break;  // no lane has pair j
        const uint32_t v = ((zp[j] & m) << bl) | __builtin_amdgcn_ubfe(zp[j], 16u, bl);
        scatter_bits(img, p, v, 2u * bl);
        p += 2u * bl;
    }
}

// Every triple is ORed in, without a wave-wide "any lane still has one" exit per field (past Lw
// the coefficients are zero): the v_cmp + branch per field cost more than the skipped fields save
// unless every lane of the wave has a short record (measured -2 % on C2).
// 4x4 RLE records when every bl of the matrix is <= 10 (EncArgs::tri: the host's launch_chain
// sets it when (rec_bits - 4) / 17 <= 10): the header, Lw and z0 in one field of 4 + 2*bl <= 24
// bits, then the coefficients THREE at a time (3*bl <= 30 bits: the field is built in a 32-bit
// v), each ORed through scatter_bits' 64-bit window: 6 fields per block instead of 9.  Past Lw
// the packed coefficients are zero, so a trailing triple only ORs zeros.
__device__ __forceinline__ void emit_block3(uint32_t* img, uint32_t p, const uint32_t (&zp)[8], uint32_t blw) {
    const uint32_t bl = blw & 0xFFu, lw = blw >> 8;
    auto z = [&](int k) -> uint32_t {  // low bl bits of zig-zag coefficient k
        return __builtin_amdgcn_ubfe(zp[k >> 1], (k & 1) ? 16u : 0u, bl);
    };
    scatter_bits(img, p, ((((bl & 0xFu) << bl) | lw) << bl) | z(0), 4u + 2u * bl);
    p += 4u + 2u * bl;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const uint32_t v = (((z(3 * j + 1) << bl) | z(3 * j + 2)) << bl) | z(3 * j + 3);
        scatter_bits(img, p, v, 3u * bl);
        p += 3u * bl;
    }
}

// emit_block3's records when every bl of the wave's slot is <= 8: the header, Lw, z0 and z1 in one
// field of 4 + 3*bl <= 28 bits, then the coefficients FOUR at a time (two packed words, 4*bl <= 32
// bits) and z14, z15: 5 fields per block instead of 6.  Each field is built left-aligned, as
// scatter_bits shifts it: a packed word gives (z_lo << bl) | z_hi in its low 2*bl bits by one
// extract and one shift-or -- whatever lies above falls off the top of v_alignbit's funnel, so no
// coefficient is masked on its own and no field is shifted left again.  The fields cover the same
// 4 + 17*bl bits as emit_block3's, so the image needs no more slack.
__device__ __forceinline__ void emit_block4(uint32_t p, const uint32_t (&zp)[8], uint32_t blw) {
    const uint32_t bl = blw & 0xFFu, lw = blw >> 8, bl2 = 2u * bl;
    const uint32_t up = 0u - bl2;  // (a shift count: the hardware takes its low 5 bits, 32 - 2*bl)
    auto pr = [&](int j) -> uint32_t {  // word j's pair in the low 2*bl bits, garbage above
        return (zp[j] << bl) | __builtin_amdgcn_ubfe(zp[j], 16u, bl);
    };
    auto put = [&](uint32_t u) {  // the left-aligned field u into the word pair at bit p
        const uint32_t a = (p >> 3) & ~3u;
        const uint32_t hi = u >> (p & 31u);
        const uint32_t lo = __builtin_amdgcn_alignbit(u, 0u, p);
        asm volatile("ds_or_b32 %0, %1\n\tds_or_b32 %0, %2 offset:4" ::"v"(a), "v"(hi), "v"(lo) : "memory");
    };
    put(__builtin_amdgcn_alignbit((bl << bl) | lw, pr(0) << (up & 31u), 4u + bl));
    p += 4u + bl + bl2;
#pragma unroll
    for (int j = 1; j < 7; j += 2) {
        put(__builtin_amdgcn_alignbit(pr(j), pr(j + 1) << (up & 31u), bl2));
        p += 2u * bl2;
    }
    put(pr(7) << (up & 31u));
}

// Where tile t sits: its chain (frame / whole batch), its position in it and this thread's
// group of blocks.
struct TileGeo {
    int frame, tif, step, chain_pos;
    int nblk, byi, bx0;  // blocks of this thread's group (nblk = 0: none)
};

template <int N, int BPT = Geo<N>::BPT, int TG = kEncTPB, class Args = EncArgs>
__device__ __forceinline__ TileGeo tile_geo(const Args& a, int t, int tid) {
    TileGeo g;
    // Independent images interleave their tiles (frame = t % nframes), so every frame's chain
    // advances together; a concatenated stream keeps chain order = tile order.
    // (wave-uniform divisions by launch constants: multiply-highs, FastDiv)
    if (a.segmented) {
        g.tif = int(fdiv(uint32_t(t), a.div_frames.mul, a.div_frames.shr));
        g.frame = t - g.tif * a.nframes;
        g.step = a.nframes;
    } else {
        g.frame = int(fdiv(uint32_t(t), a.div_tpf.mul, a.div_tpf.shr));
        g.tif = t - g.frame * a.tiles_per_frame;
        g.step = 1;
    }
    g.chain_pos = a.segmented ? g.tif : t;  // tiles before this one in its chain
    // group gi = base + tid: the division by gpr is split into a wave-uniform (scalar) part and a
    // per-lane remainder r < gpr + kEncTPB, divided by a multiply-high with ceil(2^32 / gpr)
    const int base = g.tif * TG;  // (TG groups per tile; tid: the thread's group within it)
    const int q0 = int(fdiv(uint32_t(base), a.div_gpr.mul, a.div_gpr.shr)), r0 = base - q0 * a.gpr;
    const uint32_t r = uint32_t(r0 + tid);
    const uint32_t dq = (a.gpr == 1) ? r : __umulhi(r, a.gpr_magic);  // (2^32 does not fit the magic)
    const int gi = base + tid;
    g.nblk = g.byi = g.bx0 = 0;
    if (gi < a.groups_per_frame) {
        g.byi = q0 + int(dq);
        g.bx0 = int(r - dq * uint32_t(a.gpr)) * BPT;
        g.nblk = min(BPT, a.bx - g.bx0);
    }
    return g;
}

// The launch fields a tile's geometry and pixel loads need (EncArgs' first 27 words), read from
// the kernel-argument segment in ONE scalar round trip (two s_load_dwordx16).  Read field by field,
// the compiler sinks each load into the branch that uses it: a chain of ~6 dependent round trips
// (≈1.1 µs under load, measured by stamps) before a tile's first pixel load and again at its start.
struct GeoArgs {
    const uint8_t* y;
    uint64_t stride, frame_pitch;
    int nframes, bx, by, gpr;
    uint32_t gpr_magic;
    int groups_per_frame, tiles_per_frame, ntiles;
    FastDiv div_frames, div_tpf, div_gpr;
    int segmented;
};
template <class KA>
__device__ __forceinline__ GeoArgs load_geo(KA* ka) {
    typedef uint32_t u16v __attribute__((ext_vector_type(16)));
    using P = const __attribute__((address_space(4))) u16v;
    u16v A = ((P*)ka)[0], B = ((P*)ka)[1];
    asm volatile("" : "+s"(A), "+s"(B));  // both loaded here, before any use
    auto w = [&](size_t off) -> uint32_t { return off < 64 ? A[off / 4] : B[off / 4 - 16]; };
    auto d = [&](size_t off) -> uint64_t { return uint64_t(w(off)) | (uint64_t(w(off + 4)) << 32); };
    auto fd = [&](size_t off) { return FastDiv{w(off), w(off + 4), w(off + 8)}; };
    static_assert(offsetof(EncArgs, segmented) + 4 <= 128, "geometry fields in the first 128 bytes");
    GeoArgs g;
    g.y = reinterpret_cast<const uint8_t*>(d(offsetof(EncArgs, y)));
    g.stride = d(offsetof(EncArgs, stride));
    g.frame_pitch = d(offsetof(EncArgs, frame_pitch));
    g.nframes = int(w(offsetof(EncArgs, nframes)));
    g.bx = int(w(offsetof(EncArgs, bx)));
    g.by = int(w(offsetof(EncArgs, by)));
    g.gpr = int(w(offsetof(EncArgs, gpr)));
    g.gpr_magic = w(offsetof(EncArgs, gpr_magic));
    g.groups_per_frame = int(w(offsetof(EncArgs, groups_per_frame)));
    g.tiles_per_frame = int(w(offsetof(EncArgs, tiles_per_frame)));
    g.ntiles = int(w(offsetof(EncArgs, ntiles)));
    g.div_frames = fd(offsetof(EncArgs, div_frames));
    g.div_tpf = fd(offsetof(EncArgs, div_tpf));
    g.div_gpr = fd(offsetof(EncArgs, div_gpr));
    g.segmented = int(w(offsetof(EncArgs, segmented)));
    return g;
}

template <int N, int WPR, int BPT = Geo<N>::BPT>
__device__ __forceinline__ void load_tile(const EncArgs& a, const TileGeo& g, uint32_t (&seg)[N][WPR]) {
    if (g.nblk) {
        const uint8_t* base =
            a.y + size_t(g.frame) * a.frame_pitch + size_t(g.byi) * N * a.stride + size_t(g.bx0) * N;
        load_group<N, WPR, BPT>(a, base, g.nblk, seg);
    } else {
#pragma unroll
        for (int r = 0; r < N; r++)
#pragma unroll
            for (int m = 0; m < WPR; m++) seg[r][m] = 0;
    }
}

// HIST: count the stored bytes into a per-tile LDS histogram (256 words after the misc area),
// merged into a.hist[frame] at the end: the Huffman pass's histogram without re-reading the stream.
// R > 1: R copies of each bin, bin b of lane l at b * R + l % R (the same byte in several lanes of
// one ds_add no longer serialises on one address)
template <int R = 1>
struct HistCountT {
    uint32_t* hl;
    uint64_t limit;  // bytes at stream positions >= limit are padding (the chain's last word)
    uint32_t lo = 0;  // l % R
    __device__ __forceinline__ void add(uint32_t b) const { atomicAdd(&hl[b * R + lo], 1u); }
    __device__ __forceinline__ void operator()(uint64_t gw, uint32_t v) const {
        if (limit == ~0ull) {  // (wave-uniform) not the chain's last tile: every byte counts
#pragma unroll
            for (int k = 0; k < 4; k++) add((v >> (8 * k)) & 0xFFu);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (4 * gw + k < limit) add((v >> (8 * k)) & 0xFFu);
        }
    }
};
using HistCount = HistCountT<1>;

}  // namespace ie
