// imageencoder_amd/csrc/ie_decode_rec.h -- what the record decode passes of ie_decode.hip, the
// region decode pass of ie_decode_region.hip and the scaled decode pass of ie_decode_scaled.hip
// share: bit reads from a wave's LDS copy of the stream, record lengths, the zig-zag ranks, a
// chunk's entry offset, the launch's record span, the image batch's argument rebasing and the
// staging of stream words into LDS.
#pragma once
#include "ie_decode_blocks.h"

namespace ie {

namespace {
constexpr int kZZ4[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
constexpr int kZZ8[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                          12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                          58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
}  // namespace

// bits [p, p+l) of the LDS stream copy L (MSB-first words), l <= 32, p relative to the copy
__device__ __forceinline__ uint32_t lbits(const uint32_t* L, uint32_t p, int l) {
    const uint32_t w = p >> 5, s = p & 31u;
    const uint64_t v = (uint64_t(L[w]) << 32) | L[w + 1];
    return l ? uint32_t((v << s) >> (64 - l)) : 0u;
}

// length of the record whose 20 header bits (bl:4, then the RLE length's bl bits) are `head`; 1
// if no record can start there -- a count beyond the block -- (a walk slides one bit; never on
// the true path of a well-formed stream).  bl = 0 is a record of 4 bits: no count bits, no values.
template <int N>
__device__ __forceinline__ uint32_t rec_len_head(uint32_t head, int rle) {
    constexpr int NN = N * N;
    const uint32_t bl = head >> 16;
    if (!bl) return 4u;
    if (!rle) return 4u + bl * NN;
    const uint32_t lw = (head & 0xFFFFu) >> (16 - bl);
    return lw <= uint32_t(NN) ? 4u + bl * (lw + 1u) : 1u;
}
// rec_len_head without branches (the walk loops: every lane runs it every step)
template <int N>
__device__ __forceinline__ uint32_t rec_len_sel(uint32_t head, int rle) {
    constexpr uint32_t NN = N * N;
    const uint32_t bl = head >> 16;
    const uint32_t lw = rle ? ((head & 0xFFFFu) >> (16u - bl)) : NN - 1u;  // (bl = 0: shifted out, lw = 0)
    return lw <= NN ? 4u + bl * (lw + 1u) : 1u;                            // (bl = 0: 4 bits)
}
// length of the record at p, 0 if no record can start there
template <int N>
__device__ __forceinline__ uint32_t rec_len(const uint32_t* L, uint32_t p, int rle) {
    const uint32_t l = rec_len_head<N>(lbits(L, p, 20), rle);
    return l > 1u ? l : 0u;
}

// (a multiple of 4 words, with room for stage_words16's alignment offset)
__host__ __device__ constexpr int rec_decode_stream_words(uint32_t C, int D) { return (int((C + D + 95) >> 5) + 3 + 3 + 3) & ~3; }

// zig-zag rank of every coefficient position (the inverse of kZZ4 / kZZ8)
template <int N> struct InvZZ {
    int r[N * N];
    constexpr InvZZ() : r() {
        for (int k = 0; k < N * N; k++) r[(N == 4) ? kZZ4[k] : kZZ8[k]] = k;
    }
};

// sR / sq: the FP64 cos products R[uv][ij] and the quantiser through the constant address space:
// the loads are uniform, so they become scalar loads and the FP64 multiplies take their operands
// from SGPRs
using const_f64 = const __attribute__((address_space(4))) double*;

// the chunk's entry offset (record parse): composed tables, or the predecessor's speculative exit
template <int N, bool B = false>
__device__ __forceinline__ uint32_t rec_chunk_entry(const RecParseArgs& a, int k) {
    if constexpr (B) {
        // table_entry with the levels unrolled: lvl[] is indexed by constants only, so the rebased
        // copy of the arguments (rec_image) stays in registers (a run-time index puts all of it in
        // scratch).  lvl[] itself stays image 0's: this image's arrays lie img entries after.
        constexpr int D = RecGeom<N>::D, G = RecGeom<N>::G;
        const size_t img = size_t(blockIdx.y) * a.img_tab;
        int u = k;
        for (int l = 0; l < a.levels; l++) u /= G;
        uint32_t x = a.E[u];
#pragma unroll
        for (int l = kRecMaxLevels - 1; l >= 0; l--) {
            if (l < a.levels) {
                int ul = k;
#pragma unroll
                for (int m = 0; m < l; m++) ul /= G;
                x = a.lvl[l][img + size_t(ul) * D + x];
            }
        }
        return x;
    }
    if (a.spec) return k ? a.spec[k - 1] : 0u;
    return table_entry<RecGeom<N>::D, RecGeom<N>::G>(a.E, a.lvl, a.levels, k);
}

// Image batch: the launch's arguments rebased to image blockIdx.y -- its stream, its length and its
// scratch -- so that every pass below runs on it as on a single stream.  (lvl[] is left alone: see
// rec_chunk_entry.)
template <bool B>
__device__ __forceinline__ void rec_image(RecParseArgs& a) {
    if constexpr (B) {
        const size_t y = blockIdx.y;
        a.words += y * a.img_words;
        a.nbits = a.img_nbits[y];
        a.tab += y * a.img_tab;
        a.E += y * a.img_E;
        a.pos += y * a.img_chunks * kRecPosCap;
        a.cnt += y * a.img_chunks;
        a.lbase += y * a.img_chunks;
        a.wgsum += y * a.img_wg;
        a.total += 2 * y;
        a.end_out += 2 * y;
    }
}

// The record span of a launch: [start, nbits) -- the host's, or, device-chained (a.dstart), from
// an earlier launch's end bit (clamped to the stream; ~0 = that launch found no end) for at most
// a.span bits.  Chunks past the span's end see no stream bits and hold no record.
struct RecSpan {
    uint64_t start, nbits;
};
__device__ __forceinline__ RecSpan rec_span(const RecParseArgs& a) {
    if (!a.dstart) return {a.start_bit, a.nbits};
    const uint64_t st = min(min(*a.dstart, a.nbits) + a.start_add, a.nbits);
    return {st, min(a.nbits, st + a.span)};
}
__device__ __forceinline__ uint64_t sat_sub(uint64_t x, uint64_t y) { return x > y ? x - y : 0ull; }

// L[i] = bswap(W[w0 + i]) for i < nw (zeros past nwords) by one wave with 16-byte loads, four
// per lane in flight; L must be 16-byte aligned.  The copy starts at the aligned word w0 & ~3:
// returns the offset of word w0 in L (0..3).
__device__ __forceinline__ int stage_words16(uint32_t* L, const uint32_t* W, uint64_t w0, int nw, uint64_t nbits,
                                             int lane) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    const uint64_t wa = w0 & ~3ull;
    const int off = int(w0 - wa);
    const int nq = (nw + off + 3) >> 2;  // 16-byte groups
    const uint64_t nwords = (nbits + 31) >> 5;
    const uint64_t nfull = (nbits >> 5) >> 2;  // groups of whole words wholly inside the stream
    for (int q0 = 0; q0 < nq; q0 += 64 * 4) {
        u4 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int q = q0 + u * 64 + lane;
            const uint64_t g = (wa >> 2) + uint64_t(q);
            if (q < nq && g < nfull) {
                v[u] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(W) + g);
            } else {
                u4 z = {0u, 0u, 0u, 0u};  // (kept byte-swapped back: the store below swaps again)
                if (q < nq)
                    for (int e = 0; e < 4; e++)
                        if (4 * g + e < nwords) z[e] = bswap32(tail_word(W[4 * g + e], 4 * g + e, nbits));
                v[u] = z;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int q = q0 + u * 64 + lane;
            if (q < nq) {
                u4 b = {bswap32(v[u].x), bswap32(v[u].y), bswap32(v[u].z), bswap32(v[u].w)};
                reinterpret_cast<u4*>(L)[q] = b;
            }
        }
    }
    return off;
}

}  // namespace ie
