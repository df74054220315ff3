// imageencoder_amd/csrc/ie_decode_blocks.h -- what the record decode (ie_decode.hip) and the Huffman
// decode (ie_huffman_decode.hip) share: the exact parse of a serial bit stream by transfer tables,
// composed.
//
// In both streams an item's length (a record's, a code's) is only known once its first bits are
// read, so the stream is a serial chain.  Cut it into chunks of C bits.  The first item starting at
// or after a chunk's first bit sits at an offset d < D, D = the longest item: the item straddling
// the boundary ends within D bits.  So a chunk is a FUNCTION of d: walking from offset d gives the
// offset at which the walk enters the next chunk -- its transfer table T_k[d] over all D entries,
// written by the user's own table pass.  Tables compose (T_{k+1} o T_k), and the true entry of every
// chunk follows from the stream's start by composing tables: exact for any content, with no
// speculation to converge (periodic streams, which lock speculative walks into a wrong phase, cost
// nothing extra).  The two users bind D and G (tables per composition group, [G][D] 16-bit exits in
// LDS): the record parse D = 4 + 15 * (N * N + 1) and G = 32 (RecGeom, ie_device.h), the Huffman
// parse D = 15 and G = 256.
//   compose_kernel      one workgroup per group of G tables: the group's tables in LDS, every entry
//                       chased through them; the chase writes the group-relative prefix map P_j
//                       over each table (group entry -> entry of table j) and the group's
//                       composite.  Levels repeat on the composites until at most G remain
//                       (launch_compose; compose_rows sizes the table array).
//   compose_top_kernel  one workgroup chases the stream's start through those top-level composites.
//   table_entry         a chunk's true entry: its top-level entry, then one prefix map per level.
// Also here: tail_word, the stream's last word as both sides' LDS staging reads it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ie_common.hpp"
#include "ie_device.h"

namespace ie {

// The stream word w (byte-swapped to MSB-first) with its bits at or past nbits cleared: the last
// word may be read in place from a caller's buffer, whose bytes past the stream are not zero.
__device__ __forceinline__ uint32_t tail_word(uint32_t raw, uint64_t w, uint64_t nbits) {
    const uint32_t b = bswap32(raw);
    const uint64_t vb = nbits - (w << 5);  // valid bits of this word (>= 1)
    return vb >= 32 ? b : (b & ~(0xFFFFFFFFu >> uint32_t(vb)));
}

// n 16-bit entries from global memory into LDS, 16 bytes per load where both sides allow it
// (eight 16-byte loads per thread in flight before their LDS stores: one load-to-store round trip
// per 32 KiB instead of one per 4 KiB)
__device__ __forceinline__ void stage_u16(uint16_t* S, const uint16_t* T, int n, int tid) {
    typedef uint32_t u4 __attribute__((ext_vector_type(4)));
    int head = 0;
    if (((reinterpret_cast<uintptr_t>(T) | reinterpret_cast<uintptr_t>(S)) & 15u) == 0) {
        head = n & ~7;
        const int nv = head / 8;
        const u4* src = reinterpret_cast<const u4*>(T);
        u4* dst = reinterpret_cast<u4*>(S);
        for (int i0 = 0; i0 < nv; i0 += 8 * kTPB) {
            u4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int i = i0 + u * kTPB + tid;
                if (i < nv) v[u] = src[i];
            }
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int i = i0 + u * kTPB + tid;
                if (i < nv) dst[i] = v[u];
            }
        }
    }
    for (int i = head + tid; i < n; i += kTPB) S[i] = T[i];
}

// One composition level over n tables ([n][D], 16-bit exits): prefix maps written over the
// tables, composites into comp ([ceil(n/G)][D]).
// B (image batch): blockIdx.y = the image, whose tables and composites lie img entries after the
// previous image's.
template <int D, int G, bool B = false>
__global__ __launch_bounds__(kTPB) void compose_kernel(uint16_t* tab, int n, uint16_t* comp, size_t img) {
    __shared__ __attribute__((aligned(16))) uint16_t S[G * D];
    const int tid = threadIdx.x, g = blockIdx.x;
    if constexpr (B) {
        tab += size_t(blockIdx.y) * img;
        comp += size_t(blockIdx.y) * img;
    }
    const int k0 = g * G, nk = min(G, n - k0);
    uint16_t* T = tab + size_t(k0) * D;
    stage_u16(S, T, nk * D, tid);
    __syncthreads();
    // every entry chased through the group's tables; a thread's entries (tid, tid + kTPB, ...) are
    // chased side by side, so their dependent LDS reads overlap
    constexpr int CH = (D + kTPB - 1) / kTPB;
    uint32_t x[CH];
#pragma unroll
    for (int c = 0; c < CH; c++) x[c] = uint32_t(tid + c * kTPB);
    for (int j = 0; j < nk; j++) {
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const int d = tid + c * kTPB;
            if (d < D) {
                T[j * D + d] = uint16_t(x[c]);  // P_j: group entry d -> entry of table j
                x[c] = S[j * D + x[c]];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CH; c++) {
        const int d = tid + c * kTPB;
        if (d < D) comp[size_t(g) * D + d] = uint16_t(x[c]);
    }
}

// The top chase: the stream's start (entry 0) through the ng <= G top-level composites, E[q] = the
// entry of composite q (one workgroup; a launch of its own, so the composites are visible without
// a device-wide fence in every composing workgroup).  (A segmented chase -- every entry through
// each of 8 segments, then entry 0 through the segment maps -- measured slower here and in
// compose_kernel: 9.2 -> 11.6 and 15.2 -> 18.1 us.)
template <int D, int G, bool B = false>
__global__ __launch_bounds__(kTPB) void compose_top_kernel(const uint16_t* comp, int ng, uint32_t* E, size_t img,
                                                           uint32_t img_E) {
    __shared__ __attribute__((aligned(16))) uint16_t S[G * D];
    if constexpr (B) {  // (every image's stream starts at its own first record: entry 0)
        comp += size_t(blockIdx.y) * img;
        E += size_t(blockIdx.y) * img_E;
    }
    stage_u16(S, comp, ng * D, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t x = 0;
        for (int q = 0; q < ng; q++) {
            E[q] = x;
            x = S[q * D + x];
        }
    }
}

// The composition levels over n tables: level l+1's tables are level l's composites, until at
// most G remain (the top chase).  lvl[l] receives level l's table array; returns the number of
// levels, or -1 past kRecMaxLevels.  B: `images` batches of n tables each, img entries (E: img_E
// words) apart, composed by the same launches (lvl[] receives image 0's arrays).
template <int D, int G, bool B = false>
int launch_compose(uint16_t* tab, int n, uint32_t* E, uint16_t** lvl, hipStream_t s, int images = 1, size_t img = 0,
                   uint32_t img_E = 0) {
    int cur = n, levels = 0;
    uint16_t* arr = tab;
    for (;;) {
        const int ng = (cur + G - 1) / G;
        const int top = ng <= G ? 1 : 0;
        if (levels >= kRecMaxLevels) return -1;
        lvl[levels] = arr;
        uint16_t* comp = arr + size_t(cur) * D;
        hipLaunchKernelGGL((compose_kernel<D, G, B>), dim3(ng, images), dim3(kTPB), 0, s, arr, cur, comp, img);
        levels++;
        if (top) {
            hipLaunchKernelGGL((compose_top_kernel<D, G, B>), dim3(1, images), dim3(kTPB), 0, s, comp, ng, E, img, img_E);
            return levels;
        }
        arr = comp;
        cur = ng;
    }
}

// Table rows a composition over n tables needs (the tables and every level's composites); *levels
// (optional): the levels launch_compose runs over them (not capped at kRecMaxLevels).
template <int D, int G>
size_t compose_rows(size_t n, int* levels = nullptr) {
    size_t rows = 0;
    int nl = 1;
    for (size_t cur = n;; cur = (cur + G - 1) / G, nl++) {
        rows += cur;
        if ((cur + G - 1) / G <= size_t(G)) {
            if (levels) *levels = nl;
            return rows + (cur + G - 1) / G;
        }
    }
}

// the entry offset of table k: its top-level entry, then the prefix maps of every level down
template <int D, int G>
__device__ __forceinline__ uint32_t table_entry(const uint32_t* E, uint16_t* const* lvl, int levels, int k) {
    int u = k;
    for (int l = 0; l < levels; l++) u /= G;
    uint32_t x = E[u];
    for (int l = levels - 1; l >= 0; l--) {
        int ul = k;
        for (int m = 0; m < l; m++) ul /= G;
        x = lvl[l][size_t(ul) * D + x];
    }
    return x;
}

}  // namespace ie
