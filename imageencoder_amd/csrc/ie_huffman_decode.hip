// imageencoder_amd/csrc/ie_huffman_decode.hip -- the Huffman decode on gfx950 (Huffman.cpp:354-402;
// the per-bit tree walk of :190-204), parsed exactly with the transfer tables of ie_decode_blocks.h.
//
// A code is at most 15 bits long (the dictionary stores lengths in 4 bits, Huffman.cpp:41-42), so
// the first code that starts at or after a chunk's first bit sits at an offset d < 15: a chunk of
// the code stream is a function of d, with D = 15 entries and G = 256 tables per group.
//   huf_table_kernel  walks all 15 entries of kHufTC chunks per workgroup (the chunks' bits staged
//                     in LDS; a position where no code starts slides one bit -- never on the true
//                     path of a valid stream).  Walks from different entries of a chunk fall onto
//                     the same code boundaries after a few codes (prefix codes resynchronise), so
//                     only the first kHufSync bits are walked from all 15 entries: the walks that
//                     stand on the same first boundary at or past cs + kHufSync have merged; one
//                     walk per distinct boundary (almost always one per chunk) goes on to the
//                     chunk's end, the workgroup's survivors side by side.  Every entry gets its
//                     exit, its symbol count to the exit, and the first boundary at or past the
//                     chunk's middle with the symbols before it.
//   compose_kernel, compose_top_kernel (ie_decode_blocks.h) compose the exit tables.
//   huf_count_kernel  each chunk's true entry through the composed tables and its symbol count at
//                     that entry (no walk); a workgroup scan of the counts.
//   huf_total_kernel  the symbol count: the sum of the count workgroups' totals.
//   huf_emit_kernel   every chunk again from its entry, two lanes per chunk (split at the middle
//                     boundary), writing the symbols at the chunk's place in the output.
// Exact for any content: a periodic stream (e.g. a flat image's records, Huffman-coded) cannot leave
// a speculative walk locked in a wrong phase.  The reference walks to the end of the buffer,
// padding bits of the last byte included (a code may run past it with zero bits), and so do these
// walks.
//   lut   [2^15]: sym | len << 8 for every 15-bit prefix, len 0 = no code
//   LDS   the 2^kHufL1 first-level entries (codes of <= kHufL1 bits resolve there)
#include "ie_decode_blocks.h"

namespace ie {

constexpr int kHufL1 = 11;
constexpr int kHufD = 15;   // entry offsets of a chunk: codes are at most 15 bits
#ifndef IE_HUF_G
#define IE_HUF_G 256
#endif
constexpr int kHufG = IE_HUF_G;  // tables per composition group
struct HufArgs {
    const uint32_t* words;
    uint64_t nbits, start_bit, chunk_bits;
    int nchunks;
    const uint16_t* lut;
    uint64_t* entry;
    uint32_t* count;
    uint32_t* wgsum;    // [walk workgroups] their chunks' symbol totals
    unsigned* changed;  // [1] invalid code on the emitting walk; [0] output past out_cap (not written)
    uint64_t* base;     // symbols before each chunk within its walk workgroup
    uint8_t* out;
    uint16_t* lvl[kRecMaxLevels];  // mode 2: the composition's levels
    int levels;
    const uint32_t* E;
    uint64_t out_cap;   // bytes of out (the emit launched before the total is known checks it)
    // image batch (the kernels' B instantiations; huf_image): the strides between the images' parts
    size_t img_words;           // stream words
    const uint64_t* img_nbits;  // [images] stream bits
    const uint64_t* img_start;  // [images] first bit of the code stream
    size_t img_tab;             // table entries (tables, composites, counts, middles)
    uint32_t img_chunks, img_wg, img_E;
    size_t out_pitch;           // bytes between the images' output slots (out_cap: bytes of a slot)
};

// Image batch: the launch's arguments rebased to image blockIdx.y -- its stream, its length, its
// first bit (the dictionaries differ in length, so every image's chunk grid has its own phase),
// its prefix table, its scratch, its flag pair and its output slot -- so that every pass below runs
// on it as on a single stream.  One chunk plan serves the batch (nchunks from the longest stream):
// a chunk past its image's stream holds no code.  (lvl[] is left alone: see huf_count_kernel.)
template <bool B>
__device__ __forceinline__ void huf_image(HufArgs& a) {
    if constexpr (B) {
        const size_t y = blockIdx.y;
        a.words += y * a.img_words;
        a.nbits = a.img_nbits[y];
        a.start_bit = a.img_start[y];
        a.lut += y << 15;
        a.entry += y * a.img_chunks;
        a.count += y * a.img_chunks;
        a.base += y * a.img_chunks;
        a.wgsum += y * a.img_wg;
        a.changed += 2 * y;
        a.E += y * a.img_E;
        a.out += y * a.out_pitch;
    }
}

__device__ __forceinline__ void huf_l1(const uint16_t* lut, uint16_t* l1) {
    constexpr int B = 8;  // loads in flight per thread
    for (int q0 = 0; q0 < (1 << kHufL1); q0 += B * int(blockDim.x)) {
        uint16_t e[B];
#pragma unroll
        for (int u = 0; u < B; u++) {
            const int q = q0 + u * int(blockDim.x) + int(threadIdx.x);
            e[u] = q < (1 << kHufL1) ? lut[uint32_t(q) << (15 - kHufL1)] : uint16_t(0);
        }
#pragma unroll
        for (int u = 0; u < B; u++) {
            const int q = q0 + u * int(blockDim.x) + int(threadIdx.x);
            if (q < (1 << kHufL1)) l1[q] = ((e[u] >> 8) != 0 && (e[u] >> 8) <= kHufL1) ? e[u] : uint16_t(0);  // 0: look in lut
        }
    }
    __syncthreads();
}

// The symbols before workgroup g's chunks: the totals of the workgroups before it, summed by the
// whole workgroup (every thread receives it).
__device__ __forceinline__ uint64_t huf_wg_prefix(const uint32_t* wgsum, int g, uint32_t* scratch) {
    uint64_t part = 0;
    for (int i = threadIdx.x; i < g; i += kTPB) part += wgsum[i];
    const uint64_t w = wave_sum64(part);
    if ((threadIdx.x & 63) == 0) reinterpret_cast<uint64_t*>(scratch)[threadIdx.x >> 6] = w;
    __syncthreads();
    const uint64_t* s64 = reinterpret_cast<const uint64_t*>(scratch);
    return s64[0] + s64[1] + s64[2] + s64[3];
}

// total receives the symbol count (device, 1 word): the sum of the walk's workgroup totals.
// B (image batch): blockIdx.y = the image, its totals img_wg words after the previous image's.
template <bool B = false>
__global__ __launch_bounds__(kTPB) void huf_total_kernel(const uint32_t* wgsum, int nwg, uint64_t* total,
                                                         uint32_t img_wg) {
    __shared__ alignas(8) uint32_t scratch[8];
    if constexpr (B) {
        wgsum += size_t(blockIdx.y) * img_wg;
        total += blockIdx.y;
    }
    const uint64_t t = huf_wg_prefix(wgsum, nwg, scratch);
    if (threadIdx.x == 0) *total = t;
}

// Words [w0, w0 + nw) of the stream, byte-swapped to MSB-first, zeros past the stream's nbits,
// with one pad word after every 32 (word i at i + i / 32): lanes walking chunks of
// 1 024 bits side by side read words 32 apart -- one bank -- without it (lbits_pad reads it)
__device__ __forceinline__ void stage_words_pad(uint32_t* L, const uint32_t* W, uint64_t w0, int nw, uint64_t nbits,
                                                int tid, int nthreads) {
    const uint64_t nwords = (nbits + 31) >> 5;
    constexpr int B = 8;
    for (int i0 = 0; i0 < nw; i0 += B * nthreads) {
        uint32_t v[B];
#pragma unroll
        for (int u = 0; u < B; u++) {
            const int i = i0 + u * nthreads + tid;
            const uint64_t w = w0 + i;
            if (i < nw && (w + 1) * 32 <= nbits) {
                v[u] = __builtin_nontemporal_load(W + w);
            } else if (i < nw && w < nwords) {  // the stream's last, partial word: its bytes only (the
                                                // caller's buffer may end there)
                const uint8_t* b = reinterpret_cast<const uint8_t*>(W + w);
                uint32_t x = 0;
                for (uint32_t e = 0; e < 4u && 32 * w + 8 * e < nbits; e++) x |= uint32_t(b[e]) << (8 * e);
                v[u] = x;
            } else {
                v[u] = 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < B; u++) {
            const int i = i0 + u * nthreads + tid;
            if (i < nw) L[i + (i >> 5)] = (w0 + i < nwords) ? tail_word(v[u], w0 + i, nbits) : 0u;
        }
    }
}
__host__ __device__ constexpr int pad_words(int nw) { return nw + (nw >> 5) + 1; }
__device__ __forceinline__ uint32_t lbits_pad(const uint32_t* L, uint32_t p, int l) {
    const uint32_t w = p >> 5, w1 = w + 1u, s = p & 31u;
    const uint64_t v = (uint64_t(L[w + (w >> 5)]) << 32) | L[w1 + (w1 >> 5)];
    return l ? uint32_t((v << s) >> (64 - l)) : 0u;
}

#ifndef IE_HUF_SYNC
#define IE_HUF_SYNC 64
#endif
constexpr uint32_t kHufSync = IE_HUF_SYNC;
#ifndef IE_HUF_TC
#define IE_HUF_TC 64
#endif
constexpr int kHufTC = IE_HUF_TC;  // chunks per table workgroup: its survivors fill a wave
// B (image batch): blockIdx.y = the image (huf_image), its table arrays img_tab entries after the
// previous image's.  A workgroup whose chunks all lie past its image's stream walks nothing and
// writes the rows those walks would end in: every entry leaves at the next chunk's first bit with
// no code counted, the middle boundary at the chunk's end.
template <bool B = false>
__global__ __launch_bounds__(kTPB) void huf_table_kernel(HufArgs a, uint16_t* tab, uint16_t* cnt, uint16_t* mo,
                                                          uint16_t* mc) {
    constexpr int S = kHufTC * 16, U = S / kTPB;  // walk slots (chunk, entry); slots per thread
    static_assert(S % kTPB == 0, "whole slots per thread");
    __shared__ uint16_t l1[1 << kHufL1];
    __shared__ uint32_t P[S], X[S], R[S + 1];  // boundary after the sync walk; exit; survivors
    __shared__ uint16_t K2[S];                 // a survivor's codes from P to its exit
    __shared__ uint32_t M[S];                  // its first boundary at or past the chunk's middle
    __shared__ uint16_t KM[S];                 // its codes from P to that boundary
    extern __shared__ uint32_t L[];            // the workgroup's chunks' bits (+ 64 past the last)
    const int tid = threadIdx.x;
    huf_image<B>(a);
    if constexpr (B) {
        const size_t img = size_t(blockIdx.y) * a.img_tab;
        tab += img;
        cnt += img;
        mo += img;
        mc += img;
    }
    if (tid == 0) R[S] = 0u;
    const int k0 = blockIdx.x * kHufTC;
    const uint32_t C = uint32_t(a.chunk_bits);
    const int m = min(kHufTC, a.nchunks - k0);
    const uint64_t c0 = a.start_bit + uint64_t(k0) * C;
    if constexpr (B) {
        if (c0 >= a.nbits) {
            for (int i = tid; i < m * kHufD; i += kTPB) {
                const size_t r = size_t(k0) * kHufD + i;
                tab[r] = 0;
                cnt[r] = 0;
                mo[r] = uint16_t(C);
                mc[r] = 0;
            }
            return;
        }
    }
    const uint64_t base = c0 & ~31ull;
    const uint32_t s0 = uint32_t(c0 - base);
    stage_words_pad(L, a.words, base >> 5, int((s0 + uint32_t(m) * C + 64) >> 5) + 2, a.nbits, tid, kTPB);
    huf_l1(a.lut, l1);  // (ends with a barrier: L staged too)
    const uint32_t lim = uint32_t(min<uint64_t>(a.nbits - base, uint64_t(s0) + uint64_t(m) * C));
    // one step from p: the next position (a code at p: counted in *n); past the stream: the
    // chunk's end e (the last chunk's exit is never used)
    auto step = [&](uint32_t p, uint32_t e, uint32_t* n) -> uint32_t {
        if (p >= lim) return e;
        const uint32_t p15 = lbits_pad(L, p, 15);
        uint32_t v = l1[p15 >> (15 - kHufL1)];
        if (!v) v = a.lut[p15];
        const uint32_t len = v >> 8;
        *n += len ? 1u : 0u;
        return p + (len ? len : 1u);
    };
    // slot u of this thread: s = u kTPB + tid, chunk s / 16, entry s % 16 (15: none)
    auto kc_of = [&](int u) { return (u * kTPB + tid) >> 4; };
    const int d = tid & 15;
    uint32_t p[U], n1[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        p[u] = s0 + uint32_t(kc_of(u)) * C + uint32_t(d);
        n1[u] = 0;
    }
    // the sync walks, the thread's U slots interleaved (independent chains: their LDS reads overlap)
    for (;;) {
        bool any = false;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int kc = kc_of(u);
            const uint32_t cs = s0 + uint32_t(kc) * C, ce = cs + C;
            if (d < kHufD && kc < m && p[u] < min(cs + kHufSync, ce)) {
                p[u] = step(p[u], ce, &n1[u]);
                any = true;
            }
        }
        if (!any) break;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int kc = kc_of(u);
        const bool act = d < kHufD && kc < m;
        p[u] = min(p[u], s0 + uint32_t(kc + 1) * C);
        P[u * kTPB + tid] = act ? p[u] : 0xFFFFFFFFu;
    }
    __syncthreads();
    // the first entry of the chunk standing on the same boundary leads; leaders still inside the
    // chunk are the survivors
    int lead[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int kc = kc_of(u), sl = u * kTPB + tid;
        const uint32_t ce = s0 + uint32_t(kc + 1) * C;
        lead[u] = d;
        if (d < kHufD && kc < m) {
            for (int j = 0; j < d; j++)
                if (P[(kc << 4) + j] == p[u]) {
                    lead[u] = j;
                    break;
                }
            if (lead[u] == d) {
                if (p[u] < ce) {
                    R[atomicAdd(&R[S], 1u)] = uint32_t(sl);
                } else {
                    X[sl] = p[u];
                    K2[sl] = 0;
                    M[sl] = p[u];
                    KM[sl] = 0;
                }
            }
        }
    }
    __syncthreads();
    const uint32_t nr = R[S];
    for (uint32_t r = tid; r < nr; r += kTPB) {
        const uint32_t t = R[r], e = s0 + ((t >> 4) + 1u) * C, mid = e - C / 2u;
        uint32_t q = P[t], n2 = 0;
        while (q < mid) q = step(q, e, &n2);  // (the sync walk ends well before the middle)
        M[t] = q;
        KM[t] = uint16_t(n2);
        while (q < e) q = step(q, e, &n2);
        X[t] = q;
        K2[t] = uint16_t(n2);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int kc = kc_of(u);
        if (d >= kHufD || kc >= m) continue;
        const uint32_t ce = s0 + uint32_t(kc + 1) * C;
        const int lt = (kc << 4) + lead[u], k = k0 + kc;
        tab[size_t(k) * kHufD + d] = uint16_t(X[lt] - ce);
        cnt[size_t(k) * kHufD + d] = uint16_t(n1[u] + K2[lt]);
        mo[size_t(k) * kHufD + d] = uint16_t(M[lt] - (ce - C));  // (from the chunk's first bit)
        mc[size_t(k) * kHufD + d] = uint16_t(n1[u] + KM[lt]);
    }
}

// The true entry of every chunk through the composed tables, its symbol count from the table pass,
// and the workgroup scan of the counts (base[k], wgsum[g]) -- no walk.
// B (image batch): blockIdx.y = the image; lvl[] stays image 0's -- this image's arrays lie img_tab
// entries after -- and is indexed by constants only, as in rec_chunk_entry (ie_decode.hip).  A
// chunk past its image's stream counts nothing (its table rows say so).
template <bool B = false>
__global__ __launch_bounds__(kTPB) void huf_count_kernel(HufArgs a, const uint16_t* cnt) {
    __shared__ alignas(8) uint32_t scratch[8];
    huf_image<B>(a);
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0;
    if (k < a.nchunks) {
        const uint64_t cstart = a.start_bit + uint64_t(k) * a.chunk_bits;
        int u = k;
        for (int l = 0; l < a.levels; l++) u /= kHufG;
        uint32_t x = a.E[u];
        if constexpr (B) {
            const size_t img = size_t(blockIdx.y) * a.img_tab;
            cnt += img;
#pragma unroll
            for (int l = kRecMaxLevels - 1; l >= 0; l--) {
                if (l < a.levels) {
                    int ul = k;
#pragma unroll
                    for (int m = 0; m < l; m++) ul /= kHufG;
                    x = a.lvl[l][img + size_t(ul) * kHufD + x];
                }
            }
        } else {
            for (int l = a.levels - 1; l >= 0; l--) {
                int ul = k;
                for (int m = 0; m < l; m++) ul /= kHufG;
                x = a.lvl[l][size_t(ul) * kHufD + x];
            }
        }
        a.entry[k] = cstart + x;
        c = cnt[size_t(k) * kHufD + x];
        a.count[k] = c;
    }
    uint32_t tot;
    const uint32_t ex = block_excl_scan(c, scratch, &tot);
    if (k < a.nchunks) a.base[k] = ex;
    if (threadIdx.x == 0) a.wgsum[blockIdx.x] = tot;
}

// The emitting walk: every chunk again from its entry, over the workgroup's chunks' bits staged
// in LDS (a step reads LDS, not the stream in memory: the walk is one dependent chain per lane,
// and the ~800 waves of a 4K payload are too few to hide a memory round trip per code), its
// symbols into LDS at the chunk's place in the workgroup's output, then the workgroup's output
// copied out whole (consecutive lanes, consecutive bytes) -- a lane writing its own chunk's bytes
// straight to memory touches 64 lines per store instruction.  A workgroup whose output exceeds the
// buffer writes from the walk.  A position no code prefixes flags the stream (changed[1]).
#ifndef IE_HUF_EMIT_LDS
#define IE_HUF_EMIT_LDS 40960
#endif
constexpr int kHufEmitT = 2 * kTPB;  // emit threads: two per chunk (its halves, split at the
                                     // middle boundary the table pass recorded)
// B (image batch): blockIdx.y = the image (huf_image), writing into its own slot of out_cap bytes;
// a workgroup whose chunks all lie past its image's stream has nothing to write.  (The same LDS
// as the single-stream form: the batch adds none.)
template <bool B = false>
__global__ __launch_bounds__(kHufEmitT) void huf_emit_kernel(HufArgs a, const uint16_t* mo, const uint16_t* mc) {
    __shared__ uint16_t l1[1 << kHufL1];
    __shared__ alignas(8) uint64_t scratch[kHufEmitT / 64];
    __shared__ uint8_t sym[IE_HUF_EMIT_LDS > 0 ? IE_HUF_EMIT_LDS : 1];
    extern __shared__ uint32_t L[];  // the workgroup's chunks' bits (+ 64 past the last)
    const int tid = threadIdx.x, j = tid % kTPB, half = tid / kTPB;
    huf_image<B>(a);
    if constexpr (B) {
        const size_t img = size_t(blockIdx.y) * a.img_tab;
        mo += img;
        mc += img;
    }
    const uint32_t C = uint32_t(a.chunk_bits);
    const int k0 = blockIdx.x * kTPB, m = min(kTPB, a.nchunks - k0);
    const uint64_t c0 = a.start_bit + uint64_t(k0) * C;
    if constexpr (B) {
        if (c0 >= a.nbits) return;
    }
    const uint64_t base = c0 & ~31ull;
    const uint32_t s0 = uint32_t(c0 - base);
    stage_words_pad(L, a.words, base >> 5, int((s0 + uint32_t(m) * C + 64) >> 5) + 2, a.nbits, tid, kHufEmitT);
    huf_l1(a.lut, l1);  // (ends with a barrier: L staged too)
    // the symbols before this workgroup's chunks: the totals of the workgroups before it
    uint64_t part = 0;
    for (int i = tid; i < int(blockIdx.x); i += kHufEmitT) part += a.wgsum[i];
    const uint64_t ws = wave_sum64(part);
    if ((tid & 63) == 0) scratch[tid >> 6] = ws;
    __syncthreads();
    uint64_t pre = 0;
#pragma unroll
    for (int w = 0; w < kHufEmitT / 64; w++) pre += scratch[w];
    const uint32_t tot = a.wgsum[blockIdx.x];
    const bool staged = IE_HUF_EMIT_LDS > 0 && tot <= uint32_t(IE_HUF_EMIT_LDS);
    const int k = k0 + j;
    if (j < m) {
        const uint32_t lim = uint32_t(min<uint64_t>(a.nbits - base, uint64_t(s0) + uint64_t(m) * C));
        const uint32_t cs = s0 + uint32_t(j) * C, e = cs + C;
        const uint32_t x = uint32_t(a.entry[k] - (a.start_bit + uint64_t(k) * C));  // the true entry offset
        const uint32_t mid = cs + mo[size_t(k) * kHufD + x];
        uint32_t p = half ? mid : cs + x, c = 0;
        const uint32_t end = half ? e : mid;
        const uint64_t at = a.base[k] + (half ? mc[size_t(k) * kHufD + x] : 0u);
        uint8_t* o = staged ? sym + at : a.out + pre + at;
        const uint64_t room = staged ? ~0ull : (a.out_cap > pre + at ? a.out_cap - pre - at : 0ull);
        while (p < end && p < lim) {
            const uint32_t p15 = lbits_pad(L, p, 15);
            uint32_t v = l1[p15 >> (15 - kHufL1)];
            if (!v) v = a.lut[p15];
            const uint32_t len = v >> 8;
            if (!len) {
                atomicOr(&a.changed[1], 1u);
                break;
            }
            if (c >= room) {
                atomicOr(&a.changed[0], 1u);
                break;
            }
            o[c++] = uint8_t(v);
            p += len;
        }
    }
    if (!staged) return;
    __syncthreads();
    if (pre + tot > a.out_cap && tid == 0) atomicOr(&a.changed[0], 1u);
    for (uint32_t i = tid; i < tot && pre + i < a.out_cap; i += kHufEmitT) a.out[pre + i] = sym[i];
}

// The launches of one decode over a.nchunks chunks (write = false: table pass, composition, counts
// and total; write = true: the emit), for one stream or (B) for `images` streams side by side.
template <bool B>
static int huf_launch(HufArgs a, uint16_t* tab, uint32_t* E, uint64_t* total, bool write, int images, hipStream_t s) {
    const int nchunks = a.nchunks;
    const uint64_t chunk_bits = a.chunk_bits;
    const dim3 g((nchunks + kTPB - 1) / kTPB, images), blk(kTPB);
    if (write) {
        const uint16_t* cnt = tab + compose_rows<kHufD, kHufG>(nchunks) * kHufD;
        const uint16_t* mo = cnt + size_t(nchunks) * kHufD;
        hipLaunchKernelGGL(huf_emit_kernel<B>, g, dim3(kHufEmitT), size_t(pad_words(int(((uint64_t(kTPB) * chunk_bits + 95) >> 5) + 3))) * 4, s,
                           a, mo, mo + size_t(nchunks) * kHufD);
        return 0;
    }
    const size_t lds = size_t(pad_words(int(((uint64_t(kHufTC) * chunk_bits + 95) >> 5) + 3))) * 4;
    // the symbol counts after the composition's rows (compose_kernel rewrites the exit tables)
    uint16_t* cnt = tab + compose_rows<kHufD, kHufG>(nchunks) * kHufD;
    uint16_t* mo = cnt + size_t(nchunks) * kHufD;  // then the middle boundaries and their counts
    hipLaunchKernelGGL(huf_table_kernel<B>, dim3((nchunks + kHufTC - 1) / kHufTC, images), blk, lds, s, a, tab, cnt, mo,
                       mo + size_t(nchunks) * kHufD);
    const int levels = launch_compose<kHufD, kHufG, B>(tab, nchunks, E, a.lvl, s, images, a.img_tab, a.img_E);
    if (levels < 0) return -1;
    a.levels = levels;
    a.E = E;
    hipLaunchKernelGGL(huf_count_kernel<B>, g, blk, 0, s, a, cnt);
    hipLaunchKernelGGL(huf_total_kernel<B>, dim3(1, images), blk, 0, s, a.wgsum, int(g.x), total, a.img_wg);
    return levels;
}

int huffman_decode_device(const uint32_t* W, uint64_t nbits, uint64_t start_bit, const uint16_t* lut,
                          uint64_t chunk_bits, uint64_t* entry, uint16_t* tab, uint32_t* E, uint32_t* count,
                          uint64_t* base, unsigned* changed, uint64_t* total, uint8_t* out, bool write, hipStream_t s,
                          uint64_t out_cap) {
    const uint64_t span = nbits > start_bit ? nbits - start_bit : 0;
    const int nchunks = int((span + chunk_bits - 1) / chunk_bits);
    if (nchunks == 0) return 0;
    HufArgs a{};
    a.words = W;
    a.nbits = nbits;
    a.start_bit = start_bit;
    a.chunk_bits = chunk_bits;
    a.nchunks = nchunks;
    a.lut = lut;
    a.entry = entry;
    a.count = count;
    a.wgsum = count + nchunks;  // [ceil(nchunks / kTPB)] after the counts (huffman_count_words)
    a.changed = changed;
    a.base = base;
    a.out = out;
    a.out_cap = out_cap;
    return huf_launch<false>(a, tab, E, total, write, 1, s);
}

size_t huffman_batch_tab(int nchunks) {
    return ((compose_rows<kHufD, kHufG>(nchunks) + 3 * size_t(nchunks)) * kHufD + 7) / 8 * 8;
}
uint32_t huffman_batch_wg(int nchunks) { return uint32_t((nchunks + kTPB - 1) / kTPB); }
uint32_t huffman_batch_entries() { return uint32_t(kHufG); }

int huffman_decode_images(const HufBatch& b, bool write, hipStream_t s) {
    if (b.nchunks <= 0 || b.images <= 0) return 0;
    HufArgs a{};
    a.words = b.words;
    a.chunk_bits = b.chunk_bits;
    a.nchunks = b.nchunks;
    a.lut = b.lut;
    a.entry = b.entry;
    a.count = b.count;
    a.wgsum = b.wgsum;
    a.changed = b.flags;
    a.base = b.base;
    a.out = b.out;
    a.out_cap = b.out_pitch;
    a.img_words = b.img_words;
    a.img_nbits = b.nbits;
    a.img_start = b.start_bit;
    a.img_tab = huffman_batch_tab(b.nchunks);
    a.img_chunks = uint32_t(b.nchunks);
    a.img_wg = huffman_batch_wg(b.nchunks);
    a.img_E = uint32_t(kHufG);
    a.out_pitch = b.out_pitch;
    return huf_launch<true>(a, b.tab, b.E, b.total, write, b.images, s);
}

size_t huffman_table_rows(uint64_t nbits, uint64_t start_bit, uint64_t chunk_bits) {
    const uint64_t span = nbits > start_bit ? nbits - start_bit : 0;
    const int nchunks = int((span + chunk_bits - 1) / chunk_bits);
    return nchunks ? (compose_rows<kHufD, kHufG>(nchunks) + 3 * size_t(nchunks)) * kHufD : 0;  // (+ counts, middles)
}

}  // namespace ie
