// imageencoder_amd/csrc/ie_decode_region.hip -- region decode on gfx950: the pixels of one
// rectangle of every frame (ie_decode_region) or image (ie_decode_images_region).
//
// The record parse covers the whole stream -- the records are a serial chain -- and is the one of
// ie_decode.hip, launched as it is (launch_rec_parse: tables, composition, counts).  What a
// rectangle saves is the rest: the FP64 inverse transform, the pixel stores and, for a host
// destination, the copy out.
//   rec_region_kernel  the decode pass next to rec_decode_kernel, with its mapping: a wave per
//                      kDecChunks chunks, a lane per record in block raster order.  A wave first
//                      does the index arithmetic alone -- its first block index and record count,
//                      hence its blocks' positions in the frame -- and leaves, before it stages a
//                      stream word, when none of its blocks meets the rectangle (the wave that owns
//                      the stream's last block stays: it reports that record's end).  In the waves
//                      that stay, a lane whose block lies outside skips the transform and the
//                      stores; a lane inside transforms its block exactly as decode_record does
//                      and stores the pixels that fall inside the rectangle.
#include "ie_decode_rec.h"

namespace ie {

// The rectangle in pixels and the launch's divisors (block index -> frame, block row, block column).
struct RegionArgs {
    int x0, y0, rw, rh;
    FastDiv div_bpf, div_bx;  // by blocks per frame, by blocks per row
};

struct BlockAt {
    uint32_t f, byi, bxi;  // frame relative to the wave's first block's, block row, block column
};
// rel: the block's index counted from the first block of the frame the wave starts in (< 2^31)
__device__ __forceinline__ BlockAt block_at(uint32_t rel, const DecArgs& d, const RegionArgs& g) {
    BlockAt b;
    b.f = fdiv(rel, g.div_bpf);
    const uint32_t r = rel - b.f * g.div_bpf.d;
    b.byi = fdiv(r, g.div_bx);
    b.bxi = r - b.byi * g.div_bx.d;
    return b;
}
template <int N>
__device__ __forceinline__ bool block_in_rect(const BlockAt& b, const RegionArgs& g) {
    const int px = int(b.bxi) * N, py = int(b.byi) * N;
    return px < g.x0 + g.rw && px + N > g.x0 && py < g.y0 + g.rh && py + N > g.y0;
}

// The record at p (relative to L) of block `rel` counted from frame f0's first block; returns the
// bit after it.  The block's place in the frame is formed again after the transform, from `rel`
// alone, so that one register, not the frame and block coordinates, lives through the transform
// (the 8x8 transform's N * N sums fill the budget of three waves per SIMD).  inside: the
// transform of decode_record (ie_decode.hip) -- dequantised values added in uv-ascending order,
// a term skipped when it is zero in every lane that transforms, +128, clamp, truncation -- and the
// stores of the block's pixels inside the rectangle: pixel (x, y) of the frame goes to
// out + f * frame_pitch + (y - y0) * stride + (x - x0).  Otherwise only the record's end is formed.
template <int N>
__device__ __forceinline__ uint32_t region_record(const uint32_t* L, uint32_t p, bool inside, uint64_t f0, uint32_t rel,
                                                  const DecArgs& a, const RegionArgs& g, const_f64 sR, const_f64 sq) {
    constexpr int NN = N * N;
    constexpr InvZZ<N> izz;
    const int bl = int(lbits(L, p, 4));
    p += 4;
    int length = NN;
    if (a.rle) {
        length = int(lbits(L, p, bl));
        p += bl;
    }
    if (length > NN) length = NN;
    if (inside) {
        const int sh = 16 - bl;
        double t[NN];
#pragma unroll
        for (int k = 0; k < NN; k++) t[k] = 0.0;
        // (a skipped zero term changes at most the sign of a zero sum, which +128 erases: which
        // lanes share the wave does not change a block's pixels)
#pragma unroll
        for (int uv = 0; uv < NN; uv++) {
            const int kz = izz.r[uv];
            double y = 0.0;
            if (kz < length) {
                const uint32_t raw = lbits(L, p + uint32_t(kz * bl), bl);
                y = double(int16_t(int16_t(uint16_t(raw << sh)) >> sh)) * sq[uv];  // utils.hpp:265-269
            }
            if (__ballot(y != 0.0)) {
                const_f64 R = sR + uv * NN;
#pragma unroll
                for (int ij = 0; ij < NN; ij++) t[ij] = t[ij] + R[ij] * y;
            }
        }
        asm volatile("" : "+v"(rel));  // (an opaque copy: not merged with the caller's block_at)
        const BlockAt b = block_at(rel, a, g);
        const uint64_t f = f0 + b.f;
        const int px = int(b.bxi) * N, py = int(b.byi) * N;
        // the block's columns [jl, jh) and rows with 0 <= y < rh lie inside the rectangle
        const int jl = max(g.x0 - px, 0), jh = min(g.x0 + g.rw - px, N);
        uint8_t* o = a.out + f * a.frame_pitch;
#pragma unroll
        for (int i = 0; i < N; i++) {
            const int y = py + i - g.y0;
            if (y < 0 || y >= g.rh) continue;
            uint32_t wv[N / 4];
#pragma unroll
            for (int j = 0; j < N; j++) {
                double x = t[i * N + j] + 128.0;
                x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
                const uint32_t v = uint32_t(uint8_t(x));
                if (j % 4 == 0) wv[j / 4] = v;
                else wv[j / 4] |= v << (8 * (j % 4));
            }
            // (px - x0 is negative for a block the left edge cuts: its columns below jl are not stored)
            uint8_t* row = o + uint64_t(y) * a.stride + int64_t(px - g.x0);
            if (jl == 0 && jh == N && (reinterpret_cast<uintptr_t>(row) & 3u) == 0) {
#pragma unroll
                for (int m = 0; m < N / 4; m++) reinterpret_cast<uint32_t*>(row)[m] = wv[m];
            } else {
#pragma unroll
                for (int j = 0; j < N; j++)
                    if (j >= jl && j < jh) row[j] = uint8_t(wv[j / 4] >> (8 * (j % 4)));
            }
        }
    }
    return p + uint32_t(length * bl);
}

// (waves_per_eu: at least three waves per SIMD, i.e. at most 168 VGPRs, rec_decode_kernel<8>'s
// occupancy -- the batch instantiation lands on 169 without it; measured at two waves the 8x8
// whole-frame rectangle took 1.43x ie_decode_frames' time)
template <int N, bool B = false>
__global__ __launch_bounds__(64 * kRecWPB) __attribute__((amdgpu_waves_per_eu(3))) void rec_region_kernel(RecParseArgs a, DecArgs d, RegionArgs g) {
    constexpr int D = RecGeom<N>::D;
    constexpr int P = kDecChunks;
    rec_image<B>(a);
    if constexpr (B) d.out += size_t(blockIdx.y) * d.frame_pitch;  // (d.nframes = 1: block index < bx * by)
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_all[];  // per wave: the P chunks' bits + D + 64
    const const_f64 sR = (const_f64)(d.tab->R);
    const const_f64 sq = (const_f64)(d.tab->qd);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int k0 = (blockIdx.x * kRecWPB + wv) * P;
    if (k0 >= a.nchunks) return;
    const int m = min(P, a.nchunks - k0);
    // the wave's blocks: as rec_decode_kernel finds them
    uint64_t part = 0;
    for (int q = lane; q < k0 / (4 * a.seg); q += 64) part += a.wgsum[q];
    const uint64_t first = wave_sum64(part) + a.lbase[k0];
    uint32_t R[P], Rall = 0;
    bool listed = true;
#pragma unroll
    for (int j = 0; j < P; j++) {
        R[j] = j < m ? a.cnt[k0 + j] : 0u;
        Rall += R[j];
        listed = listed && R[j] <= uint32_t(kRecPosCap);
    }
    if (k0 + m == a.nchunks && lane == 0) *a.total = first + Rall;
    const uint64_t bpf = uint64_t(d.bx) * d.by;
    const uint64_t nblocks = uint64_t(d.nframes) * bpf;
    if (first >= nblocks) return;
    const uint32_t nmine = uint32_t(min<uint64_t>(Rall, nblocks - first));  // the wave's records that are blocks
    const uint64_t f0 = first / bpf;                // (wave-uniform)
    const uint32_t r0 = uint32_t(first - f0 * bpf);  // block i of the wave is block r0 + i counted from frame f0
    bool any = false;
    for (uint32_t i = lane; i < nmine; i += 64) any = any || block_in_rect<N>(block_at(r0 + i, d, g), g);
    const bool has_last = first + nmine == nblocks;
    if (!__ballot(any) && !has_last) return;

    uint32_t* L = dyn_all + size_t(wv) * rec_decode_stream_words(uint32_t(P) * a.C, D);
    const RecSpan sp = rec_span(a);
    const uint64_t c0 = sp.start + uint64_t(k0) * a.C;
    const uint64_t base = c0 & ~31ull;
    const int off = stage_words16(L, a.words, base >> 5, int((uint32_t(c0 - base) + uint32_t(m) * a.C + D + 64) >> 5) + 2,
                                  sp.nbits, lane);
    const uint32_t ob = 32u * uint32_t(off);
    const uint32_t s0 = uint32_t(c0 - base) + ob;
    const uint64_t lbase0 = base - ob;  // stream bit of L's bit 0
    wave_sync();
    if (listed) {
        for (uint32_t i = lane; i < nmine; i += 64) {
            const BlockAt at = block_at(r0 + i, d, g);
            const bool inside = block_in_rect<N>(at, g), last = first + i == nblocks - 1;
            if (!inside && !last) continue;
            uint32_t j = 0, r = i;
#pragma unroll
            for (int jj = 0; jj < P - 1; jj++)
                if (j == uint32_t(jj) && r >= R[jj]) {
                    r -= R[jj];
                    j++;
                }
            const uint32_t q = region_record<N>(L, ob + j * a.C + a.pos[size_t(k0 + j) * kRecPosCap + r], inside, f0, r0 + i,
                                                d, g, sR, sq);
            if (last) *a.end_out = lbase0 + q;
        }
        return;
    }
    // a chunk with more records than its position list holds: walk the chunks again, 64 records
    // at a time
    uint32_t gi = 0;  // records of the wave walked so far
    for (int j = 0; j < m; j++) {
        uint32_t p = s0 + uint32_t(j) * a.C + rec_chunk_entry<N, B>(a, k0 + j);
        const uint32_t wend = uint32_t(min<uint64_t>(s0 + uint64_t(j + 1) * a.C, sat_sub(sp.nbits, lbase0)));
        while (p < wend && gi < nmine) {
            uint32_t mine = 0, n = 0;
            while (n < 64u && p < wend) {
                const uint32_t len = rec_len<N>(L, p, d.rle);
                if (!len) {
                    p++;
                    continue;
                }
                if (n == uint32_t(lane)) mine = p;
                n++;
                p += len;
            }
            const uint32_t i = gi + uint32_t(lane);
            if (uint32_t(lane) < n && i < nmine) {
                const BlockAt at = block_at(r0 + i, d, g);
                const bool inside = block_in_rect<N>(at, g), last = first + i == nblocks - 1;
                if (inside || last) {
                    const uint32_t q = region_record<N>(L, mine, inside, f0, r0 + i, d, g, sR, sq);
                    if (last) *a.end_out = lbase0 + q;
                }
            }
            gi += n;
        }
    }
}

// The parse passes of ie_decode.hip, then the region pass; B: over `images` independent streams.
template <int N, bool B>
int launch_region_t(RecParseArgs a, const DecArgs& d, const RegionArgs& g, int images, hipStream_t s) {
    if (a.nchunks <= 0) return 0;
    const int levels = launch_rec_parse(a, N, images, B, s);
    if (levels < 0) return -1;
    const int nb = (a.nchunks + kRecWPB * kDecChunks - 1) / (kRecWPB * kDecChunks);
    hipLaunchKernelGGL((rec_region_kernel<N, B>), dim3(nb, images), dim3(64 * kRecWPB), rec_decode_lds(a.C, N), s, a, d, g);
    return levels;
}

int launch_rec_parse_decode_region(const RecParseArgs& a, const DecArgs& d, int n, int images, bool batch, int x0, int y0,
                                   int rw, int rh, hipStream_t s) {
    const RegionArgs g{x0, y0, rw, rh, make_fastdiv(uint32_t(d.bx) * uint32_t(d.by)), make_fastdiv(uint32_t(d.bx))};
    if (batch) return n == 4 ? launch_region_t<4, true>(a, d, g, images, s) : launch_region_t<8, true>(a, d, g, images, s);
    return n == 4 ? launch_region_t<4, false>(a, d, g, 1, s) : launch_region_t<8, false>(a, d, g, 1, s);
}

}  // namespace ie
