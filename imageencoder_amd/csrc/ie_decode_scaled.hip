// imageencoder_amd/csrc/ie_decode_scaled.hip -- scaled decode on gfx950: every frame
// (ie_decode_scaled) or image (ie_decode_images_scaled) at 1/S of its width and height, S = 1, 2,
// 4 or 8 and at most the block size: the thumbnail out of the decode pass.
//
// The record parse covers the whole stream and is the one of ie_decode.hip, launched as it is
// (launch_rec_parse: tables, composition, counts).  What a scale saves is behind the transform: a
// block stores (N/S)^2 bytes in place of N^2, and a host destination is copied 1/S^2 of the bytes.
//   rec_scaled_kernel  the decode pass next to rec_decode_kernel, with its mapping: a wave per
//                      kDecChunks chunks, a lane per record in block raster order.  Every block
//                      contributes, so no wave leaves early.  A lane transforms its block exactly
//                      as decode_record does, down to the truncated 8-bit pixels, sums them as
//                      integers over the block's S x S cells, rounds half up and stores the cells'
//                      means: out[Y][X] = (sum of full[Y*S+dy][X*S+dx] + S*S/2) >> (2 log2 S).
#include "ie_decode_rec.h"

namespace ie {

// The record at p (relative to L) of block `rel` counted from frame f0's first block; returns the
// bit after it.  The transform is decode_record's (ie_decode.hip): dequantised values added in
// uv-ascending order, a term skipped when it is zero in every lane that transforms (it can change
// at most the sign of a zero sum, which +128 erases), un-contracted FP64, +128, clamp, truncation.
// The block's place in the frame is formed after the transform from `rel` alone (one register, not
// frame, row and column, lives through the 8x8 transform's 64 sums) by two 32-bit divisions: they
// measured the same as region_record's multiply-high divisions and need no launch constants.  The
// block's M = N/S rows of M bytes go to out + f * frame_pitch + (byi * M + Y) * stride + bxi * M,
// each with the widest store its address allows: words for M >= 4, a halfword for M = 2, else bytes.
template <int N, int S>
__device__ __forceinline__ uint32_t scaled_record(const uint32_t* L, uint32_t p, uint64_t f0, uint32_t rel, const DecArgs& a,
                                                  const_f64 sR, const_f64 sq) {
    constexpr int NN = N * N, M = N / S;
    constexpr int kShift = S == 1 ? 0 : S == 2 ? 2 : S == 4 ? 4 : 6;  // 2 log2 S
    constexpr InvZZ<N> izz;
    const int bl = int(lbits(L, p, 4));
    p += 4;
    int length = NN;
    if (a.rle) {
        length = int(lbits(L, p, bl));
        p += bl;
    }
    if (length > NN) length = NN;
    const int sh = 16 - bl;
    double t[NN];
#pragma unroll
    for (int k = 0; k < NN; k++) t[k] = 0.0;
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
    asm volatile("" : "+v"(rel));  // (an opaque copy: the place is formed here, not before the transform)
    const uint32_t bpf = uint32_t(a.bx) * uint32_t(a.by);
    const uint32_t f = rel / bpf, r = rel - f * bpf;
    const uint32_t byi = r / uint32_t(a.bx), bxi = r - byi * uint32_t(a.bx);
    uint8_t* o = a.out + (f0 + f) * a.frame_pitch + uint64_t(byi) * M * a.stride + uint64_t(bxi) * M;
#pragma unroll
    for (int Y = 0; Y < M; Y++) {
        uint32_t sum[M];
#pragma unroll
        for (int X = 0; X < M; X++) sum[X] = 0u;
#pragma unroll
        for (int dy = 0; dy < S; dy++)
#pragma unroll
            for (int j = 0; j < N; j++) {
                double x = t[(Y * S + dy) * N + j] + 128.0;
                x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
                sum[j / S] += uint32_t(uint8_t(x));  // the integer pixel of the full decode
            }
        uint32_t wv[(M + 3) / 4];
#pragma unroll
        for (int X = 0; X < M; X++) {
            const uint32_t v = (sum[X] + uint32_t(S * S / 2)) >> kShift;  // <= 255: the mean, rounded half up
            if (X % 4 == 0) wv[X / 4] = v;
            else wv[X / 4] |= v << (8 * (X % 4));
        }
        uint8_t* row = o + uint64_t(Y) * a.stride;
        const uintptr_t ra = reinterpret_cast<uintptr_t>(row);
        if (M >= 4 && (ra & 3u) == 0) {
#pragma unroll
            for (int m = 0; m < M / 4; m++) reinterpret_cast<uint32_t*>(row)[m] = wv[m];
        } else if (M == 2 && (ra & 1u) == 0) {
            *reinterpret_cast<uint16_t*>(row) = uint16_t(wv[0]);
        } else {
#pragma unroll
            for (int X = 0; X < M; X++) row[X] = uint8_t(wv[X / 4] >> (8 * (X % 4)));
        }
    }
    return p + uint32_t(length * bl);
}

// (the 8x8 instantiations take 153 - 157 VGPRs: three waves per SIMD, rec_decode_kernel<8>'s
// occupancy, without an occupancy attribute)
template <int N, int S, bool B = false>
__global__ __launch_bounds__(64 * kRecWPB) void rec_scaled_kernel(RecParseArgs a, DecArgs d) {
    constexpr int D = RecGeom<N>::D;
    constexpr int P = kDecChunks;
    rec_image<B>(a);
    if constexpr (B) d.out += size_t(blockIdx.y) * d.frame_pitch;  // (d.nframes = 1: block index < bx * by)
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_all[];  // per wave: the P chunks' bits + D + 64
    const const_f64 sR = (const_f64)(d.tab->R);
    const const_f64 sq = (const_f64)(d.tab->qd);
    // (the wave's index through readfirstlane: what follows from it -- the chunk range, the staged
    // span, the first block index -- stays in scalar registers, out of the transform's VGPR budget)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    const int k0 = (blockIdx.x * kRecWPB + wv) * P;
    if (k0 >= a.nchunks) return;
    const int m = min(P, a.nchunks - k0);
    uint32_t* L = dyn_all + size_t(wv) * rec_decode_stream_words(uint32_t(P) * a.C, D);
    const RecSpan sp = rec_span(a);
    const uint64_t c0 = sp.start + uint64_t(k0) * a.C;
    const uint64_t base = c0 & ~31ull;
    // the chunks' bits first (16-byte loads in flight while the indices below are read)
    const int off = stage_words16(L, a.words, base >> 5, int((uint32_t(c0 - base) + uint32_t(m) * a.C + D + 64) >> 5) + 2,
                                  sp.nbits, lane);
    const uint32_t ob = 32u * uint32_t(off);
    const uint32_t s0 = uint32_t(c0 - base) + ob;
    const uint64_t lbase0 = base - ob;  // stream bit of L's bit 0
    // the wave's blocks: as rec_decode_kernel finds them
    uint64_t part = 0;
    for (int q = lane; q < k0 / (4 * a.seg); q += 64) part += a.wgsum[q];
    const uint64_t fsum = wave_sum64(part) + a.lbase[k0];
    const uint64_t first = uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(fsum))))) |
                           (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(fsum >> 32))))) << 32);
    uint32_t R[P], Rall = 0;
    bool listed = true;
#pragma unroll
    for (int j = 0; j < P; j++) {
        R[j] = j < m ? a.cnt[k0 + j] : 0u;
        Rall += R[j];
        listed = listed && R[j] <= uint32_t(kRecPosCap);
    }
    if (k0 + m == a.nchunks && lane == 0) *a.total = first + Rall;
    wave_sync();
    const uint64_t bpf = uint64_t(d.bx) * d.by;
    const uint64_t nblocks = uint64_t(d.nframes) * bpf;
    if (first >= nblocks) return;
    const uint32_t nmine = uint32_t(min<uint64_t>(Rall, nblocks - first));  // the wave's records that are blocks
    const uint64_t f0 = first / bpf;                // (wave-uniform)
    const uint32_t r0 = uint32_t(first - f0 * bpf);  // block i of the wave is block r0 + i counted from frame f0
    if (listed) {
        for (uint32_t i = lane; i < nmine; i += 64) {
            uint32_t j = 0, r = i;
#pragma unroll
            for (int jj = 0; jj < P - 1; jj++)
                if (j == uint32_t(jj) && r >= R[jj]) {
                    r -= R[jj];
                    j++;
                }
            const uint32_t q = scaled_record<N, S>(L, ob + j * a.C + a.pos[size_t(k0 + j) * kRecPosCap + r], f0, r0 + i, d, sR, sq);
            if (first + i == nblocks - 1) *a.end_out = lbase0 + q;
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
                const uint32_t q = scaled_record<N, S>(L, mine, f0, r0 + i, d, sR, sq);
                if (first + i == nblocks - 1) *a.end_out = lbase0 + q;
            }
            gi += n;
        }
    }
}

// The parse passes of ie_decode.hip, then the scaled pass; B: over `images` independent streams.
template <int N, int S, bool B>
int launch_scaled_t(RecParseArgs a, const DecArgs& d, int images, hipStream_t s) {
    if (a.nchunks <= 0) return 0;
    const int levels = launch_rec_parse(a, N, images, B, s);
    if (levels < 0) return -1;
    const int nb = (a.nchunks + kRecWPB * kDecChunks - 1) / (kRecWPB * kDecChunks);
    hipLaunchKernelGGL((rec_scaled_kernel<N, S, B>), dim3(nb, B ? images : 1), dim3(64 * kRecWPB), rec_decode_lds(a.C, N), s, a,
                       d);
    return levels;
}
template <int N, bool B>
int launch_scaled_n(const RecParseArgs& a, const DecArgs& d, int scale, int images, hipStream_t s) {
    switch (scale) {
    case 1: return launch_scaled_t<N, 1, B>(a, d, images, s);
    case 2: return launch_scaled_t<N, 2, B>(a, d, images, s);
    case 4: return launch_scaled_t<N, 4, B>(a, d, images, s);
    case 8:
        if constexpr (N == 8) return launch_scaled_t<N, 8, B>(a, d, images, s);
    }
    return -2;
}

int launch_rec_parse_decode_scaled(const RecParseArgs& a, const DecArgs& d, int n, int images, bool batch, int scale,
                                   hipStream_t s) {
    if (batch) return n == 4 ? launch_scaled_n<4, true>(a, d, scale, images, s) : launch_scaled_n<8, true>(a, d, scale, images, s);
    return n == 4 ? launch_scaled_n<4, false>(a, d, scale, images, s) : launch_scaled_n<8, false>(a, d, scale, images, s);
}

}  // namespace ie
