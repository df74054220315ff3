// imageencoder_amd/csrc/ie_decode.hip -- the record parse and decode on gfx950, the inverse path
// (ImageDecoder.cpp:55-122).
//
// The reference parses block records serially (Block::loadFromStream, Block.cpp:442-472) because a
// record's length is only known once its header is read (4 + bl * (Lw + 1) bits with RLE, 4 +
// bl * N * N without; bl = 0 is a record of 4 bits, a block of zeros -- the reference reads its
// count and values with get(0) = 0, BitStream.cpp:30-40).  Here the stream is cut into chunks and
// parsed exactly with the transfer tables of ie_decode_blocks.h: D = the longest record, 4 + 15 *
// (N * N + 1) bits, and G = 32 tables per group (RecGeom, ie_device.h).
//   rec_table2_kernel  a wave per tm chunks writes their transfer tables: the D walks of a chunk
//                      share their work through claims in LDS -- the first walk to reach a position
//                      owns it, a later walk that lands there stops and takes the owner's exit --
//                      so about one walk per chunk survives.
//   compose_kernel, compose_top_kernel (ie_decode_blocks.h) compose the tables.
//   rec_count_kernel   a lane per chunk: entry = the prefix maps applied to its top-level entry;
//                      the chunk's true records are walked from it: their positions and their
//                      count; the workgroup scans its chunks' counts and stores their total.
//   rec_decode_kernel  a wave per kDecChunks chunks: first block index = the totals of the count
//                      workgroups before the chunk's, plus the counts before it in its own; a
//                      record per lane: dequantise (Block.cpp:163-169), FP64 IDCT in the
//                      reference's order (algo.cpp:343-363), +128, clamp, truncate
//                      (Block.cpp:100-107).
//   rec_spec_kernel    the optional speculative parse in place of tables and composition: a lane
//                      per chunk walks from a warm-up distance before it; the count pass verifies
//                      every exit and the decode writes nothing if one was wrong.
//   gop_init_kernel    the position and total arrays of a device-chained video decode.
//   gop_cont_kernel    the same arrays for a chunk of frames that starts where an earlier chunk
//                      ended (ie_vdec): the first bit is read from that chunk's end word.
#include <algorithm>
#include <cstdlib>

#include "ie_decode_rec.h"
#include "ie_recbits.h"

namespace ie {

constexpr uint32_t kRoot = 0x8000u;  // table pass: a walk result that is an exit, not an owner

__host__ __device__ constexpr int rec_table_stream_words(uint32_t C) { return int((C + 95) >> 5) + 3; }
// a count wave's LDS words: seg chunks' bits + 64 + alignment slack, a multiple of 4 (16-byte rows)
__host__ __device__ constexpr int rec_count_wave_words(uint32_t C, int seg) {
    return (int((uint64_t(seg) * C + 95) >> 5) + 3 + 3 + 3) & ~3;
}
int rec_count_seg(uint32_t C) {  // chunks per count wave: <= 16, a wave's bits within 10 KB
    return int(std::max<uint64_t>(1, std::min<uint64_t>(16, (uint64_t(10 * 1024) * 8 - 256) / C)));
}

// decode the record at p (relative to L) as block g; returns the bit after it.  Coefficient uv
// (row-major) is value number izz[uv] of the record, read straight from its bit position, so the
// IDCT runs in the reference's uv-ascending order without a zig-zag array.
template <int N>
__device__ __forceinline__ uint32_t decode_record(const uint32_t* L, uint32_t p, uint64_t g, const DecArgs& a,
                                                  const_f64 sR, const_f64 sq) {
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
    const int sh = 16 - bl;
    double t[NN];
#pragma unroll
    for (int k = 0; k < NN; k++) t[k] = 0.0;
    // Block::processIDCTMulQ: Y *= q, then temp[ij] += R[uv][ij] * Y[uv] over uv ascending.  A
    // zero Y term adds +-0: it leaves every partial sum unchanged but possibly the sign of a zero,
    // which +128 and the clamp erase, so a term is skipped when it is zero in every lane (the
    // branch stays uniform and the R rows come through the scalar cache).
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
    const uint64_t bpf = uint64_t(a.bx) * a.by;
    const uint64_t f = g / bpf, r = g - f * bpf;
    const int byi = int(r / a.bx), bxi = int(r - uint64_t(byi) * a.bx);
    uint8_t* o = a.out + f * a.frame_pitch + uint64_t(byi) * N * a.stride + uint64_t(bxi) * N;
#pragma unroll
    for (int i = 0; i < N; i++) {
        uint32_t wv[N / 4];
#pragma unroll
        for (int j = 0; j < N; j++) {
            double x = t[i * N + j] + 128.0;
            if (a.add_base) x = double(o[uint64_t(i) * a.stride + j]) + x;  // expandDifferences
            x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
            const uint32_t b = uint32_t(uint8_t(x));
            if (j % 4 == 0) wv[j / 4] = b;
            else wv[j / 4] |= b << (8 * (j % 4));
        }
        uint8_t* row = o + uint64_t(i) * a.stride;
        if ((reinterpret_cast<uintptr_t>(row) & 3u) == 0) {
#pragma unroll
            for (int m = 0; m < N / 4; m++) reinterpret_cast<uint32_t*>(row)[m] = wv[m];
        } else {
#pragma unroll
            for (int j = 0; j < N; j++) row[j] = uint8_t(wv[j / 4] >> (8 * (j % 4)));
        }
    }
    return p + uint32_t(length * bl);
}

// Table pass (rec_table2_kernel, below): one wave tabulates tm consecutive chunks (runtime,
// rec_table_geometry) and walks only from positions where a record can start.  Entry d of a chunk
// first slides to the next
// valid position nv(d) -- every entry between two valid positions shares one walk -- so the walks
// start at the valid positions of [0, min(D, C)) plus, for the entries past the last of them, the
// first valid position after (v*, entry slot D of the chunk).  The walk list is compacted from the
// bitmap and lanes take walks from it as theirs end, across all tm chunks, so a wave's 64 lanes
// carry several chunks' surviving walks side by side.  Claims: one open-addressing table per wave,
// keyed by the wave-relative position (walks of different chunks never meet: a walk stops at its
// chunk's end).  Results: a walk that merged takes its owner's exit (owner chains are read-only
// chases; only non-roots are written).  The valid-header bitmap comes 32 positions at a time from
// bitwise operations on shifted windows (valid_mask32, ie_recbits.h).

// The first valid position at or after p before ce (ce: a chunk end, a multiple of 32), else ce.
// NZ[i]: the first bitmap word at or after word i holding a valid position (a sentinel past the
// last), so a run of positions where no record can start costs one read, not one per word.
template <int N>
__device__ __forceinline__ uint32_t next_valid(const uint32_t* VB, const uint16_t* NZ, uint32_t p, uint32_t ce) {
    if (p >= ce) return p;
    uint32_t wi = p >> 5, msk = VB[wi] & (0xFFFFFFFFu << (p & 31u));
    if (!msk) {
        wi = NZ[wi + 1];
        if (wi >= (ce >> 5)) return ce;
        msk = VB[wi];
    }
    return (wi << 5) + uint32_t(__builtin_ctz(msk));
}

// next_valid without branches, for the loops every lane runs: the bitmap word, the next non-empty
// word and that word's bits are all read (the last only matters past an empty word); word
// indices are clamped to the chunk's last bitmap word, so every read stays inside the chunk.
__device__ __forceinline__ uint32_t next_valid_sel(const uint32_t* VB, const uint16_t* NZ, uint32_t p, uint32_t ce) {
    const uint32_t cw = (ce >> 5) - 1u;  // the chunk's last bitmap word
    const uint32_t wi = min(p >> 5, cw), nz = NZ[wi + 1];
    const uint32_t mk = VB[wi] & (0xFFFFFFFFu << (p & 31u));
    const uint32_t m2 = VB[min(uint32_t(nz), cw)];
    const uint32_t q = mk ? (wi << 5) + uint32_t(__builtin_ctz(mk))
                          : (nz <= cw ? (uint32_t(nz) << 5) + uint32_t(__builtin_ctz(m2)) : ce);
    return p >= ce ? p : q;
}

__host__ __device__ constexpr int rec_table2_words(uint32_t C, int D, int tm, int hbits) {
    // L (stream words, 16-byte aligned staging: +4), VB, claims, then the u16 walk results (an
    // exit with kRoot set, or the owner a merged walk joined), the u16 walk list (walk ids: the
    // start position follows from the id, except a chunk's v*), the chunks' v* positions and the
    // u16 next-valid-word table (tm CW + 1 entries)
    return (rec_table_stream_words(uint32_t(tm) * C) + 4 + 3) / 4 * 4 + tm * int(C >> 5) + (1 << hbits) +
           2 * ((tm * (D + 1) + 1) / 2) + tm + (tm * int(C >> 5) + 2) / 2;
}

template <int N, bool B = false>
__global__ __launch_bounds__(64) void rec_table2_kernel(RecParseArgs a) {
    constexpr int D = RecGeom<N>::D, D1 = D + 1;
    rec_image<B>(a);
    extern __shared__ __attribute__((aligned(16))) uint32_t Ls[];
    const int lane = threadIdx.x, tm = a.tm;
    const int k0 = blockIdx.x * tm;
    const int m = min(tm, a.nchunks - k0);
    const uint32_t C = a.C, CW = C >> 5;
#if IE_PROFILE
    unsigned long long* ws = a.wstamp ? a.wstamp + size_t(blockIdx.x) * 8 : nullptr;
    auto wstamp = [&](int i) {
        if (ws && lane == 0) ws[i] = __builtin_amdgcn_s_memrealtime();
    };
    wstamp(0);
#else
    auto wstamp = [](int) {};
#endif
    const int SW = (rec_table_stream_words(uint32_t(tm) * C) + 4 + 3) / 4 * 4;
    uint32_t* L = Ls;
    uint32_t* VB = Ls + SW;
    uint32_t* H = VB + tm * int(CW);
    const uint32_t HM = (1u << a.hbits) - 1u;
    // res[id]: kRoot | the exit of a walk that left its chunk, or the id of the walk it merged into
    // (ids < D1 * tm < kRoot; one u16 per walk keeps a wave in 4.8 KB of LDS: 32 waves per CU)
    uint16_t* res = reinterpret_cast<uint16_t*>(H + HM + 1);
    const int RW = (tm * D1 + 1) / 2;                                  // words of res, and of wl
    uint16_t* wl = reinterpret_cast<uint16_t*>(H + HM + 1 + RW);
    uint32_t* vst = H + HM + 1 + 2 * RW;                               // [tm] every chunk's v* position
    uint16_t* NZ = reinterpret_cast<uint16_t*>(vst + tm);
    const RecSpan sp = rec_span(a);
    const uint64_t c0 = sp.start + uint64_t(k0) * C;
    const uint64_t base = c0 & ~31ull;
    const int off = stage_words16(L, a.words, base >> 5, int(((c0 - base) + uint64_t(m) * C + 64) >> 5) + 2,
                                  sp.nbits, lane);
    const uint32_t s0 = uint32_t(c0 - base) + 32u * uint32_t(off);  // the wave's first bit in L
    // positions below are relative to s0; no record starts at or past the stream's end
    const uint32_t lim = uint32_t(min<uint64_t>(sat_sub(sp.nbits, c0), uint64_t(m) * C));
    for (uint32_t i = lane; i <= HM; i += 64) H[i] = 0xFFFFFFFFu;
    __syncthreads();
    wstamp(1);
    // 1. valid-header bitmap, 32 positions per word
    for (uint32_t i = lane; i < uint32_t(m) * CW; i += 64) {
        const uint32_t p0 = i << 5;
        uint32_t msk = 0;
        if (p0 < lim) {
            const uint32_t q = s0 + p0, w0 = q >> 5, sb = q & 31u;
            const uint64_t v = (((uint64_t(L[w0]) << 32) | L[w0 + 1]) << sb) |
                               (sb ? (uint64_t(L[w0 + 2]) >> (32 - sb)) : 0ull);
            msk = valid_mask32<N>(v, a.rle);
            const uint32_t cut = lim - p0;
            if (cut < 32u) msk &= (1u << cut) - 1u;
        }
        VB[i] = msk;
    }
    __syncthreads();
    {  // NZ: a suffix minimum over the bitmap words, 64 at a time from the end (lane l takes
       // word b0 + 63 - l, so the suffix is a DPP prefix over the lanes)
        const uint32_t nwd = uint32_t(m) * CW;
        uint32_t carry = nwd;
        for (int b0 = int((nwd - 1) & ~63u); b0 >= 0; b0 -= 64) {
            const uint32_t i = uint32_t(b0 + 63 - lane);
            const uint32_t v = min(wave_incl_min_dpp((i < nwd && VB[i]) ? i : nwd), carry);
            if (i < nwd) NZ[i] = uint16_t(v);
            carry = __builtin_amdgcn_readlane(v, 63);
        }
        if (lane == 0) NZ[nwd] = uint16_t(nwd);
    }
    __syncthreads();
    wstamp(2);
    // 2. the walk list: valid positions of [0, min(D, C)) of every chunk, then every chunk's v*
    const uint32_t De = min(uint32_t(D), C), DW = (De + 31) >> 5;
    uint32_t nw = 0;  // (wave-uniform)
    for (uint32_t i0 = 0; i0 < uint32_t(m) * DW; i0 += 64) {
        const uint32_t i = i0 + lane;
        uint32_t bits = 0, j = 0, w = 0;
        if (i < uint32_t(m) * DW) {
            j = i / DW;
            w = i - j * DW;
            bits = VB[j * CW + w];
            const uint32_t rem = De - (w << 5);
            if (rem < 32u) bits &= (1u << rem) - 1u;
        }
        const uint32_t cnt = __popc(bits);
        uint32_t incl = cnt;  // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        uint32_t at = nw + incl - cnt;
        while (bits) {
            const uint32_t b = __builtin_ctz(bits);
            bits &= bits - 1u;
            wl[at++] = uint16_t(j * D1 + (w << 5) + b);  // (starts at j C + (w << 5) + b)
        }
        nw += __shfl(incl, 63, 64);
    }
    {
        uint32_t vs = 0xFFFFFFFFu;
        if (lane < m && De < C) {
            const uint32_t cs = uint32_t(lane) * C, ce = cs + C;
            const uint32_t v = next_valid<N>(VB, NZ, cs + De, ce);
            if (v < ce) vs = v;
        }
        const uint64_t bm = __ballot(vs != 0xFFFFFFFFu);
        if (vs != 0xFFFFFFFFu) {
            const uint32_t r = __builtin_amdgcn_mbcnt_hi(uint32_t(bm >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(bm), 0u));
            wl[nw + r] = uint16_t(uint32_t(lane) * D1 + D);
            vst[lane] = vs;
        }
        nw += uint32_t(__popcll(bm));
    }
    __syncthreads();
    wstamp(3);
    // 3. the walks: lanes take the next walk of the list as theirs ends
    {
        uint32_t nxt = 0, p = 0, id = 0, ce = 0, nsteps = 0, wsteps = 0, rsteps = 0;
        bool act = false;
        // One step of an active walk at p (< ce, a valid position): the record's header, the claim
        // and the next position.  The claim's result is read last, so the atomic's round trip
        // overlaps the header read and the bitmap reads of the next position.  The claim table is
        // direct-mapped and lossy: a slot another position holds is not probed on -- the walk goes
        // on unclaimed there and meets its owner's claims further on.
        auto walk_step = [&]() {
            nsteps++;
            wsteps++;
            const uint32_t head = lbits(L, s0 + p, 20);
            const uint32_t o = atomicCAS(&H[(p * 2654435761u) >> 16 & HM], 0xFFFFFFFFu, (p << 16) | id);
            const uint32_t np = next_valid_sel(VB, NZ, p + rec_len_sel<N>(head, a.rle), ce);
            if (o != 0xFFFFFFFFu && (o >> 16) == p) {  // an earlier walk was here: take its exit
                res[id] = uint16_t(o & 0xFFFFu);
                act = false;
                wsteps = 0;
            } else if (np >= ce) {  // left the chunk
                res[id] = uint16_t(kRoot | (np - ce));
                act = false;
                rsteps += wsteps;  // (profiling: steps of walks that reached the chunk's end)
                wsteps = 0;
            } else {
                p = np;
            }
        };
        // (a) while the list lasts: idle lanes take the next walks, every step claims its position
        // (claiming 4-16 steps longer measured equal or slower)
        while (nxt < nw) {  // (wave-uniform)
            const uint64_t need = __ballot(!act);
            if (!act) {
                const uint32_t r = nxt + __builtin_amdgcn_mbcnt_hi(uint32_t(need >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(need), 0u));
                if (r < nw) {
                    id = wl[r];
                    const uint32_t j = id / D1, d = id - j * D1;
                    p = (d < uint32_t(D)) ? j * C + d : vst[j];  // (< the chunk's end: d < min(D, C))
                    ce = (j + 1u) * C;
                    act = true;
                }
            }
            nxt += uint32_t(__popcll(need));
            if (act) walk_step();
        }
        // (b) the list is empty.  The walks still going are many (a lane per walk when the list ran
        // out, most of them on the same few paths).  8x8: they keep claiming until every lane's walk
        // has left its chunk or merged -- they merge into each other.  4x4: they run to the chunk's
        // end unclaimed, a third cheaper per step.  Measured on one 4K noise frame (tools/ab.py --op
        // decode, same process): claims to the end take the 4x4 walk from 575 to 222 lane-steps per
        // chunk and 47.6 to 32.7 steps of the longest lane (tools/dec_stamps.py), yet the decode
        // 132.0 -> 135.4 us; 8x8 210.3 -> 206.6 us.
        constexpr bool kClaimToEnd = N == 8;
        if (kClaimToEnd) {
            while (__ballot(act)) {
                if (act) walk_step();
            }
        } else if (act) {
            while (p < ce) {
                nsteps++;
                wsteps++;
                p = next_valid_sel(VB, NZ, p + rec_len_sel<N>(lbits(L, s0 + p, 20), a.rle), ce);
            }
            res[id] = uint16_t(kRoot | (p - ce));
            rsteps += wsteps;
        }
#if IE_PROFILE
        if (ws) {
            const uint32_t mx = __reduce_max_sync(~0ull, nsteps);
            const uint32_t sm = __reduce_add_sync(~0ull, nsteps);
            const uint32_t rs = __reduce_add_sync(~0ull, rsteps);
            if (lane == 0) {
                ws[6] = (uint64_t(mx) << 32) | sm;
                ws[7] = (uint64_t(nw) << 32) | rs;  // walks, steps of the walks that left the chunk
            }
        }
#endif
        (void)nsteps;
        (void)rsteps;
    }
    __syncthreads();
    wstamp(4);
    // 4. merged walks take their root's exit.  A lane may overwrite an entry another lane's chase
    // passes through: it writes the root's own value (kRoot | exit), so that chase ends there with
    // the same answer.
    for (uint32_t r = lane; r < nw; r += 64) {
        const uint32_t id = wl[r];
        uint32_t x = res[id];
        if (x & kRoot) continue;
        while (!(x & kRoot)) x = res[x];
        res[id] = uint16_t(x);
    }
    __syncthreads();
    // 5. every entry: its walk's exit
    uint16_t* T = a.tab + size_t(k0) * D;
    for (uint32_t e = lane; e < uint32_t(m) * D; e += 64) {
        const uint32_t j = e / D, d = e - j * D;
        uint32_t out;
        if (d >= C) {
            out = d - C;
        } else {
            const uint32_t cs = j * C, ce = cs + C;
            const uint32_t nv = next_valid_sel(VB, NZ, cs + d, ce);
            if (nv >= ce) {
                out = nv - ce;
            } else {
                out = res[j * D1 + min(nv - cs, uint32_t(D))] & ~kRoot;
            }
        }
        T[e] = uint16_t(out);
    }
    wstamp(5);
}

// Speculative pass: one lane per chunk k walks from the first bit of chunk k - W (W = a.warm
// chunks of warm-up; from the stream's first record, an exact entry, when k - W <= 0) through chunk
// k, sliding one bit past positions where no record can start, and stores where it leaves chunk k.
// A walk from an arbitrary bit meets the true record boundaries after a few records on typical
// content, long before the warm-up ends; the count pass proves it did (or flags the stream).
template <int N>
__global__ __launch_bounds__(kTPB) void rec_spec_kernel(RecParseArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t Lall[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int seg = a.seg, W = a.warm;
    const int k0 = (blockIdx.x * 4 + wv) * seg;
    const int m = max(0, min(seg, a.nchunks - k0));
    if (blockIdx.x == 0 && tid == 0) *a.fail = 0u;  // (the count pass runs after this launch)
    if (m == 0) return;
    const int kw = max(k0 - W, 0);  // the wave's first staged chunk
    uint32_t* L = Lall + size_t(wv) * rec_count_wave_words(a.C, seg + W);
    const RecSpan sp = rec_span(a);
    const uint64_t c0 = sp.start + uint64_t(kw) * a.C;
    const uint64_t base = c0 & ~31ull;
    const int off = stage_words16(L, a.words, base >> 5,
                                  int(((c0 - base) + uint64_t(k0 + m - kw) * a.C + 64) >> 5) + 2, sp.nbits, lane);
    const uint32_t s0 = uint32_t(c0 - base) + 32u * uint32_t(off);  // chunk kw's first bit in L
    wave_sync();
    const int k = k0 + lane;
    if (lane < m && k < a.nchunks - 1) {  // (the last chunk's exit enters nothing)
        const uint32_t ce = s0 + uint32_t(k + 1 - kw) * a.C;
        uint32_t p = s0 + uint32_t(max(k - W, 0) - kw) * a.C;
        while (p < ce) p += rec_len_head<N>(lbits(L, p, 20), a.rle);
        a.spec[k] = p - ce;
    }
}

// Count pass: each wave stages `seg` consecutive chunks' bits in LDS and one lane per chunk walks
// its true records from its entry (the prefix maps applied to its top-level entry), storing up to
// kRecPosCap record positions (relative to the chunk's first word) and the count; the workgroup
// then scans its 4 * seg chunks' counts (records before each chunk among them, and their total).
template <int N, bool B = false>
__global__ __launch_bounds__(kTPB) void rec_count_kernel(RecParseArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t Lall[];
    __shared__ alignas(8) uint32_t scratch[8];
    rec_image<B>(a);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int seg = a.seg;
    const int k0 = (blockIdx.x * 4 + wv) * seg;  // this wave's first chunk
    const int m = max(0, min(seg, a.nchunks - k0));
    uint32_t* L = Lall + size_t(wv) * rec_count_wave_words(a.C, seg);
    uint32_t s0 = 0;
    const RecSpan sp = rec_span(a);
    if (m > 0) {
        const uint64_t c0 = sp.start + uint64_t(k0) * a.C;
        const uint64_t base = c0 & ~31ull;
        const int off = stage_words16(L, a.words, base >> 5, int(((c0 - base) + uint64_t(m) * a.C + 64) >> 5) + 2,
                                      sp.nbits, lane);
        s0 = uint32_t(c0 - base) + 32u * uint32_t(off);  // the wave's first bit, relative to L
    }
    const int k = k0 + lane;
    const bool mine = lane < m;
    const uint32_t x = mine ? rec_chunk_entry<N, B>(a, k) : 0u;
    wave_sync();
    uint32_t R = 0;
    if (mine) {
        const uint64_t c0 = sp.start + uint64_t(k0) * a.C;  // = bit s0 of L
        const uint32_t lim = uint32_t(min<uint64_t>(sat_sub(sp.nbits, c0) + s0, uint64_t(s0) + uint64_t(m) * a.C));
        const uint32_t cs = s0 + uint32_t(lane) * a.C;
        const uint32_t cb = cs & ~31u;  // the chunk's first word
        const uint32_t ce = min(cs + a.C, lim);  // no record starts at or past the stream's end
        uint16_t* pos = a.pos + size_t(k) * kRecPosCap;
        uint32_t p = cs + x;
        while (p < ce) {
            const uint32_t l = rec_len_sel<N>(lbits(L, p, 20), a.rle);
            if (l > 1u) {
                if (R < uint32_t(kRecPosCap)) pos[R] = uint16_t(p - cb);
                R++;
            }
            p += l;
        }
        // speculative entries: this walk started at the true entry if every earlier one did; its
        // exit must be the entry the next chunk's walk took
        if (a.spec && k < a.nchunks - 1 && p - (cs + a.C) != a.spec[k]) *a.fail = 1u;
    }
    // records before each chunk within the workgroup (thread order = chunk order; idle lanes add 0)
    uint32_t tot;
    const uint32_t ex = block_excl_scan(R, scratch, &tot);
    if (mine) {
        a.cnt[k] = R;
        a.lbase[k] = ex;
    }
    if (tid == 0) a.wgsum[blockIdx.x] = tot;
}

// Decode pass: a wave decodes the records of kDecChunks consecutive chunks (about 64 records: a
// chunk holds about 32), one record per lane, so the FP64 IDCT -- the pass's cost -- runs on full
// waves.  Record positions come from the count pass (relative to each chunk's first word; chunk j
// of the wave starts j * C bits after chunk 0, C a multiple of 32).
template <int N, bool B = false>
__global__ __launch_bounds__(64 * kRecWPB) void rec_decode_kernel(RecParseArgs a, DecArgs d) {
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
    if (a.spec && *a.fail) {  // a speculative entry was wrong: nothing is written, the host re-runs
        if (k0 == 0 && lane == 0) *a.total = ~0ull;
        return;
    }
    const int m = min(P, a.nchunks - k0);
    uint32_t* L = dyn_all + size_t(wv) * rec_decode_stream_words(uint32_t(P) * a.C, D);
    const RecSpan sp = rec_span(a);
    const uint64_t c0 = sp.start + uint64_t(k0) * a.C;
    const uint64_t base = c0 & ~31ull;
    // the chunks' bits first (16-byte loads in flight while the indices below are read); bit
    // positions in L are relative to word `off` of L, which holds the first chunk's first word
    const int off = stage_words16(L, a.words, base >> 5, int((uint32_t(c0 - base) + uint32_t(m) * a.C + D + 64) >> 5) + 2,
                                  sp.nbits, lane);
    const uint32_t ob = 32u * uint32_t(off);
    const uint32_t s0 = uint32_t(c0 - base) + ob;
    const uint64_t lbase0 = base - ob;  // stream bit of L's bit 0
    // first block index: the totals of the count pass's workgroups before chunk k0's, plus the
    // records before it in its own (no separate scan launch); the next chunks follow on
    uint64_t part = 0;
    for (int g = lane; g < k0 / (4 * a.seg); g += 64) part += a.wgsum[g];
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
    wave_sync();
    const uint64_t nblocks = uint64_t(d.nframes) * d.bx * d.by;
    if (listed) {
        for (uint32_t i = lane; i < Rall; i += 64) {
            const uint64_t b = first + i;
            if (b >= nblocks) break;
            uint32_t j = 0, r = i;
#pragma unroll
            for (int jj = 0; jj < P - 1; jj++)
                if (j == uint32_t(jj) && r >= R[jj]) {
                    r -= R[jj];
                    j++;
                }
            const uint32_t q = decode_record<N>(L, ob + j * a.C + a.pos[size_t(k0 + j) * kRecPosCap + r], b, d, sR, sq);
            if (b == nblocks - 1) *a.end_out = lbase0 + q;
        }
        return;
    }
    // a chunk with more records than its position list holds: walk the chunks again, 64 records
    // at a time
    uint64_t gi = first;
    for (int j = 0; j < m; j++) {
        uint32_t p = s0 + uint32_t(j) * a.C + rec_chunk_entry<N, B>(a, k0 + j);
        const uint32_t wend = uint32_t(min<uint64_t>(s0 + uint64_t(j + 1) * a.C, sat_sub(sp.nbits, lbase0)));
        while (p < wend && gi < nblocks) {
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
            const uint64_t b = gi + lane;
            if (uint32_t(lane) < n && b < nblocks) {
                const uint32_t q = decode_record<N>(L, mine, b, d, sR, sq);
                if (b == nblocks - 1) *a.end_out = lbase0 + q;
            }
            gi += n;
        }
    }
}

int rec_group_chunks(int n) { return n == 4 ? RecGeom<4>::G : RecGeom<8>::G; }
int rec_entry_span(int n) { return n == 4 ? RecGeom<4>::D : RecGeom<8>::D; }
size_t rec_table_rows(size_t nchunks, int n, int* levels) {
    return n == 4 ? compose_rows<RecGeom<4>::D, RecGeom<4>::G>(nchunks, levels)
                  : compose_rows<RecGeom<8>::D, RecGeom<8>::G>(nchunks, levels);
}
// chunks per table wave and claim slots: tm chunks' positions fit the 16-bit claim keys.  The
// claim table is small on purpose (lossy, direct-mapped): measured on 4K streams, the occupancy a
// small LDS footprint buys beats the merges a larger table finds (IE_REC_TM / IE_REC_HB override)
void rec_table_geometry(uint32_t C, int n, int* tm, int* hbits) {
    static const char* et = getenv("IE_REC_TM");
    static const char* eh = getenv("IE_REC_HB");
    int t = et ? atoi(et) : (n == 4 ? 2 : 1);
    while (t > 1 && uint64_t(t) * C > 65535u) t--;
    t = std::max(1, t);
    int hb = eh ? atoi(eh) : ((n == 4 ? 7 : 9) + (t >= 4 ? 2 : t >= 2 ? 1 : 0));
    *tm = t;
    *hbits = std::min(14, std::max(6, hb));
}
size_t rec_decode_lds(uint32_t C, int n) {
    return size_t(rec_decode_stream_words(uint32_t(kDecChunks) * C, rec_entry_span(n))) * 4 * kRecWPB;
}

// The parse passes (tables, composition, counts); B: over `images` independent streams, the image as
// every grid's y dimension.  Fills a.tm, a.hbits and a.levels for the decode pass that follows.
template <int N, bool B>
int launch_rec_parse_t(RecParseArgs& a, int images, hipStream_t s) {
    rec_table_geometry(a.C, N, &a.tm, &a.hbits);
    const int nt2 = (a.nchunks + a.tm - 1) / a.tm;
    const size_t l2 = size_t(rec_table2_words(a.C, RecGeom<N>::D, a.tm, a.hbits)) * 4;
    hipLaunchKernelGGL((rec_table2_kernel<N, B>), dim3(nt2, images), dim3(64), l2, s, a);
    const int levels = launch_compose<RecGeom<N>::D, RecGeom<N>::G, B>(a.tab, a.nchunks, a.E, a.lvl, s, images, a.img_tab,
                                                                       a.img_E);
    if (levels < 0) return -1;
    a.levels = levels;
    const int nbc = (a.nchunks + 4 * a.seg - 1) / (4 * a.seg);
    const size_t lc = size_t(rec_count_wave_words(a.C, a.seg)) * 4 * 4;
    hipLaunchKernelGGL((rec_count_kernel<N, B>), dim3(nbc, images), dim3(kTPB), lc, s, a);
    return levels;
}
int launch_rec_parse(RecParseArgs& a, int n, int images, bool batch, hipStream_t s) {
    if (!batch) return n == 4 ? launch_rec_parse_t<4, false>(a, 1, s) : launch_rec_parse_t<8, false>(a, 1, s);
    return n == 4 ? launch_rec_parse_t<4, true>(a, images, s) : launch_rec_parse_t<8, true>(a, images, s);
}

// The five passes: the parse, then the decode.
template <int N, bool B>
int launch_rec_parse_decode_t(RecParseArgs a, const DecArgs& d, int images, hipStream_t s) {
    if (a.nchunks <= 0) return 0;
    const int nb = (a.nchunks + kRecWPB * kDecChunks - 1) / (kRecWPB * kDecChunks);  // decode blocks
    const int levels = launch_rec_parse_t<N, B>(a, images, s);
    if (levels < 0) return -1;
    hipLaunchKernelGGL((rec_decode_kernel<N, B>), dim3(nb, images), dim3(64 * kRecWPB), rec_decode_lds(a.C, N), s, a, d);
    return levels;
}

int launch_rec_parse_decode(RecParseArgs a, const DecArgs& d, int n, hipStream_t s) {
    return n == 4 ? launch_rec_parse_decode_t<4, false>(a, d, 1, s) : launch_rec_parse_decode_t<8, false>(a, d, 1, s);
}
int launch_rec_parse_decode_images(RecParseArgs a, const DecArgs& d, int n, int images, hipStream_t s) {
    return n == 4 ? launch_rec_parse_decode_t<4, true>(a, d, images, s) : launch_rec_parse_decode_t<8, true>(a, d, images, s);
}

__global__ void gop_init_kernel(uint64_t* pos, uint64_t* tot, int n, uint64_t start) {
    for (int i = threadIdx.x; i <= n; i += blockDim.x) {
        pos[i] = i ? ~0ull : start;
        if (i < n) tot[i] = 0;
    }
}
void launch_gop_init(uint64_t* pos, uint64_t* tot, int n, uint64_t start, hipStream_t s) {
    hipLaunchKernelGGL(gop_init_kernel, dim3(1), dim3(256), 0, s, pos, tot, n, start);
}

// Chain continuation (ie_vdec): the arrays of a chunk of frames whose first bit is the end bit an
// earlier chunk's last decode wrote -- read here, on the device, so no host round trip separates
// two chunks.  ~0 (that chunk found no end: a truncated stream) is passed on: the span of every
// launch that starts there is empty (rec_span).
__global__ void gop_cont_kernel(uint64_t* pos, uint64_t* tot, int n, const uint64_t* prev_end) {
    const uint64_t start = *prev_end;
    for (int i = threadIdx.x; i <= n; i += blockDim.x) {
        pos[i] = i ? ~0ull : start;
        if (i < n) tot[i] = 0;
    }
}
void launch_gop_continue(uint64_t* pos, uint64_t* tot, int n, const uint64_t* prev_end, hipStream_t s) {
    hipLaunchKernelGGL(gop_cont_kernel, dim3(1), dim3(256), 0, s, pos, tot, n, prev_end);
}

void launch_rec_spec_decode(const RecParseArgs& a, const DecArgs& d, int n, hipStream_t s) {
    if (a.nchunks <= 0) return;
    const int nb = (a.nchunks + kRecWPB * kDecChunks - 1) / (kRecWPB * kDecChunks);
    const int nbc = (a.nchunks + 4 * a.seg - 1) / (4 * a.seg);
    const size_t lc = size_t(rec_count_wave_words(a.C, a.seg)) * 4 * 4;
    const size_t lw = size_t(rec_count_wave_words(a.C, a.seg + a.warm)) * 4 * 4;
    if (n == 4) {
        hipLaunchKernelGGL((rec_spec_kernel<4>), dim3(nbc), dim3(kTPB), lw, s, a);
        hipLaunchKernelGGL((rec_count_kernel<4>), dim3(nbc), dim3(kTPB), lc, s, a);
        hipLaunchKernelGGL((rec_decode_kernel<4>), dim3(nb), dim3(64 * kRecWPB), rec_decode_lds(a.C, 4), s, a, d);
    } else {
        hipLaunchKernelGGL((rec_spec_kernel<8>), dim3(nbc), dim3(kTPB), lw, s, a);
        hipLaunchKernelGGL((rec_count_kernel<8>), dim3(nbc), dim3(kTPB), lc, s, a);
        hipLaunchKernelGGL((rec_decode_kernel<8>), dim3(nb), dim3(64 * kRecWPB), rec_decode_lds(a.C, 8), s, a, d);
    }
}

}  // namespace ie
