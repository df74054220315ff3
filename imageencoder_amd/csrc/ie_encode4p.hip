// imageencoder_amd/csrc/ie_encode4p.hip -- encode4p_kernel, the wave-local 4x4 FAST encoder for
// gfx950 (MI355X), and its launcher; the design is described above the kernel.
#include "ie_encode_blocks.h"

namespace ie {

// Look-back windows after the first probe, for launches that fill the chip (one small window at a
// time: the nearest inclusive prefix is seldom far, and each probed predecessor is an uncached
// load -- C4's one 8 128-tile chain: 2 windows of 64 108.6 us, 1 of 64 102.4, 1 of 32 101.1, 1 of
// 16 104.4 us per 64-frame launch; C2 and one 4K frame unchanged; tools/ab.py, round 6)
#ifndef IE_W_AHEAD
#define IE_W_AHEAD 1  // windows per round trip (each holds 4 VGPRs live beside slots 2-3)
#endif
#ifndef IE_W_LBW
#define IE_W_LBW 32  // predecessors per window
#endif
constexpr int kWTask = 128;  // words per wave: fix-up tasks [64] + results [64]
// FP64 rows in LDS (doubles): P[16][16] then S, rq, qd of every coefficient (the structural
// three alone measured equal: the LDS they would free does not add a tile per CU at 78 VGPRs)
constexpr int kWRows = 16 * 16 + 3 * 16;
// HIST: copies of the byte histogram (tools/ab.py --op counted, 16 4K frames: counting costs 20.3 us
// over a launch without it at 1 copy, 15.8 at 4; 8 and 16 copies cost a tile per CU and are slower,
// two 16-bit bins per word slower still -- the LDS read-modify-write of 112 M byte-adds is the floor)
constexpr int kWHistRep = 4;

// Inclusive scan over the 64 lanes of a wave by DPP row shifts and row broadcasts (six VALU).
__device__ __forceinline__ uint32_t wave_incl_scan_dpp(uint32_t v) {
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x111, 0xF, 0xF, true));   // row_shr:1
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x112, 0xF, 0xF, true));   // row_shr:2
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x114, 0xF, 0xF, true));   // row_shr:4
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x118, 0xF, 0xF, true));   // row_shr:8
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x142, 0xA, 0xF, false));  // row_bcast:15
    v += uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x143, 0xC, 0xF, false));  // row_bcast:31
    return v;
}

// One slot image I (bit 0 at absolute stream bit X) to the output words, by one wave: words
// [r0, nw) counted from floor(X / 32), word r = alignbit(I[r - 1], I[r], X % 32) with I[-1] =
// prev (the 32 bits before X); the partial word nw is left to whoever writes the next bits.
template <typename Cnt = NoCount>
__device__ __forceinline__ void store_slot(uint32_t* __restrict__ out, const uint32_t* I, uint64_t X, uint32_t nw,
                                           uint32_t r0, uint32_t prev, int lane, const Cnt& cnt = Cnt{}) {
    if (nw <= r0) return;
    const uint64_t w0 = X >> 5;
    const uint32_t s = uint32_t(X) & 31u;
    auto word = [&](uint32_t r) -> uint32_t {
        const uint32_t am = I[max(r, 1u) - 1u];
        return bswap32(__builtin_amdgcn_alignbit(r ? am : prev, I[r], s));
    };
    uint32_t hd = min(nw - r0, uint32_t((4u - uint32_t((w0 + r0) & 3u)) & 3u));
    if (r0 + hd == 0u) hd = min(nw, 4u);  // (the quad loop needs I[r - 1]: word -1 is prev)
    if (uint32_t(lane) < hd) {
        const uint32_t v = word(r0 + lane);
        out[w0 + r0 + lane] = v;
        cnt(w0 + r0 + lane, v);
    }
    const uint32_t rq = r0 + hd, nq = (nw - rq) >> 2;
    // output quad q = words rq + 4q .. +3 (16-byte aligned in out) needs I[rq + 4q - 1 ..
    // rq + 4q + 3]: five words at offset d of the two 16-byte LDS quads from (rq - 1) / 4 + q,
    // read whole (consecutive lanes, consecutive quads: no bank conflicts), d wave-uniform
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const uint32_t d = (rq - 1u) & 3u;
    const v4u* I4 = reinterpret_cast<const v4u*>(I) + ((rq - 1u) >> 2);
    uint32_t* const ob = out + (w0 + rq);
    auto quads = [&](auto dc) {
        constexpr uint32_t D = decltype(dc)::value;
        for (uint32_t q = lane; q < nq; q += 64) {
            const v4u A = I4[q], B = I4[q + 1];
            const uint32_t W[8] = {A.x, A.y, A.z, A.w, B.x, B.y, B.z, B.w};
            const v4u v = {bswap32(__builtin_amdgcn_alignbit(W[D], W[D + 1], s)), bswap32(__builtin_amdgcn_alignbit(W[D + 1], W[D + 2], s)),
                           bswap32(__builtin_amdgcn_alignbit(W[D + 2], W[D + 3], s)), bswap32(__builtin_amdgcn_alignbit(W[D + 3], W[D + 4], s))};
            __builtin_nontemporal_store(v, reinterpret_cast<v4u*>(ob + 4u * q));
            cnt(w0 + rq + 4u * q, v.x);
            cnt(w0 + rq + 4u * q + 1u, v.y);
            cnt(w0 + rq + 4u * q + 2u, v.z);
            cnt(w0 + rq + 4u * q + 3u, v.w);
        }
    };
    if (d == 0u) quads(std::integral_constant<uint32_t, 0>{});
    else if (d == 1u) quads(std::integral_constant<uint32_t, 1>{});
    else if (d == 2u) quads(std::integral_constant<uint32_t, 2>{});
    else quads(std::integral_constant<uint32_t, 3>{});

    const uint32_t rt = rq + 4u * nq;
    if (uint32_t(lane) < nw - rt) {
        const uint32_t v = word(rt + lane);
        out[w0 + rt + lane] = v;
        cnt(w0 + rt + lane, v);
    }
}

// The last 32 bits of the stream up to the end of a slot image of n bits, given the 32 bits
// before it (prev).
__device__ __forceinline__ uint32_t slot_tail32(const uint32_t* I, uint32_t n, uint32_t prev) {
    if (n >= 32) return image_tail32(I, n);
    return n ? ((prev << n) | (I[0] >> (32u - n))) : prev;
}

// profiling builds (IE_PROFILE, IE_STAMPS set): lane 0 of each wave stamps s_memtime at its phase
// boundaries, [tile][wave][12] (tools/stamps_w.py)
#define WSTAMP(i)                                                                                                   \
    do {                                                                                                            \
        if (IE_PROFILE && a.stamps && lane == 0 && wv < 4) a.stamps[size_t(t) * kStamps + wv * 16 + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
// the chip-wide 100 MHz clock (comparable across CUs and XCDs) at the wave's start (14) and end (15)
#define WRTSTAMP(i)                                                                                                 \
    do {                                                                                                            \
        if (IE_PROFILE && a.stamps && lane == 0 && wv < 4) a.stamps[size_t(t) * kStamps + wv * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)

// =============================================================================================
// encode4p_kernel<HIST, TICKET> -- the 4x4 FAST encoder with WAVE-LOCAL emission and the integer
// half of the transform on the matrix pipe.
//
// Same tile (1024 blocks, 256 threads, one chain element, the same chain granules) and the same
// FP64 fix-up as encode_kernel<4, false> (the Trk exactness argument carries over with quot4j's own
// limits), laid out so that a wave rarely needs its workgroup:
//   * wave w owns the tile's blocks [256w, 256w + 256) (64 groups of four, raster order); lane l
//     computes block 64b + l of that run in SLOT b = 0..3, so a slot is 64 consecutive blocks of
//     the stream and one wave scan (DPP) places every record inside its slot;
//   * the pixels land in the wave's own LDS region by DMA as [row][256 blocks] words (a slot
//     reads them conflict-free, no other wave touches them); after the fix-up the same region
//     holds the wave's slot images (all four at once when they fit, slot pairs in turn otherwise);
//   * a word shared by two waves of the tile is written by the earlier wave, which ORs in the
//     later wave's first bits (its head word, saved in LDS before the position barrier); a word
//     shared with the predecessor tile is completed with that tile's tail granule as in
//     encode_kernel.
// Preconditions (launch_encode checks them): whole 16-byte groups (vec_ok, bx % 4 == 0), at
// least 8 groups in every tile (groups_per_frame % 8 == 0: every wave segment >= 160 bits) and
// slot images that fit half a region (rec_bits <= 252).
// HIST (ie_encode_images_counted): every stored byte also counted into a per-tile LDS histogram
// (kWHistRep copies of 256 words), merged into a.hist[frame] at the end -- the Huffman pass's byte
// counts without reading the stream back.
// One workgroup per tile.  TICKET = false: tile = blockIdx.x, the tiles in dispatch order.
// TICKET = true (the host's redo after a look-back timeout, IE_FORCE_TICKET): tile = an atomic
// ticket, so tile order is start order whatever the dispatcher does.  Every wait in the kernel is
// either on the waves of the tile's own workgroup (the count flags, the barriers) or on chain
// predecessors t - step (d + 1) -- the first probe and lookback_wave's windows, the deep windows
// of all four waves, wait_tail(t - step) --, which hold lower tickets and have therefore started
// and wait only on still lower ones: ticket order cannot deadlock.
//   * Matrix pipe: per slot (64 blocks of one wave), ONE v_mfma_i32_32x32x32_i8 forms the sixteen
//     integer basis sums J of every block (ie_dct.h quot4j: pixels as signed bytes x ^ 0x80, the
//     {-1,0,1} A fragment from EncTables::mfma_w), which replaces the 16 pixel unpacks and the
//     integer butterflies on the VALU; the FP32 stage (36 mul/fma) and the rounding follow, with
//     the tie limits of quot4j's own tracked run (lim4j).
//   * Count by polling: each wave stores its bit count and a flag; wave 0 alone waits for the
//     four flags, publishes the tile aggregate and issues its look-back probe, while waves 1-3 go
//     straight on to their emission.  One workgroup barrier per tile (the position).
//   * Whole-wave images: when a wave's image fits its 4 KB region, all four slots are emitted
//     before the position barrier, beside wave 0's look-back; slot pairs in turn otherwise.
// Measured and not kept: a persistent grid walking the tiles -- by per-chain claim
// atomics (126.7 against 93.5 us) or in static order g, g + G, ... (110.3 against 88.4 us: a tile
// whose chain predecessor sits in a slower workgroup waits for it, where the dispatcher starts
// tiles in chain order as slots free) --, a software-pipelined persistent variant with two buffers
// per wave (126.7 against 93.6 us: four tiles per CU instead of six), an L2 prefetch of the tile
// about d dispatches later (neutral at d = 256-1024 on HBM-resident frames).
// =============================================================================================
constexpr int kPWfrag = 256;  // the matrix-pipe A fragments [64 lanes][4 words]
// encode4p_kernel's misc words: [0, 4) wave bit counts, H the waves' head words, E the tile's
// exclusive prefix (2), PT the tail before the chain start, PD the pending first word, TK the
// tile's ticket (TICKET), F the count flags, D the deep look-back sums (2 per wave), FD their
// found flags
struct PMisc {
    static constexpr int H = 4, E = 8, PT = 10, PD = 11, TK = 12, F = 16, D = 20, FD = 28, S = 32;
    static_assert(FD + 4 <= S && F % 4 == 0, "misc layout");
};
constexpr int p_lds_bytes() { return (4 * 4 * 256 + 4 * kWTask + PMisc::S + kPWfrag) * 4 + kWRows * 8; }

typedef int v4i32 __attribute__((ext_vector_type(4)));
typedef int v16i32 __attribute__((ext_vector_type(16)));

// round_block<4> with the limits passed in (quot4j's own), the rounding done pair by pair in
// zig-zag order and each packed word pinned as soon as it exists: the 16 magic-added quotients
// never live at once (register pressure of the fourth slot).  Same results bit for bit.
__device__ __forceinline__ float round_block_lean4j(const float (&t)[16], uint32_t (&zp)[8], uint32_t* sflags, bool dcx,
                                                    float l0, float l1, float l2) {
    constexpr int S0 = Structural<4>::k[0], S1 = Structural<4>::k[1], S2 = Structural<4>::k[2];
    float emax = 0.0f;
    uint32_t sf = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        uint32_t yb[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int k = ZigZag<4>::idx[2 * j + h];
            const float y = t[k] + kMagic;
            const float e = fabsf(t[k] - (y - kMagic));
            yb[h] = __float_as_uint(y);
            if (k == 0) {
                const uint32_t dc = uint32_t(int(truncf(t[0] + copysignf(0.5f, t[0]))));
                yb[h] = dcx ? dc : yb[h];
                emax = dcx ? emax : fmaxf(emax, e);
            } else if (k == S0) {
                sf |= (e >= l0) ? 1u : 0u;
            } else if (k == S1) {
                sf |= (e >= l1) ? 2u : 0u;
            } else if (k == S2) {
                sf |= (e >= l2) ? 4u : 0u;
            } else {
                emax = fmaxf(emax, e);
            }
        }
        zp[j] = __builtin_amdgcn_perm(yb[1], yb[0], 0x05040100u);
        asm volatile("" : "+v"(zp[j]));
    }
    *sflags = sf;
    return emax;
}

#ifndef IE_P_PXAUX
#define IE_P_PXAUX 2  // cache-policy bits of encode4p's pixel DMA: nt (pixels are read once; HBM-resident
                      // frames 98.2 against 101.1 us per 16-frame launch, MALL-resident 97.9 against 92.8)
#endif
#ifndef IE_P_WAVES
#define IE_P_WAVES 6  // __launch_bounds__ occupancy hint (waves per SIMD)
#endif
#ifndef IE_P_WAVES_HIST
#define IE_P_WAVES_HIST 6  // the counting instantiation (5: 89 VGPRs; measured 124.7 against 119.4 us)
#endif
#ifndef IE_P_ABL
#define IE_P_ABL 0  // (profiling builds) phases left out: 1 FP64 fix-up, 2 emission, 4 look-back, 8 store, 16 transform
#endif

template <bool HIST, bool TICKET>
__global__ __launch_bounds__(256, HIST ? IE_P_WAVES_HIST : IE_P_WAVES) void encode4p_kernel(EncArgs a_, const EncTables* __restrict__ tab) {
    constexpr int N = 4, NN = 16, NP = 8, NS = 4, PS = 2;  // slots per lane, slots per pair
    constexpr int GW = 64, BW = 256, TG = 256;  // groups / blocks per wave, groups per tile
    constexpr int RW = 4 * BW;  // words per wave region
    using ML = PMisc;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int wv = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
    uint32_t* const reg = smem + wv * RW;  // this wave's pixels, later its slot images
    uint32_t* const task = smem + 4 * RW + wv * kWTask;
    uint32_t* const res = task + 64;
    uint32_t* const misc = smem + 4 * RW + 4 * kWTask;  // [ML::S]
    uint32_t* const wl = misc + ML::S;  // [64][4]: the matrix-pipe A fragment of every lane
    uint32_t* const hl = wl + kPWfrag;  // HIST: the tile's byte histogram
    constexpr int HR = kWHistRep, HWORDS = 256 * HR;
    double* const srow = reinterpret_cast<double*>(hl + (HIST ? HWORDS : 0));
    int t = int(blockIdx.x);
    if constexpr (TICKET) {  // tiles in ticket order; t wave-uniform, in a scalar register
        if (threadIdx.x == 0) misc[ML::TK] = uint32_t(atomicAdd(a_.ticket, 1ull) - a_.ticket_base);
        lds_barrier();
        t = __builtin_amdgcn_readfirstlane(int(misc[ML::TK]));
    }
    // The launch arguments are read through a pointer to the kernel-argument segment (constant
    // address space): the geometry words in one scalar round trip (load_geo), the rest where used.
    using KArgs = const __attribute__((address_space(4))) EncArgs;
    KArgs* ka = (KArgs*)(__builtin_amdgcn_kernarg_segment_ptr());
    const GeoArgs ga = load_geo(ka);
    if (t >= ga.ntiles) return;  // (a ticket desync after a failed launch: never touch memory)
    // The lane id is re-derived at every phase (fresh_lane): a lane-derived VGPR held across the
    // whole tile was spilled at higher occupancy.
    int lane = fresh_lane();
    // (profiling: the workgroup's entry on the chip-wide clock, wave 0's word 13)
    if (IE_PROFILE && a_.stamps && lane == 0) a_.stamps[size_t(t) * kStamps + wv * 16 + 13] = __builtin_amdgcn_s_memrealtime();
    const TileGeo g = tile_geo<4, 4, TG>(ga, t, GW * wv + lane);
    // the wave's pixel rows into its own region (row r of the wave's block j at reg[r BW + j]: a
    // lane's 16 bytes are its group's row)
    if (g.nblk) {
        const uint8_t* base = ga.y + size_t(g.frame) * ga.frame_pitch + size_t(g.byi) * N * ga.stride + size_t(g.bx0) * N;
#pragma unroll
        for (int r = 0; r < N; r++)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + size_t(r) * ga.stride),
                                             (__attribute__((address_space(3))) void*)(reg + r * BW), 16, 0, IE_P_PXAUX);
    }
    if (IE_PROFILE == 2 && a_.stamps && lane == 0) a_.stamps[size_t(t) * kStamps + wv * 16 + 1] = __builtin_amdgcn_s_memrealtime();
    // the FP64 rows (waves 0-2: 2432 bytes) and the matrix-pipe A fragments (wave 3; read back per
    // slot) by DMA too: no register round trip, one wait for everything
    {
        static_assert(kWRows * 8 == 2 * 1024 + 24 * 16, "rows: two full waves and 24 lanes of 16 bytes");
        if (wv < 2 || (wv == 2 && lane < 24))
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(&tab->rows4[wv * 128 + 2 * lane]),
                                             (__attribute__((address_space(3))) void*)(srow + wv * 128), 16, 0, 0);
        else if (wv == 3)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(&tab->mfma_w[lane][0]),
                                             (__attribute__((address_space(3))) void*)(wl), 16, 0, 0);
    }
    if constexpr (HIST)
        for (int i = 64 * wv + lane; i < HWORDS; i += 256) hl[i] = 0u;
    if (lane == 0) misc[ML::F + wv] = 0u;  // the waves' count flags
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the DMA above and this wave's pixels)
    if (IE_PROFILE && a_.stamps && lane == 0) a_.stamps[size_t(t) * kStamps + wv * 16 + 12] = __builtin_amdgcn_s_memrealtime();
    const uint64_t start_bit = a_.start_dev ? *a_.start_dev : a_.start_bit;
    const bool deep = a_.deep_lb != 0;
    lds_barrier();  // every wave's pixels, the rows, the A fragments (and the HIST bins) visible
    if (IE_PROFILE && a_.stamps && lane == 0) a_.stamps[size_t(t) * kStamps + wv * 16 + 11] = __builtin_amdgcn_s_memrealtime();
    KArgs& a = *ka;
    // (the tile's geometry is uniform: held in SGPRs, not in VGPRs the compiler would keep -- and
    // spill -- across the tile)
    const int frame = __builtin_amdgcn_readfirstlane(g.frame), tif = __builtin_amdgcn_readfirstlane(g.tif),
              step = __builtin_amdgcn_readfirstlane(g.step), chain_pos = __builtin_amdgcn_readfirstlane(g.chain_pos);
    const int ng = min(TG, ga.groups_per_frame - tif * TG);
    const int nbw = __builtin_amdgcn_readfirstlane(4 * min(GW, max(0, ng - GW * wv)));  // blocks of this wave
    const int wlast = (ng - 1) / GW;                    // the tile's last non-empty wave
    WSTAMP(0);
    WRTSTAMP(14);
    if (IE_PROFILE != 2) WSTAMP(1);
    asm volatile("; PHASE p1" ::: "memory");

    // ------------------------------------------------------------ transform + quantise, 4 slots
    using KTab = const __attribute__((address_space(4))) EncTables;
    KTab* tb = (KTab*)(tab);  // constant address space: scalar loads
    const bool dcx = tb->dc_exact4j != 0;
    const float lim_s0 = tb->lim4j[Structural<4>::k[0]], lim_s1 = tb->lim4j[Structural<4>::k[1]],
                lim_s2 = tb->lim4j[Structural<4>::k[2]], lim_min = tb->lim_min4j;
    uint32_t zp[NS][NP];
    uint32_t flags = 0;  // 4 bits per slot: structural s (bits 0-2), whole block (bit 3)
#pragma unroll
    for (int b = 0; b < NS; b++) {
        __builtin_amdgcn_sched_barrier(0);
        uint32_t sf;
        float emax;
        if (IE_P_ABL & 16) {  // (profiling) no transform: quotients = pixels / 64
            float x[NN];
#pragma unroll
            for (int k = 0; k < NN; k++) x[k] = float((reg[(k >> 2) * BW + 64 * b + lane] >> (8 * (k & 3))) & 0xFFu) * 0.015625f;
            emax = round_block_lean4j(x, zp[b], &sf, dcx, lim_s0, lim_s1, lim_s2);
        } else {
            v4i32 px;
#pragma unroll
            for (int r = 0; r < N; r++) px[r] = int(reg[r * BW + 64 * b + lane] ^ 0x80808080u);  // x - 128 as i8
            const v4i32 wfrag = *reinterpret_cast<const v4i32*>(wl + 4 * lane);
            const v16i32 Jc = __builtin_amdgcn_mfma_i32_32x32x32_i8(wfrag, px, v16i32{}, 0, 0, 0);
            float Jf[16], x[16];
#pragma unroll
            for (int k = 0; k < 16; k++) Jf[k] = float(Jc[k]);
            quot4j(Jf, x, tb->plan4j, FloatOp());
            emax = round_block_lean4j(x, zp[b], &sf, dcx, lim_s0, lim_s1, lim_s2);
        }
        const uint32_t fb = (emax >= lim_min) ? 8u : sf;
        if (64 * b + lane < nbw) flags |= fb << (4 * b);
#pragma unroll
        for (int j = 0; j < NP; j++) asm volatile("" : "+v"(zp[b][j]));
        asm volatile("" : "+v"(flags));
    }
    WSTAMP(2);
    asm volatile("; PHASE p2" ::: "memory");

    // ------------------------------------------------------------ FP64 fix-up
    lane = fresh_lane();
    auto block_px = [&](int b, int owner) {
        BlockPx<N> px;
#pragma unroll
        for (int r = 0; r < N; r++) px.w[r] = reg[r * BW + 64 * b + owner];
        return px;
    };
    uint32_t wave_req = 0;  // statistics: FP64 requests of this wave
    if (!(IE_P_ABL & 1) && __ballot(flags != 0)) {
        const uint32_t sf = flags & 0x7777u;
        const uint32_t cnt = __popc(sf);
        // the lanes' request counts placed by one DPP wave scan
        const uint32_t incl = wave_incl_scan_dpp(cnt);
        const uint32_t pre = incl - cnt;
        const uint32_t total = __builtin_amdgcn_readlane(incl, 63);
        wave_req = total;
        auto task_y = [&](uint32_t tk) -> uint32_t {  // one structural coefficient in FP64
            const int s = int(tk & 3u), b = int((tk >> 2) & 3u), owner = int(tk >> 4);
            const BlockPx<N> px = block_px(b, owner);
            const int k = Structural<N>::k[0] * (s == 0) + Structural<N>::k[1] * (s == 1) + Structural<N>::k[2] * (s == 2);
            const int y = (IE_P_ABL & 32) ? int(px.w[0] & 1u)  // (profiling) no FP64 arithmetic (a small value: records stay in bound)
                                          : exact_coef_row<N>(srow + k * NN, srow[NN * NN + k], srow[NN * NN + NN + k],
                                                              srow[NN * NN + 2 * NN + k], px);
            return uint32_t(y) & 0xFFFFu;
        };
        static_assert(Structural<4>::zpos(0) & Structural<4>::zpos(1) & Structural<4>::zpos(2) & 1,
                      "4x4 structural coefficients sit in high halves");
        constexpr int z0 = Structural<N>::zpos(0) >> 1, z1 = Structural<N>::zpos(1) >> 1, z2 = Structural<N>::zpos(2) >> 1;
        static_assert(z0 != z1 && z1 != z2 && z0 != z2, "one structural coefficient per packed word");
        if (total <= 64u) {
            // One round (all but the densest waves), straight-line: every request has a task slot,
            // so nothing is range-checked, and the owners read their results back slot by slot --
            // a lane's requests of one slot are consecutive in res, so three unconditional reads
            // per slot, six in flight at once, replace one dependent LDS round trip per flagged
            // position.  (A read past a lane's last request, at most res[65], stays inside the
            // task area or the words behind it and is not selected.)
            if (sf) {
                uint32_t m = sf, i = pre;
                do {
                    task[i++] = (uint32_t(lane) << 4) | uint32_t(__ffs(m) - 1);
                    m &= m - 1;
                } while (m);
            }
            wave_sync();
            if (uint32_t(lane) < total) res[lane] = task_y(task[lane]);
            wave_sync();
            uint32_t i = pre;
#pragma unroll
            for (int h = 0; h < NS; h += 2) {
                uint32_t q[2][3];
#pragma unroll
                for (int d = 0; d < 2; d++) {
#pragma unroll
                    for (int ss = 0; ss < 3; ss++) q[d][ss] = res[i + ss];
                    i += __popc(sf & (7u << (4 * (h + d))));
                }
#pragma unroll
                for (int d = 0; d < 2; d++)
#pragma unroll
                    for (int ss = 0; ss < 3; ss++) asm volatile("" : "+v"(q[d][ss]));  // (all six reads issued before the first use)
#pragma unroll
                for (int d = 0; d < 2; d++) {
                    const int b = h + d;
                    const bool f0 = (sf >> (4 * b)) & 1u, f1 = (sf >> (4 * b + 1)) & 1u, f2 = (sf >> (4 * b + 2)) & 1u;
                    const uint32_t v1 = f0 ? q[d][1] : q[d][0];
                    const uint32_t v2 = f1 ? (f0 ? q[d][2] : q[d][1]) : v1;
                    if (f0) zp[b][z0] = __builtin_amdgcn_perm(q[d][0], zp[b][z0], 0x05040100u);  // res low -> high half
                    if (f1) zp[b][z1] = __builtin_amdgcn_perm(v1, zp[b][z1], 0x05040100u);
                    if (f2) zp[b][z2] = __builtin_amdgcn_perm(v2, zp[b][z2], 0x05040100u);
                }
            }
            wave_sync();
        } else {
            // more than 64 requests (dense structural ties): rounds of 64, range-checked
            for (uint32_t r0 = 0; r0 < total; r0 += 64) {
                uint32_t m = sf, i = pre - r0;
                while (m) {
                    const int bit = __ffs(m) - 1;
                    m &= m - 1;
                    if (i < 64u) task[i] = (uint32_t(lane) << 4) | uint32_t(bit);
                    i++;
                }
                wave_sync();
                if (uint32_t(lane) < total - r0) res[lane] = task_y(task[lane]);
                wave_sync();
                // the owners take their results back: the flagged positions in bit order, each a
                // constant register (the three structural coefficients are high halves of packed
                // words), so no per-request select over every slot and coefficient
                i = pre - r0;
#pragma unroll
                for (int b = 0; b < NS; b++)
#pragma unroll
                    for (int ss = 0; ss < 3; ss++) {
                        if ((sf >> (4 * b + ss)) & 1u) {
                            const int zw = Structural<N>::zpos(ss) >> 1;
                            if (i < 64u) zp[b][zw] = __builtin_amdgcn_perm(res[i], zp[b][zw], 0x05040100u);  // res low -> high half
                            i++;
                        }
                    }
                wave_sync();
            }
        }
        // whole-block requests (rare): all 16 coefficients in FP64, one per lane, four blocks a round
        const uint32_t wf = flags & 0x8888u;
        if (__ballot(wf != 0)) {
            const uint32_t nb = __popc(wf);
            uint32_t pb = 0, tb = 0;
#pragma unroll
            for (int k = 0; k < 3; k++) {  // nb <= 4
                const uint64_t bm = __ballot((nb >> k) & 1u);
                pb += __builtin_amdgcn_mbcnt_hi(uint32_t(bm >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(bm), 0u)) << k;
                tb += uint32_t(__popcll(bm)) << k;
            }
            wave_req += tb;
            for (uint32_t r0 = 0; r0 < tb; r0 += 4) {
                uint32_t m = wf, j = pb - r0;
                while (m) {
                    const int b = (__ffs(m) - 1) >> 2;
                    m &= m - 1;
                    if (j < 4u) task[j] = (uint32_t(lane) << 4) | uint32_t(b);
                    j++;
                }
                wave_sync();
                if (uint32_t(lane >> 4) < tb - r0) {
                    const uint32_t tk = task[lane >> 4];
                    const int b = int(tk & 3u), owner = int(tk >> 4), k = lane & 15;
                    const BlockPx<N> px = block_px(b, owner);
                    const int y = exact_coef_row<N>(srow + k * NN, srow[NN * NN + k], srow[NN * NN + NN + k],
                                                    srow[NN * NN + 2 * NN + k], px);
                    res[lane] = uint32_t(y) & 0xFFFFu;
                }
                wave_sync();
                m = wf;
                j = pb - r0;
                while (m) {
                    const int b = (__ffs(m) - 1) >> 2;
                    m &= m - 1;
                    if (j < 4u) {
                        const uint32_t* rr = res + 16 * j;
#pragma unroll
                        for (int jj = 0; jj < NP; jj++) {
                            const uint32_t w = rr[ZigZag<N>::idx[2 * jj]] | (rr[ZigZag<N>::idx[2 * jj + 1]] << 16);
#pragma unroll
                            for (int bb = 0; bb < NS; bb++) zp[bb][jj] = (b == bb) ? w : zp[bb][jj];
                        }
                    }
                    j++;
                }
                wave_sync();
            }
        }
    }
    // statistics: FP64 requests of this wave (one store) -- the structural scan's total plus the
    // whole-block count, both already in scalar registers
    if (lane == 0) a.wave_fix[size_t(t) * 4 + wv] = wave_req;
    WSTAMP(3);
    asm volatile("; PHASE p3" ::: "memory");

    // ------------------------------------------------------------ sizing + the wave's offsets
    lane = fresh_lane();
    uint32_t blw[NS], rb[NS];
    const uint32_t k0 = uint32_t(tif * TG + GW * wv) * 4u;  // the wave's first block (frame raster order)
#pragma unroll
    for (int b = 0; b < NS; b++) {
        const bool valid = 64 * b + lane < nbw;
        if (a.coef && valid) {
            int16_t* dst = a.coef + (size_t(frame) * a.by * a.bx + k0 + 64 * b + lane) * NN;
#pragma unroll
            for (int k = 0; k < NN; k++) {
                const int kz = ZigZagInv<N>::pos[k];
                dst[k] = int16_t(kz & 1 ? (zp[b][kz >> 1] >> 16) : (zp[b][kz >> 1] & 0xFFFFu));
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        blw[b] = size_block4(zp[b], a.rle, &rb[b]);
        rb[b] = valid ? rb[b] : 0u;
        asm volatile("" : "+v"(blw[b]), "+v"(rb[b]));
#pragma unroll
        for (int j = 0; j < NP; j++) asm volatile("" : "+v"(zp[b][j]));
        __builtin_amdgcn_sched_barrier(0);
    }
    uint32_t T[NS], off[NS];
#pragma unroll
    for (int h = 0; h < NS / 2; h++) {  // two slots per 32-bit scan (16-bit halves)
        const uint32_t sv = rb[2 * h] | (rb[2 * h + 1] << 16);
        const uint32_t iv = wave_incl_scan_dpp(sv);
        const uint32_t tv = __builtin_amdgcn_readlane(iv, 63), ev = iv - sv;
        T[2 * h] = tv & 0xFFFFu;
        T[2 * h + 1] = tv >> 16;
        off[2 * h] = ev & 0xFFFFu;
        off[2 * h + 1] = ev >> 16;
    }
    uint32_t Sb[NS];  // slot starts in the wave image
    Sb[0] = 0u;
#pragma unroll
    for (int b = 1; b < NS; b++) Sb[b] = Sb[b - 1] + T[b - 1];
    const uint32_t Tw = Sb[NS - 1] + T[NS - 1];
    const uint32_t S2 = Sb[2];  // the end of slot pair 0
    // The tile's bit count: wave 0 alone waits for the four waves' counts (their flags, cleared
    // before the tile) and publishes it; the other waves go on to their emission and learn their
    // place in the tile after the position barrier.  (A launch too small to fill the chip -- deep
    // look-back -- keeps a workgroup barrier here: all four waves read predecessor windows.)
    if (lane == 0) {
        misc[wv] = Tw;
        __hip_atomic_store(&misc[ML::F + wv], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    WSTAMP(4);
    asm volatile("; PHASE p4" ::: "memory");
    if (deep) {
        lds_barrier();
    } else if (wv == 0) {
        for (;;) {
            const u32x4 f = *reinterpret_cast<const volatile u32x4*>(misc + ML::F);
            if (__builtin_amdgcn_readfirstlane(f.x & f.y & f.z & f.w)) break;
            __builtin_amdgcn_s_sleep(1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    WSTAMP(5);
    asm volatile("; PHASE p5" ::: "memory");

    lane = fresh_lane();
    uint32_t A = 0;  // (wave 0, or every wave in deep mode; the others after the position barrier)
#pragma unroll
    for (int w = 0; w < 4; w++) A += __builtin_amdgcn_readfirstlane(misc[w]);
    if (wv == 0 && lane == 0) chain_publish_count(a.st, t, chain_pos, a.tag, A);  // successors may resolve now
    // look-back probes, in flight while emitting.  Deep (a launch too small to fill the chip: its
    // tiles reach their look-back together, so a tile's nearest inclusive prefix is far away): the
    // four waves read predecessors [64 DW wv, 64 DW (wv + 1)) in DW windows each -- 256 DW in one
    // round trip; otherwise wave 0 reads the nearest kProbe0.
    constexpr int DW = 2;
    Probe pr[DW];
#pragma unroll
    for (int i = 0; i < DW; i++) pr[i] = Probe{0, 0, 0};
    if (chain_pos != 0) {
        if (deep) {
#pragma unroll
            for (int i = 0; i < DW; i++) pr[i] = probe_issue(a.st, t, chain_pos, step, 64 * (DW * wv + i), 64);
        } else if (wv == 0 && !(IE_P_ABL & 4)) {  // (look-back left out: no probe either)
            pr[0] = probe_issue(a.st, t, chain_pos, step, 0, kProbe0);
        }
    }

    const uint32_t reg_bit0 = uint32_t(wv * RW) * 32u;
    auto zero_img = [&](uint32_t bits) {
        const uint32_t nq = (bits + 127u) >> 7;  // 16-byte groups
        uint32_t z;
        asm volatile("v_mov_b32 %0, 0" : "=v"(z));  // (a hoisted zero vector was spilled)
        for (uint32_t q = lane; q < nq; q += 64) *reinterpret_cast<u32x4*>(reg + 4 * q) = u32x4{z, z, z, z};
    };
    // The wave's whole image fits its region (the last record's trailing zero fields reach at
    // most rec_bits past its start, plus the 64-bit window): all four slots are emitted before
    // the position barrier -- beside wave 0's look-back -- and stored in one pass after it.
    // Otherwise slot pairs in turn (pair 1 after pair 0 is stored).
    const bool whole = Tw + uint32_t(a.rec_bits) + 64u <= 32u * RW;
    auto emit_slot = [&](int b) {  // slot b at its place in the (whole or pair) image
        if (!(IE_P_ABL & 2) && rb[b]) {
            const uint32_t p = reg_bit0 + (whole ? Sb[b] : Sb[b] - Sb[(b / PS) * PS]) + off[b];
            if (a.tri && a.rle) {
                // (wave-uniform: a slot whose every record has bl <= 8 takes the four-coefficient fields)
                if (!__ballot((blw[b] & 0xFFu) > 8u)) emit_block4(p, zp[b], blw[b]);
                else emit_block3(smem, p, zp[b], blw[b]);
            } else {
                emit_block2<N>(smem, p, zp[b], blw[b], a.rle);
            }
        }
    };
    zero_img(whole ? Tw : S2);
    wave_sync();
#pragma unroll
    for (int b = 0; b < PS; b++) emit_slot(b);
    if (whole) {
#pragma unroll
        for (int b = PS; b < NS; b++) emit_slot(b);
    }
    wave_sync();
    WSTAMP(6);
    asm volatile("; PHASE p6" ::: "memory");
    if (lane == 0 && Tw) misc[ML::H + wv] = reg[0];  // the wave's first 32 bits

    // ------------------------------------------------------------ look-back (wave 0)
    lane = fresh_lane();
    const bool chain_last = a.segmented ? (tif == a.tiles_per_frame - 1) : (t == a.ntiles - 1);
    uint32_t* const out = a.out + (a.segmented ? uint64_t(frame) * a.out_pitch_words : 0ull);
    if (deep && chain_pos != 0) {
        // every wave sums its windows in order, up to the first with an inclusive prefix (read
        // again until every value it needs is published; its predecessors never wait on this
        // tile), for wave 0 to combine
        uint64_t sm = 0;
        bool found = false;
        unsigned spins = 0;
        for (;;) {
            bool ready = true;
            sm = 0;
            found = false;
#pragma unroll
            for (int i = 0; i < DW; i++) {
                const WinSum r = window_sum(pr[i], chain_pos, 64 * (DW * wv + i), 64, a.tag);
                if (!found) {
                    ready = ready && r.ready;
                    sm += r.sum;
                    found = r.found;
                }
            }
            if (ready) break;
            if (++spins > kSpinLimit) {
                if (lane == 0) atomicAdd(&a.err[0], 1u);
                break;
            }
            __builtin_amdgcn_s_sleep(1);
#pragma unroll
            for (int i = 0; i < DW; i++) pr[i] = probe_issue(a.st, t, chain_pos, step, 64 * (DW * wv + i), 64);
        }
        if (lane == 0) {
            misc[ML::D + 2 * wv] = uint32_t(sm);
            misc[ML::D + 2 * wv + 1] = uint32_t(sm >> 32);
            misc[ML::FD + wv] = found ? 1u : 0u;
        }
        lds_barrier();
    }
    if (wv == 0) {
        uint64_t excl = 0;
        uint32_t ptail = 0, pend = 0;
        if (chain_pos == 0) {
            const uint32_t s = uint32_t(start_bit & 31);
            ptail = s ? (bswap32(out[start_bit >> 5]) >> (32 - s)) : 0u;
        } else {
            bool done = false;
            if (deep) {
#pragma unroll
                for (int w = 0; w < 4; w++) {
                    if (!done) {
                        excl += uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(misc[ML::D + 2 * w]))) |
                                (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(misc[ML::D + 2 * w + 1]))) << 32);
                        done = __builtin_amdgcn_readfirstlane(misc[ML::FD + w]) != 0;
                    }
                }
                if (!done) excl = 0;  // more than 256 DW predecessors back: the wave-0 walk from the start
            }
            if (!done) {
                const Probe p0 = deep ? probe_issue(a.st, t, chain_pos, step, 0, kProbe0) : pr[0];
                excl = (IE_P_ABL & 4) ? uint64_t(chain_pos) * 30000u
                                      : lookback_wave<IE_W_AHEAD, IE_W_LBW>(p0, a.st, t, chain_pos, step, a.tag, a.err, nullptr, deep);
            }
            const bool have = uint32_t(pr[0].gt >> 56) == a.tag;
            const bool split = ((start_bit + excl) & 31) != 0;
            ptail = have ? uint32_t(pr[0].gt) : 0u;
            pend = (!have && split) ? 1u : 0u;
        }
        if (lane == 0) {
            if (chain_pos != 0) publish(a.st, t, 1, a.tag, excl + A);
            misc[ML::E] = uint32_t(excl);
            misc[ML::E + 1] = uint32_t(excl >> 32);
            misc[ML::PT] = ptail;
            misc[ML::PD] = pend;
            const uint64_t P = start_bit + excl;
            if (tif == 0) a.frame_start[frame] = P;
            if (chain_last) a.chain_end[a.segmented ? frame : 0] = P + A;
        }
    }
    WSTAMP(7);
    asm volatile("; PHASE p7" ::: "memory");
    lds_barrier();  // ---- the tile's position
    WSTAMP(8);
    asm volatile("; PHASE p8" ::: "memory");
    lane = fresh_lane();
    uint32_t W = 0;
    A = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint32_t v = __builtin_amdgcn_readfirstlane(misc[w]);
        A += v;
        W += (w < wv) ? v : 0u;
    }

    // ------------------------------------------------------------ store, slot pair by slot pair
    if (Tw) {
        // (readfirstlane returns int: zero-extend each half, or a prefix of 2^31 bits or more
        // would sign-extend into the high word)
        const uint64_t excl = uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(misc[ML::E]))) |
                              (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(misc[ML::E + 1]))) << 32);
        const uint64_t Xw = start_bit + excl + W;
        const bool pend = __builtin_amdgcn_readfirstlane(misc[ML::PD]) != 0u;
        // the wave's first word is written by the previous wave (or, pending, later by this one)
        const uint64_t skipw = ((Xw & 31) && (wv > 0 || pend)) ? (Xw >> 5) : ~0ull;
        uint32_t prev = (wv == 0) ? __builtin_amdgcn_readfirstlane(misc[ML::PT]) : 0u;
        // HIST: bytes at or past the chain's last byte are padding
        const HistCountT<HR> hc{hl, chain_last ? (start_bit + excl + A + 7) / 8 : ~0ull, uint32_t(lane % HR)};
        auto count = [&](uint64_t gw, uint32_t v) {
            if constexpr (HIST) hc(gw, v);
        };
        auto store_pair = [&](uint32_t S0, uint32_t n) {
            if (!n || (IE_P_ABL & 8)) return;
            const uint64_t Xb = Xw + S0;
            const uint32_t nw = uint32_t(((Xb + n) >> 5) - (Xb >> 5));
            if constexpr (HIST) store_slot(out, reg, Xb, nw, ((Xb >> 5) == skipw) ? 1u : 0u, prev, lane, hc);
            else store_slot(out, reg, Xb, nw, ((Xb >> 5) == skipw) ? 1u : 0u, prev, lane);
            prev = slot_tail32(reg, n, prev);
        };
        if constexpr (HIST) {
            if (wv == 0 && chain_pos == 0)  // the words before the first record word: the caller's header
                for (uint32_t i = lane; i < uint32_t(start_bit >> 5); i += 64) hc(i, out[i]);
        }
        const uint64_t E = Xw + Tw;
        const uint32_t e = uint32_t(E) & 31u;
        store_pair(0u, whole ? Tw : S2);
        WSTAMP(9);
        asm volatile("; PHASE p9" ::: "memory");
        if (!whole && Tw > S2) {
            wave_sync();  // pair 0's image has been read
            zero_img(Tw - S2);
            wave_sync();
#pragma unroll
            for (int b = PS; b < NS; b++) emit_slot(b);
            wave_sync();
            store_pair(S2, Tw - S2);
        }
        const uint32_t nexthead = (e && wv < wlast) ? misc[ML::H + wv + 1] : 0u;
        if (lane == 0) {
            if (e && (wv < wlast || chain_last)) {  // the wave's last, partial word
                const uint32_t v = bswap32((prev << (32u - e)) | (nexthead >> e));
                out[E >> 5] = v;
                count(E >> 5, v);
            }
            if (wv == wlast) publish(a.st, t, 2, a.tag, prev);  // the tile's last 32 bits
            if (wv == 0 && pend) {  // the first word, with the predecessor's tail
                const uint32_t pt = wait_tail(a.st, t - step, a.tag, a.err);
                const uint32_t s = uint32_t(Xw) & 31u;
                const uint32_t v = bswap32((pt << (32u - s)) | (misc[ML::H] >> s));
                out[Xw >> 5] = v;
                count(Xw >> 5, v);
            }
        }
        WSTAMP(10);
        asm volatile("; PHASE p10" ::: "memory");
        WRTSTAMP(15);
    }
    if constexpr (HIST) {
        lds_barrier();  // every wave's bytes counted
        uint32_t c = 0;
        const int th = 64 * wv + fresh_lane();
#pragma unroll
        for (int r = 0; r < HR; r++) c += hl[th * HR + r];
        if (c) atomicAdd(&a.hist[size_t(frame) * 256 + th], c);
    }
}

// Returns the FP64-statistics words per tile the launched kernel writes (its waves per tile).
// One workgroup per tile, in dispatch order or (a.ticket: the host's redo after a look-back
// timeout) in ticket order.
int launch_encode4p(const EncArgs& a, hipStream_t s) {
    const size_t lds = p_lds_bytes() + (a.hist ? 1024 * kWHistRep : 0);
    auto kernel = a.hist ? (a.ticket ? encode4p_kernel<true, true> : encode4p_kernel<true, false>)
                         : (a.ticket ? encode4p_kernel<false, true> : encode4p_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(a.ntiles), dim3(256), lds, s, a, a.tab);
    return 4;
}

}  // namespace ie
