// imageencoder_amd/csrc/ie_encode.hip -- the general block encoder for gfx950 (MI355X).  (Aligned 4x4
// FAST launches run encode4p_kernel, ie_encode4p.hip; shared block-level code: ie_encode_blocks.h.)
//
// One launch encodes a batch of frames.  Work decomposition:
//   lane      = one "group" of BPT horizontally adjacent N x N blocks (4 x 4x4 or 1 x 8x8), so a
//               wave reads 64 x 16 B (or 64 x 8 B) contiguous bytes per pixel row;
//   workgroup = one tile of kTPB groups (<= 1024 blocks), never straddling a frame.
// Per tile, in one pass over the pixels (each input byte is read from HBM once, each output word
// written once):
//   1. level shift + forward DCT + quantise every block (Block.cpp:139-153, algo.cpp:309-331):
//      FAST = the butterfly FP32 DCT of ie_dct.h, whose error the host bounds rigorously;
//      coefficients whose quotient lies within that bound of a rounding tie are re-evaluated in
//      the reference's exact FP64 operation order.  EXACT = every coefficient in FP64 order.
//   2. zig-zag RLE sizing (Block.cpp:186-232, :383-397): bl, Lw, record length;
//   3. workgroup exclusive scan of record lengths; the records are written MSB-first into an
//      LDS image of the tile's bit stream (Block.cpp:372-413, BitStream.cpp:61-77);
//   4. decoupled look-back over the preceding tiles of the chain for the tile's global bit offset
//      (the whole workgroup reads 1024 predecessor states per round trip);
//   5. funnel-shifted, coalesced store of the LDS image into the output words.
#include "ie_encode_blocks.h"

namespace ie {

#ifndef IE_PX_AUX8
#define IE_PX_AUX8 2  // cache-policy bits of encode_kernel<8>'s pixel DMA: nt (HBM-resident C3 141.7 against 143.1 us)
#endif

// The tile's LDS bit image: kEncTPB * BPT records of at most rec_bits bits (the matrix's bound,
// ie_capi.cpp build_tables), plus slack for the zero pairs emit_block2 may OR in past the last
// record (<= 16 * N*N bits) and the store's look-ahead word; at least the fix-up's scratch.
// Sized per launch (dynamic LDS): a smaller image measured faster at equal occupancy.
constexpr int image_words_for(int n, int rec_bits) {
    const int bpt = n == 4 ? Geo<4>::BPT : Geo<8>::BPT;
    return ((kEncTPB * bpt * rec_bits + 31) / 32 + 4 + (n * n + 3) + 3) / 4 * 4;  // keeps misc 16-B aligned
}

// FAST 4x4: the tile's pixels go straight from HBM into LDS (global_load_lds_dwordx4, no VGPR
// destination) in the fix-up's pixel area, laid out per wave as [row r][lane][4 words] (block b
// of a lane = word b of each row), and every block reads its four rows back when it is
// transformed: no pixel registers live across the tile's phases.
// Structural fix-up compaction: per-wave LDS task slots in the tile image (not yet built), after it.
constexpr int kFixPix = 0;  // [BPT][TPB] x 4 words: the pixels
constexpr int kFixTasks = kFixPix + Geo<4>::BPT * kEncTPB * 4;  // per wave: [64] tasks, [64] results
constexpr int kFixWords = kFixTasks + (kEncTPB / 64) * 128;     // the image is never smaller
// 8x8: one 16-word block per lane at a 20-word stride (16-byte writes land on distinct banks)
constexpr int kFix8Stride = 20;
constexpr int kFix8Tasks = kFix8Stride * kEncTPB;
constexpr int kNsStage = 4;  // non-structural rows staged per pass, per wave
constexpr int kFix8Stage = kFix8Tasks + (kEncTPB / 64) * 128;
constexpr int kFix8Words = kFix8Stage + (kEncTPB / 64) * kNsStage * 64 * 2;

// Profiling stamps (IE_STAMPS): thread 0's s_memtime at the phase boundaries of each tile.
#define STAMP(i)                                                                                  \
    do {                                                                                          \
        if (stamps && tid == 0) stamps[size_t(t) * kStamps + (i)] = __builtin_amdgcn_s_memtime(); \
    } while (0)

// Occupancy hint: __launch_bounds__'s second argument (Geo<N>::WAVES; stating it as
// amdgpu_waves_per_eu instead measured slower).
// The EXACT 4x4 kernel (FP64 for every coefficient) keeps four waves per SIMD.
template <int N, bool EXACT> constexpr int enc_waves() { return (N == 4 && EXACT) ? 4 : Geo<N>::WAVES; }
#define IE_ENC_BOUNDS(N, EXACT) __launch_bounds__(kEncTPB, (enc_waves<N, EXACT>()))

// A lane's group is Geo<N>::BPT blocks: four 4x4 blocks, not one.  (One block per lane was measured
// and dropped: on one 4K frame, 2 025 tiles of one block per lane took 36 us against 20 us for 506
// tiles of four: the longer look-back chain costs more than the shorter tiles save.)
template <int N, bool EXACT, bool HIST = false>
__global__ IE_ENC_BOUNDS(N, EXACT) void encode_kernel(EncArgs a, const EncTables* __restrict__ tab) {
    constexpr int NN = N * N;
    constexpr int NP = NN / 2;
    constexpr int BPT = Geo<N>::BPT;
    constexpr int WPR = BPT * N / 4;
    constexpr int TPB = kEncTPB;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];  // [a.img_words + 32]
    // Dynamic LDS: [tile image: img_words][misc: 32 words][HIST: 256 words][srow]; the image at
    // LDS address 0, so its addresses need no base.
    uint32_t* img = smem;
    uint32_t* misc = smem + a.img_words;  // [0..15] scan scratch (one word per wave)
    uint32_t* ctl = misc + 16;     // [4] ticket, [5..6] exclusive prefix, [7] predecessor tail
    // FAST mode, the fix-up's FP64 rows.  4x4: all NN rows of P, then S, rq, qd of every coefficient
    // (kRowDoubles); 8x8: the three structural rows P[3][NN], then their S, rq, qd (3 * NN + 9)
    double* const srow = reinterpret_cast<double*>(misc + 32 + (HIST ? 256 : 0));
    constexpr bool kFullRows = N == 4 && !EXACT;
    // 4x4 FAST: row / S / rq / qd of coefficient k
    auto rowP = [&](int k) -> const double* { return srow + k * NN; };
    auto rowS = [&](int k) { return srow[NN * NN + k]; };
    auto rowRq = [&](int k) { return srow[NN * NN + NN + k]; };
    auto rowQd = [&](int k) { return srow[NN * NN + 2 * NN + k]; };

    const int tid = threadIdx.x;
    // Profiling hooks (IE_ABLATE / IE_STAMPS) exist only in IE_PROFILE builds (tools/variants.sh):
    // in the product build they are constants, so they hold no scalar registers.  (Round 3 kept them
    // live in the 8x8 kernel to dodge a spill; with its pixels in LDS and the fix-up reading them
    // from there the 8x8 kernel has no scratch without that.)
    constexpr bool kProf = IE_PROFILE != 0;
    const int ablate = kProf ? a.ablate : 0;
    uint64_t* const stamps = kProf ? a.stamps : nullptr;
    // Tile order = dispatch order.  Workgroups are dispatched in increasing blockIdx, so every
    // chain predecessor of a resident tile is resident or done and the look-back cannot
    // deadlock; the bounded spins report (never hang) should that ever not hold, and the host
    // then re-runs with an atomic ticket (a.ticket != nullptr), which orders tiles explicitly.
    int t;
    if (a.ticket) {
        if (tid == 0) ctl[4] = uint32_t(atomicAdd(a.ticket, 1ull) - a.ticket_base);
        lds_barrier();
        t = __builtin_amdgcn_readfirstlane(int(ctl[4]));  // uniform: tile geometry stays in SGPRs
        if (t >= a.ntiles) return;  // ticket desync (a failed earlier launch): never touch memory
    } else {
        t = int(blockIdx.x);
    }
    STAMP(0);
    uint32_t* const hl = misc + 32;  // HIST: the tile's byte histogram
    if constexpr (HIST)
        for (int i = tid; i < 256; i += TPB) hl[i] = 0u;  // (visible after the scan's barriers)
    if constexpr (kFullRows) {
        // 4x4: every coefficient's FP64 row P[k][*] and its S, rq, qd (304 doubles): the fix-up's
        // structural AND whole-block evaluations read them from LDS, never from global memory
        constexpr int kRowDoubles = NN * NN + 3 * NN;
        for (int i = tid; i < kRowDoubles; i += TPB)
            srow[i] = (i < NN * NN) ? tab->P[i] : (i < NN * NN + NN) ? tab->S[i - NN * NN]
                    : (i < NN * NN + 2 * NN) ? tab->rq[i - NN * NN - NN] : tab->qd[i - NN * NN - 2 * NN];
    } else if constexpr (!EXACT) {
        // issued before the pixel loads, so waiting for it does not wait for them
        for (int i = tid; i < 3 * NN + 9; i += TPB) srow[i] = tab->srow[i];
    }
    const TileGeo g = tile_geo<N, BPT>(a, t, tid);
    // the chain's first bit: the host's value, or (streamed video, ie_vstream_*) the previous
    // launch's chain end on the device, written before this launch started (stream order)
    const uint64_t start_bit = a.start_dev ? *a.start_dev : a.start_bit;
    const int frame = g.frame, tif = g.tif, step = g.step, chain_pos = g.chain_pos;
    const int nblk = g.nblk, byi = g.byi, bx0 = g.bx0;
    constexpr bool kLdsPix = N == 4 && !EXACT;
    // 8x8 FAST: the pixels in LDS too, [8 rows][64 lanes][2 words] per wave (block row r of lane l
    // = words r*128 + 2l, 2l+1): no pixel registers live through the transform and the fix-up
    constexpr bool kLdsPix8 = N == 8 && !EXACT;
    // kLdsPix: this wave's [4 rows][64 lanes][BPT] words; block b of a lane = word b of each row
    constexpr int kRowW = (N == 8) ? 128 : 64 * BPT;
    uint32_t* const pwave = img + kFixPix + (tid >> 6) * (N * kRowW);
    const int lane = tid & 63;
    uint32_t seg[N][WPR];
    if constexpr (kLdsPix8) {
        // DMA when the wave's blocks pair up within rows (even bx): lanes 0-31 fetch row r, lanes
        // 32-63 row r+1, 16 bytes = the row pieces of blocks 2c, 2c+1 (c = lane & 31) each.  Its
        // 16-byte source must be 16-byte aligned (kVec16: base, stride and pitch are; the piece
        // starts at an even block): rows that are only 8-byte aligned go through registers.
        const int wfirst = tif * TPB + (tid & ~63);                          // the wave's first block
        const int nwb = min(64, max(0, a.groups_per_frame - wfirst));        // its blocks in this frame
        if ((a.vec_ok & kVec16) && !(a.bx & 1) && nwb > 0) {
            const int c = lane & 31, half = lane >> 5;
            const int bi = wfirst + 2 * c;                                    // block of this lane's piece
            const bool live = 2 * c < nwb;
            const int by_ = bi / a.bx, bx_ = bi - by_ * a.bx;
            const uint8_t* src = a.y + size_t(frame) * a.frame_pitch + size_t(by_) * N * a.stride + size_t(bx_) * N;
#pragma unroll
            for (int r = 0; r < N; r += 2)
                if (live)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + size_t(r + half) * a.stride),
                                                     (__attribute__((address_space(3))) void*)(pwave + r * kRowW), 16, 0, IE_PX_AUX8);
        } else {  // odd bx / rows not 16-byte aligned: through registers (8-byte loads, or bytes)
            load_tile<N, WPR, BPT>(a, g, seg);
#pragma unroll
            for (int r = 0; r < N; r++) {
                u32x2 v;
                v.x = seg[r][0];
                v.y = seg[r][1];
                *reinterpret_cast<u32x2*>(pwave + r * kRowW + 2 * lane) = v;
            }
        }
    } else if constexpr (kLdsPix) {
        static_assert(BPT == 4 && WPR == BPT && TPB % 64 == 0, "LDS pixel layout: 16 bytes per lane per row");
        if (ablate & 4096) {
            // profiling: no pixel loads at all (the LDS holds whatever the previous tile left)
        } else if (!__ballot(!(a.vec_ok && nblk == BPT))) {  // every group of the wave is whole: DMA
            const uint8_t* base =
                a.y + size_t(frame) * a.frame_pitch + size_t(byi) * N * a.stride + size_t(bx0) * N;
#pragma unroll
            for (int r = 0; r < N; r++)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + size_t(r) * a.stride),
                                                 (__attribute__((address_space(3))) void*)(pwave + r * kRowW), 16, 0, 0);
        } else {  // ragged (frame edge, unaligned rows): through registers
            load_tile<N, WPR, BPT>(a, g, seg);
#pragma unroll
            for (int r = 0; r < N; r++) {
                u32x4 v;
                v.x = seg[r][0]; v.y = seg[r][1]; v.z = seg[r][2]; v.w = seg[r][3];
                *reinterpret_cast<u32x4*>(pwave + r * kRowW + lane * 4) = v;
            }
        }
    } else if (ablate & 128) {  // profiling: no pixel loads (synthetic pixels from the thread id)
#pragma unroll
        for (int r = 0; r < N; r++)
#pragma unroll
            for (int m = 0; m < WPR; m++) seg[r][m] = (uint32_t(tid) * 0x9E3779B1u + uint32_t(t) * 0x85EBCA77u) ^ (r * 0x27D4EB2Fu + m);
    } else {
        load_tile<N, WPR, BPT>(a, g, seg);
    }
    if constexpr (!EXACT) lds_barrier();  // srow visible (the pixel loads stay in flight)
    if constexpr (kLdsPix || kLdsPix8) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's pixels landed

    asm volatile("; PHASE load_done" ::: "memory");
    if (ablate & 512) return;  // profiling: instruction count of the prologue + load alone
    if (stamps) {  // profiling: wait for the pixels so the stamp marks their arrival
        uint32_t acc = 0;
#pragma unroll
        for (int r = 0; r < N; r++)
#pragma unroll
            for (int m = 0; m < WPR; m++) acc ^= seg[r][m];
        if (acc == 0x9E3779B9u) a.err[1] = acc;
    }
    STAMP(2);
    // ---------------------------------------------------------------- 1. transform + quantise
    uint32_t zp[BPT][NP];
    // fix-up requests, 4 bits per block: bits 0-2 structural coefficient s, bit 3 the whole block
    uint32_t flags = 0;
    uint64_t near8 = 0;  // 8x8: per-coefficient requests of the lane's one block
    uint32_t pix_next[N];  // the odd block's rows, read with the even block's
#pragma unroll
    for (int b = 0; b < BPT; b++) {
        __builtin_amdgcn_sched_barrier(0);  // one block at a time: keeps the live set small
        if constexpr (EXACT) {
            BlockPx<N> px;
#pragma unroll
            for (int i = 0; i < N; i++)
#pragma unroll
                for (int m = 0; m < N / 4; m++) px.w[i * (N / 4) + m] = seg[i][(b * N) / 4 + m];
            uint32_t yb[NN];
            for (int k = 0; k < NN; k++) yb[k] = uint32_t(exact_coef<N>(tab, k, px));
#pragma unroll
            for (int j = 0; j < NP; j++)
                zp[b][j] = __builtin_amdgcn_perm(yb[ZigZag<N>::idx[2 * j + 1]], yb[ZigZag<N>::idx[2 * j]], 0x05040100u);
        } else {
            float x[NN];
            if constexpr (kLdsPix8) {
                uint32_t rows[N][2];
#pragma unroll
                for (int r = 0; r < N; r++) {
                    const u32x2 v = *reinterpret_cast<const u32x2*>(pwave + r * kRowW + 2 * lane);
                    rows[r][0] = v.x;
                    rows[r][1] = v.y;
                }
                block_pixels<N, 2>(rows, 0, x);
            } else if constexpr (kLdsPix) {
                uint32_t rows[N][1];
                // two blocks' rows per 8-byte read (2-way instead of 4-way bank conflicts: -0.6 %)
                if (b % 2 == 0) {
#pragma unroll
                    for (int r = 0; r < N; r++) {
                        const u32x2 v = *reinterpret_cast<const u32x2*>(pwave + r * kRowW + lane * BPT + b);
                        rows[r][0] = v.x;
                        pix_next[r] = v.y;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < N; r++) rows[r][0] = pix_next[r];
                }
                block_pixels<N, 1>(rows, 0, x);
            } else {
                block_pixels<N, WPR>(seg, b, x);
            }
            if (!(ablate & 16)) quotients<N>(tab, x);
            if constexpr (N == 8) {
                static_assert(BPT == 1, "8x8: one block per lane");
                near8 = round_block_mask<N>(tab, x, zp[b]);
                if (b >= nblk || (ablate & 1)) near8 = 0;
#pragma unroll
                for (int j = 0; j < NP; j++) asm volatile("" : "+v"(zp[b][j]));  // packed here, not at first use
                continue;
            }
            uint32_t sf;
            const float emax = round_block<N>(tab, x, zp[b], &sf);
            uint32_t fb = (emax >= tab->lim_min) ? 8u : sf;  // a whole-block fix covers s
            if (ablate & 32) fb &= 7u;   // profiling: drop whole-block fixes
            if (ablate & 64) fb &= 8u;   // profiling: drop structural fixes
            if (b < nblk && !(ablate & 1)) flags |= fb << (4 * b);
        }
    }
    asm volatile("; PHASE quant_done" ::: "memory");
    if (ablate & 1024) {  // profiling: ... + transform + rounding (keep the results live)
        uint32_t acc = flags;
#pragma unroll
        for (int b = 0; b < BPT; b++)
#pragma unroll
            for (int j = 0; j < NP; j++) acc ^= zp[b][j];
        if (acc == 0x9E3779B9u) a.err[1] = acc;
        return;
    }
    STAMP(3);

    // ---------------------------------------------------------------- 1b. FP64 fix-up
    // Requests compacted per wave into an LDS task list, evaluated one per lane in the
    // reference's FP64 order, patched back by their owners (below: 8x8, then 4x4).
    if constexpr (!EXACT && N == 8) {
        // 8x8: one task per flagged coefficient, compacted per wave as for 4x4: the lane's block
        // (16 words) goes to an LDS slot, lane i evaluates task i in FP64 -- the structural
        // coefficients' rows from the LDS copy, any other row from the (L2-resident) table --
        // and the owners patch their results in.
        const unsigned nfix = unsigned(__popcll(near8));
        if (__ballot(near8 != 0)) {
            const uint32_t cnt = nfix;
            uint32_t pre = 0, total = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) {  // cnt <= 64
                const uint64_t bm = __ballot((cnt >> k) & 1u);
                pre += __builtin_amdgcn_mbcnt_hi(uint32_t(bm >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(bm), 0u)) << k;
                total += uint32_t(__popcll(bm)) << k;
            }
            uint32_t* task = img + kFix8Tasks + (tid >> 6) * 128;  // [64] tasks, then [64] results
            uint32_t* res = task + 64;
            for (uint32_t r0 = 0; r0 < total; r0 += 64) {
                uint64_t m = near8;
                uint32_t i = pre - r0;
                while (m) {
                    const int k = __ffsll((unsigned long long)m) - 1;
                    m &= m - 1;
                    if (i < 64u) task[i] = (uint32_t(tid) << 6) | uint32_t(k);
                    i++;
                }
                wave_sync();
                const bool busy = uint32_t(lane) < total - r0;
                const uint32_t tk = busy ? task[lane] : 0u;
                const int k = int(tk & 63u), owner = int(tk >> 6);
                const int s = (k == Structural<N>::k[0]) ? 0 : (k == Structural<N>::k[1]) ? 1
                            : (k == Structural<N>::k[2]) ? 2 : -1;
                // Structural rows come from the LDS copy; any other task's row (rare) is staged
                // through LDS by the whole wave first, kNsStage rows per pass (one coalesced row
                // per load), so no dependent add of the FP64 chain waits on global memory.
                uint64_t ns = __ballot(busy && s < 0);
                bool done = !busy;
                double* stage = reinterpret_cast<double*>(img + kFix8Stage) + (tid >> 6) * (kNsStage * NN);
                do {
                    int slot = -1;
                    for (int r = 0; r < kNsStage && ns; r++) {
                        const int L = __ffsll((unsigned long long)ns) - 1;
                        ns &= ns - 1;
                        const int kr = __builtin_amdgcn_readlane(k, L);
                        stage[r * NN + lane] = tab->P[kr * NN + lane];  // NN = 64 = one double per lane
                        if (lane == L) slot = r;
                    }
                    wave_sync();
                    if (!done && (s >= 0 || slot >= 0)) {
                        const double* P = (s >= 0) ? srow + s * NN : stage + slot * NN;
                        const double S = (s >= 0) ? srow[3 * NN + s] : tab->S[k];
                        const double rq = (s >= 0) ? srow[3 * NN + 3 + s] : tab->rq[k];
                        const double qd = (s >= 0) ? srow[3 * NN + 6 + s] : tab->qd[k];
                        res[lane] = uint32_t(exact_coef_rows8(P, S, rq, qd, pwave + 2 * (owner & 63))) & 0xFFFFu;
                        done = true;
                    }
                    wave_sync();  // the next pass rewrites the staged rows
                } while (ns);
                wave_sync();
                m = near8;
                i = pre - r0;
                while (m) {
                    const int k = __ffsll((unsigned long long)m) - 1;
                    m &= m - 1;
                    if (i < 64u) {
                        const uint32_t v = res[i];
                        const int kz = ZigZagInv<N>::pos[k];
#pragma unroll
                        for (int j = 0; j < NP; j++)
                            if ((kz >> 1) == j)
                                zp[0][j] = (kz & 1) ? ((zp[0][j] & 0xFFFFu) | (v << 16)) : ((zp[0][j] & 0xFFFF0000u) | v);
                    }
                    i++;
                }
                wave_sync();  // the next round rewrites the task list
            }
        }
        const unsigned wsum = unsigned(wave_sum64(nfix));
        if ((tid & 63) == 0) a.wave_fix[size_t(t) * (TPB / 64) + (tid >> 6)] = wsum;
    } else if constexpr (!EXACT) {
        // Structural requests, compacted per wave: the wave's pixels go to LDS (so the pixel
        // registers die here), every request gets a task number (a 4-plane ballot prefix), lane i
        // evaluates task i in FP64 and the owners patch their results in.  One FP64 evaluation
        // per 64 requests instead of one per lane per request.
        if (__ballot(flags != 0)) {
            // the pixels of block b of thread `owner` (of this wave): the tile's LDS pixel layout
            auto block_px = [&](int b, int owner) {
                BlockPx<N> px;
#pragma unroll
                for (int r = 0; r < N; r++) px.w[r] = pwave[r * kRowW + (owner & 63) * BPT + b];
                return px;
            };
            const uint32_t sf = flags & (0x77777777u >> (32 - 4 * BPT));
            const uint32_t cnt = __popc(sf);
            uint32_t pre = 0, total = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {  // cnt <= 3 * BPT <= 12
                const uint64_t bm = __ballot((cnt >> k) & 1u);
                pre += __builtin_amdgcn_mbcnt_hi(uint32_t(bm >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(bm), 0u)) << k;
                total += uint32_t(__popcll(bm)) << k;
            }
            uint32_t* task = img + kFixTasks + (tid >> 6) * 128;  // [64] tasks, then [64] results
            uint32_t* res = task + 64;
            for (uint32_t r0 = 0; r0 < total; r0 += 64) {
                uint32_t m = sf, i = pre - r0;
                while (m) {
                    const int bit = __ffs(m) - 1;
                    m &= m - 1;
                    if (i < 64u) task[i] = (uint32_t(tid) << 4) | uint32_t(bit);
                    i++;
                }
                wave_sync();
                if (uint32_t(lane) < total - r0) {
                    const uint32_t tk = task[lane];
                    const int s = int(tk & 3u), b = int((tk >> 2) & 3u), owner = int(tk >> 4);
                    const BlockPx<N> px = block_px(b, owner);
                    const int ks = Structural<N>::k[0] * (s == 0) + Structural<N>::k[1] * (s == 1) +
                                   Structural<N>::k[2] * (s == 2);
                    res[lane] = (ablate & 256) ? (px.w[0] & 0xFFFFu)  // profiling: no FP64 arithmetic
                                                 : uint32_t(exact_coef_row<N>(rowP(ks), rowS(ks), rowRq(ks),
                                                                              rowQd(ks), px)) & 0xFFFFu;
                }
                wave_sync();
                m = sf;
                i = pre - r0;
                while (m) {
                    const int bit = __ffs(m) - 1;
                    m &= m - 1;
                    if (i < 64u) {
                        const uint32_t v = res[i];
                        const int b = bit >> 2, s = bit & 3;
#pragma unroll
                        for (int bb = 0; bb < BPT; bb++)
#pragma unroll
                            for (int ss = 0; ss < 3; ss++) {
                                const int zpos = Structural<N>::zpos(ss);
                                if (b == bb && s == ss)
                                    zp[bb][zpos >> 1] = (zpos & 1) ? ((zp[bb][zpos >> 1] & 0xFFFFu) | (v << 16))
                                                                   : ((zp[bb][zpos >> 1] & 0xFFFF0000u) | v);
                            }
                    }
                    i++;
                }
                wave_sync();  // the next round rewrites the task list
            }
            // Whole-block requests (rare: an ordinary coefficient near a tie): all NN coefficients
            // of the block are re-evaluated in FP64, one per lane, four blocks per round.
            const uint32_t wf = flags & (0x88888888u >> (32 - 4 * BPT));
            if (__ballot(wf != 0)) {
                const uint32_t nb = __popc(wf);
                uint32_t pb = 0, tb = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) {  // nb <= BPT <= 4
                    const uint64_t bm = __ballot((nb >> k) & 1u);
                    pb += __builtin_amdgcn_mbcnt_hi(uint32_t(bm >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(bm), 0u)) << k;
                    tb += uint32_t(__popcll(bm)) << k;
                }
                for (uint32_t r0 = 0; r0 < tb; r0 += 4) {
                    uint32_t m = wf, j = pb - r0;
                    while (m) {
                        const int b = (__ffs(m) - 1) >> 2;
                        m &= m - 1;
                        if (j < 4u) task[j] = (uint32_t(tid) << 4) | uint32_t(b);
                        j++;
                    }
                    wave_sync();
                    if (uint32_t(lane >> 4) < tb - r0) {
                        const uint32_t tk = task[lane >> 4];
                        const int b = int(tk & 3u), owner = int(tk >> 4), k = lane & 15;
                        const BlockPx<N> px = block_px(b, owner);
                        res[lane] = uint32_t(exact_coef_row<N>(rowP(k), rowS(k), rowRq(k), rowQd(k), px)) & 0xFFFFu;
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
                                for (int bb = 0; bb < BPT; bb++) zp[bb][jj] = (b == bb) ? w : zp[bb][jj];
                            }
                        }
                        j++;
                    }
                    wave_sync();
                }
            }
        }
        const unsigned wsum = unsigned(wave_sum64(__popc(flags)));
        if ((tid & 63) == 0) a.wave_fix[size_t(t) * (TPB / 64) + (tid >> 6)] = wsum;
    }
    asm volatile("; PHASE fix_done" ::: "memory");
    STAMP(4);

    // ---------------------------------------------------------------- 1c. zig-zag RLE sizing
    uint32_t blw[BPT];  // bl | Lw << 8
    uint32_t rbits[BPT];
    uint32_t mybits = 0;
#pragma unroll
    for (int b = 0; b < BPT; b++) {
        if (a.coef && b < nblk) {
            int16_t* dst = a.coef + (size_t(frame) * a.by * a.bx + size_t(byi) * a.bx + bx0 + b) * NN;
#pragma unroll
            for (int k = 0; k < NN; k++) {
                const int kz = ZigZagInv<N>::pos[k];
                dst[k] = int16_t(kz & 1 ? (zp[b][kz >> 1] >> 16) : (zp[b][kz >> 1] & 0xFFFFu));
            }
        }
        blw[b] = size_block<N>(zp[b], a.rle, &rbits[b]);
        rbits[b] = (b < nblk) ? rbits[b] : 0u;
        mybits += rbits[b];
    }
    asm volatile("; PHASE size_done" ::: "memory");
    if (ablate & 2048) {  // profiling: ... + FP64 fix-up + sizing
        uint32_t acc = mybits;
#pragma unroll
        for (int b = 0; b < BPT; b++)
#pragma unroll
            for (int j = 0; j < NP; j++) acc ^= zp[b][j] + blw[b];
        if (acc == 0x9E3779B9u) a.err[1] = acc;
        return;
    }
    STAMP(5);
    // (the fix-up slots alias the tile image: the scan's barrier below orders them before the
    // image is zeroed)

    // ---------------------------------------------------------------- 2. tile scan + LDS image
    uint32_t A;
    const uint32_t off = block_excl_scan<TPB>(mybits, misc, &A);
    if (tid == 0) chain_publish_count(a.st, t, chain_pos, a.tag, A);  // successors may resolve now
    Probe pr{0, 0, 0};
    if (tid < 64 && chain_pos != 0 && !(ablate & 4)) pr = probe_issue(a.st, t, chain_pos, step, 0, kProbe0);  // in flight during emission
    const uint32_t nw = (A + 31) >> 5;
    for (uint32_t w = 4 * tid; w < nw + 2; w += 4 * TPB) *reinterpret_cast<u32x4*>(img + w) = u32x4{0u, 0u, 0u, 0u};
    lds_barrier();
    asm volatile("; PHASE scan_done" ::: "memory");
    STAMP(6);
    if (!(ablate & 2)) {  // the records: header + Lw + z0 and coefficient triples, or pairs
        uint32_t p = off;
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            if (N == 4 && a.tri && a.rle) {
                if constexpr (N == 4)
                    if (rbits[b]) emit_block3(img, p, zp[b], blw[b]);
            } else {
                if (rbits[b]) emit_block2<N>(img, p, zp[b], blw[b], a.rle);
            }
            p += rbits[b];
        }
    }
    lds_barrier();
    asm volatile("; PHASE emit_done" ::: "memory");
    STAMP(7);

    // ---------------------------------------------------------------- 3. look-back
    const bool chain_last = a.segmented ? (tif == a.tiles_per_frame - 1) : (t == a.ntiles - 1);
    uint32_t* out = a.out + (a.segmented ? uint64_t(frame) * a.out_pitch_words : 0ull);
    uint64_t excl;
    if (ablate & 4) {
        if (tid == 0) {
            publish(a.st, t, 1, a.tag, A);
            ctl[7] = 0;
            ctl[8] = 0;
        }
        lds_barrier();
        excl = uint64_t(tif) * (110u * TPB);
    } else {
        excl = chain_resolve(a.st, t, chain_pos, step, a.tag, img, A, out, start_bit, a.err, ctl, pr,
                             stamps ? &stamps[size_t(t) * kStamps + 1] : nullptr, true, a.deep_lb != 0);
    }
    if (tid == 0) {
        const uint64_t P = start_bit + excl;
        if (tif == 0) a.frame_start[frame] = P;
        if (chain_last) a.chain_end[a.segmented ? frame : 0] = P + A;
    }
    asm volatile("; PHASE lookback_done" ::: "memory");
    STAMP(8);

    // ---------------------------------------------------------------- 4. store
    if constexpr (HIST) {
        if (tif == 0)  // the words before the first record word hold only the caller's header
            for (uint32_t i = tid; i < uint32_t(start_bit >> 5); i += TPB) {
                const uint32_t v = out[i];
#pragma unroll
                for (int k = 0; k < 4; k++) atomicAdd(&hl[(v >> (8 * k)) & 0xFFu], 1u);
            }
        const uint64_t end = start_bit + excl + A;
        const HistCount cnt{hl, chain_last ? (end + 7) / 8 : ~0ull};
        store_tile<TPB>(out, img, A, start_bit + excl, ctl, chain_last, a.st, t - step, a.tag, a.err, cnt);
        lds_barrier();
        for (int i = tid; i < 256; i += TPB)
            if (hl[i]) atomicAdd(&a.hist[size_t(frame) * 256 + i], hl[i]);
    } else if (!(ablate & 8)) {
        store_tile<TPB>(out, img, A, start_bit + excl, ctl, chain_last, a.st, t - step, a.tag, a.err);
    }
    STAMP(9);
}

// The streamed host path's per-image header words: word i (read from page-locked host memory
// the device maps, one PCIe read per image) to dst[i * pitch_words] -- instead of an SDMA copy
// that would queue behind the chunk's pixel upload on the copy engine.
__global__ void word_scatter_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint64_t pitch_words,
                                    int n) {
    const int i = int(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) dst[size_t(i) * pitch_words] = src[i];
}

void launch_word_scatter(const uint32_t* src, uint32_t* dst, uint64_t pitch_words, int n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(word_scatter_kernel, dim3(unsigned((n + 63) / 64)), dim3(64), 0, s, src, dst, pitch_words, n);
}

int encode_blocks_per_thread(int n) { return n == 4 ? Geo<4>::BPT : Geo<8>::BPT; }
#ifndef IE_SMALL_TILES
#define IE_SMALL_TILES 1024
#endif
int encode_small_tiles() {
    static const char* e = getenv("IE_SMALL_TILES");  // (A/B aid: 0 disables the small-launch geometry)
    static const int v = e ? atoi(e) : IE_SMALL_TILES;
    return v;
}

int encode_threads_per_tile() { return kEncTPB; }

int launch_encode(const EncArgs& a0, int n, bool exact, hipStream_t s) {
    EncArgs a = a0;
    // 4x4 FAST over whole 16-byte groups: the wave-local encoder (encode4p_kernel)
    if (n == 4 && !exact && Geo<4>::BPT == 4 && a.vec_ok && a.bx % 4 == 0 &&
        a.groups_per_frame % 8 == 0 && a.rec_bits <= 252 && !a.ablate)
        return launch_encode4p(a, s);
    a.img_words = image_words_for(n, a.rec_bits);
    if (n == 4 && a.img_words < kFixWords) a.img_words = kFixWords;
    if (n == 8 && a.img_words < kFix8Words) a.img_words = kFix8Words;
    const size_t rows = exact ? 0 : (n == 4 ? size_t(n * n * n * n + 3 * n * n) : size_t(3 * n * n + 9));
    const size_t lds = (size_t(a.img_words) + 32 + (a.hist ? 256 : 0)) * sizeof(uint32_t) + rows * sizeof(double);
    const dim3 grid(a.ntiles), block(kEncTPB);
    if (a.hist) {  // segmented 4x4 FAST launches only (ie_encode_images_counted; 8x8 would spill)
        hipLaunchKernelGGL((encode_kernel<4, false, true>), grid, block, lds, s, a, a.tab);
        return kEncTPB / 64;
    }
    if (n == 4) {
        if (exact) hipLaunchKernelGGL((encode_kernel<4, true>), grid, block, lds, s, a, a.tab);
        else hipLaunchKernelGGL((encode_kernel<4, false>), grid, block, lds, s, a, a.tab);
    } else {
        if (exact) hipLaunchKernelGGL((encode_kernel<8, true>), grid, block, lds, s, a, a.tab);
        else hipLaunchKernelGGL((encode_kernel<8, false>), grid, block, lds, s, a, a.tab);
    }
    return kEncTPB / 64;
}

}  // namespace ie
