// imageencoder_amd/csrc/ie_probe.hip -- ie_probe_sizes on gfx950: the payload bits of every frame
// under many candidate quantisation matrices, in one pass over the pixels.
//
// The unquantised coefficient D = acc * S[k] of the exact path (exact_coef_inl, ie_encode_blocks.h) does
// not depend on the matrix; only round(D / q) does, and a record's length follows from the rounded
// values alone (size_block, ie_encode_blocks.h; size4 / rec_len, ie_pframe.hip).  So D is formed once
// per coefficient, in FP64 in the reference's operation order (this file is compiled with
// -ffp-contract=off), and every candidate divides, rounds and sizes from it.  No stream is written
// and no look-back chain exists: the lengths are summed.
//
// Layout of the work: one coefficient per lane, lane = zig-zag position -- one 8x8 block or four
// 4x4 blocks per wave and step, so D is one register pair per lane for either block size.  A
// workgroup (four waves) stages a tile of kTileSteps * 4 steps' blocks through LDS, pixels once per
// tile; the transform rows P live in LDS transposed ([ij][lane]: consecutive lanes read consecutive
// doubles, the pixel words are broadcast reads), the candidates as uint16 in zig-zag order.  Per
// candidate: the IEEE division, std::round, "any / last non-zero" from one __ballot, the widest
// value from a DPP OR over the block's lanes, the record length in the block's last lane, a DPP sum
// over the wave, and lane m keeps candidate m's running sum.  A wave adds its sums to
// bits[m * nframes + f] with one 64-bit atomic per candidate when its frame changes or its work
// ends; the sums are integers, so the order does not matter.
//
// ie_probe_rd (probe_kernel<N, true>) adds the distortion of every candidate to the same pass: once a
// candidate's rounded values are in registers, everything the decoder would see is known, so the
// lanes dequantise, run the inverse transform in the reference's order, clamp and compare with
// the staged pixel.  See the comment at probe_rd_sse.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ie_device.h"

namespace ie {
namespace {

constexpr int kProbeSteps = 16;  // steps per wave and tile: 64 8x8 or 256 4x4 blocks per tile, 4 KiB of pixels
constexpr int kProbeWaves = kTPB / 64;

// algo.cpp:68-87: natural index of zig-zag position z
__constant__ uint8_t kProbeZz4[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
__constant__ uint8_t kProbeZz8[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                      12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                      35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                      58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

template <int N> __device__ __forceinline__ int probe_zz(int z) { return N == 4 ? kProbeZz4[z] : kProbeZz8[z]; }

// DPP reductions (the form of wave_sum, ie_pframe.hip): quad permutes and row shifts leave a
// 16-lane row's result in its lane 15, the two row broadcasts the wave's in lane 63.  Lanes whose
// DPP source lies outside the row take 0.
__device__ __forceinline__ uint32_t row_or(uint32_t v) {
    int x = int(v);
    x |= __builtin_amdgcn_update_dpp(0, x, 0xb1, 0xf, 0xf, false);   // quad_perm [1,0,3,2]
    x |= __builtin_amdgcn_update_dpp(0, x, 0x4e, 0xf, 0xf, false);   // quad_perm [2,3,0,1]
    x |= __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x |= __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);  // row_shr:8 (the row's OR in lane 15)
    return uint32_t(x);
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    int x = int(row_or(v));
    x |= __builtin_amdgcn_update_dpp(0, x, 0x142, 0xf, 0xf, false);  // row_bcast:15
    x |= __builtin_amdgcn_update_dpp(0, x, 0x143, 0xf, 0xf, false);  // row_bcast:31 (the wave's OR in lane 63)
    return uint32_t(x);
}
__device__ __forceinline__ uint32_t probe_wave_sum(uint32_t v) {
    int x = int(v);
    x += __builtin_amdgcn_update_dpp(0, x, 0xb1, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x4e, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xf, 0xf, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xf, 0xf, false);
    return uint32_t(__builtin_amdgcn_readlane(x, 63));
}

// Dynamic LDS: [NN][NN] doubles (P transposed; for 4x4 the four blocks' lanes read the same 16
// columns), with the distortion the inverse rows R [uv][ij] as EncTables holds them, then the
// tile's pixel words [NN/4][TB], then the candidates [nq][NN] uint16 (zig-zag order).
template <int N> struct ProbeGeo {
    static constexpr int NN = N * N;
    static constexpr int BPW = 64 / NN;                              // blocks per wave and step
    static constexpr int TB = kProbeWaves * kProbeSteps * BPW;       // blocks per tile
    static constexpr int P_DOUBLES = NN * NN;
    static constexpr int PIX_WORDS = (NN / 4) * TB;
    static constexpr size_t lds_bytes(int nq, bool rd = false) {
        return size_t(P_DOUBLES) * 8 * (rd ? 2 : 1) + size_t(PIX_WORDS) * 4 + ((size_t(nq) * NN * 2 + 7) & ~size_t(7));
    }
};

// zig-zag rank of every natural index (the inverse of kProbeZz4 / kProbeZz8)
struct ProbeIzz4 {
    int r[16];
    constexpr ProbeIzz4() : r() {
        constexpr int zz[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
        for (int z = 0; z < 16; z++) r[zz[z]] = z;
    }
};
__constant__ uint8_t kProbeIzz8[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                       3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                       10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                       21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// 4x4, terms UV .. 15 of a pixel's inverse transform: Y[uv] of the lane's own block comes from the
// row's lane izz(uv) by a DPP row broadcast, R[uv][ij] from LDS (consecutive lanes, consecutive doubles)
template <int UV>
__device__ __forceinline__ void probe_idct4_terms(uint32_t any, int ylo, int yhi, const double* Rl, double& t) {
    if constexpr (UV < 16) {
        constexpr ProbeIzz4 izz;
        constexpr int z = izz.r[UV];
        if ((any >> z) & 1u) {  // (wave-uniform)
            const int lo = __builtin_amdgcn_update_dpp(0, ylo, 0x150 + z, 0xf, 0xf, false);  // row_newbcast:z
            const int hi = __builtin_amdgcn_update_dpp(0, yhi, 0x150 + z, 0xf, 0xf, false);
            t = t + Rl[UV * 16] * __hiloint2double(hi, lo);
        }
        probe_idct4_terms<UV + 1>(any, ylo, yhi, Rl, t);
    }
}

// The squared error of the lane's pixel under one candidate.  vd: the lane's quantised value as the
// decoder reads it (lane = zig-zag position kz of its block), qd: the candidate's entry there,
// Rl: the R column of the lane's pixel (pixel ij = the lane's position within its block, natural
// order), px: that pixel's byte.
//
// Block::processIDCTMulQ (Block.cpp:162-175, algo.cpp:348-358): Y = double(v) * q, then temp[ij] =
// temp[ij] + R[uv][ij] * Y[uv] over uv ascending in natural order, un-contracted; x = temp + 128.0,
// clamped to [0, 255] and truncated (Block.cpp:100-107).  The order over uv is kept; what each lane
// sums is its own pixel.  A zero Y term adds +-0: it leaves every partial sum unchanged but possibly
// the sign of a zero, which + 128 and the clamp erase (the argument of decode_record,
// ie_decode.hip), so a term that is zero in every lane of the wave is skipped -- and, for the same
// reason, a term that is zero may be added where skipping it would cost a branch.  At coarse
// scales most terms are skipped; at fine scales the 2 N^2 FP64 operations per pixel are the cost.
//  - 8x8: the wave is one block.  Y moves to natural order through the LDS crossbar (ds_bpermute),
//    one __ballot gives the non-zero terms as a scalar mask, and a scalar loop walks its bits in
//    ascending order, four per trip (the R reads of a trip are issued together; a trip's missing
//    terms are Y = 0 at uv = 0).  Y[uv] is a readlane: the multiply takes it from SGPRs.
//  - 4x4: four blocks, one per DPP row; a term is skipped when it is zero in all four.
// d8 receives the decoded byte itself (the store of probe_kernel<N, true, true>).
template <int N>
__device__ __forceinline__ uint32_t probe_rd_sse(int vd, double qd, const double* Rl, uint32_t px, int lane, uint32_t& d8) {
    constexpr int NN = N * N;
    const double Y = double(vd) * qd;
    int ylo = __double2loint(Y), yhi = __double2hiint(Y);
    double t = 0.0;
    if constexpr (N == 8) {
        const int src = int(kProbeIzz8[lane]) * 4;
        ylo = __builtin_amdgcn_ds_bpermute(src, ylo);
        yhi = __builtin_amdgcn_ds_bpermute(src, yhi);
        uint64_t todo = __ballot(yhi != 0);  // |Y| >= 1 or Y == +0: the high word tells
        while (todo) {
            double r[4], y[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int uv = todo ? __builtin_ctzll(todo) : 0;
                const int lo = __builtin_amdgcn_readlane(ylo, uv), hi = __builtin_amdgcn_readlane(yhi, uv);
                y[e] = todo ? __hiloint2double(hi, lo) : 0.0;
                r[e] = Rl[uv * NN];
                todo &= todo - 1;
            }
#pragma unroll
            for (int e = 0; e < 4; e++) t = t + r[e] * y[e];
        }
    } else {
        const uint64_t nz = __ballot(vd != 0);
        const uint32_t any = uint32_t(nz | (nz >> 16) | (nz >> 32) | (nz >> 48)) & 0xFFFFu;
        probe_idct4_terms<0>(any, ylo, yhi, Rl, t);
    }
    double x = t + 128.0;
    x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
    d8 = uint32_t(uint8_t(x));
    const int err = int(d8) - int(px);  // in [-255, 255]
    return uint32_t(err * err);
}

// RD = false: the sizes alone (ie_probe_sizes); RD = true: the distortion too (ie_probe_rd).
// ST (ie_probe_gop_rd's I-frames): the sums go to [m * out_m + f * out_f], and every candidate's
// decoded pixels of the frames before dec_frames are stored -- the lane of a block row's first
// pixel collects its quad's four bytes by DPP and writes one word.
template <int N, bool RD, bool ST = false>
__global__ __launch_bounds__(kTPB) void probe_kernel(ProbeArgs a, unsigned long long* sse) {
    static_assert(!ST || RD, "only the distortion pass decodes pixels");
    using G = ProbeGeo<N>;
    constexpr int NN = G::NN, BPW = G::BPW, TB = G::TB;
    extern __shared__ __attribute__((aligned(16))) unsigned char probe_lds[];
    double* Pt = reinterpret_cast<double*>(probe_lds);                        // [ij][kz]
    double* Rn = Pt + G::P_DOUBLES;                                           // RD: [uv][ij]
    uint32_t* pixw = reinterpret_cast<uint32_t*>(Pt + G::P_DOUBLES * (RD ? 2 : 1));  // [word][block of the tile]
    uint16_t* qz = reinterpret_cast<uint16_t*>(pixw + G::PIX_WORDS);          // [m][kz]

    const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int kz = lane % NN, g = lane / NN;     // zig-zag position, block of the step
    const int k = probe_zz<N>(kz);               // natural index

    for (int e = tid; e < NN * NN; e += kTPB) {  // Pt[ij][z] = P[zz(z)][ij]
        const int ij = e / NN, z = e % NN;
        Pt[e] = a.tab->P[probe_zz<N>(z) * NN + ij];
    }
    for (int e = tid; e < a.nq * NN; e += kTPB) qz[e] = a.q[e];
    if constexpr (RD)
        for (int e = tid; e < NN * NN; e += kTPB) Rn[e] = a.tab->R[e];
    const double S = a.tab->S[k];

    const int nblk = a.bx * a.by;
    const uint64_t tpf = uint64_t((nblk + TB - 1) / TB);
    const uint64_t total = tpf * uint64_t(a.nframes);
    uint32_t mine = 0;  // lane m: candidate m's bits of frame cur_f so far (this wave)
    // RD, lane m: candidate m's squared error of frame cur_f so far.  A step adds at most 64 * 255^2,
    // a wave's steps of one frame are not bounded by 2^32: 64 bits.
    uint64_t mine_se = 0;
    int64_t cur_f = -1;
    const bool owner = kz == NN - 1;  // the block's last lane holds its DPP results
    const auto sum_index = [&](int m, int64_t f) {  // candidate m's sum of frame f
        return ST ? uint64_t(m) * a.out_m + uint64_t(f) * a.out_f : uint64_t(m) * uint64_t(a.nframes) + uint64_t(f);
    };

    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const int64_t f = int64_t(it / tpf);
        const int b0 = int(it % tpf) * TB;
        if (f != cur_f) {
            if (cur_f >= 0 && lane < a.nq) {
                if (!RD || a.bits) atomicAdd(&a.bits[sum_index(lane, cur_f)], (unsigned long long)mine);
                if constexpr (RD) atomicAdd(&sse[sum_index(lane, cur_f)], (unsigned long long)mine_se);
            }
            mine = 0;
            mine_se = 0;
            cur_f = f;
        }
        __syncthreads();  // the previous tile's pixels have been read (first pass: the tables are written)
        const uint8_t* fy = a.y + uint64_t(f) * a.frame_pitch;
        for (int s = tid; s < TB * N; s += kTPB) {  // row r of tile block b: N bytes
            const int r = s / TB, b = s % TB;
            const int blk = b0 + b;
            uint32_t w0 = 0, w1 = 0;
            if (blk < nblk) {
                const int byi = blk / a.bx, bxi = blk - byi * a.bx;
                const uint8_t* p = fy + uint64_t(byi * N + r) * a.stride + uint64_t(bxi * N);
                if (a.vec_ok) {
                    w0 = *reinterpret_cast<const uint32_t*>(p);
                    if (N == 8) w1 = *reinterpret_cast<const uint32_t*>(p + 4);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; e++) w0 |= uint32_t(p[e]) << (8 * e);
                    if (N == 8) {
#pragma unroll
                        for (int e = 0; e < 4; e++) w1 |= uint32_t(p[4 + e]) << (8 * e);
                    }
                }
            }
            pixw[(r * (N / 4)) * TB + b] = w0;
            if (N == 8) pixw[(r * 2 + 1) * TB + b] = w1;
        }
        __syncthreads();

        for (int st = 0; st < kProbeSteps; st++) {
            const int j0 = (wave * kProbeSteps + st) * BPW;  // the step's first block within the tile
            if (b0 + j0 >= nblk) break;                      // (wave-uniform)
            const int j = j0 + g;
            const bool valid = b0 + j < nblk;
            // D in the reference's order (algo.cpp:314-325): acc = acc + P[k][ij] * x[ij], then * S
            double acc = 0.0;
#pragma unroll 4
            for (int w = 0; w < NN / 4; w++) {
                const uint32_t px4 = pixw[w * TB + j];
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const double x = double(int((px4 >> (8 * e)) & 0xFFu) - 128);  // == double(p) + (-128.0), exactly
                    acc = acc + Pt[(4 * w + e) * NN + kz] * x;
                }
            }
            const double D = acc * S;
            uint32_t px = 0;  // RD: the byte of the lane's pixel (pixel kz of block j), before the level shift
            if constexpr (RD) px = (pixw[(kz >> 2) * TB + j] >> (8 * (kz & 3))) & 0xFFu;
            // ST: where the lane's quad of decoded pixels goes (row kz / N of block j, from column kz % N),
            // written by the quad's first lane
            uint8_t* dst = nullptr;
            if constexpr (ST) {
                if (valid && (lane & 3) == 0 && f < a.dec_frames) {
                    const int blk = b0 + j, byi = blk / a.bx, bxi = blk - byi * a.bx;
                    dst = a.dec + uint64_t(f) * a.f_dec + (uint64_t(byi * N + kz / N) * uint64_t(a.bx) + uint64_t(bxi)) * N + kz % N;
                }
            }
#pragma unroll 1
            for (int m = 0; m < a.nq; m++) {
                const double qd = double(qz[m * NN + kz]);
                const double t = D / qd;  // IEEE division (Block.cpp:149-152)
                double r = trunc(t);
                if (fabs(t - r) >= 0.5) r += copysign(1.0, t);  // std::round: half away from zero
                const int v = int(r);
                // bits_needed (utils.hpp:226-243) of the widest value: the bit length of the OR of v ^ sign, + 1
                const uint32_t av = uint32_t(v ^ (v >> 31));
                const uint64_t nzw = __ballot(v != 0);
                uint32_t mo, L, lw;
                if constexpr (N == 8) {
                    mo = wave_or(av);
                    L = nzw ? 64u - uint32_t(__clzll((long long)nzw)) : 0u;
                    lw = L;
                    if (L == 64u && !((nzw >> 62) & 1ull)) {  // RLE drops the last element (Block.cpp:388-390)
                        const uint64_t mm = nzw & ((1ull << 63) - 1);
                        lw = mm ? 64u - uint32_t(__clzll((long long)mm)) : 0u;
                    }
                } else {
                    mo = row_or(av);
                    const uint32_t nz = uint32_t(nzw >> (16 * g)) & 0xFFFFu;
                    L = 32u - uint32_t(__clz(int(nz)));  // 0 for nz == 0
                    lw = L;
                    if (L == 16u && !((nz >> 14) & 1u)) lw = 32u - uint32_t(__clz(int(nz & 0x7FFFu)));
                }
                const uint32_t maxb = 33u - uint32_t(__clz(int(mo)));
                const uint32_t ffsL = L ? 32u - uint32_t(__clz(int(L))) : 1u;  // utils.hpp:210-216, ffs(0) == 1
                const uint32_t bl = maxb > ffsL ? maxb : ffsL;
                const uint32_t len = a.rle ? 4u + bl * (lw + 1u) : 4u + bl * uint32_t(NN);
                const uint32_t sum = probe_wave_sum((owner && valid) ? len : 0u);
                if (lane == m) mine += sum;
                if constexpr (RD) {
                    // what the decoder reads: v, but the last value of a record RLE cut short (L == NN, value
                    // NN - 2 zero: lw above; Block.cpp:388-390) is 0
                    const int vd = (a.rle && L == uint32_t(NN) && lw != L && owner) ? 0 : v;
                    uint32_t d8;
                    const uint32_t se = probe_rd_sse<N>(vd, qd, Rn + kz, px, lane, d8);
                    if constexpr (ST) {
                        if (f < a.dec_frames) {  // (wave-uniform: every lane takes part in the quad broadcasts)
                            const int d = int(d8);
                            const uint32_t w4 = d8 | uint32_t(__builtin_amdgcn_update_dpp(0, d, 0x55, 0xf, 0xf, false)) << 8 |
                                                uint32_t(__builtin_amdgcn_update_dpp(0, d, 0xAA, 0xf, 0xf, false)) << 16 |
                                                uint32_t(__builtin_amdgcn_update_dpp(0, d, 0xFF, 0xf, 0xf, false)) << 24;
                            if (dst) *reinterpret_cast<uint32_t*>(dst + uint64_t(m) * a.m_dec) = w4;
                        }
                    }
                    const uint32_t ssum = probe_wave_sum(valid ? se : 0u);  // <= 64 * 255^2
                    if (lane == m) mine_se += ssum;
                }
            }
        }
    }
    if (cur_f >= 0 && lane < a.nq) {
        if (!RD || a.bits) atomicAdd(&a.bits[sum_index(lane, cur_f)], (unsigned long long)mine);
        if constexpr (RD) atomicAdd(&sse[sum_index(lane, cur_f)], (unsigned long long)mine_se);
    }
}

}  // namespace

void launch_probe_sizes(const ProbeArgs& a, int n, hipStream_t s) {
    const int tb = n == 4 ? ProbeGeo<4>::TB : ProbeGeo<8>::TB;
    const uint64_t total = uint64_t((a.bx * a.by + tb - 1) / tb) * uint64_t(a.nframes);
    const unsigned grid = unsigned(total < 1024 ? total : 1024);  // persistent workgroups: the tables are staged once each
    if (n == 4)
        hipLaunchKernelGGL((probe_kernel<4, false>), dim3(grid), dim3(kTPB), ProbeGeo<4>::lds_bytes(a.nq), s, a, nullptr);
    else
        hipLaunchKernelGGL((probe_kernel<8, false>), dim3(grid), dim3(kTPB), ProbeGeo<8>::lds_bytes(a.nq), s, a, nullptr);
}

int probe_rd_max_workgroups(int n) { return n == 4 ? 1024 : 512; }

void launch_probe_rd_store(const ProbeArgs& a, unsigned long long* sse, hipStream_t s) {
    const uint64_t total = uint64_t((a.bx * a.by + ProbeGeo<4>::TB - 1) / ProbeGeo<4>::TB) * uint64_t(a.nframes);
    const uint64_t cap = uint64_t(probe_rd_max_workgroups(4));
    if (total)
        hipLaunchKernelGGL((probe_kernel<4, true, true>), dim3(unsigned(total < cap ? total : cap)), dim3(kTPB),
                           ProbeGeo<4>::lds_bytes(a.nq, true), s, a, sse);
}

void launch_probe_rd(const ProbeArgs& a, unsigned long long* sse, int n, hipStream_t s) {
    const int tb = n == 4 ? ProbeGeo<4>::TB : ProbeGeo<8>::TB;
    const uint64_t total = uint64_t((a.bx * a.by + tb - 1) / tb) * uint64_t(a.nframes);
    // persistent workgroups, as above; 8x8 holds P and R in LDS (64 KiB + pixels + candidates: two
    // workgroups per CU), so 512 of them are all resident at once
    const uint64_t cap = uint64_t(probe_rd_max_workgroups(n));
    const unsigned grid = unsigned(total < cap ? total : cap);
    if (n == 4) {
        hipLaunchKernelGGL((probe_kernel<4, true>), dim3(grid), dim3(kTPB), ProbeGeo<4>::lds_bytes(a.nq, true), s, a, sse);
    } else {
        // more than the 64 KiB a launch may ask for by default (a refusal shows as the launch's error)
        const size_t lds = ProbeGeo<8>::lds_bytes(a.nq, true);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&probe_kernel<8, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        hipLaunchKernelGGL((probe_kernel<8, true>), dim3(grid), dim3(kTPB), lds, s, a, sse);
    }
}

}  // namespace ie
