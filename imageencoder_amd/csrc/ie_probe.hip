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
// columns), then the tile's pixel words [NN/4][TB], then the candidates [nq][NN] uint16 (zig-zag order).
template <int N> struct ProbeGeo {
    static constexpr int NN = N * N;
    static constexpr int BPW = 64 / NN;                              // blocks per wave and step
    static constexpr int TB = kProbeWaves * kProbeSteps * BPW;       // blocks per tile
    static constexpr int P_DOUBLES = NN * NN;
    static constexpr int PIX_WORDS = (NN / 4) * TB;
    static constexpr size_t lds_bytes(int nq) {
        return size_t(P_DOUBLES) * 8 + size_t(PIX_WORDS) * 4 + ((size_t(nq) * NN * 2 + 7) & ~size_t(7));
    }
};

template <int N>
__global__ __launch_bounds__(kTPB) void probe_sizes_kernel(ProbeArgs a) {
    using G = ProbeGeo<N>;
    constexpr int NN = G::NN, BPW = G::BPW, TB = G::TB;
    extern __shared__ __attribute__((aligned(16))) unsigned char probe_lds[];
    double* Pt = reinterpret_cast<double*>(probe_lds);                        // [ij][kz]
    uint32_t* pixw = reinterpret_cast<uint32_t*>(Pt + G::P_DOUBLES);          // [word][block of the tile]
    uint16_t* qz = reinterpret_cast<uint16_t*>(pixw + G::PIX_WORDS);          // [m][kz]

    const int tid = int(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int kz = lane % NN, g = lane / NN;     // zig-zag position, block of the step
    const int k = probe_zz<N>(kz);               // natural index

    for (int e = tid; e < NN * NN; e += kTPB) {  // Pt[ij][z] = P[zz(z)][ij]
        const int ij = e / NN, z = e % NN;
        Pt[e] = a.tab->P[probe_zz<N>(z) * NN + ij];
    }
    for (int e = tid; e < a.nq * NN; e += kTPB) qz[e] = a.q[e];
    const double S = a.tab->S[k];

    const int nblk = a.bx * a.by;
    const uint64_t tpf = uint64_t((nblk + TB - 1) / TB);
    const uint64_t total = tpf * uint64_t(a.nframes);
    uint32_t mine = 0;  // lane m: candidate m's bits of frame cur_f so far (this wave)
    int64_t cur_f = -1;
    const bool owner = kz == NN - 1;  // the block's last lane holds its DPP results

    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const int64_t f = int64_t(it / tpf);
        const int b0 = int(it % tpf) * TB;
        if (f != cur_f) {
            if (cur_f >= 0 && lane < a.nq)
                atomicAdd(&a.bits[uint64_t(lane) * uint64_t(a.nframes) + uint64_t(cur_f)], (unsigned long long)mine);
            mine = 0;
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
#pragma unroll 1
            for (int m = 0; m < a.nq; m++) {
                const double t = D / double(qz[m * NN + kz]);  // IEEE division (Block.cpp:149-152)
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
            }
        }
    }
    if (cur_f >= 0 && lane < a.nq)
        atomicAdd(&a.bits[uint64_t(lane) * uint64_t(a.nframes) + uint64_t(cur_f)], (unsigned long long)mine);
}

}  // namespace

void launch_probe_sizes(const ProbeArgs& a, int n, hipStream_t s) {
    const int tb = n == 4 ? ProbeGeo<4>::TB : ProbeGeo<8>::TB;
    const uint64_t total = uint64_t((a.bx * a.by + tb - 1) / tb) * uint64_t(a.nframes);
    const unsigned grid = unsigned(total < 1024 ? total : 1024);  // persistent workgroups: the tables are staged once each
    if (n == 4)
        hipLaunchKernelGGL(probe_sizes_kernel<4>, dim3(grid), dim3(kTPB), ProbeGeo<4>::lds_bytes(a.nq), s, a);
    else
        hipLaunchKernelGGL(probe_sizes_kernel<8>, dim3(grid), dim3(kTPB), ProbeGeo<8>::lds_bytes(a.nq), s, a);
}

}  // namespace ie
