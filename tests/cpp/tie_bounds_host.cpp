// tests/cpp/tie_bounds_host.cpp -- the per-matrix tie limits of ie_tables.cpp checked against the
// reference's FP64 quotient, on the host alone (no device, no library).
// usage: tie_bounds_host MATRIX_FILE N BLOCKS SEED OUT_PREFIX [TIE_BLOCKS_FILE]
//
// It builds the tables, then runs the templates the kernels instantiate (quot4, quot8, dct4j_ints +
// quot4j, quot4j<true>; ie_dct.h) through HostFloatOp, the host twin of the device-only FloatOp
// (plain float + - * and __builtin_fmaf; the file is compiled with -ffp-contract=off), over BLOCKS
// seeded blocks -- uniform noise, 0/255 noise, low-amplitude noise around a random level -- and the
// N*N-byte blocks of TIE_BLOCKS_FILE.  For every coefficient it forms the reference's FP64 quotient
// from the tables' own P, S and qd in the reference's order (Block.cpp:139-153, algo.cpp:309-331)
// and checks, per variant:
//   bound     |t32 - t64| <= the bound the tables claim (thr/2; (1/2 - lim4j)/2, plus the 2^-27 that
//             rounding lim4j to a float can hide; the tighter of dlo4h and 1 - dhi4h, halved); a
//             dc_exact* coefficient matches exactly
//   decision  where the kernel's flag rule (ie_encode_blocks.h: the rounding residual against lim,
//             lim4j; fract(t + 1/2) against dlo4h/dhi4h) does not flag a coefficient, the FP32
//             rounding equals std::round of the FP64 quotient
//   size      the block's record, bl and Lw as the reference sizes them (Block.cpp:186-232,
//             372-413), is at most rec_bits
// It prints "ratio VARIANT X", the largest |t32 - t64| / bound seen, and writes the first blocks of
// every kind with their FP64-rounded coefficients to OUT_PREFIX.pix (bytes) and OUT_PREFIX.coef
// (int16, natural order), which tests/test_tie_bounds_host.py compares with the oracle.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "ie_ctx.hpp"

namespace {

struct HostFloatOp {
    float add(float a, float b) const { return a + b; }
    float sub(float a, float b) const { return a - b; }
    float mul(float a, float c) const { return a * c; }
    float fma(float a, float c, float b) const { return __builtin_fmaf(a, c, b); }
    float fms(float a, float c, float b) const { return __builtin_fmaf(a, c, -b); }
    float addc(float a, float c) const { return a + c; }
    float fmac(float a, float c, float k) const { return __builtin_fmaf(a, c, k); }
};
struct IntOp {
    int add(int a, int b) const { return a + b; }
    int sub(int a, int b) const { return a - b; }
};

constexpr float kMagic = 12582912.0f;  // 1.5 * 2^23 (ie_encode_blocks.h)
constexpr int kDump = 1024;            // blocks of every kind written for the oracle comparison

uint64_t rng_state;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return uint32_t((z ^ (z >> 31)) >> 32);
}

// utils.hpp:226-243
int bits_needed(int16_t value) {
    int bits = 1;
    while (int16_t(int16_t((value & ((1 << bits) - 1)) << (16 - bits)) >> (16 - bits)) != value) bits++;
    return bits;
}

struct Variant {
    const char* name;
    double ratio = 0.0;
    long flagged = 0;
};

const char* g_matrix;
[[noreturn]] void fail(const Variant& v, const char* what, int k, const char* kind, long b, const uint8_t* px, int nn,
                       double t32, double t64, double bound) {
    std::fprintf(stderr, "%s: %s FAILED for variant %s, coefficient %d, %s block %ld: t32 = %.9g, t64 = %.17g, bound = %.6g, "
                         "largest error/bound so far %.4f\npixels:",
                 g_matrix, what, v.name, k, kind, b, t32, t64, bound, v.ratio);
    for (int i = 0; i < nn; i++) std::fprintf(stderr, " %d", px[i]);
    std::fprintf(stderr, "\n");
    std::exit(1);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6 && argc != 7) return 2;
    g_matrix = argv[1];
    const int n = std::atoi(argv[2]);
    const long blocks = std::atol(argv[3]);
    rng_state = std::strtoull(argv[4], nullptr, 10);
    const std::string prefix = argv[5];
    if ((n != 4 && n != 8) || blocks < 3) return 2;
    const int nn = n * n;
    std::vector<uint16_t> q;
    {
        FILE* f = std::fopen(argv[1], "r");
        if (!f) return 2;
        for (unsigned v; std::fscanf(f, "%u", &v) == 1;) q.push_back(uint16_t(v));
        std::fclose(f);
        if (int(q.size()) != nn) return 2;
    }
    std::vector<uint8_t> ties;
    if (argc == 7) {
        FILE* f = std::fopen(argv[6], "rb");
        if (!f) return 2;
        uint8_t buf[4096];
        for (size_t r; (r = std::fread(buf, 1, sizeof(buf), f)) > 0;) ties.insert(ties.end(), buf, buf + r);
        std::fclose(f);
        if (ties.size() % size_t(nn)) return 2;
    }
    auto T = std::make_unique<ie::EncTables>();
    if (!iec::build_tables(n, q.data(), T.get())) {
        std::fprintf(stderr, "%s: build_tables rejects the matrix\n", argv[1]);
        return 1;
    }
    // zig-zag order: (x, y) sorted by (x + y, (x - y) odd ? y : x)  (algo.cpp:33-37, 68-87)
    std::vector<int> zz(nn);
    for (int i = 0; i < nn; i++) zz[i] = i;
    auto key = [n](int i) {
        const int x = i % n, y = i / n;
        return std::make_pair(x + y, ((x - y) & 1) ? y : x);
    };
    std::sort(zz.begin(), zz.end(), [&](int a, int b) { return key(a) < key(b); });

    FILE* fpix = std::fopen((prefix + ".pix").c_str(), "wb");
    FILE* fcoef = std::fopen((prefix + ".coef").c_str(), "wb");
    if (!fpix || !fcoef) return 2;

    Variant v32{n == 4 ? "quot4" : "quot8"}, v4j{"quot4j"}, v4h{"quot4j<true>"};
    const char* kinds[4] = {"uniform", "0/255", "low-amplitude", "tie"};
    const long per = (blocks + 2) / 3;
    int rec_max = 0;
    for (int kind = 0; kind < 4; kind++) {
        const long count = (kind < 3) ? per : long(ties.size() / size_t(nn));
        for (long b = 0; b < count; b++) {
            uint8_t px[64];
            if (kind == 0) {
                for (int i = 0; i < nn; i++) px[i] = uint8_t(rnd());
            } else if (kind == 1) {
                for (int i = 0; i < nn; i++) px[i] = (rnd() & 1) ? 255 : 0;
            } else if (kind == 2) {
                const int level = int(rnd() % 256), amp = 1 + int(rnd() % 4);
                for (int i = 0; i < nn; i++) px[i] = uint8_t(std::clamp(level + int(rnd() % (2 * amp + 1)) - amp, 0, 255));
            } else {
                for (int i = 0; i < nn; i++) px[i] = ties[size_t(b) * nn + i];
            }
            // the reference: acc = acc + P * x in row-major order, D = acc * S, round(D / q)
            double t64[64];
            int16_t ref[64];
            for (int k = 0; k < nn; k++) {
                double acc = 0.0;
                for (int ij = 0; ij < nn; ij++) acc = acc + T->P[k * nn + ij] * (double(px[ij]) + double(-128));
                const double D = acc * T->S[k];
                t64[k] = D / T->qd[k];
                ref[k] = int16_t(std::round(t64[k]));
            }
            if (b < kDump || kind == 3) {
                std::fwrite(px, 1, nn, fpix);
                std::fwrite(ref, sizeof(int16_t), nn, fcoef);
            }
            // size (createRLESequence + streamEncoded): with RLE 4 + bl + bl * Lw, without 4 + bl * N*N
            {
                int L = 0, maxbits = 0;
                for (int k = 0; k < nn; k++)
                    if (ref[zz[k]] != 0) {
                        L = k + 1;
                        maxbits = std::max(maxbits, bits_needed(ref[zz[k]]));
                    }
                const int bl = std::max(maxbits, L == 0 ? 1 : 32 - __builtin_clz(unsigned(L)));
                int lw = L;
                if (L == nn && ref[zz[nn - 2]] == 0) {
                    lw = 0;
                    for (int k = 0; k < nn - 1; k++)
                        if (ref[zz[k]] != 0) lw = k + 1;
                }
                const int rec = std::max(4 + bl + bl * lw, 4 + bl * nn);
                rec_max = std::max(rec_max, rec);
                if (rec > T->rec_bits) {
                    std::fprintf(stderr, "%s: size FAILED, %s block %ld: record of %d bits (bl %d, Lw %d) > rec_bits %d\n", argv[1],
                                 kinds[kind], b, rec, bl, lw, T->rec_bits);
                    return 1;
                }
            }
            // residual rule of round_block / round_block_mask / fix_block / round_block_lean4j
            auto residual_rule = [&](Variant& v, const float* t, const float* lim, const double* bound2, bool dcx) {
                for (int k = 0; k < nn; k++) {
                    const double err = std::fabs(double(t[k]) - t64[k]);
                    if (k == 0 && dcx) {
                        if (double(t[0]) != t64[0]) fail(v, "exactness", 0, kinds[kind], b, px, nn, t[0], t64[0], 0.0);
                        const int got = int(std::trunc(t[0] + std::copysign(0.5f, t[0])));
                        if (int16_t(got) != ref[0]) fail(v, "decision", 0, kinds[kind], b, px, nn, t[0], t64[0], 0.0);
                        continue;
                    }
                    const double bound = bound2[k] / 2.0;
                    v.ratio = std::max(v.ratio, err / bound);
                    if (err > bound) fail(v, "bound", k, kinds[kind], b, px, nn, t[k], t64[k], bound);
                    const float y = t[k] + kMagic;
                    const float e = std::fabs(t[k] - (y - kMagic));
                    if (e >= lim[k]) {
                        v.flagged++;
                        continue;
                    }
                    uint32_t yb;
                    std::memcpy(&yb, &y, 4);
                    if (int16_t(yb & 0xFFFFu) != ref[k]) fail(v, "decision", k, kinds[kind], b, px, nn, t[k], t64[k], bound);
                }
            };
            float x[64];
            for (int i = 0; i < nn; i++) x[i] = float(px[i]);
            if (n == 4) ie::quot4(x, T->plan4, HostFloatOp());
            else ie::quot8(x, T->dct, T->g, HostFloatOp());
            double b2[64];
            for (int k = 0; k < nn; k++) b2[k] = double(T->thr[k]);
            residual_rule(v32, x, T->lim, b2, T->dc_exact != 0);
            if (n == 4) {
                int xi[16], Ji[16];
                for (int i = 0; i < 16; i++) xi[i] = int(px[i]) - 128;
                ie::dct4j_ints(xi, Ji, IntOp());
                float Jf[16], t[16], th[16];
                for (int i = 0; i < 16; i++) Jf[i] = float(Ji[i]);
                ie::quot4j(Jf, t, T->plan4j, HostFloatOp());
                // lim4j is 1/2 - 2 * bound rounded to the nearest float, which gives 2 * bound back only to
                // half an ulp of the binade below 1/2 (2^-26): a bound below that rounds lim4j to 1/2 itself
                for (int k = 0; k < 16; k++) b2[k] = (0.5 - double(T->lim4j[k])) + 0x1p-26;
                residual_rule(v4j, t, T->lim4j, b2, T->dc_exact4j != 0);
                // t + 1/2: floor is the rounding, fract at or outside (dlo4h, dhi4h) the flag
                ie::quot4j<true>(Jf, th, T->plan4j, HostFloatOp());
                for (int k = 0; k < 16; k++) {
                    const double err = std::fabs((double(th[k]) - 0.5) - t64[k]);
                    if (k == 0 && T->dc_exact4h) {
                        if (err != 0.0) fail(v4h, "exactness", 0, kinds[kind], b, px, nn, th[0], t64[0], 0.0);
                        continue;
                    }
                    const double bound = double(std::min(T->dlo4h[k], 1.0f - T->dhi4h[k])) / 2.0;
                    v4h.ratio = std::max(v4h.ratio, err / bound);
                    if (err > bound) fail(v4h, "bound", k, kinds[kind], b, px, nn, th[k], t64[k], bound);
                    const float fl = std::floor(th[k]), fr = th[k] - fl;
                    if (fr <= T->dlo4h[k] || fr >= T->dhi4h[k]) {
                        v4h.flagged++;
                        continue;
                    }
                    if (int16_t(int(fl)) != ref[k]) fail(v4h, "decision", k, kinds[kind], b, px, nn, th[k], t64[k], bound);
                }
            }
        }
    }
    std::fclose(fpix);
    std::fclose(fcoef);
    std::printf("blocks %ld\nrec_bits %d %d\n", 3 * per + long(ties.size() / size_t(nn)), rec_max, T->rec_bits);
    std::printf("ratio %s %.6f\nflagged %s %ld\n", v32.name, v32.ratio, v32.name, v32.flagged);
    if (n == 4) {
        std::printf("ratio %s %.6f\nflagged %s %ld\n", v4j.name, v4j.ratio, v4j.name, v4j.flagged);
        std::printf("ratio %s %.6f\nflagged %s %ld\n", v4h.name, v4h.ratio, v4h.name, v4h.flagged);
    }
    return 0;
}
