// imageencoder_amd/csrc/ie_tables.cpp -- the per-matrix tables (ie::EncTables) and the tracked
// transform that bounds the FP32 fast path's error.  A pure host function of (n, q): nothing
// here touches the device, so it links and runs alone (tests/cpp/tables_host.cpp).
#include <cmath>

#include "ie_ctx.hpp"

namespace {

// ---- rigorous error bound of the FP32 fast path -----------------------------------------
// Trk = an exact real affine form c0 + sum_k a_k x_k of the block's RAW pixels x_k in [0, 255]
// plus a bound E on the FP32 rounding error accumulated so far.  TrkOp mirrors every operation
// of the quotient transforms in ie_dct.h: the real coefficients follow the FP32 constants
// exactly; each rounded operation adds u*(|result| + E) with |result| <= |c0 + 127.5 sum a| +
// 127.5 sum|a| (the box bound).  Results that are integers below 2^24 are exact (integ), and so
// is a product of an exact value by a power of two.
struct Trk {
    double a[64];
    double c0;
    double E;
    bool integ;
};

struct TrkOp {
    int nn;
    static constexpr double u = 1.0 / 16777216.0;  // 2^-24
    double mag(const Trk& t) const {
        double s = 0, m = 0;
        for (int k = 0; k < nn; k++) {
            s += t.a[k];
            m += std::fabs(t.a[k]);
        }
        return std::fabs(t.c0 + 127.5 * s) + 127.5 * m;
    }
    static bool is_int(double c) { return c == std::rint(c); }
    static bool is_pow2(double c) {
        int e = 0;
        return c != 0.0 && std::fabs(std::frexp(c, &e)) == 0.5;
    }
    Trk lin(const Trk& x, double cx, const Trk* y, double cy, double cadd, double Ein, bool integ, bool exact) const {
        Trk r;
        for (int k = 0; k < nn; k++) r.a[k] = cx * x.a[k] + (y ? cy * y->a[k] : 0.0);
        for (int k = nn; k < 64; k++) r.a[k] = 0.0;
        r.c0 = cx * x.c0 + (y ? cy * y->c0 : 0.0) + cadd;
        const double m = mag(r);
        r.integ = integ && m < 16777216.0;
        r.E = Ein + ((r.integ || exact) ? 0.0 : u * (m + Ein));
        return r;
    }
    Trk add(const Trk& x, const Trk& y) const { return lin(x, 1, &y, 1, 0, x.E + y.E, x.integ && y.integ, false); }
    Trk sub(const Trk& x, const Trk& y) const { return lin(x, 1, &y, -1, 0, x.E + y.E, x.integ && y.integ, false); }
    Trk mul(const Trk& x, float c) const {
        const bool exact = x.E == 0.0 && is_pow2(double(c));
        return lin(x, double(c), nullptr, 0, 0, std::fabs(double(c)) * x.E, x.integ && is_int(c), exact);
    }
    Trk fma(const Trk& x, float c, const Trk& y) const {
        return lin(x, double(c), &y, 1, 0, std::fabs(double(c)) * x.E + y.E, x.integ && y.integ && is_int(c), false);
    }
    Trk fms(const Trk& x, float c, const Trk& y) const {
        return lin(x, double(c), &y, -1, 0, std::fabs(double(c)) * x.E + y.E, x.integ && y.integ && is_int(c), false);
    }
    Trk addc(const Trk& x, float c) const { return lin(x, 1, nullptr, 0, double(c), x.E, x.integ && is_int(c), false); }
    // x * c + k (one rounding, constant k)
    Trk fmac(const Trk& x, float c, float k) const {
        return lin(x, double(c), nullptr, 0, double(k), std::fabs(double(c)) * x.E, x.integ && is_int(c) && is_int(k), false);
    }
};

inline double Cf(int i) { return i == 0 ? 0.5 : M_SQRT1_2; }  // algo.cpp:294-297

}  // namespace

namespace iec {

// Build the per-matrix tables.  The cos values are the reference's own expression evaluated with
// the host libm (algo.cpp:312,318-319); P, S and R are the double products it forms.  For the
// FP32 path, the tracked run of the kernel's quotient transform (quot4 / quot8 in ie_dct.h) on
// raw pixels gives per coefficient k the real affine map the FP32 code implements and its
// rounding bound E_k.  With alpha*_k the reference's map (S*P/q on centred pixels) the FP32
// quotient is within
//     bound_k = E_k + 128 * sum|alpha_k - alpha*_k| + |value of our map at x = 128| + 1e-9
// of the reference's FP64 quotient (1e-9 covers the reference's own FP64 rounding, <= 1e-10);
// |t32 - rint(t32)| >= 0.5 - 2*bound_k flags a possible tie.  Returns false if alpha deviates
// from alpha* beyond FP32 constant rounding (a transform bug).
bool build_tables(int n, const uint16_t* q, ie::EncTables* T) {
    const int nn = n * n;
    std::memset(T, 0, sizeof(*T));
    const double factor = M_PI_2 / double(n);
    for (int u = 0; u < n; u++)
        for (int i = 0; i < n; i++) T->c[u * n + i] = std::cos(double(2.0 * i + 1.0) * double(u) * factor);
    std::vector<double> sq(nn);
    for (int u = 0; u < n; u++)
        for (int v = 0; v < n; v++) {
            const int k = u * n + v;
            T->S[k] = Cf(u) * Cf(v);
            T->qd[k] = double(q[k]);
            int e2 = 0;
            T->rq[k] = (std::frexp(double(q[k]), &e2) == 0.5) ? 1.0 / double(q[k]) : 0.0;
            sq[k] = T->S[k] / T->qd[k];
            T->g[k] = float(sq[k]);
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++) {
                    T->P[k * nn + i * n + j] = T->c[u * n + i] * T->c[v * n + j];
                    T->R[k * nn + i * n + j] = Cf(u) * Cf(v) * T->c[u * n + i] * T->c[v * n + j];
                }
        }
    for (int k = 0; k < nn; k++) T->cf[k] = float(T->c[k]);
    for (int k = 0; k <= 8; k++) T->dct.K[k] = float(std::cos(double(k) * M_PI / 16.0));
    // 4x4 plan: K2 = cos(pi/8), K4 = cos(pi/4), K6 = cos(3pi/8); row outputs R1, R3 carry 1/K2
    {
        const double K2 = std::cos(M_PI / 8.0), K4 = std::cos(M_PI / 4.0), K6 = std::cos(3.0 * M_PI / 8.0);
        T->plan4.r = float(K6 / K2);
        if (n == 4) {
            for (int v = 0; v < 4; v++) {
                const double Kv = (v == 0) ? 1.0 : (v == 2) ? K4 : K2;
                float* G = T->plan4.col[v];
                G[0] = float(Kv * sq[0 * 4 + v]);
                G[1] = float(K4 * Kv * sq[2 * 4 + v]);
                G[2] = float(K2 * Kv * sq[1 * 4 + v]);
                G[3] = float(K6 * Kv * sq[1 * 4 + v]);
                G[4] = float(K6 * Kv * sq[3 * 4 + v]);
                G[5] = float(-K2 * Kv * sq[3 * 4 + v]);
            }
        }
    }

    // 4x4 matrix-pipe plan (quot4j): G[k][m] = S/q * the row and column basis factors of term m
    if (n == 4) {
        const double K2 = std::cos(M_PI / 8.0), K4 = std::cos(M_PI / 4.0), K6 = std::cos(3.0 * M_PI / 8.0);
        auto f = [&](int u, int m) -> double {  // factor of basis dct4j_b(u, m) in 1-D row u
            if (u == 0) return 1.0;
            if (u == 2) return K4;
            if (u == 1) return m == 0 ? K2 : K6;
            return m == 0 ? K6 : -K2;
        };
        for (int u = 0; u < 4; u++)
            for (int v = 0; v < 4; v++) {
                int m = 0;
                for (int a = 0; a < ie::dct4j_nb(u); a++)
                    for (int bb = 0; bb < ie::dct4j_nb(v); bb++) T->plan4j.G[4 * u + v][m++] = float(sq[4 * u + v] * f(u, a) * f(v, bb));
            }
        static const int B[4][4] = {{1, 1, 1, 1}, {1, -1, -1, 1}, {1, 0, 0, -1}, {0, 1, -1, 0}};
        for (int l = 0; l < 64; l++) {
            const int r = l & 31, h = l >> 5, rho = (r & 3) + 4 * (r >> 3), hr = (r >> 2) & 1;
            for (int w = 0; w < 4; w++) T->mfma_w[l][w] = 0u;
            if (h != hr) continue;
            for (int j = 0; j < 16; j++) {
                const int c = B[rho >> 2][j >> 2] * B[rho & 3][j & 3];
                T->mfma_w[l][j >> 2] |= uint32_t(uint8_t(int8_t(c))) << (8 * (j & 3));
            }
        }
    }

    // tracked run of the kernel's transform on raw pixels
    std::vector<Trk> b(nn);
    for (int k = 0; k < nn; k++) {
        for (int m = 0; m < 64; m++) b[k].a[m] = (m == k) ? 1.0 : 0.0;
        b[k].c0 = 0.0;
        b[k].E = 0.0;
        b[k].integ = true;
    }
    TrkOp op{nn};
    // the matrix-pipe form: the sixteen J exact (pixels - 128), then quot4j's FP32 stage
    std::vector<Trk> bj(nn), bh(nn);
    if (n == 4) {
        std::vector<Trk> xs(b), J(nn);
        for (int k = 0; k < nn; k++) xs[k].c0 = -128.0;
        ie::dct4j_ints(xs.data(), J.data(), op);
        for (int k = 0; k < nn; k++)
            if (!J[k].integ || J[k].E != 0.0) return false;  // the integer stage must be exact
        ie::quot4j(J.data(), bj.data(), T->plan4j, op);
        ie::quot4j<true>(J.data(), bh.data(), T->plan4j, op);
    }
    if (n == 4) ie::quot4(b.data(), T->plan4, op);
    else ie::quot8(b.data(), T->dct, T->g, op);
    // Largest record: |Q_k| <= 128 * sum_ij |S_k P_k[ij]| / q_k (|x| <= 128), so bl <= the widest
    // bits_needed over k (utils.hpp:226-243; int16 caps it at 16) and >= ffs(N*N) (the L field);
    // an RLE record is 4 + bl * (1 + N*N) bits at most (Block.cpp:372-413).
    {
        int bl = 32 - __builtin_clz(unsigned(nn));
        for (int k = 0; k < nn; k++) {
            double m = 0.0;
            for (int ij = 0; ij < nn; ij++) m += std::fabs(T->S[k] * T->P[k * nn + ij]);
            const double qmax = std::ceil(128.0 * m / T->qd[k]) + 1.0;
            const int b = (qmax >= 32768.0) ? 16 : std::min(16, (32 - __builtin_clz(unsigned(qmax))) + 1);
            bl = std::max(bl, b);
        }
        T->rec_bits = 4 + bl * (1 + nn);
    }
    if (n == 4) {  // every coefficient's FP64 row and its S, rq, qd, contiguous (encode4p_kernel's DMA)
        for (int i = 0; i < nn * nn; i++) T->rows4[i] = T->P[i];
        for (int k = 0; k < nn; k++) {
            T->rows4[nn * nn + k] = T->S[k];
            T->rows4[nn * nn + nn + k] = T->rq[k];
            T->rows4[nn * nn + 2 * nn + k] = T->qd[k];
        }
    }
    {  // the fix-up's structural rows, contiguous (encode_kernel copies them to LDS)
        const int h = n / 2, ks[3] = {h, h * n, h * n + h};
        for (int si = 0; si < 3; si++) {
            for (int ij = 0; ij < nn; ij++) T->srow[si * nn + ij] = T->P[ks[si] * nn + ij];
            T->srow[3 * nn + si] = T->S[ks[si]];
            T->srow[3 * nn + 3 + si] = T->rq[ks[si]];
            T->srow[3 * nn + 6 + si] = T->qd[ks[si]];
        }
    }
    bool ok = true;
    // per coefficient of one tracked transform: its tie limit (lim), the bound (thr), whether the
    // DC quotient is exact, and the loosest limit of the non-structural coefficients (lim_min)
    auto limits = [&](const std::vector<Trk>& tv, float* lim, float* thr, float* lim_min, int* dc_exact, float g0) {
        *dc_exact = 0;
        *lim_min = 0.5f;
        for (int k = 0; k < nn; k++) {
            const Trk& t = tv[k];
            double dev = 0.0, amax = 0.0, sa = 0.0;
            for (int m = 0; m < nn; m++) {
                const double ref = sq[k] * T->P[k * nn + m];
                dev += std::fabs(t.a[m] - ref);
                amax = std::max(amax, std::fabs(ref));
                sa += t.a[m];
            }
            if (dev > 1e-5 * (amax + 1e-30) * nn) ok = false;  // FP32 constants differ by ~1e-7 relative
            const double bound = t.E + 128.0 * dev + std::fabs(t.c0 + 128.0 * sa) + 1e-9;
            // coefficient 0: an integer sum (minus 128*N*N) scaled by a power of two is exact in FP32,
            // and the reference computes it exactly too (c[0][*] = 1, C(0)^2 = 1/4, q a power of two)
            if (k == 0 && t.E == 0.0 && double(g0) == sq[0] && TrkOp::is_pow2(sq[0])) {
                if (thr) thr[k] = -1.0f;
                lim[k] = 1.0f;  // never flagged
                *dc_exact = 1;
            } else {
                if (thr) thr[k] = float(2.0 * bound);
                lim[k] = float(0.5 - 2.0 * bound);
                // the structural coefficients (0,N/2), (N/2,0), (N/2,N/2) are flagged one by one
                const int h = n / 2;
                const bool structural = (k == h) || (k == h * n) || (k == h * n + h);
                if (!structural) *lim_min = std::min(*lim_min, lim[k]);
            }
        }
    };
    limits(b, T->lim, T->thr, &T->lim_min, &T->dc_exact, T->g[0]);
    if (n == 4) limits(bj, T->lim4j, nullptr, &T->lim_min4j, &T->dc_exact4j, T->plan4j.G[0][0]);
    if (n == 4) {  // t + 1/2: the tie test on fract(t + 1/2), limits rounded outward
        T->dc_exact4h = 0;
        T->dlo_max4h = 0.0f;
        T->dhi_min4h = 1.0f;
        for (int k = 0; k < nn; k++) {
            const Trk& t = bh[k];
            double dev = 0.0, sa = 0.0;
            for (int m = 0; m < nn; m++) {
                dev += std::fabs(t.a[m] - sq[k] * T->P[k * nn + m]);
                sa += t.a[m];
            }
            // (the map's value at x = 128 is the 1/2 itself)
            const double bound = t.E + 128.0 * dev + std::fabs(t.c0 + 128.0 * sa - 0.5) + 1e-9;
            // DC: exact in quot4j (dc_exact4j) stays exact with the 1/2 added (J0 * G (a power of two)
            // has at most 12 significant bits; the tracked fmac does not see that)
            if (k == 0 && T->dc_exact4j) {
                T->dlo4h[k] = -1.0f;  // never flagged
                T->dhi4h[k] = 2.0f;
                T->dc_exact4h = 1;
                continue;
            }
            const double d = 2.0 * bound;
            T->dlo4h[k] = std::nextafter(float(d), 1.0f);          // >= d
            T->dhi4h[k] = std::nextafter(float(1.0 - d), 0.0f);    // <= 1 - d
            const int h = n / 2;
            const bool structural = (k == h) || (k == h * n) || (k == h * n + h);
            if (!structural) {
                T->dlo_max4h = std::max(T->dlo_max4h, T->dlo4h[k]);
                T->dhi_min4h = std::min(T->dhi_min4h, T->dhi4h[k]);
            }
        }
    }
    return ok;
}

}  // namespace iec
