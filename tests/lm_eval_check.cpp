// Stand-alone memory-safety check of the host LM's residual evaluation
// (madpose_amd/csrc/host/lm_eval.inc through lm_eval_range_w4, and lm_eval_range_w8 when
// built with -DLM_EVAL_CHECK_W8 on a CPU with AVX-512): every array -- the coordinates, the
// depths and the three index lists -- lives on the heap at exactly its needed length, the
// ranges [b0, b1) end at every residue of the vector width and lists of length 0 and 1 are
// included, so a tail load past an index list or a coordinate array is an
// AddressSanitizer report.  The evaluation of a range must also equal the sum of the
// evaluations of its single blocks up to the rounding of the two summation orders, and a
// block range past the lists must leave the accumulators untouched.  Built with -fsanitize=address,undefined and run as a
// program by tests/test_lm_system_cpu.py.  Prints "ok" and returns 0, or says what failed
// and returns 1.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "lm_eval.h"

using namespace mp;

#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

static unsigned long long g_x = 0x9E3779B97F4A7C15ull;
static double uniform() {
    g_x ^= g_x << 13;
    g_x ^= g_x >> 7;
    g_x ^= g_x << 17;
    return (double)(g_x >> 11) / 9007199254740992.0;
}

typedef void (*EvalFn)(const LmEvalIn &, const LmEvalParams &, bool, size_t, size_t, double *, double *, double *);

struct Sys {
    double H[kNPack], g[kNFull], cost;
    void clear() { std::memset(this, 0, sizeof(*this)); }
};

// a list of exactly `len` ints on the heap (len 0: a zero-length allocation)
static std::unique_ptr<int[]> make_list(size_t len, int n, int first) {
    std::unique_ptr<int[]> p(new int[len]);
    for (size_t k = 0; k < len; ++k) p[k] = (first + 7 * (int)k) % n;
    return p;
}

static void run(EvalFn eval, int variant) {
    // the pair: n correspondences, arrays of exactly 2n / n doubles; some lists end on
    // the last correspondence
    const int n = 23;
    std::unique_ptr<double[]> x0(new double[2 * n]), x1(new double[2 * n]), d0(new double[n]), d1(new double[n]);
    for (int i = 0; i < n; ++i) {
        const double s = variant == 0 ? 500.0 : 1.0, c = variant == 0 ? 300.0 : 0.0;
        x0[2 * i] = c + s * (uniform() - 0.5);
        x0[2 * i + 1] = c + s * (uniform() - 0.5);
        x1[2 * i] = c + s * (uniform() - 0.5);
        x1[2 * i + 1] = c + s * (uniform() - 0.5);
        d0[i] = 2.0 + 3.0 * uniform();
        d1[i] = 2.0 + 3.0 * uniform();
    }
    const double f = variant == 0 ? 500.0 : 1.0, pp = variant == 0 ? 300.0 : 0.0;
    std::unique_ptr<double[]> K(new double[9]), Ki(new double[9]);
    const double Kv[9] = {f, 0, pp, 0, f, pp, 0, 0, 1}, Kiv[9] = {1 / f, 0, -pp / f, 0, 1 / f, -pp / f, 0, 0, 1};
    std::memcpy(K.get(), Kv, sizeof(Kv));
    std::memcpy(Ki.get(), Kiv, sizeof(Kiv));
    LmEvalParams p;
    const double c5 = std::cos(0.05), s5 = std::sin(0.05);
    const double R[9] = {c5, -s5, 0, s5, c5, 0, 0, 0, 1};
    std::memcpy(p.R, R, sizeof(R));
    p.t[0] = 0.1;
    p.t[1] = -0.05;
    p.t[2] = 0.2;
    p.s = 1.1;
    p.o0 = 0.05;
    p.o1 = -0.03;
    p.f0 = 1.2;
    p.f1 = 1.1;
    const size_t lens[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17};
    const size_t nl = sizeof(lens) / sizeof(lens[0]);
    size_t calls = 0;
    for (size_t i0 = 0; i0 < nl; ++i0)
        for (size_t i1 = 0; i1 < nl; i1 += 2)
            for (size_t i2 = (i0 + i1) % 3; i2 < nl; i2 += 3) {
                const size_t n0 = lens[i0], n1 = lens[i1], n2 = lens[i2], nb = n0 + n1 + n2;
                auto s0 = make_list(n0, n, n - 1), s1 = make_list(n1, n, 3), s2 = make_list(n2, n, n - 2);
                LmEvalIn E;
                E.variant = variant;
                E.x0 = x0.get();
                E.x1 = x1.get();
                E.d0 = d0.get();
                E.d1 = d1.get();
                E.K0 = E.K1 = K.get();
                E.K0i = E.K1i = Ki.get();
                E.s0 = s0.get();
                E.s1 = s1.get();
                E.s2 = s2.get();
                E.n0 = n0;
                E.n1 = n1;
                E.n2 = n2;
                E.w_sampson = 2.5;
                // every block alone, with and without the Jacobian
                std::unique_ptr<Sys[]> one(new Sys[nb + 1]);
                for (size_t b = 0; b < nb; ++b) {
                    one[b].clear();
                    eval(E, p, true, b, b + 1, one[b].H, one[b].g, &one[b].cost);
                    Sys c;
                    c.clear();
                    eval(E, p, false, b, b + 1, c.H, c.g, &c.cost);
                    CHECK(std::isfinite(one[b].cost) && c.cost == one[b].cost);
                    for (int q = 0; q < kNPack; ++q) CHECK(c.H[q] == 0.0);
                    calls += 2;
                }
                // every range [b0, b1): ends at every residue of the width, across the lists
                for (size_t b0 = 0; b0 <= nb; ++b0)
                    for (size_t b1 = b0; b1 <= nb; ++b1) {
                        Sys a;
                        a.clear();
                        eval(E, p, true, b0, b1, a.H, a.g, &a.cost);
                        ++calls;
                        Sys e;
                        e.clear();
                        for (size_t b = b0; b < b1; ++b) {
                            e.cost += one[b].cost;
                            for (int q = 0; q < kNPack; ++q) e.H[q] += one[b].H[q];
                            for (int k = 0; k < kNFull; ++k) e.g[k] += one[b].g[k];
                        }
                        // both are sums of the same <= 82 row terms in another order: they differ
                        // by at most rows * 2^-53 of the terms' magnitude sum on each side, and
                        // Cauchy-Schwarz bounds that sum by sqrt(H_aa H_bb) (for g: sqrt(2 cost H_aa))
                        const double tol = 4 * 128 * 1.1103e-16;
                        CHECK(std::fabs(a.cost - e.cost) <= tol * e.cost);
                        int q = 0;
                        for (int k = 0; k < kNFull; ++k) {
                            const double hk = e.H[k * kNFull - k * (k - 1) / 2];
                            CHECK(std::fabs(a.g[k] - e.g[k]) <= tol * std::sqrt(2 * e.cost * hk));
                            for (int l = k; l < kNFull; ++l, ++q) {
                                const double hl = e.H[l * kNFull - l * (l - 1) / 2];
                                CHECK(std::fabs(a.H[q] - e.H[q]) <= tol * std::sqrt(hk * hl));
                            }
                        }
                    }
                // a range past the end adds nothing
                Sys z;
                z.clear();
                eval(E, p, true, nb, nb + 8, z.H, z.g, &z.cost);
                CHECK(z.cost == 0.0);
            }
    std::printf("variant %d: %zu calls\n", variant, calls);
}

int main() {
    for (int v = 0; v < 3; ++v) run(lm_eval_range_w4, v);
#ifdef LM_EVAL_CHECK_W8
    for (int v = 0; v < 3; ++v) run(lm_eval_range_w8, v);
#endif
    std::printf("ok\n");
    return 0;
}
