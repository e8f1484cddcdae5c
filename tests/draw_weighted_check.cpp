// Stand-alone check of the host side of the confidence-weighted draw (madpose_amd/csrc/include/
// mp_draw.h draw_cum_find / draw_sample_weighted, include/mp_draw_weights.h draw_quantise), built
// with -fsanitize=address,undefined and run as a program by tests/test_draw_weighted_cpu.py.  The
// tables are heap arrays of exactly n + 1 entries, so a read past c[n] is caught.  Prints "ok"
// and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "mp_draw_weights.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

int main() {
    // ---- the quantisation's edges ----
    uint32_t q = 7;
    CHECK(draw_quantise(0.0, &q) && q == 0);
    CHECK(draw_quantise(-0.0, &q) && q == 0);
    CHECK(draw_quantise(std::ldexp(1.0, -17), &q) && q == 0);
    CHECK(draw_quantise(std::ldexp(1.0, -16), &q) && q == 1);
    CHECK(draw_quantise(std::nextafter(std::ldexp(1.0, -16), 0.0), &q) && q == 0);
    CHECK(draw_quantise(std::numeric_limits<double>::denorm_min(), &q) && q == 0);
    CHECK(draw_quantise(0.5, &q) && q == 32768);
    CHECK(draw_quantise(std::nextafter(1.0, 0.0), &q) && q == 65535);
    CHECK(draw_quantise(1.0, &q) && q == 65535);
    CHECK(draw_quantise((double)std::nextafter(1.0f, 0.0f), &q) && q == 65535);
    const double bad[] = {std::nextafter(1.0, 2.0), 2.0, -std::numeric_limits<double>::denorm_min(), -1.0,
                          std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                          std::numeric_limits<double>::quiet_NaN()};
    for (double b : bad) CHECK(!draw_quantise(b, &q) && q == 0);

    std::mt19937_64 rng(12345);
    const int sizes[] = {3, 4, 5, 7, 8, 63, 64, 65, 300, 4095, 65535};
    for (int v = 0; v < 3; ++v) {
        const int kmd = draw_k_md(v), kpt = draw_k_pt(v);
        for (int n : sizes) {
            if (n < kmd) continue;
            for (int mode = 0; mode < 3; ++mode) { // mixed weights; all at the maximum; as few positive as allowed
                std::vector<uint32_t> qs((size_t)n, 0);
                const int need = draw_weighted_need(n, kmd, kpt);
                if (mode == 0) {
                    for (auto &x : qs) x = (rng() % 3 == 0) ? 0u : (uint32_t)(rng() % 65536);
                    for (int i = 0; i < need; ++i) qs[(size_t)(rng() % (uint64_t)n)] = 1 + (uint32_t)(rng() % 65535);
                } else if (mode == 1) {
                    for (auto &x : qs) x = kDrawWeightQMax;
                } else {
                    qs[(size_t)n - 1] = 1; // (the last index: the search's upper end)
                    qs[0] = kDrawWeightQMax;
                }
                int pos = 0;
                for (uint32_t x : qs) pos += x > 0;
                for (int i = 0; pos < need; ++i)
                    if (!qs[(size_t)i]) {
                        qs[(size_t)i] = 1;
                        ++pos;
                    }
                uint32_t *c = new uint32_t[(size_t)n + 1]; // exactly n + 1 entries
                c[0] = 0;
                uint64_t W = 0;
                for (int i = 0; i < n; ++i) {
                    W += qs[(size_t)i];
                    c[i + 1] = (uint32_t)W;
                }
                CHECK(W < (1ull << 32) && W == c[n]);
                // the search: every boundary and its neighbours
                for (int i = 0; i < n; ++i) {
                    if (!qs[(size_t)i]) continue;
                    CHECK(draw_cum_find(c, n, c[i]) == i);
                    CHECK(draw_cum_find(c, n, c[i + 1] - 1) == i);
                }
                CHECK(qs[(size_t)draw_cum_find(c, n, 0)] > 0);
                CHECK(qs[(size_t)draw_cum_find(c, n, (uint32_t)(W - 1))] > 0);
                // samples: distinct indices below n with q > 0, zeros past the sample's size
                for (uint32_t s = 0; s < 400; ++s) {
                    int idx[8];
                    bool fill = false;
                    const int share = (int)(s % 3) * 128;
                    const int type = draw_sample_weighted(n, kmd, kpt, 0x1234567890ABCDEFull + mode, share, 7u, s, c, idx,
                                                          &fill);
                    CHECK(type == draw_type(n, kpt, 0x1234567890ABCDEFull + mode, share, 7u, s));
                    const int k = type ? kpt : kmd;
                    for (int a = 0; a < 8; ++a) {
                        if (a >= k) {
                            CHECK(idx[a] == 0);
                            continue;
                        }
                        CHECK(idx[a] >= 0 && idx[a] < n && qs[(size_t)idx[a]] > 0);
                        for (int b = 0; b < a; ++b) CHECK(idx[a] != idx[b]);
                    }
                    if (mode == 1) { // equal weights: the uniform draw, fill included
                        int uni[8];
                        bool ufill = false;
                        CHECK(draw_sample(n, kmd, kpt, 0x1234567890ABCDEFull + mode, share, 7u, s, uni, &ufill) == type);
                        for (int a = 0; a < 8; ++a) CHECK(uni[a] == idx[a]);
                        CHECK(ufill == fill);
                    }
                }
                delete[] c;
            }
        }
    }
    std::printf("ok\n");
    return 0;
}
