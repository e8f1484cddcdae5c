// Stand-alone check of the weighted stopping rule of madpose_amd/csrc/host/ransac_stop.h
// (required_samples_mass) and of the host gather inlier_mass_host, built with
// -fsanitize=address,undefined and run as a program by tests/test_weighted_stop_cpu.py.
// Prints "ok" and returns 0, or says what failed and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ransac_stop.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// a small generator of its own (xorshift64*): the check needs no library's
static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1Dull;
}

static void check_rule() {
    const StopOptions d{0.99, 8, 10000};
    const uint32_t kmd[3] = {3, 4, 4}, kpt[3] = {5, 6, 7};
    // the issue's setting: 300 correspondences, 90 true matches at q = 65535, 210 at q = 3276
    const uint32_t W = 90u * 65535u + 210u * 3276u;
    const uint32_t m90[3] = {90u * 65535u, 90u * 65535u, 90u * 65535u};
    const int32_t c90[3] = {90, 90, 90};
    const uint32_t want_count[3][2] = {{6316, 1894}, {10000, 6316}, {10000, 10000}};
    const uint32_t want_mass[3][2] = {{8, 8}, {10, 8}, {10, 8}};
    for (int v = 0; v < 3; ++v)
        for (int s = 0; s < 2; ++s) {
            CHECK(required_samples(s, (int)kmd[v], (int)kpt[v], 300, c90, d) == want_count[v][s]);
            CHECK(required_samples_mass(s, (int)kmd[v], (int)kpt[v], W, m90, d) == want_mass[v][s]);
        }
    // total 0, no winner, mass 0, mass = total
    const uint32_t zero[3] = {0, 0, 0};
    const uint32_t big = 65535u * 65535u;
    const uint32_t full[3] = {big, big, big}, one[3] = {1, 1, 1};
    for (int s = 0; s < 2; ++s) {
        CHECK(required_samples_mass(s, 3, 5, 0, full, d) == 10000);
        CHECK(required_samples_mass(s, 3, 5, big, nullptr, d) == 10000);
        CHECK(required_samples_mass(s, 3, 5, big, zero, d) == 10000);
        CHECK(required_samples_mass(s, 3, 5, big, full, d) == 8);
        // 1 of 65535^2: p_bad is 1 in double, the p_bad bound
        CHECK(required_samples_mass(s, 3, 5, big, one, d) == 10000);
    }
    // the MD solver reads lists 0 and 1, the point solver list 2 alone
    const uint32_t mix[3] = {big, big, 0};
    CHECK(required_samples_mass(0, 3, 5, big, mix, d) == 8 && required_samples_mass(1, 3, 5, big, mix, d) == 10000);
    // a pair that is not weighted (mass = counts, total = n) and equal weights (mass = q counts,
    // total = q n): the count rule's value, for every q
    for (int it = 0; it < 20000; ++it) {
        const uint32_t n = 1 + (uint32_t)(rnd() % 65535u);
        int32_t c[3];
        for (int t = 0; t < 3; ++t) c[t] = (int32_t)(rnd() % (n + 1));
        const int v = (int)(rnd() % 3);
        const StopOptions o{it % 3 == 0 ? 0.999999 : 0.99, (uint32_t)(rnd() % 20), 50u + (uint32_t)(rnd() % 100000)};
        for (uint32_t q : {1u, 1000u, 65535u}) {
            uint32_t m[3];
            for (int t = 0; t < 3; ++t) m[t] = q * (uint32_t)c[t];
            for (int s = 0; s < 2; ++s)
                CHECK(required_samples_mass(s, (int)kmd[v], (int)kpt[v], q * n, m, o) ==
                      required_samples(s, (int)kmd[v], (int)kpt[v], n, c, o));
        }
    }
    // monotone in the mass, within [min .. max]
    for (int s = 0; s < 2; ++s) {
        uint32_t before = 0;
        for (int64_t q = big; q >= 0; q -= big / 16) {
            const uint32_t m[3] = {(uint32_t)q, (uint32_t)q, (uint32_t)q};
            const uint32_t r = required_samples_mass(s, 4, 7, big, m, d);
            CHECK(r >= 8 && r <= 10000 && r >= before);
            before = r;
        }
    }
}

static void check_gather() {
    // empty lists
    {
        const std::vector<uint32_t> cum = {0, 5, 5, 70000};
        const int64_t off[4] = {0, 0, 0, 0};
        uint32_t mass[3] = {9, 9, 9};
        inlier_mass_host(cum.data(), off, nullptr, mass);
        CHECK(mass[0] == 0 && mass[1] == 0 && mass[2] == 0);
    }
    // full lists of n = 65535 rows of q = 65535: 4294836225, no wrap
    {
        const int64_t n = 65535;
        std::vector<uint32_t> cum((size_t)n + 1);
        for (int64_t i = 0; i <= n; ++i) cum[(size_t)i] = (uint32_t)i * 65535u;
        std::vector<int32_t> idx(3 * (size_t)n);
        for (int t = 0; t < 3; ++t)
            for (int64_t i = 0; i < n; ++i) idx[(size_t)(t * n + i)] = (int32_t)i;
        const int64_t off[4] = {0, n, 2 * n, 3 * n};
        uint32_t mass[3];
        inlier_mass_host(cum.data(), off, idx.data(), mass);
        for (int t = 0; t < 3; ++t) CHECK(mass[t] == 4294836225u && mass[t] == cum[(size_t)n]);
    }
    // random tables and ascending lists of exactly their lengths (the sanitizer sees the bounds)
    for (int it = 0; it < 200; ++it) {
        const int64_t n = 1 + (int64_t)(rnd() % 700);
        std::vector<uint32_t> cum((size_t)n + 1, 0u);
        for (int64_t i = 0; i < n; ++i) {
            const uint64_t r = rnd();
            const uint32_t q = r % 5 == 0 ? 0u : (r % 7 == 0 ? 65535u : (uint32_t)((r >> 8) % 65536u));
            cum[(size_t)i + 1] = cum[(size_t)i] + q;
        }
        std::vector<int32_t> idx;
        int64_t off[4] = {0, 0, 0, 0};
        uint64_t want[3] = {0, 0, 0};
        for (int t = 0; t < 3; ++t) {
            for (int64_t i = 0; i < n; ++i)
                if (rnd() % 3 == (uint64_t)t) {
                    idx.push_back((int32_t)i);
                    want[t] += cum[(size_t)i + 1] - cum[(size_t)i];
                }
            off[t + 1] = (int64_t)idx.size();
        }
        idx.shrink_to_fit();
        uint32_t mass[3];
        inlier_mass_host(cum.data(), off, idx.empty() ? nullptr : idx.data(), mass);
        for (int t = 0; t < 3; ++t) CHECK((uint64_t)mass[t] == want[t] && mass[t] <= cum[(size_t)n]);
    }
}

int main() {
    check_rule();
    check_gather();
    std::printf("ok\n");
    return 0;
}
