// Stand-alone check of madpose_amd/csrc/host/ransac_stop.h (the termination rule and the
// rounds of mp_ransac_adaptive_set) and of the planning form of host/candidates_plan.h that
// takes a per-entry first sample, built with -fsanitize=address,undefined and run as a
// program by tests/test_ransac_adaptive_cpu.py.  Prints "ok" and returns 0, or says what
// failed and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "candidates_plan.h"
#include "ransac_stop.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static void check_rule() {
    const StopOptions d{0.99, 8, 10000};
    // 80 % inliers on the 5-point solver: 13 samples (the issue's example)
    const int32_t c80[3] = {240, 240, 240};
    CHECK(required_samples(1, 3, 5, 300, c80, d) == 13);
    // the MD solver reads lists 0 and 1 (k_md each), the point solver list 2 alone
    const int32_t cmix[3] = {300, 300, 0};
    CHECK(required_samples(0, 3, 5, 300, cmix, d) == 8);      // p_all = 1: min_num_iterations
    CHECK(required_samples(1, 3, 5, 300, cmix, d) == 10000);  // p_all = 0: the bound
    // no winner, no correspondences
    CHECK(required_samples(0, 4, 7, 700, nullptr, d) == 10000);
    CHECK(required_samples(1, 4, 7, 0, c80, d) == 10000);
    // 2 / 700 on five points: p_bad = 1 - 1.9e-13 is below the threshold and `it` is about
    // 2.4e13, above 2^32: it must come out as the bound, for every bound (the clamp is made
    // in double); on seven points p_bad is 1 and the threshold gives the bound
    const int32_t ctiny[3] = {2, 2, 2};
    CHECK(std::ceil(std::log(0.01) / std::log(1.0 - std::pow(2.0 / 700.0, 5.0)) + 0.5) > 4294967296.0);
    for (uint32_t mx : {50u, 10000u, 4000000000u}) {
        const StopOptions o{0.99, 8, mx};
        CHECK(required_samples(1, 3, 5, 700, ctiny, o) == mx);
        CHECK(required_samples(1, 4, 7, 700, ctiny, o) == mx);
    }
    // success_probability 1: log(0) = -inf over a negative log: +inf, the bound; 0.5 and a
    // min above the bound: the min wins
    const StopOptions one{1.0, 0, 50}, hi{0.5, 100, 50};
    CHECK(required_samples(1, 3, 5, 300, c80, one) == 50);
    CHECK(required_samples(1, 3, 5, 300, c80, hi) == 100);
    // every value on a lattice is within [min(min, max) .. max(min, max)] and monotone in the counts
    for (int v = 0; v < 3; ++v)
        for (int64_t n : {1, 5, 64, 700})
            for (int s = 0; s < 2; ++s) {
                uint32_t before = 0;
                for (int64_t q = n; q >= 0; q -= (n + 7) / 8) {
                    const int32_t c[3] = {(int32_t)q, (int32_t)q, (int32_t)q};
                    const uint32_t r = required_samples(s, draw_k_md(v), draw_k_pt(v), n, c, d);
                    CHECK(r >= 8 && r <= 10000 && r >= before);
                    before = r;
                }
            }
    // the stop test: a solver that drew nothing never stops a pair
    const uint32_t req[2] = {8, 13};
    const int64_t a[2] = {0, 12}, b[2] = {0, 13}, c[2] = {8, 0}, e[2] = {7, 12};
    const uint32_t zero[2] = {0, 0};
    CHECK(!stop_reached(req, a) && stop_reached(req, b) && stop_reached(req, c) && !stop_reached(req, e));
    const int64_t none[2] = {0, 0};
    CHECK(!stop_reached(zero, none) && stop_reached(zero, a));
}

// rounds of `step` up to `budget`: the checkpoints are min(k step, budget), the last round partial
static void check_rounds(int32_t step, int32_t budget) {
    int32_t first = 0, k = 0;
    while (true) {
        const int32_t c = round_count(first, step, budget);
        if (c == 0) break;
        ++k;
        CHECK(c >= 1 && c <= step);
        first += c;
        CHECK((int64_t)first == std::min<int64_t>((int64_t)k * step, budget));
    }
    CHECK(first == budget);
    CHECK(round_count(budget, step, budget) == 0);
}

// One round of a selection: entry j takes count[j] samples from first[j] on.  The items must
// cover every sample of every entry once, in order, with the pair's own sample numbers.
static void check_items(const std::vector<int32_t> &first, const std::vector<int32_t> &count, int64_t sample_chunk,
                        int64_t base) {
    const int32_t np = (int32_t)first.size();
    std::vector<int64_t> soff(1, base);
    for (int32_t c : count) soff.push_back(soff.back() + c);
    const int64_t S = soff.back() - base;
    std::vector<int> seen((size_t)S, 0);
    std::vector<DrawItem> items, plain;
    for (const HypSlab &s : hyp_slabs(S, sample_chunk)) {
        draw_items(np, soff.data(), first.data(), s, items);
        draw_items(np, soff.data(), s, plain); // the form without a first sample: the same items from 0
        CHECK(items.size() == plain.size());
        CHECK((int64_t)items.size() <= s.s1 - s.s0);
        int64_t next = 0;
        for (size_t i = 0; i < items.size(); ++i) {
            const DrawItem &it = items[i];
            CHECK(it.pair >= 0 && it.pair < np);
            CHECK(it.pair == plain[i].pair && it.count == plain[i].count && it.out == plain[i].out);
            CHECK(it.s0 == plain[i].s0 + first[(size_t)it.pair]);
            CHECK(it.count >= 1 && it.count <= kDrawItemSamples);
            CHECK(it.out == next && (int64_t)it.out + it.count <= s.s1 - s.s0);
            CHECK(it.s0 >= first[(size_t)it.pair]);
            CHECK((int64_t)it.s0 + it.count <= (int64_t)first[(size_t)it.pair] + count[(size_t)it.pair]);
            for (int q = 0; q < it.count; ++q) {
                const int64_t g = soff[(size_t)it.pair] - base + (it.s0 - first[(size_t)it.pair]) + q;
                CHECK(g == s.s0 + it.out + q);
                CHECK(seen[(size_t)g]++ == 0);
            }
            next += it.count;
        }
        CHECK(next == s.s1 - s.s0);
    }
    for (int64_t g = 0; g < S; ++g) CHECK(seen[(size_t)g] == 1);
}

int main() {
    check_rule();
    for (int32_t step : {1, 7, 48, 64, 512, 600})
        for (int32_t budget : {0, 1, 47, 48, 49, 512, 1000}) check_rounds(step, budget);
    // the rounds of three pairs that stop at different checkpoints, step 48 of 512 (the last
    // round is 32 samples), cut by slabs that cut through entries and items
    for (int64_t chunk : {0, 1, 33, 64, 100})
        for (int64_t base : {0, 5}) {
            std::vector<int32_t> first = {0, 0, 0}, count;
            std::vector<int32_t> stop_at = {48, 240, 512};
            while (!first.empty()) {
                count.clear();
                for (int32_t f : first) count.push_back(round_count(f, 48, 512));
                check_items(first, count, chunk, base);
                std::vector<int32_t> nf, ns;
                for (size_t j = 0; j < first.size(); ++j)
                    if (first[j] + count[j] < stop_at[j]) {
                        nf.push_back(first[j] + count[j]);
                        ns.push_back(stop_at[j]);
                    }
                first.swap(nf);
                stop_at.swap(ns);
            }
            // entries without samples between others, a first sample near the budget's bound
            check_items({0, 100, 7, (1 << 20) - 130}, {65, 0, 1, 130}, chunk, base);
            check_items({3}, {0}, chunk, base);
        }
    std::printf("ok\n");
    return 0;
}
