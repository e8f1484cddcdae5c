// Stand-alone check of the plain-C++ parts of mp_lsq_fit_set / mp_ransac_lo_steps_set:
// madpose_amd/csrc/include/mp_subset.h (the subset rule's host form and the size rules),
// madpose_amd/csrc/host/lsq_fit_plan.h (the entries' runs and argument checks) and
// madpose_amd/csrc/host/ransac_lo_steps.h (the f_i schedule, the stream packing, the offers).
// Built with -fsanitize=address,undefined and run as a program by
// tests/test_ransac_lo_steps_cpu.py.  Prints "ok" and returns 0, or says what failed and
// returns 1.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <set>
#include <stdexcept>
#include <tuple>
#include <vector>

#include "lsq_fit_plan.h"
#include "ransac_lo_steps.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static uint64_t g_x = 0x9E3779B97F4A7C15ull;
static uint64_t next() {
    g_x ^= g_x << 13;
    g_x ^= g_x >> 7;
    g_x ^= g_x << 17;
    return g_x;
}

// m strictly ascending indices out of 0 .. 2 m + 2
static std::vector<int> ascending(int m) {
    std::set<int> s;
    while ((int)s.size() < m) s.insert((int)(next() % (uint64_t)(2 * m + 3)));
    return std::vector<int>(s.begin(), s.end());
}

// the rule stated by a full sort of (masked key, t, i)
static void by_sort(const std::vector<int> L[3], int64_t k, uint64_t seed, uint32_t pair, uint32_t stream,
                    uint32_t substream, uint64_t mask, std::vector<int> out[3]) {
    std::vector<std::tuple<uint64_t, int, int>> all;
    for (int t = 0; t < 3; ++t)
        for (int i : L[t]) all.emplace_back(subset_key(seed, pair, stream, substream, t, (uint32_t)i) & mask, t, i);
    std::sort(all.begin(), all.end());
    for (int t = 0; t < 3; ++t) out[t].clear();
    const int64_t take = std::min<int64_t>(std::max<int64_t>(k, 0), (int64_t)all.size());
    for (int64_t j = 0; j < take; ++j) out[std::get<1>(all[(size_t)j])].push_back(std::get<2>(all[(size_t)j]));
    for (int t = 0; t < 3; ++t) std::sort(out[t].begin(), out[t].end());
}

static void check_subset() {
    const int lengths[][3] = {{0, 0, 0},   {1, 0, 0},       {0, 0, 63},    {64, 65, 0},  {63, 64, 65},
                              {255, 0, 257}, {256, 256, 256}, {257, 1, 255}, {700, 0, 0},  {0, 700, 64},
                              {700, 257, 65}, {700, 700, 700}, {1, 1, 1}};
    const uint64_t masks[3] = {kSubsetMaskAll, (uint64_t)0xFF << 56, 0};
    for (const auto &len : lengths) {
        std::vector<int> L[3] = {ascending(len[0]), ascending(len[1]), ascending(len[2])};
        const int M[3] = {len[0], len[1], len[2]};
        const int *ptr[3] = {L[0].data(), L[1].data(), L[2].data()};
        const int64_t total = (int64_t)M[0] + M[1] + M[2];
        const int64_t ks[] = {0, 1, total - 1, total, total + 1, 24, 294};
        for (int64_t k : ks) {
            if (k < 0) continue;
            for (uint64_t mask : masks) {
                const uint64_t seed = next();
                const uint32_t pair = (uint32_t)(next() % 1000), stream = (uint32_t)(next() >> 33),
                               sub = (uint32_t)(next() >> 34);
                std::vector<int> got[3], want[3];
                subset_select_host(ptr, M, k, seed, pair, stream, sub, mask, got);
                by_sort(L, k, seed, pair, stream, sub, mask, want);
                int64_t size = 0;
                for (int t = 0; t < 3; ++t) {
                    CHECK(got[t] == want[t]);
                    CHECK(std::is_sorted(got[t].begin(), got[t].end()));
                    CHECK(std::includes(L[t].begin(), L[t].end(), got[t].begin(), got[t].end()));
                    size += (int64_t)got[t].size();
                }
                CHECK(size == std::min(k, total));
                if (mask == 0 && k < total) { // the first k elements in (t, i) order
                    int64_t left = k;
                    for (int t = 0; t < 3; ++t) {
                        const int64_t z = std::min<int64_t>(left, M[t]);
                        CHECK((int64_t)got[t].size() == z && std::equal(got[t].begin(), got[t].end(), L[t].begin()));
                        left -= z;
                    }
                }
            }
        }
    }
    // the key: word 0 high, word 1 low; stream, substream, type and pair all reach it
    uint32_t w[4];
    philox4x32_10(17u, (5u << 2) | 2u, 3u, 0x80000000u | 9u, 0x11111111u, 0x22222222u, w);
    CHECK(subset_key(0x2222222211111111ull, 3, 9, 5, 2, 17) == (((uint64_t)w[0] << 32) | w[1]));
    const uint64_t base = subset_key(1, 2, 3, 4, 1, 5);
    CHECK(base != subset_key(2, 2, 3, 4, 1, 5) && base != subset_key(1, 3, 3, 4, 1, 5) &&
          base != subset_key(1, 2, 4, 4, 1, 5) && base != subset_key(1, 2, 3, 5, 1, 5) &&
          base != subset_key(1, 2, 3, 4, 2, 5) && base != subset_key(1, 2, 3, 4, 1, 6));
}

static void check_sizes() {
    int64_t k = -1;
    const int big[3] = {300, 300, 300};
    // the defaults (mu = 7, nu = 3): k = 294 / 392 / 392 for the MD type, 245 / 294 / 343 for the point type
    const int64_t md[3] = {294, 392, 392}, pt[3] = {245, 294, 343};
    for (int v = 0; v < 3; ++v) {
        CHECK(subset_size(kSubsetLsq, 0, v, 7, 3, big, &k) && k == md[v]);
        CHECK(subset_size(kSubsetLsq, 1, v, 7, 3, big, &k) && k == pt[v]);
        CHECK(subset_size(kSubsetLsq, 0, v, 2, 3, big, &k) && k == 2 * (2 * draw_k_md(v)) * 2);
        CHECK(subset_size(kSubsetLsq, 1, v, 2, 3, big, &k) && k == 2 * 2 * draw_k_pt(v));
        // the skip: one list below the solver's size
        const int kmd = draw_k_md(v), kpt = draw_k_pt(v);
        const int a[3] = {kmd - 1, 300, 300}, b[3] = {300, kmd - 1, 300}, c[3] = {300, 300, kpt - 1};
        const int d[3] = {kmd, kmd, 0}, e[3] = {0, 0, kpt};
        CHECK(!subset_size(kSubsetLsq, 0, v, 7, 3, a, &k) && k == 0);
        CHECK(!subset_size(kSubsetLsq, 0, v, 7, 3, b, &k) && k == 0);
        CHECK(subset_size(kSubsetLsq, 0, v, 7, 3, c, &k)); // (the MD type asks nothing of list 2)
        CHECK(!subset_size(kSubsetLsq, 1, v, 7, 3, c, &k) && k == 0);
        CHECK(subset_size(kSubsetLsq, 1, v, 7, 3, a, &k) && subset_size(kSubsetLsq, 1, v, 7, 3, b, &k));
        // exactly the minimal sizes: mu * (min(ss mu, M)) clamped to M
        CHECK(subset_size(kSubsetLsq, 0, v, 7, 3, d, &k) && k == 2 * kmd);
        CHECK(subset_size(kSubsetLsq, 1, v, 7, 3, e, &k) && k == kpt);
        // nonmin: max(35 / 36, min(k_pt nu, M / 2)), never skipped, clamped to M
        const int64_t f = v == 0 ? 35 : 36;
        CHECK(subset_size(kSubsetNonmin, 0, v, 7, 3, big, &k) && k == f);
        CHECK(subset_size(kSubsetNonmin, 1, v, 7, 20, big, &k) && k == std::max<int64_t>(f, 20 * kpt));
        CHECK(subset_size(kSubsetNonmin, 1, v, 7, 1000, big, &k) && k == 450); // (M / 2)
        const int few[3] = {3, 4, 5}, none[3] = {0, 0, 0};
        CHECK(subset_size(kSubsetNonmin, 0, v, 7, 3, few, &k) && k == 12);
        CHECK(subset_size(kSubsetNonmin, 0, v, 7, 3, none, &k) && k == 0);
    }
    // 64-bit products
    const int huge[3] = {1 << 28, 1 << 28, 1 << 28};
    CHECK(subset_size(kSubsetLsq, 0, 0, INT32_MAX, 3, huge, &k) && k == 3 * (int64_t)(1 << 28));
    CHECK(subset_size(kSubsetLsq, 1, 2, 1 << 20, 3, huge, &k) && k == 3 * (int64_t)(1 << 28)); // (7 * 2^40, clamped)
    const int wide[3] = {0, 0, 1 << 28};
    CHECK(subset_size(kSubsetLsq, 1, 2, 1 << 12, 3, wide, &k) && k == (int64_t)7 * (1 << 24));
    CHECK(subset_size(kSubsetNonmin, 1, 2, 7, INT32_MAX, huge, &k) && k == 3 * (int64_t)(1 << 28) / 2);
}

static void check_schedule() {
    // the example options: lambda 5, Q 4 -> 5, 11/3, 7/3, 1 by the one expression
    CHECK(lo_step_factor(0, 4, 5.0) == 5.0);
    CHECK(lo_step_factor(1, 4, 5.0) == 5.0 - (1.0 * 4.0) / 3.0);
    CHECK(lo_step_factor(2, 4, 5.0) == 5.0 - (2.0 * 4.0) / 3.0);
    CHECK(lo_step_factor(3, 4, 5.0) == 1.0);
    CHECK(lo_step_factor(0, 1, 5.0) == 5.0 && lo_step_factor(0, 0, 2.5) == 2.5);
    CHECK(lo_step_factor(0, 2, 2.5) == 2.5 && lo_step_factor(1, 2, 2.5) == 1.0);
    for (int Q = 2; Q <= kLoStepLsqIterMax; Q += 7)
        for (double lam : {1.0, 1.5, 5.0, 1e3}) {
            CHECK(lo_step_factor(0, Q, lam) == lam);
            for (int i = 1; i < Q; ++i) CHECK(lo_step_factor(i, Q, lam) <= lo_step_factor(i - 1, Q, lam));
            CHECK(std::fabs(lo_step_factor(Q - 1, Q, lam) - 1.0) <= 1e-12 * lam);
        }
    // the packing: one substream per (step, stage), all below the bound; word 1 keeps the type
    std::set<int32_t> seen;
    for (int r = 0; r < kLoStepsMax; ++r)
        for (int q = 0; q <= 1 + kLoStepLsqIterMax; ++q) {
            const int32_t s = lo_step_substream(r, q);
            CHECK(s >= 0 && (uint32_t)s < kSubsetSubstreamMax && seen.insert(s).second);
        }
    CHECK(lo_step_substream(0, 0) == 0 && lo_step_substream(2, 5) == 517);
    std::set<uint32_t> words;
    for (uint32_t s : {0u, 1u, 517u, kSubsetSubstreamMax - 1})
        for (int t = 0; t < 3; ++t) CHECK(words.insert(subset_word1(s, t)).second);
    CHECK(subset_word1(kSubsetSubstreamMax - 1, 2) == 0xFFFFFFFEu);
    CHECK(subset_word3(0) == 0x80000000u && subset_word3(kSubsetStreamMax - 1) == 0xFFFFFFFFu);
}

static void check_offers() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int32_t c1[3] = {10, 11, 12}, c2[3] = {20, 21, 22}, c3[3] = {30, 31, 32};
    LoTrack K;
    LoStepTrack S;
    CHECK(S.lo_step == -1 && S.lo_stage == -1 && S.offers == 0 && S.accepted == 0);
    // an empty best takes any score below DBL_MAX, nothing else
    CHECK(!lo_step_offer(K, S, 4, 0, 0, nan, c1) && !lo_step_offer(K, S, 4, 0, 0, DBL_MAX, c1));
    CHECK(S.offers == 2 && S.accepted == 0 && K.source == 0 && S.lo_step == -1);
    lo_take_minimal(K, 100.0, c1);
    lo_step_clear(S);
    CHECK(!lo_step_offer(K, S, 4, 1, 0, 100.0, c2)); // (equal: strict <)
    CHECK(!lo_step_offer(K, S, 4, 1, 1, nan, c2));
    CHECK(K.score == 100.0 && K.lo_index == -1 && K.source == 1 && S.lo_step == -1 && S.offers == 4);
    CHECK(lo_step_offer(K, S, 4, 2, 3, 90.0, c2));
    CHECK(K.score == 90.0 && K.lo_index == 4 && K.source == kLoSourceStep && K.counts[1] == 21 && S.lo_step == 2 &&
          S.lo_stage == 3 && S.accepted == 1 && S.offers == 5);
    CHECK(K.lo_runs == 0 && K.lo_accepted == 0); // (the LO counters are ransac_lo_track.h's alone)
    CHECK(!lo_step_offer(K, S, 4, 0, 6, 95.0, c3) && S.lo_step == 2 && S.lo_stage == 3);
    CHECK(lo_step_offer(K, S, 4, 0, 6, 80.0, c3) && S.lo_step == 0 && S.lo_stage == 6 && K.counts[2] == 32);
    // a later minimal model or LO result takes the best back: the step fields are cleared, the counters stay
    CHECK(lo_take_refined(K, 9, 1, 70.0, c1));
    lo_step_clear(S);
    CHECK(K.lo_index == 9 && K.source == 2 && S.lo_step == -1 && S.lo_stage == -1 && S.offers == 7 && S.accepted == 2);
    // random sequences against the rule over the history: the first of the lowest scores wins
    for (int trial = 0; trial < 1000; ++trial) {
        LoTrack T;
        LoStepTrack Z;
        double best = DBL_MAX;
        int br = -1, bq = -1, acc = 0;
        const int n = (int)(next() % 20);
        for (int j = 0; j < n; ++j) {
            const double sc = next() % 7 == 0 ? nan : (double)(next() % 5);
            const int r = (int)(next() % 64), q = (int)(next() % 8);
            const bool took = lo_step_offer(T, Z, 1, r, q, sc, c1);
            CHECK(took == (sc < best));
            if (sc < best) best = sc, br = r, bq = q, ++acc;
            CHECK(T.score == best && Z.lo_step == br && Z.lo_stage == bq && Z.offers == j + 1 && Z.accepted == acc);
        }
    }
}

static void check_runs() {
    const int64_t n[] = {5, 63, 0, 700, 64, 64, 257, 1};
    const int ne = 8;
    auto covers = [&](const std::vector<LsqRun> &runs) {
        int32_t at = 0;
        for (const LsqRun &r : runs) {
            CHECK(r.e0 == at && r.e1 > r.e0);
            at = r.e1;
        }
        CHECK(at == ne);
    };
    std::vector<LsqRun> runs = lsq_fit_runs(ne, n, 0);
    CHECK(runs.size() == 1);
    covers(runs);
    runs = lsq_fit_runs(ne, n, 1);
    CHECK(runs.size() == 8);
    covers(runs);
    runs = lsq_fit_runs(ne, n, 3);
    CHECK(runs.size() == 3);
    covers(runs);
    // a small bound: no run above it unless it is one entry
    for (int64_t bound : {1, 200, 2100, 2101, 5000}) {
        runs = lsq_fit_runs(ne, n, 0, bound);
        covers(runs);
        for (const LsqRun &r : runs) {
            int64_t sum = 0;
            for (int32_t e = r.e0; e < r.e1; ++e) sum += 3 * n[e];
            CHECK(sum <= bound || r.e1 - r.e0 == 1);
        }
    }
    CHECK(lsq_fit_runs(0, n, 0).empty());
    // the entries' checks: a repeated pair is fine, everything out of range is named
    const int32_t ids[] = {2, 2, 0, 2}, types[] = {0, 1, 1, 0}, st[] = {0, 5, INT32_MAX, 7}, sub[] = {0, 1, (1 << 30) - 1, 3};
    const double fac[] = {1.0, 2.5, 5.0, 1e-3};
    check_lsq_entries(3, 4, ids, types, fac, kSubsetLsq, st, sub, 0);
    check_lsq_entries(4, 4, nullptr, types, fac, kSubsetNonmin, st, sub, 2);
    check_lsq_entries(0, 0, nullptr, nullptr, nullptr, kSubsetLsq, nullptr, nullptr, 0);
    auto refused = [&](auto f) {
        try {
            f();
        } catch (const std::invalid_argument &) {
            return true;
        }
        return false;
    };
    CHECK(refused([&] { check_lsq_entries(3, -1, ids, types, fac, 0, st, sub, 0); }));
    CHECK(refused([&] { check_lsq_entries(3, 4, nullptr, types, fac, 0, st, sub, 0); }));
    CHECK(refused([&] { check_lsq_entries(2, 4, ids, types, fac, 0, st, sub, 0); }));
    CHECK(refused([&] { check_lsq_entries(3, 4, ids, types, fac, 2, st, sub, 0); }));
    CHECK(refused([&] { check_lsq_entries(3, 4, ids, types, fac, 0, st, sub, -1); }));
    CHECK(refused([&] { check_lsq_entries(3, 4, ids, nullptr, fac, 0, st, sub, 0); }));
    const int32_t bad_t[] = {0, 2, 1, 0}, bad_s[] = {0, -1, 0, 0}, bad_sub[] = {0, 1 << 30, 0, 0};
    const double bad_f[] = {1.0, 0.0, 1.0, 1.0}, nan_f[] = {1.0, std::nan(""), 1.0, 1.0},
                 inf_f[] = {1.0, std::numeric_limits<double>::infinity(), 1.0, 1.0};
    CHECK(refused([&] { check_lsq_entries(3, 4, ids, bad_t, fac, 0, st, sub, 0); }));
    CHECK(refused([&] { check_lsq_entries(3, 4, ids, types, fac, 0, bad_s, sub, 0); }));
    CHECK(refused([&] { check_lsq_entries(3, 4, ids, types, fac, 0, st, bad_sub, 0); }));
    CHECK(refused([&] { check_lsq_entries(3, 4, ids, types, bad_f, 0, st, sub, 0); }));
    CHECK(refused([&] { check_lsq_entries(3, 4, ids, types, nan_f, 0, st, sub, 0); }));
    CHECK(refused([&] { check_lsq_entries(3, 4, ids, types, inf_f, 0, st, sub, 0); }));
}

int main() {
    check_subset();
    check_sizes();
    check_schedule();
    check_offers();
    check_runs();
    std::printf("ok\n");
    return 0;
}
