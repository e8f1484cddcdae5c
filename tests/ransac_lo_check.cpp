// Stand-alone check of madpose_amd/csrc/host/ransac_lo_track.h (the two-track bookkeeping of
// mp_ransac_lo_set), built with -fsanitize=address,undefined and run as a program by
// tests/test_ransac_lo_cpu.py.  Prints "ok" and returns 0, or says what failed and returns 1.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "ransac_lo_track.h"
#include "ransac_stop.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static bool same(const LoTrack &a, const LoTrack &b) {
    return a.score == b.score && a.counts[0] == b.counts[0] && a.counts[1] == b.counts[1] &&
           a.counts[2] == b.counts[2] && a.lo_index == b.lo_index && a.lo_runs == b.lo_runs &&
           a.lo_accepted == b.lo_accepted && a.source == b.source;
}

static void check_steps() {
    const int32_t c1[3] = {10, 11, 12}, c2[3] = {20, 21, 22}, c3[3] = {30, 31, 32};
    const double nan = std::numeric_limits<double>::quiet_NaN();
    LoTrack K;
    CHECK(K.score == DBL_MAX && K.lo_index == -1 && K.lo_runs == 0 && K.lo_accepted == 0 && K.source == 0);
    // nothing replaces an empty best but a score below DBL_MAX
    CHECK(!lo_take_minimal(K, DBL_MAX, c1) && !lo_take_minimal(K, nan, c1) && K.source == 0);
    CHECK(!lo_take_refined(K, 3, 1, nan, c1) && K.lo_runs == 1 && K.lo_accepted == 0 && K.source == 0);
    // step 1, then an LO that was not accepted, one that did not score lower, one that did
    CHECK(lo_take_minimal(K, 100.0, c1) && K.source == 1 && K.lo_index == -1 && K.counts[2] == 12);
    LoTrack before = K;
    CHECK(!lo_take_refined(K, 7, 0, 50.0, c2)); // (no round accepted: the given model, whatever its score)
    CHECK(!lo_take_refined(K, 7, 1, 100.0, c2)); // (equal: strict <)
    CHECK(!lo_take_refined(K, 7, 2, nan, c2));
    before.lo_runs += 3;
    CHECK(same(K, before));
    CHECK(lo_take_refined(K, 7, 1, 90.0, c2));
    CHECK(K.score == 90.0 && K.lo_index == 7 && K.lo_runs == 5 && K.lo_accepted == 1 && K.source == 2 &&
          K.counts[0] == 20);
    // a later minimal best between the two: the minimal track moved, the overall best did not
    before = K;
    CHECK(!lo_take_minimal(K, 95.0, c3) && !lo_take_minimal(K, 90.0, c3) && !lo_take_minimal(K, nan, c3));
    CHECK(same(K, before));
    // ... whose LO then wins
    CHECK(lo_take_refined(K, 19, 3, 80.0, c3) && K.lo_index == 19 && K.lo_accepted == 2 && K.counts[1] == 31);
    // a minimal model below everything: lo_index back to -1, the counters stay
    CHECK(lo_take_minimal(K, 10.0, c1) && K.lo_index == -1 && K.source == 1 && K.lo_runs == 6 && K.lo_accepted == 2);
    CHECK(!lo_take_refined(K, 23, 1, 10.0, c2) && K.lo_index == -1 && K.lo_runs == 7);
    // -inf is a score like any other
    CHECK(lo_take_refined(K, 29, 1, -std::numeric_limits<double>::infinity(), c2) && K.lo_index == 29);
    CHECK(!lo_take_minimal(K, -std::numeric_limits<double>::infinity(), c1));
}

// random round sequences against the rule stated over the whole history: the overall best is
// the first of the lowest eligible scores in the order (minimal_0, lo_0, minimal_1, lo_1, ...)
static void check_random() {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
    };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int trial = 0; trial < 2000; ++trial) {
        const int rounds = (int)(next() % 12);
        LoTrack K;
        double best = DBL_MAX;
        int best_src = 0, best_idx = -1, runs = 0, acc = 0;
        std::vector<int32_t> best_c(3, 0);
        for (int r = 0; r < rounds; ++r) {
            // scores from a small lattice, so that equal scores are common; some NaN
            const double ms = next() % 9 == 0 ? nan : (double)(next() % 6);
            const double ls = next() % 9 == 0 ? nan : (double)(next() % 6);
            const int32_t accepted = (int32_t)(next() % 3), cand = (int32_t)(next() % 1000);
            const int32_t mc[3] = {(int32_t)(next() % 50), (int32_t)(next() % 50), (int32_t)(next() % 50)};
            const int32_t lc[3] = {(int32_t)(next() % 50), (int32_t)(next() % 50), (int32_t)(next() % 50)};
            const bool t1 = lo_take_minimal(K, ms, mc);
            CHECK(t1 == (ms < best));
            if (ms < best) {
                best = ms;
                best_src = 1;
                best_idx = -1;
                best_c.assign(mc, mc + 3);
            }
            const bool t2 = lo_take_refined(K, cand, accepted, ls, lc);
            ++runs;
            CHECK(t2 == (accepted >= 1 && ls < best));
            if (accepted >= 1 && ls < best) {
                best = ls;
                best_src = 2;
                best_idx = cand;
                ++acc;
                best_c.assign(lc, lc + 3);
            }
            CHECK(K.score == best && K.source == best_src && K.lo_index == best_idx && K.lo_runs == runs &&
                  K.lo_accepted == acc);
            for (int t = 0; t < 3; ++t) CHECK(K.counts[t] == best_c[(size_t)t]);
            CHECK(K.score == K.score); // (never NaN)
        }
    }
}

// the rule reads the overall best's counts: a pair whose LO raised the counts needs fewer samples
static void check_rule_input() {
    const StopOptions d{0.99, 8, 10000};
    LoTrack K;
    const int32_t minimal[3] = {150, 150, 150}, refined[3] = {240, 240, 240};
    CHECK(required_samples(1, 3, 5, 300, K.source != 0 ? K.counts : nullptr, d) == 10000);
    lo_take_minimal(K, 50.0, minimal);
    const uint32_t before = required_samples(1, 3, 5, 300, K.counts, d);
    lo_take_refined(K, 4, 1, 40.0, refined);
    const uint32_t after = required_samples(1, 3, 5, 300, K.counts, d);
    CHECK(after == 13 && before > after);
}

int main() {
    check_steps();
    check_random();
    check_rule_input();
    std::printf("ok\n");
    return 0;
}
