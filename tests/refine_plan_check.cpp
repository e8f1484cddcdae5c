// Stand-alone check of madpose_amd/csrc/host/refine_plan.h (chunk planning and the packed
// device layout of mp_refine_batch), built with -fsanitize=address,undefined and run as a
// program by tests/test_refine_batch_cpu.py.  Prints "ok" and returns 0, or says what
// failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "refine_plan.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

static std::vector<int64_t> offsets_of(const std::vector<int64_t> &sizes, int64_t first = 0) {
    std::vector<int64_t> o(1, first);
    for (int64_t n : sizes) o.push_back(o.back() + n);
    return o;
}

// the runs cover the pairs once, in order, and their totals are their pairs' sizes
static void check_cover(const std::vector<RefineRun> &runs, const std::vector<int64_t> &o) {
    const int32_t np = (int32_t)o.size() - 1;
    int32_t p = 0;
    for (const RefineRun &r : runs) {
        CHECK(r.p0 == p && r.p1 > r.p0 && r.p1 <= np);
        CHECK(r.total == o[r.p1] - o[r.p0]);
        p = r.p1;
    }
    CHECK(p == np);
}

// every row and list of every pair of a run lies inside the run's allocations, no two
// overlap, the uploaded rows fill the first 6 T doubles exactly and the packing puts
// each value where the rows say
static void check_layout(const RefineRun &r, const std::vector<int64_t> &o) {
    const int64_t T = r.total;
    std::vector<int> owner_d((size_t)(kRefineRows * T), 0), owner_i((size_t)(6 * T), 0);
    std::vector<double> stage((size_t)(6 * T), -1.0);
    for (int32_t p = r.p0; p < r.p1; ++p) {
        const int64_t n = o[p + 1] - o[p], off = o[p] - o[r.p0];
        for (int k = 0; k < kRefineRows; ++k) {
            const int64_t at = refine_row(T, off, n, k);
            CHECK(at >= 0 && at + n <= kRefineRows * T);
            CHECK(k >= 6 || at + n <= 6 * T);
            CHECK(k < 6 || at >= 6 * T);
            for (int64_t i = 0; i < n; ++i) CHECK(owner_d[(size_t)(at + i)]++ == 0);
        }
        for (int b = 0; b < 2; ++b)
            for (int t = 0; t < 3; ++t) {
                const int64_t at = refine_list(T, off, n, b, t);
                CHECK(at >= 0 && at + n <= 6 * T);
                // inside a buffer: the caller's layout (pair at 3 off, list t at + t n)
                CHECK(at == b * 3 * T + 3 * off + t * n);
                for (int64_t i = 0; i < n; ++i) CHECK(owner_i[(size_t)(at + i)]++ == 0);
            }
        // pack: value (p, row k, i) = 1000 p + 10 i + k
        std::vector<double> x0((size_t)(2 * n)), x1((size_t)(2 * n)), d0((size_t)n), d1((size_t)n);
        for (int64_t i = 0; i < n; ++i) {
            x0[2 * i] = 1000.0 * p + 10.0 * i + 0;
            x0[2 * i + 1] = 1000.0 * p + 10.0 * i + 1;
            x1[2 * i] = 1000.0 * p + 10.0 * i + 2;
            x1[2 * i + 1] = 1000.0 * p + 10.0 * i + 3;
            d0[i] = 1000.0 * p + 10.0 * i + 4;
            d1[i] = 1000.0 * p + 10.0 * i + 5;
        }
        refine_pack_pair(x0.data(), x1.data(), d0.data(), d1.data(), n, off, stage.data());
    }
    for (int v : owner_d) CHECK(v == 1);
    for (int v : owner_i) CHECK(v == 1);
    for (int32_t p = r.p0; p < r.p1; ++p) {
        const int64_t n = o[p + 1] - o[p], off = o[p] - o[r.p0];
        for (int k = 0; k < 6; ++k)
            for (int64_t i = 0; i < n; ++i)
                CHECK(stage[(size_t)(refine_row(T, off, n, k) + i)] == 1000.0 * p + 10.0 * i + k);
    }
}

static void check_all(const std::vector<int64_t> &sizes, int64_t chunk, int64_t bound, int64_t first = 0) {
    const std::vector<int64_t> o = offsets_of(sizes, first);
    const int32_t np = (int32_t)sizes.size();
    const std::vector<RefineRun> runs = refine_plan(np, o.data(), chunk, bound);
    check_cover(runs, o);
    for (const RefineRun &r : runs) {
        if (chunk > 0) {
            // runs of exactly `chunk` pairs, the last one the rest
            CHECK(r.p1 - r.p0 == chunk || (r.p1 == np && r.p1 - r.p0 < chunk));
        } else {
            // within the bound, or one oversized pair (only zero-length pairs may follow it
            // in its run); greedy: the next pair did not fit
            const int64_t first_n = o[r.p0 + 1] - o[r.p0];
            CHECK(r.total <= bound || (first_n > bound && r.total == first_n));
            if (r.p1 < np) CHECK(r.total + (o[r.p1 + 1] - o[r.p1]) > bound);
        }
        check_layout(r, o);
    }
}

int main() {
    // no pairs: no runs
    {
        const int64_t o[1] = {0};
        CHECK(refine_plan(0, o, 0).empty());
        CHECK(refine_plan(0, o, 3).empty());
    }
    const std::vector<std::vector<int64_t>> cases = {
        {5, 63, 64, 65, 257, 700},
        {0, 5, 7},          // a zero-length pair at the front
        {5, 0, 0, 7},       // in the middle
        {5, 7, 0},          // at the end
        {0},                // alone
        {0, 0, 0},
        {1},
        {3, 1000, 2, 2, 2}, // one pair larger than the bound (bound 100 below)
        {1000},
        {1000, 0, 0, 1},
        {100, 100, 1, 99, 100},
    };
    for (const auto &sizes : cases)
        for (int64_t chunk : {int64_t(1), int64_t(2), int64_t(0), int64_t(1000)})
            for (int64_t first : {int64_t(0), int64_t(17)}) check_all(sizes, chunk, 100, first);
    // the exact runs of a few plans
    {
        const std::vector<int64_t> o = offsets_of({3, 1000, 2, 2, 2});
        const auto runs = refine_plan(5, o.data(), 0, 100);
        CHECK(runs.size() == 3);
        CHECK(runs[0].p0 == 0 && runs[0].p1 == 1 && runs[0].total == 3);
        CHECK(runs[1].p0 == 1 && runs[1].p1 == 2 && runs[1].total == 1000);
        CHECK(runs[2].p0 == 2 && runs[2].p1 == 5 && runs[2].total == 6);
        const auto by2 = refine_plan(5, o.data(), 2, 100);
        CHECK(by2.size() == 3 && by2[0].p1 == 2 && by2[1].p1 == 4 && by2[2].p1 == 5 && by2[2].total == 2);
        const auto by1 = refine_plan(5, o.data(), 1, 100);
        CHECK(by1.size() == 5);
    }
    {
        const std::vector<int64_t> o = offsets_of({100, 100, 1, 99, 100});
        const auto runs = refine_plan(5, o.data(), 0, 100);
        CHECK(runs.size() == 4 && runs[2].p0 == 2 && runs[2].p1 == 4 && runs[2].total == 100);
    }
    // the default bound: 1500 pairs of 2000 run together, and stay under 1 GiB
    {
        const std::vector<int64_t> o = offsets_of(std::vector<int64_t>(1500, 2000));
        const auto runs = refine_plan(1500, o.data(), 0);
        CHECK(runs.size() == 1 && runs[0].total == 3000000);
        CHECK(refine_run_bytes(kRefineRunCorr) < (int64_t(1) << 30));
        const std::vector<int64_t> big = offsets_of(std::vector<int64_t>(3000, 2000));
        const auto runs2 = refine_plan(3000, big.data(), 0);
        CHECK(runs2.size() == 2 && runs2[0].total <= kRefineRunCorr && runs2[0].p1 == 2097);
    }
    // list positions of the largest legal pair stay inside int64 and the LM's int offsets
    CHECK(2 * kRefinePairMax < (int64_t(1) << 31));
    std::printf("ok\n");
    return 0;
}
