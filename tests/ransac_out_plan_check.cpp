// Stand-alone check of the output stage's plan in madpose_amd/csrc/host/residuals_plan.h
// (ransac_out_items, ransac_out_pair, ransac_out_overlap and the byte counts), built and run by
// tests/test_ransac_out_cpu.py under AddressSanitizer and UBSan.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "residuals_plan.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// One call: selected pairs of the given sizes, pairs[j] their index in the set, winner[j] whether
// entry j has a model, cut into runs under (max_rows, max_entries).  The stage's arrays hold the
// whole call, so an item's row is a row of the call.
static void check_call(const std::vector<int64_t> &n, const std::vector<int32_t> &pairs,
                       const std::vector<unsigned char> &winner, int64_t max_rows, int32_t max_entries) {
    const int32_t ns = (int32_t)n.size();
    std::vector<int64_t> off((size_t)ns + 1, -1);
    resid_offsets(ns, n.data(), off.data());
    const int64_t R = off[(size_t)ns];
    std::vector<ResidRun> runs;
    resid_runs(ns, off.data(), max_rows, max_entries, runs);
    std::vector<int> seen((size_t)R, 0), entry_seen((size_t)ns, 0);
    int32_t next = 0;
    for (const ResidRun &r : runs) {
        CHECK(r.e0 == next && r.e1 > r.e0 && r.e1 <= ns);
        next = r.e1;
        std::vector<ResidItem> items;
        std::vector<int64_t> first_item;
        ransac_out_items(r, pairs.data(), winner.data(), off.data(), items, first_item);
        CHECK((int32_t)first_item.size() == r.e1 - r.e0 + 1);
        CHECK(first_item.front() == 0 && first_item.back() == (int64_t)items.size());
        CHECK((int64_t)items.size() <= (int64_t)(r.e1 - r.e0) + r.rows / kResidItemRows);
        for (int32_t e = r.e0; e < r.e1; ++e) {
            ++entry_seen[(size_t)e];
            const int64_t j0 = first_item[(size_t)(e - r.e0)], j1 = first_item[(size_t)(e - r.e0) + 1];
            CHECK(j1 - j0 == (n[(size_t)e] + kResidItemRows - 1) / kResidItemRows); // (n = 0: no item)
            int64_t at = 0;
            for (int64_t j = j0; j < j1; ++j) {
                const ResidItem &it = items[(size_t)j];
                // a winner's items read the entry's record of the run, the others none
                CHECK(it.rec == (winner[(size_t)e] ? e - r.e0 : kResidFill));
                CHECK(it.rec < r.e1 - r.e0);
                CHECK(it.pair == pairs[(size_t)e] && it.factor == 1.0);
                CHECK(it.first == at && it.count >= 1 && it.count <= kResidItemRows);
                CHECK(j + 1 == j1 || it.count == kResidItemRows);
                CHECK((int64_t)it.first + it.count <= n[(size_t)e]); // inside the pair
                CHECK(it.row == off[(size_t)e] + it.first);
                // ... and inside the pair's rows of the outputs: an item never crosses a pair
                CHECK(it.row >= off[(size_t)e] && it.row + it.count <= off[(size_t)e + 1]);
                for (int q = 0; q < it.count; ++q) ++seen[(size_t)(it.row + q)];
                at += it.count;
            }
            CHECK(at == n[(size_t)e]);
        }
    }
    CHECK(next == ns);
    for (int64_t i = 0; i < R; ++i) CHECK(seen[(size_t)i] == 1);         // every row once
    for (int32_t e = 0; e < ns; ++e) CHECK(entry_seen[(size_t)e] == 1);   // every pair in one run
    // the per-pair rows: one per entry, whatever its size
    for (int32_t e = 0; e < ns; ++e) {
        double model[17];
        for (int i = 0; i < 17; ++i) model[i] = 1.5 + e + 0.25 * i;
        const int32_t count[3] = {e + 1, e + 2, e + 3};
        const RansacOutPair p = ransac_out_pair(winner[(size_t)e] != 0, model, 7 + e, count);
        if (winner[(size_t)e]) {
            CHECK(std::memcmp(p.model, model, sizeof(model)) == 0 && p.index == 7 + e);
            CHECK(p.count[0] == e + 1 && p.count[1] == e + 2 && p.count[2] == e + 3);
        } else {
            for (int i = 0; i < 17; ++i) CHECK(p.model[i] == 0.0 && !std::signbit(p.model[i]));
            CHECK(p.index == -1 && p.count[0] == 0 && p.count[1] == 0 && p.count[2] == 0);
        }
    }
}

int main() {
    static_assert(sizeof(RansacOutPair) == 152, "17 doubles, the index and three counts");
    static_assert(kResidFill < 0 && kRansacOutArrays == 5, "constants");
    const std::vector<int64_t> edge = {0, 1, 4095, 4096, 4097, 8193};
    // every size alone, with and without a winner, and every ordered pair of sizes
    for (int64_t a : edge)
        for (unsigned char wa = 0; wa < 2; ++wa) {
            check_call({a}, {0}, {wa}, (int64_t)1 << 26, 1 << 15);
            check_call({a}, {3}, {wa}, 1, 1);
            for (int64_t b : edge)
                for (unsigned char wb = 0; wb < 2; ++wb) {
                    check_call({a, b}, {1, 0}, {wa, wb}, (int64_t)1 << 26, 1 << 15);
                    check_call({a, b}, {0, 1}, {wa, wb}, 4096, 1 << 15);
                }
        }
    check_call({}, {}, {}, (int64_t)1 << 26, 1 << 15);
    // winners and non-winners first, last and in the middle; all pairs without a winner
    const std::vector<int64_t> mixed = {0, 8193, 0, 1, 4096, 1, 4097, 0, 4095, 0};
    const std::vector<int32_t> ids = {9, 1, 4, 3, 0, 2, 8, 7, 6, 5};
    const std::vector<std::vector<unsigned char>> winners = {
        {1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 1, 1, 1, 1, 1, 1, 1, 1},
        {1, 1, 1, 1, 1, 1, 1, 1, 1, 0}, {1, 1, 1, 1, 0, 0, 1, 1, 1, 1}, {0, 1, 0, 1, 0, 1, 0, 1, 0, 1},
        {1, 0, 1, 0, 1, 0, 1, 0, 1, 0}, {0, 0, 0, 0, 1, 0, 0, 0, 0, 0}};
    for (const std::vector<unsigned char> &w : winners)
        for (int64_t max_rows : {(int64_t)1, (int64_t)4096, (int64_t)8193, (int64_t)12290, (int64_t)1 << 26})
            for (int32_t max_entries : {1, 2, 3, 1 << 15}) check_call(mixed, ids, w, max_rows, max_entries);

    // ---- byte counts ----
    const int64_t lim = std::numeric_limits<int64_t>::max();
    CHECK(ransac_out_models_bytes(0) == 0 && ransac_out_index_bytes(0) == 0 && ransac_out_counts_bytes(0) == 0);
    CHECK(ransac_out_models_bytes(13) == 13 * 136 && ransac_out_index_bytes(13) == 52 && ransac_out_counts_bytes(13) == 156);
    CHECK(ransac_out_models_bytes(-1) == -1 && ransac_out_index_bytes(-1) == -1 && ransac_out_counts_bytes(-1) == -1);
    CHECK(ransac_out_models_bytes(lim / 136) == (lim / 136) * 136 && ransac_out_models_bytes(lim / 136 + 1) == -1);
    CHECK(ransac_out_index_bytes(lim / 4) == (lim / 4) * 4 && ransac_out_index_bytes(lim / 4 + 1) == -1);
    CHECK(ransac_out_counts_bytes(lim / 12) == (lim / 12) * 12 && ransac_out_counts_bytes(lim / 12 + 1) == -1);
    CHECK(ransac_out_models_bytes(lim) == -1 && ransac_out_counts_bytes(lim) == -1);

    // ---- overlap over five extents: differences only, also near INT64_MAX and the top ----
    const uint64_t top = std::numeric_limits<uint64_t>::max();
    int a = -1, b = -1;
    {
        const uint64_t addr[5] = {1000, 2000, 3000, 4000, 5000};
        const int64_t bytes[5] = {1000, 1000, 1000, 1000, 1000}; // back to back
        CHECK(!ransac_out_overlap(addr, bytes, &a, &b) && a == -1 && b == -1);
    }
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j) { // exactly one pair shares its last byte, in either address order
            for (int flip = 0; flip < 2; ++flip) {
                uint64_t addr[5] = {1000, 3000, 5000, 7000, 9000};
                int64_t bytes[5] = {1000, 1000, 1000, 1000, 1000};
                const int lo = flip ? j : i, hi = flip ? i : j;
                addr[hi] = addr[lo] + 999;
                CHECK(ransac_out_overlap(addr, bytes, &a, &b) && a == i && b == j);
                addr[hi] = addr[lo] + 1000; // one further, filling the gap behind it: disjoint
                CHECK(!ransac_out_overlap(addr, bytes, &a, &b));
            }
        }
    {
        // an array that is not given (address 0) or has no byte overlaps nothing
        const uint64_t addr[5] = {0, 1000, 1000, 0, 1500};
        const int64_t bytes[5] = {lim, 1000, 0, lim, 10};
        CHECK(ransac_out_overlap(addr, bytes, &a, &b) && a == 1 && b == 4);
        const int64_t none[5] = {lim, 1000, 0, lim, 0};
        CHECK(!ransac_out_overlap(addr, none, &a, &b));
        const int64_t refused[5] = {lim, 1000, -1, lim, -1}; // (a refused byte count: no extent)
        CHECK(!ransac_out_overlap(addr, refused, &a, &b));
    }
    {
        // lengths of INT64_MAX and addresses at the top: no sum of an address and a length
        const uint64_t addr[5] = {1, (uint64_t)lim + 1, top - 10, top - 5, top};
        const int64_t bytes[5] = {lim, lim - 20, 5, 5, 1};
        CHECK(!ransac_out_overlap(addr, bytes, &a, &b)); // [1, lim], [lim + 1, top - 20], ...
        const int64_t one_more[5] = {lim, lim - 9, 5, 5, 1}; // the second reaches top - 10
        CHECK(ransac_out_overlap(addr, one_more, &a, &b) && a == 1 && b == 2);
        const int64_t first[5] = {lim, lim - 20, 5, 6, 1}; // the fourth reaches top
        CHECK(ransac_out_overlap(addr, first, &a, &b) && a == 3 && b == 4);
        const uint64_t low[5] = {0x7ffffffffffffff0ull, 0x7ffffffffffffff8ull, 8, 16, 24};
        const int64_t eight[5] = {8, lim, 8, 8, 8};
        CHECK(!ransac_out_overlap(low, eight, &a, &b));
        const int64_t nine[5] = {9, lim, 8, 8, 8};
        CHECK(ransac_out_overlap(low, nine, &a, &b) && a == 0 && b == 1);
    }
    std::printf("ok\n");
    return 0;
}
