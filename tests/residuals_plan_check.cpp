// Stand-alone check of madpose_amd/csrc/host/residuals_plan.h, built and run by
// tests/test_residuals_cpu.py under AddressSanitizer and UBSan: the row offsets, the cut into
// items and into runs, and the extent arithmetic of caller-owned outputs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

// One call: entries of the given sizes on the given pairs, cut into runs under (max_rows,
// max_entries); device: the outputs are the whole call's (row_base 0), else a run's scratch.
static void check_call(const std::vector<int64_t> &n, const std::vector<int32_t> &pairs, bool with_pairs,
                       bool with_factors, int64_t max_rows, int32_t max_entries, bool device) {
    const int32_t ne = (int32_t)n.size();
    std::vector<int64_t> off((size_t)ne + 1, -1);
    resid_offsets(ne, n.data(), off.data());
    CHECK(off[0] == 0);
    for (int32_t e = 0; e < ne; ++e) CHECK(off[(size_t)e + 1] - off[(size_t)e] == n[(size_t)e]);
    const int64_t R = off[(size_t)ne];
    std::vector<double> factors((size_t)ne);
    for (int32_t e = 0; e < ne; ++e) factors[(size_t)e] = 1.0 + 0.25 * e;

    std::vector<ResidRun> runs;
    resid_runs(ne, off.data(), max_rows, max_entries, runs);
    // every row of the call, and which entry covered it
    std::vector<int> seen((size_t)R, 0);
    int32_t next = 0;
    for (const ResidRun &r : runs) {
        CHECK(r.e0 == next && r.e1 > r.e0 && r.e1 <= ne);
        next = r.e1;
        CHECK(r.row0 == off[(size_t)r.e0] && r.rows == off[(size_t)r.e1] - off[(size_t)r.e0]);
        // the bound: rows and entries, but for a run of one entry
        CHECK(r.e1 - r.e0 <= max_entries);
        CHECK(r.rows <= max_rows || r.e1 - r.e0 == 1);
        // maximal: the next entry would not have fitted
        if (r.e1 < ne)
            CHECK(r.e1 - r.e0 == max_entries || off[(size_t)r.e1 + 1] - off[(size_t)r.e0] > max_rows);
        std::vector<ResidItem> items;
        std::vector<int64_t> first_item;
        const int64_t base = device ? 0 : r.row0;
        resid_items(r, with_pairs ? pairs.data() : nullptr, with_factors ? factors.data() : nullptr, off.data(), base,
                    items, first_item);
        CHECK((int32_t)first_item.size() == r.e1 - r.e0 + 1);
        CHECK(first_item.front() == 0 && first_item.back() == (int64_t)items.size());
        CHECK((int64_t)items.size() <= (int64_t)(r.e1 - r.e0) + r.rows / kResidItemRows);
        for (int32_t e = r.e0; e < r.e1; ++e) {
            const int64_t j0 = first_item[(size_t)(e - r.e0)], j1 = first_item[(size_t)(e - r.e0) + 1];
            const int64_t want = (n[(size_t)e] + kResidItemRows - 1) / kResidItemRows;
            CHECK(j1 - j0 == want); // (n = 0: no item)
            int64_t at = 0;
            for (int64_t j = j0; j < j1; ++j) {
                const ResidItem &it = items[(size_t)j];
                CHECK(it.rec == e - r.e0);
                CHECK(it.pair == (with_pairs ? pairs[(size_t)e] : e));
                CHECK(it.factor == (with_factors ? factors[(size_t)e] : 1.0));
                CHECK(it.first == at && it.count >= 1 && it.count <= kResidItemRows);
                CHECK(j + 1 == j1 || it.count == kResidItemRows);
                // inside the entry, and inside the launch's outputs
                CHECK((int64_t)it.first + it.count <= n[(size_t)e]);
                CHECK(it.row == off[(size_t)e] + it.first - base);
                CHECK(it.row >= 0 && it.row + it.count <= (device ? R : r.rows));
                for (int q = 0; q < it.count; ++q) {
                    const int64_t row = base + it.row + q;
                    CHECK(row >= off[(size_t)e] && row < off[(size_t)e + 1]);
                    ++seen[(size_t)row];
                }
                at += it.count;
            }
            CHECK(at == n[(size_t)e]);
        }
    }
    CHECK(next == ne);
    for (int64_t i = 0; i < R; ++i) CHECK(seen[(size_t)i] == 1);
}

int main() {
    static_assert(kResidItemRows == 4096, "16 trips of 256");
    static_assert(sizeof(ResidItem) == 32 && sizeof(ResidCount) == 16, "record sizes");
    const std::vector<int64_t> edge = {0, 1, 4095, 4096, 4097, 8193};
    // every size alone, and every ordered pair of sizes
    for (int64_t a : edge) {
        check_call({a}, {0}, true, false, 1 << 21, 1 << 15, false);
        check_call({a}, {0}, false, true, 1, 1, true);
        for (int64_t b : edge)
            for (int dev = 0; dev < 2; ++dev) {
                check_call({a, b}, {1, 0}, true, true, 1 << 21, 1 << 15, dev != 0);
                check_call({a, b}, {0, 1}, false, false, 4096, 1 << 15, dev != 0);
            }
    }
    // no entry at all
    check_call({}, {}, false, false, 1 << 21, 1 << 15, false);
    {
        std::vector<ResidRun> runs;
        int64_t off0 = 0;
        resid_runs(0, &off0, 1 << 21, 1 << 15, runs);
        CHECK(runs.empty());
    }
    // repeated pairs; empty entries first, last and in the middle; only empty entries
    const std::vector<int64_t> mixed = {0, 8193, 0, 0, 4096, 1, 4097, 0, 4095, 0};
    const std::vector<int32_t> rep = {3, 1, 1, 3, 0, 2, 1, 2, 1, 0};
    for (int64_t max_rows : {(int64_t)1, (int64_t)4096, (int64_t)8193, (int64_t)12290, (int64_t)1 << 21})
        for (int32_t max_entries : {1, 2, 3, 1 << 15})
            for (int dev = 0; dev < 2; ++dev) check_call(mixed, rep, true, true, max_rows, max_entries, dev != 0);
    check_call({0, 0, 0}, {0, 0, 0}, true, false, 1 << 21, 1 << 15, false);
    check_call({0, 0, 0}, {0, 1, 2}, false, false, 1, 2, true);
    // the library's constants: a run of the bound's rows at 25 bytes a row stays a fixed size
    CHECK(kResidRunRows > 0 && kResidRunRows * 25 <= ((int64_t)1 << 26));
    CHECK(kResidRunEntries >= 1 && kResidEntriesMax == 1 << 24);
    // ... and a run into caller-owned device outputs has a bounded number of items
    CHECK(kResidRunRowsDevice >= kResidRunRows && kResidRunRowsDevice / kResidItemRows + kResidRunEntries <= 1 << 16);

    // ---- extent arithmetic ----
    const int64_t lim = std::numeric_limits<int64_t>::max();
    CHECK(resid_mask_bytes(0) == 0 && resid_error_bytes(0) == 0);
    CHECK(resid_mask_bytes(8193) == 8193 && resid_error_bytes(8193) == 3 * 8 * 8193);
    CHECK(resid_mask_bytes(lim) == lim);
    CHECK(resid_mask_bytes(-1) == -1 && resid_error_bytes(-1) == -1);
    CHECK(resid_error_bytes(lim / 24) == (lim / 24) * 24);
    CHECK(resid_error_bytes(lim / 24 + 1) == -1); // (would leave int64)
    CHECK(resid_error_bytes(lim / 3) == -1 && resid_error_bytes(lim / 3 + 1) == -1 && resid_error_bytes(lim) == -1);
    // the range check takes the refused count and addresses at the top of the address space
    const uint64_t top = std::numeric_limits<uint64_t>::max();
    CHECK(ingest_extent_error(4096, 4096, 1 << 20, resid_error_bytes(lim), 8) != nullptr);
    CHECK(ingest_extent_error(top - 7, top - 4095, 4095, 8, 8) != nullptr);  // ends past the allocation
    CHECK(ingest_extent_error(top - 15, top - 4095, 4095, 8, 8) == nullptr); // (ptr + bytes would be fine too)
    CHECK(ingest_extent_error(top - 4095 + 4088, top - 4095, 4095, 8, 8) != nullptr);
    CHECK(ingest_extent_error(4097, 4096, 1 << 20, 100, 1) == nullptr); // the mask: any byte offset
    CHECK(ingest_extent_error(4097, 4096, 1 << 20, 8, 8) != nullptr);   // the errors: aligned to 8
    CHECK(ingest_extent_error(4096, 4096, 100, 100, 1) == nullptr);
    CHECK(ingest_extent_error(4096, 4096, 100, 101, 1) != nullptr); // one element short
    CHECK(ingest_extent_error(4095, 4096, 100, 1, 1) != nullptr);
    CHECK(ingest_extent_error(4096, 4096, lim, lim, 1) == nullptr);
    // overlap: differences only, also at the top of the address space
    CHECK(!resid_overlap(100, 10, 110, 10) && !resid_overlap(110, 10, 100, 10));
    CHECK(resid_overlap(100, 11, 110, 10) && resid_overlap(110, 10, 100, 11));
    CHECK(resid_overlap(100, 10, 100, 1) && resid_overlap(100, 100, 150, 1) && resid_overlap(150, 1, 100, 100));
    CHECK(!resid_overlap(100, 0, 100, 10) && !resid_overlap(100, 10, 105, 0) && !resid_overlap(100, -1, 100, 10));
    CHECK(resid_overlap(top - 10, lim, top - 5, 1) && !resid_overlap(top - 10, 5, top - 5, 5));
    CHECK(resid_overlap(0, lim, top / 4, lim) && !resid_overlap(0, lim, (uint64_t)lim, lim));
    std::printf("ok\n");
    return 0;
}
