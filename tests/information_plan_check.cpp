// Stand-alone check of madpose_amd/csrc/host/information_plan.h, built and run by
// tests/test_information_cpu.py under AddressSanitizer and UBSan: the cut of a call into runs and
// items, the partial records an entry's finishing workgroup adds, the workspace and output byte
// counts, the pairwise overlap test, and the active columns.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "information_plan.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// One call as information_set plans it: entries of the given sizes, runs under (max_rows,
// max_entries); per run the items, and per entry the partial records first_item .. + nitems - 1
// and its row of the outputs (device: the call's row e; host: the run's scratch row e - e0).
static void check_call(const std::vector<int64_t> &n, const std::vector<int32_t> &pairs, int64_t max_rows,
                       int32_t max_entries, bool device) {
    const int32_t ne = (int32_t)n.size();
    std::vector<int64_t> off((size_t)ne + 1, -1);
    resid_offsets(ne, n.data(), off.data());
    const int64_t R = off[(size_t)ne];
    std::vector<ResidRun> runs;
    resid_runs(ne, off.data(), max_rows, max_entries, runs);
    std::vector<int> seen((size_t)R, 0), out_seen((size_t)ne, 0);
    int32_t next = 0;
    for (const ResidRun &r : runs) {
        CHECK(r.e0 == next && r.e1 > r.e0 && r.e1 <= ne);
        next = r.e1;
        CHECK(r.e1 - r.e0 <= max_entries);
        CHECK(r.rows <= max_rows || r.e1 - r.e0 == 1);
        if (r.e1 < ne) CHECK(r.e1 - r.e0 == max_entries || off[(size_t)r.e1 + 1] - off[(size_t)r.e0] > max_rows);
        std::vector<ResidItem> items;
        std::vector<int64_t> first_item;
        resid_items(r, pairs.data(), nullptr, off.data(), r.row0, items, first_item);
        // the workspace of the run holds every item's partial record
        CHECK((int64_t)items.size() <= info_max_items(r));
        CHECK(info_workspace_bytes(info_max_items(r)) == info_max_items(r) * kInfoPartialBytes);
        std::vector<int> part_used(items.size(), 0);
        for (int32_t e = r.e0; e < r.e1; ++e) {
            InfoJob J{};
            J.first_item = first_item[(size_t)(e - r.e0)];
            J.nitems = (int)(first_item[(size_t)(e - r.e0) + 1] - J.first_item);
            J.out_row = device ? (int64_t)e : (int64_t)(e - r.e0);
            CHECK(J.nitems == (n[(size_t)e] + kInfoItemRows - 1) / kInfoItemRows); // (a function of n alone)
            CHECK(J.out_row >= 0 && J.out_row < (device ? ne : r.e1 - r.e0));
            ++out_seen[(size_t)(device ? J.out_row : J.out_row + r.e0)];
            int64_t at = 0;
            for (int k = 0; k < J.nitems; ++k) {
                const int64_t j = J.first_item + k;
                CHECK(j >= 0 && j < (int64_t)items.size());
                ++part_used[(size_t)j];
                const ResidItem &it = items[(size_t)j];
                // the item is the entry's: its record, its pair, consecutive rows in item order
                CHECK(it.rec == e - r.e0 && it.pair == pairs[(size_t)e]);
                CHECK(it.first == at && it.count >= 1 && it.count <= kInfoItemRows);
                CHECK(k + 1 == J.nitems || it.count == kInfoItemRows);
                CHECK((int64_t)it.first + it.count <= n[(size_t)e]);
                for (int q = 0; q < it.count; ++q) ++seen[(size_t)(off[(size_t)e] + it.first + q)];
                at += it.count;
            }
            CHECK(at == n[(size_t)e]);
        }
        for (int u : part_used) CHECK(u == 1); // no item crosses entries; none is left over
    }
    CHECK(next == ne);
    for (int64_t i = 0; i < R; ++i) CHECK(seen[(size_t)i] == 1);
    for (int32_t e = 0; e < ne; ++e) CHECK(out_seen[(size_t)e] == 1);
}

int main() {
    static_assert(kInfoItemRows == 4096, "16 trips of 256");
    static_assert(kInfoN == 11 && kInfoPack == 66 && kInfoRed == 78, "the full layout");
    static_assert(sizeof(InfoPartial) == 78 * 8 + 16 && sizeof(InfoRecord) == 17 * 4, "record sizes");
    static_assert(sizeof(InfoJob) == 17 * 8 + 8 + 16 + 16, "InfoJob");
    const int64_t I = kInfoItemRows;
    const std::vector<int64_t> edge = {0, 1, I - 1, I, I + 1, 3 * I + 1};
    for (int64_t a : edge) {
        check_call({a}, {0}, kInfoRunRows, kInfoRunEntries, false);
        check_call({a}, {0}, 1, 1, true);
        for (int64_t b : edge)
            for (int dev = 0; dev < 2; ++dev) {
                check_call({a, b}, {1, 0}, kInfoRunRows, kInfoRunEntries, dev != 0);
                check_call({a, b}, {0, 0}, I, kInfoRunEntries, dev != 0);
            }
    }
    check_call({}, {}, kInfoRunRows, kInfoRunEntries, false);
    // repeated pairs; empty entries first, last and in the middle; only empty entries; run cuts
    const std::vector<int64_t> mixed = {0, 3 * I + 1, 0, 0, I, 1, I + 1, 0, I - 1, 0};
    const std::vector<int32_t> rep = {3, 1, 1, 3, 0, 2, 1, 2, 1, 0};
    for (int64_t max_rows : {(int64_t)1, I, 2 * I + 1, 3 * I + 2, kInfoRunRows})
        for (int32_t max_entries : {1, 2, 3, kInfoRunEntries})
            for (int dev = 0; dev < 2; ++dev) check_call(mixed, rep, max_rows, max_entries, dev != 0);
    check_call({0, 0, 0}, {0, 1, 2}, 1, 2, true);
    // the library's constants: a run's records, items and scratch stay a fixed size
    CHECK(kInfoRunRows / kInfoItemRows + kInfoRunEntries <= 1 << 14);
    CHECK((int64_t)kInfoRunEntries * (kInfoRed + kInfoN * kInfoN) * 8 <= (int64_t)1 << 24);
    CHECK(kInfoEntriesMax == 1 << 24);

    // ---- byte counts at the int64 edge ----
    const int64_t lim = std::numeric_limits<int64_t>::max();
    CHECK(info_H_bytes(0) == 0 && info_g_bytes(0) == 0 && info_cost_bytes(0) == 0 && info_cov_bytes(0) == 0);
    CHECK(info_H_bytes(3) == 3 * 66 * 8 && info_g_bytes(3) == 3 * 88 && info_cost_bytes(3) == 24 &&
          info_cov_bytes(3) == 3 * 968);
    CHECK(info_H_bytes(-1) == -1 && info_cov_bytes(-1) == -1 && info_workspace_bytes(-1) == -1);
    CHECK(info_cov_bytes(lim / 968) == (lim / 968) * 968 && info_cov_bytes(lim / 968 + 1) == -1);
    CHECK(info_H_bytes(lim / 528) == (lim / 528) * 528 && info_H_bytes(lim / 528 + 1) == -1);
    CHECK(info_g_bytes(lim / 88 + 1) == -1 && info_cost_bytes(lim / 8) == (lim / 8) * 8 &&
          info_cost_bytes(lim / 8 + 1) == -1 && info_cost_bytes(lim) == -1);
    CHECK(info_workspace_bytes(lim / kInfoPartialBytes) == (lim / kInfoPartialBytes) * kInfoPartialBytes);
    CHECK(info_workspace_bytes(lim / kInfoPartialBytes + 1) == -1);
    // the range check refuses a refused count
    CHECK(ingest_extent_error(4096, 4096, 1 << 20, info_cov_bytes(lim), 8) != nullptr);
    CHECK(ingest_extent_error(4096, 4096, 968, info_cov_bytes(1), 8) == nullptr);
    CHECK(ingest_extent_error(4096, 4096, 967, info_cov_bytes(1), 8) != nullptr);
    CHECK(ingest_extent_error(4100, 4096, 1 << 20, info_g_bytes(1), 8) != nullptr); // aligned to 8

    // ---- the pairwise overlap test: touching, nested, absent, the top of the address space ----
    int a = -1, b = -1;
    {
        const uint64_t addr[4] = {1000, 1528, 1616, 1624}; // one entry, back to back: touching only
        const int64_t by[4] = {528, 88, 8, 968};
        CHECK(!info_out_overlap(addr, by, &a, &b));
    }
    {
        const uint64_t addr[4] = {1000, 1527, 1616, 1624}; // g starts on H's last byte
        const int64_t by[4] = {528, 88, 8, 968};
        CHECK(info_out_overlap(addr, by, &a, &b) && a == 0 && b == 1);
    }
    {
        const uint64_t addr[4] = {5000, 100, 2000, 1624}; // cost nested inside cov
        const int64_t by[4] = {528, 88, 8, 968};
        CHECK(info_out_overlap(addr, by, &a, &b) && a == 2 && b == 3);
    }
    {
        const uint64_t addr[4] = {1000, 0, 1000, 1000}; // absent arrays and empty extents share nothing
        const int64_t by[4] = {528, 88, 0, -1};
        CHECK(!info_out_overlap(addr, by, &a, &b));
    }
    {
        const uint64_t top = std::numeric_limits<uint64_t>::max();
        const uint64_t addr[4] = {top - 10, top - 5, 8, 16};
        const int64_t by[4] = {5, 5, 8, lim};
        CHECK(!info_out_overlap(addr, by, &a, &b));
        const int64_t by2[4] = {6, 5, 8, lim};
        CHECK(info_out_overlap(addr, by2, &a, &b) && a == 0 && b == 1);
        const int64_t by3[4] = {5, 5, 9, lim};
        CHECK(info_out_overlap(addr, by3, &a, &b) && a == 2 && b == 3);
    }

    // ---- the active columns (lm_setup.inc's) ----
    int32_t col[11], status = -1, rows = -1;
    auto is = [&](std::initializer_list<int> want) {
        int k = 0;
        for (int w : want) CHECK(col[k++] == w);
        CHECK(k == 11);
    };
    info_columns(kCal, 0, 0, 0, 1, col, &status, &rows);
    is({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
    CHECK(status == 0 && rows == 0);
    info_columns(kTF, 0, 0, 0, 1, col, &status, &rows);
    is({0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
    info_columns(kCal, 3, 2, 5, 1, col, &status, &rows);
    is({1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0});
    CHECK(status == 1 && rows == 2 * 5 + 5);
    info_columns(kCal, 3, 2, 5, 0, col, &status, &rows);
    is({1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0});
    info_columns(kSF, 0, 0, 7, 1, col, &status, &rows);
    is({1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0});
    CHECK(status == 1 && rows == 7);
    info_columns(kTF, 4, 0, 0, 1, col, &status, &rows);
    is({1, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1});
    info_columns(kTF, 0, 4, 0, 1, col, &status, &rows);
    is({1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1});
    CHECK(rows == 8);
    std::printf("ok\n");
    return 0;
}
