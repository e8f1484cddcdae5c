// Plan and output-extent arithmetic of the per-correspondence stage (mp_residuals_set;
// kernels/residuals.h): plain C++, no HIP, so it is checked on the CPU under a sanitizer
// (tests/residuals_plan_check.cpp).
//
// A call has ne entries; entry e is a model on a pair of n[e] correspondences (a pair may occur
// in any number of entries).  Its rows are row_off[e] .. row_off[e] + n[e] - 1 of the outputs,
// row_off[e] the sum of n over the entries before e and R = row_off[ne].
//   * A work item (one workgroup) is one entry and up to kResidItemRows consecutive rows of it:
//     16 trips of kBlock = 256, the cut ingest_items makes.  An item never crosses entries and
//     an entry without correspondences has none.
//   * Entries go through the device in runs of consecutive entries.  A run holds at most
//     `max_rows` rows and `max_entries` entries, but always at least one entry, so the records,
//     items and (for host outputs) the device scratch of a run are bounded by constants and by
//     the largest single entry, never by R.
// A row's outputs depend on its entry alone, so neither cut changes a result.
// The byte counts of caller-owned outputs are ingest_bytes' (overflow-checked) and the range
// check is ingest_extent_error's: no sum of an address and a length is formed.
#pragma once
#include <cstdint>
#include <vector>

#include "ingest_plan.h"

namespace mp {

constexpr int kResidItemRows = 4096;           // rows per item: 16 trips of kBlock
constexpr int64_t kResidRunRows = 1 << 21;     // rows per run (host outputs: 25 bytes of scratch each)
constexpr int64_t kResidRunRowsDevice = 1 << 26;  // ... into the caller's device arrays: no scratch, 2^14 items
constexpr int32_t kResidRunEntries = 1 << 15;  // entries (score records) per run
constexpr int32_t kResidEntriesMax = 1 << 24;  // entries per call

// One item of residuals_kernel: rows first .. first + count - 1 of pair `pair` under the run's
// record `rec` and the thresholds times `factor`; row first goes to row `row` of the launch's
// outputs (the following rows after it).
struct ResidItem {
    int rec, pair, first, count;
    int64_t row;
    double factor;
};
// Its outcome: the rows of the item with err_t < thr_t * factor.
struct ResidCount {
    int count[3], pad;
};

struct ResidRun {
    int32_t e0, e1;  // entries e0 .. e1 - 1
    int64_t row0;    // row_off[e0]
    int64_t rows;    // row_off[e1] - row_off[e0]
};

// row_off (ne + 1 values) from the entries' sizes (each 0 .. 2^31 - 1; ne <= 2^24, so no sum
// leaves int64)
inline void resid_offsets(int32_t ne, const int64_t *n, int64_t *row_off) {
    row_off[0] = 0;
    for (int32_t e = 0; e < ne; ++e) row_off[e + 1] = row_off[e] + n[e];
}

// The runs of a call, in entry order; every entry is in exactly one.
inline void resid_runs(int32_t ne, const int64_t *row_off, int64_t max_rows, int32_t max_entries,
                       std::vector<ResidRun> &runs) {
    runs.clear();
    int32_t e0 = 0;
    while (e0 < ne) {
        int32_t e1 = e0 + 1; // (a run of one entry is always allowed)
        while (e1 < ne && e1 - e0 < max_entries && row_off[e1 + 1] - row_off[e0] <= max_rows) ++e1;
        runs.push_back(ResidRun{e0, e1, row_off[e0], row_off[e1] - row_off[e0]});
        e0 = e1;
    }
}

// The items of run r.  pairs (nullable: entry e is pair e), factors (nullable: 1.0); row_base:
// what the launch's outputs start at (the run's row0 for a scratch of the run, 0 for outputs
// of the whole call).  first_item (r.e1 - r.e0 + 1 values): entry e's items are
// first_item[e - e0] .. first_item[e - e0 + 1] - 1.
inline void resid_items(const ResidRun &r, const int32_t *pairs, const double *factors, const int64_t *row_off,
                        int64_t row_base, std::vector<ResidItem> &items, std::vector<int64_t> &first_item) {
    items.clear();
    first_item.assign((size_t)(r.e1 - r.e0) + 1, 0);
    for (int32_t e = r.e0; e < r.e1; ++e) {
        first_item[(size_t)(e - r.e0)] = (int64_t)items.size();
        const int64_t n = row_off[e + 1] - row_off[e];
        for (int64_t first = 0; first < n; first += kResidItemRows) {
            const int64_t left = n - first;
            items.push_back(ResidItem{e - r.e0, pairs ? pairs[e] : e, (int)first,
                                      (int)(left < kResidItemRows ? left : kResidItemRows),
                                      row_off[e] + first - row_base, factors ? factors[e] : 1.0});
        }
    }
    first_item[(size_t)(r.e1 - r.e0)] = (int64_t)items.size();
}

// Bytes of the caller-owned outputs for R rows: the mask (one byte a row) and the errors
// (three doubles a row); -1 when the count leaves int64.
inline int64_t resid_mask_bytes(int64_t R) { return ingest_bytes(R, 1, 1); }
inline int64_t resid_error_bytes(int64_t R) { return ingest_bytes(R, 3, 8); }

// Whether [a, a + la) and [b, b + lb) share a byte (la, lb >= 0): differences only
inline bool resid_overlap(uint64_t a, int64_t la, uint64_t b, int64_t lb) {
    if (la <= 0 || lb <= 0) return false;
    return a <= b ? b - a < (uint64_t)la : a - b < (uint64_t)lb;
}

// ---- the output stage of mp_ransac_out_set (kernels/ransac_out.h) ----
// Its entries are the selected pairs in selection order, each under at most one model: the
// offsets, runs and items are the ones above (row_base 0: the caller's arrays hold the whole
// call).  An entry without a winner keeps its items, marked as fill items: they store mask 0 and
// NaN errors and read no record.  Every entry, also one without a correspondence (which has no
// item), has one per-pair row: the model's 17 doubles, the winner's index and three counts.
constexpr int kResidFill = -1; // ResidItem::rec of a fill item
constexpr int kRansacOutArrays = 5;

struct RansacOutPair {
    double model[17];
    int32_t index, count[3];
};

// resid_items for the output stage: winner[e] != 0 for the entries with a model
inline void ransac_out_items(const ResidRun &r, const int32_t *pairs, const unsigned char *winner,
                             const int64_t *row_off, std::vector<ResidItem> &items, std::vector<int64_t> &first_item) {
    resid_items(r, pairs, nullptr, row_off, 0, items, first_item);
    for (int32_t e = r.e0; e < r.e1; ++e) {
        if (winner[e]) continue;
        for (int64_t j = first_item[(size_t)(e - r.e0)]; j < first_item[(size_t)(e - r.e0) + 1]; ++j)
            items[(size_t)j].rec = kResidFill;
    }
}

// The per-pair row of an entry: the model's bytes, its index and its counts, or zeros, -1 and
// zeros without a winner.
inline RansacOutPair ransac_out_pair(bool winner, const double *model17, int32_t index, const int32_t *count) {
    RansacOutPair p;
    for (int i = 0; i < 17; ++i) p.model[i] = winner ? model17[i] : 0.0;
    p.index = winner ? index : -1;
    for (int t = 0; t < 3; ++t) p.count[t] = winner ? count[t] : 0;
    return p;
}

// Bytes of the caller-owned per-pair outputs for ns entries; -1 when the count leaves int64
inline int64_t ransac_out_models_bytes(int64_t ns) { return ingest_bytes(ns, 17, 8); }
inline int64_t ransac_out_index_bytes(int64_t ns) { return ingest_bytes(ns, 1, 4); }
inline int64_t ransac_out_counts_bytes(int64_t ns) { return ingest_bytes(ns, 3, 4); }

// The first two of the kRansacOutArrays extents (address, bytes; a null address or bytes <= 0: not
// given) that share a byte: their indices to *a < *b and true, or false.  Differences only.
inline bool ransac_out_overlap(const uint64_t *addr, const int64_t *bytes, int *a, int *b) {
    for (int i = 0; i < kRansacOutArrays; ++i)
        for (int j = i + 1; j < kRansacOutArrays; ++j) {
            if (!addr[i] || !addr[j]) continue;
            if (resid_overlap(addr[i], bytes[i], addr[j], bytes[j])) {
                *a = i, *b = j;
                return true;
            }
        }
    return false;
}

} // namespace mp
