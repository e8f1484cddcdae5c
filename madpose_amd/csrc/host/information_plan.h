// Plan and output-extent arithmetic of the information stage (mp_information_set;
// kernels/information.h): plain C++, no HIP, so it is checked on the CPU under a sanitizer
// (tests/information_plan_check.cpp).
//
// A call has ne entries; entry e is a model on a pair of n[e] correspondences (a pair may occur
// in any number of entries) and owns row e of every output: 66 doubles of H, 11 of g, one cost,
// 121 of cov, and one InfoRecord that always returns to the host.
//   * A work item (one workgroup of information_kernel) is one entry and up to kInfoItemRows =
//     kResidItemRows = 4096 consecutive rows of it: the cut of the residuals stage, whose
//     offsets, runs and items (resid_offsets, resid_runs, resid_items) are used as they are.
//     The item size depends on nothing but the entry's n: an entry of n rows has
//     ceil(n / kInfoItemRows) items, none for n = 0.  Sixteen trips of 256 rows carry the fixed
//     cost of an item, the reduction of 78 sums over the workgroup and a partial record of
//     kInfoPartialBytes bytes.
//   * Item j of a run writes partial record j of the run's workspace; information_finish_kernel
//     adds the records first_item .. first_item + nitems - 1 of an entry in that order.
//   * Entries go through the device in runs of consecutive entries of at most kInfoRunRows rows
//     and kInfoRunEntries entries, always at least one entry: records, items, partials and (for
//     host outputs) the scratch of a run are bounded by constants and the largest single entry.
// An entry's outputs depend on the entry alone, so no cut changes a result.
// Byte counts of caller-owned outputs are ingest_bytes' (overflow-checked), the range check is
// ingest_extent_error's and the overlap test forms differences only.
#pragma once
#include <cstdint>
#include <vector>

#include "../include/mp_information.h"
#include "residuals_plan.h"

namespace mp {

constexpr int kInfoItemRows = kResidItemRows;  // rows per item: 16 trips of kBlock
constexpr int64_t kInfoRunRows = 1 << 22;      // rows per run: at most 2^10 items beside one per entry
constexpr int32_t kInfoRunEntries = 1 << 13;   // entries per run (host outputs: 199 doubles of scratch each)
constexpr int32_t kInfoEntriesMax = kResidEntriesMax; // entries per call
constexpr int kInfoArrays = 4;                 // the caller-owned outputs: H, g, cost, cov

// One item's outcome: the sums of its rows' blocks in the full 11-parameter layout (H packed 66,
// then g 11, then the cost) and its three inlier counts before gating.
struct InfoPartial {
    double v[kInfoRed];
    int count[3], pad;
};
constexpr int64_t kInfoPartialBytes = (int64_t)sizeof(InfoPartial);

// One entry of a run, read by both kernels: the model in problem units, the job flags of
// make_lm_job (w_sampson, use_shift, and which block types the LO type leaves), the entry's
// partial records and the row of the launch's outputs it owns.
struct InfoJob {
    double m[17]; // Model
    double w_sampson;
    int use_reproj, use_sampson, use_shift, nitems;
    int64_t first_item, out_row;
};

// The per-entry record (mp_information_entry): the active mask, pd (1 inverted, 0 not positive
// definite, -1 nothing evaluated), status (1: at least one block), rows = 2 (n0 + n1) + n2 after
// gating, and the three inlier counts before gating.
struct InfoRecord {
    int32_t col[kInfoN];
    int32_t pd, status, rows;
    int32_t counts[3];
};

// Items a run can have at most: an entry of n rows has ceil(n / kInfoItemRows) <= n /
// kInfoItemRows + 1 items
inline int64_t info_max_items(const ResidRun &r) { return (int64_t)(r.e1 - r.e0) + r.rows / kInfoItemRows; }

// Bytes of a workspace of `items` partial records; -1 when the count leaves int64
inline int64_t info_workspace_bytes(int64_t items) { return ingest_bytes(items, 1, kInfoPartialBytes); }

// Bytes of the caller-owned outputs for ne entries; -1 when the count leaves int64
inline int64_t info_H_bytes(int64_t ne) { return ingest_bytes(ne, kInfoPack, 8); }
inline int64_t info_g_bytes(int64_t ne) { return ingest_bytes(ne, kInfoN, 8); }
inline int64_t info_cost_bytes(int64_t ne) { return ingest_bytes(ne, 1, 8); }
inline int64_t info_cov_bytes(int64_t ne) { return ingest_bytes(ne, kInfoN * kInfoN, 8); }

// The first two of the kInfoArrays extents (address, bytes; a null address or bytes <= 0: not
// given) that share a byte: their indices to *a < *b and true, or false.  Differences only.
inline bool info_out_overlap(const uint64_t *addr, const int64_t *bytes, int *a, int *b) {
    for (int i = 0; i < kInfoArrays; ++i)
        for (int j = i + 1; j < kInfoArrays; ++j) {
            if (!addr[i] || !addr[j]) continue;
            if (resid_overlap(addr[i], bytes[i], addr[j], bytes[j])) {
                *a = i, *b = j;
                return true;
            }
        }
    return false;
}

// The active mask, status and rows of an entry from its gated block counts and flags: the
// columns of lm_setup.inc (kernels/), which are lm_refine's.  variant: kCal / kSF / kTF.
MP_HD void info_columns(int variant, int n0, int n1, int n2, int use_shift, int32_t *col, int32_t *status,
                        int32_t *rows) {
    const bool any = n0 + n1 + n2 > 0;
    const bool has_o0 = n0 > 0, has_s_o1 = n1 > 0;
    for (int k = 0; k < kInfoN; ++k) col[k] = 0;
    if (any) {
        for (int k = 0; k < 6; ++k) col[k] = 1;
        if (has_s_o1) col[6] = 1;
        if (has_o0 && use_shift) col[7] = 1;
        if (has_s_o1 && use_shift) col[8] = 1;
        if (variant == kSF) col[9] = 1;
        if (variant == kTF) col[9] = col[10] = 1;
    }
    *status = any ? 1 : 0;
    *rows = 2 * (n0 + n1) + n2;
}

} // namespace mp
