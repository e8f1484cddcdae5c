// The runs of mp_lsq_fit_set's entries and its argument checks: plain C++, no HIP, so they are
// checked on the CPU under a sanitizer (tests/lsq_subset_check.cpp).
//
// An entry of pair size n owns a workspace slice of 6 n ints: its three wide lists (3 n), then
// its subset's three lists (3 n).  Entries are cut, in order, into runs whose wide-list slices
// total at most kLsqRunWideInts ints, so the workspace is bounded whatever the call's size; a
// run of one entry is always allowed.  entry_chunk > 0 also bounds a run's entries (the
// invariance tests); results depend on neither.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../include/mp_subset.h"

namespace mp {

constexpr int64_t kLsqRunWideInts = int64_t(1) << 26; // 256 MiB of wide lists, as much again for the subsets
constexpr int32_t kLsqEntriesMax = 1 << 24;           // entries of one call

struct LsqRun {
    int32_t e0, e1; // entries e0 .. e1 - 1
};

// n[e]: the pair size of entry e (each at most 2^28)
inline std::vector<LsqRun> lsq_fit_runs(int32_t num_entries, const int64_t *n, int64_t entry_chunk,
                                        int64_t wide_ints = kLsqRunWideInts) {
    std::vector<LsqRun> runs;
    int32_t e0 = 0;
    int64_t sum = 0;
    for (int32_t e = 0; e < num_entries; ++e) {
        const int64_t w = 3 * n[e];
        const bool full = e > e0 && (sum + w > wide_ints || (entry_chunk > 0 && e - e0 >= entry_chunk));
        if (full) {
            runs.push_back(LsqRun{e0, e});
            e0 = e;
            sum = 0;
        }
        sum += w;
    }
    if (num_entries > e0) runs.push_back(LsqRun{e0, num_entries});
    return runs;
}

// The entries of a call on a set of num_pairs pairs.  pair_ids null: entry e is pair e and
// num_entries must be the pair count; otherwise any indices in range -- a pair MAY repeat
// (each entry has its own workspace slice; check_selection, which the other stages use, still
// refuses repeats).  Throws std::invalid_argument naming the position.
inline void check_lsq_entries(int32_t num_pairs, int32_t num_entries, const int32_t *pair_ids,
                              const int32_t *solver_types, const double *factors, int rule, const int32_t *streams,
                              const int32_t *substreams, int64_t entry_chunk) {
    if (num_entries < 0) throw std::invalid_argument("negative entry count");
    if (num_entries > kLsqEntriesMax) throw std::invalid_argument("more than 2^24 entries");
    if (rule != kSubsetLsq && rule != kSubsetNonmin) throw std::invalid_argument("rule must be 0 (lsq) or 1 (nonmin)");
    if (entry_chunk < 0) throw std::invalid_argument("entry_chunk must not be negative");
    if (!pair_ids && num_entries != num_pairs)
        throw std::invalid_argument("pair_ids is null: num_entries must equal the set's pair count (" +
                                    std::to_string(num_pairs) + ")");
    if (num_entries == 0) return;
    if (!solver_types || !factors || !streams || !substreams)
        throw std::invalid_argument("null solver_types, factors, streams or substreams");
    for (int32_t e = 0; e < num_entries; ++e) {
        const std::string at = "[" + std::to_string(e) + "]";
        if (pair_ids && (pair_ids[e] < 0 || pair_ids[e] >= num_pairs))
            throw std::invalid_argument("pair_ids" + at + " = " + std::to_string(pair_ids[e]) + " is outside the set");
        if (solver_types[e] != 0 && solver_types[e] != 1)
            throw std::invalid_argument("solver_types" + at + " must be 0 (MD) or 1 (point)");
        if (!(factors[e] > 0.0) || !(factors[e] <= 1.7976931348623157e308))
            throw std::invalid_argument("factors" + at + " must be positive and finite");
        if (streams[e] < 0) throw std::invalid_argument("streams" + at + " must be in 0 .. 2^31 - 1");
        if (substreams[e] < 0 || (uint32_t)substreams[e] >= kSubsetSubstreamMax)
            throw std::invalid_argument("substreams" + at + " must be in 0 .. 2^30 - 1");
    }
}

} // namespace mp
