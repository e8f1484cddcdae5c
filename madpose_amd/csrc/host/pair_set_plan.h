// Work items of the multi-pair preparation launch (kernels.hip prep_pairs_kernel) and the
// selection check of the pair-set calls (mp_*_set): plain C++, no HIP, so both are checked
// on the CPU under a sanitizer (tests/pair_set_plan_check.cpp).
//
// An item is one 256-thread workgroup: `count` (1 .. kPrepItemMax) consecutive
// correspondences of one pair, starting at `first` inside the pair.  An item never crosses
// a pair, and a pair without correspondences gives none.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace mp {

constexpr int kPrepItemMax = 256; // correspondences per item == threads per workgroup
// correspondences of one pair set (MP_PAIR_SET_MAX_CORRESPONDENCES): 120 bytes resident
// each (12 doubles and 2 x 3 ints, host/refine_plan.h refine_run_bytes), 7.5 GiB at the bound
constexpr int64_t kPairSetMaxCorr = int64_t(1) << 26;

struct PrepItem {
    int pair, first, count, pad;
};

// n[k]: the correspondences of pair k (0 .. np - 1, each below 2^31)
inline void prep_items(int np, const int64_t *n, std::vector<PrepItem> &items) {
    items.clear();
    for (int k = 0; k < np; ++k)
        for (int64_t first = 0; first < n[k]; first += kPrepItemMax) {
            const int64_t left = n[k] - first;
            items.push_back(PrepItem{k, (int)first, (int)(left < kPrepItemMax ? left : kPrepItemMax), 0});
        }
}

// The selection of a call on a set of `num_pairs` pairs.  pair_ids null: all pairs in
// order, num_sel must be the set's pair count.  Otherwise num_sel indices, each in range
// and at most once (two items of one pair would share its list buffers).  Throws
// std::invalid_argument naming the position; `seen` is scratch.
inline void check_selection(int32_t num_pairs, int32_t num_sel, const int32_t *pair_ids, std::vector<char> &seen) {
    if (num_sel < 0) throw std::invalid_argument("negative selection size");
    if (!pair_ids) {
        if (num_sel != num_pairs)
            throw std::invalid_argument("pair_ids is null: num_sel must equal the set's pair count (" +
                                        std::to_string(num_pairs) + ")");
        return;
    }
    seen.assign((size_t)(num_pairs > 0 ? num_pairs : 0), 0);
    for (int32_t j = 0; j < num_sel; ++j) {
        const int32_t k = pair_ids[j];
        if (k < 0 || k >= num_pairs)
            throw std::invalid_argument("pair_ids[" + std::to_string(j) + "] = " + std::to_string(k) +
                                        " is outside the set");
        if (seen[(size_t)k])
            throw std::invalid_argument("pair_ids[" + std::to_string(j) + "] = " + std::to_string(k) +
                                        " occurs twice");
        seen[(size_t)k] = 1;
    }
}

} // namespace mp
