// Slab and work-item planning of mp_select_batch: plain C++, no HIP, so the index
// arithmetic is checked on the CPU under a sanitizer (tests/select_plan_check.cpp).
//
// The pairs of a run (host/refine_plan.h) are resident at once; their candidates, M in
// all, are numbered 0 .. M - 1 in pair order (pair k of the run owns moff[k] - moff[0] ..
// moff[k + 1] - moff[0]).  The score records of `model_chunk` consecutive candidates -- a
// slab -- are on the device at a time; a slab may cut through a pair's candidates.  A slab
// is cut into work items, one workgroup each: up to `tile` consecutive candidates of one
// pair, never across a pair boundary or the slab's end.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../include/mp_types.h"

namespace mp {

constexpr int64_t kSelectSlabModels = int64_t(1) << 16; // candidates per slab when model_chunk == 0
constexpr int64_t kSelectModelsMax = int64_t(1) << 28;  // candidates of one call
constexpr int kSelectTile = 1;                          // candidates per work item

struct SelectSlab {
    int64_t m0, m1; // candidates m0 .. m1 - 1 of the run
};
// (SelectItem, mp_types.h: `count` candidates of pair `pair` of the run, their records at
// rec .. rec + count - 1 of the slab)

// M candidates in slabs of model_chunk (0: kSelectSlabModels); none is empty
inline std::vector<SelectSlab> select_slabs(int64_t M, int64_t model_chunk) {
    const int64_t c = model_chunk > 0 ? model_chunk : kSelectSlabModels;
    std::vector<SelectSlab> slabs;
    for (int64_t m = 0; m < M; m += c) slabs.push_back(SelectSlab{m, std::min(M, m + c)});
    return slabs;
}

// The work items of one slab, in candidate order.  moff: the np + 1 non-decreasing
// candidate offsets of the run's pairs (any base: moff[0] is candidate 0 of the run).
inline void select_items(int32_t np, const int64_t *moff, const SelectSlab &s, int tile,
                         std::vector<SelectItem> &items) {
    items.clear();
    if (s.m0 >= s.m1 || np <= 0) return;
    // the pair that owns candidate m0: the last k with moff[k] - moff[0] <= m0
    int32_t k = (int32_t)(std::upper_bound(moff, moff + np + 1, s.m0 + moff[0]) - moff) - 1;
    int64_t m = s.m0;
    while (m < s.m1 && k < np) {
        const int64_t end = std::min(s.m1, moff[k + 1] - moff[0]); // of this pair inside the slab
        for (int64_t a = m; a < end; a += tile) {
            SelectItem it;
            it.pair = k;
            it.rec = (int)(a - s.m0);
            it.count = (int)std::min<int64_t>(tile, end - a);
            it.pad = 0;
            items.push_back(it);
        }
        m = end; // (end >= m: pair k owns m, or starts at it)
        ++k;
    }
}

} // namespace mp
