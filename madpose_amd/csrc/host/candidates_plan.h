// Host planning of mp_draw_set, mp_candidates_set and mp_ransac_set: plain C++, no HIP, so the
// index arithmetic is checked on the CPU under a sanitizer (tests/candidates_plan_check.cpp).
//
// Samples are numbered as in host/hypothesis_plan.h: 0 .. S - 1 in pair order over the
// selection's entries, entry j owning soff[j] - soff[0] .. soff[j + 1] - soff[0], cut into
// slabs that may cut through an entry.
//   * draw_items: the work items of the device sampler for one slab -- up to
//     kDrawItemSamples consecutive samples of one entry, never across an entry boundary.
//   * CandPlan: the candidates of a call.  The solve stages leave counts[b] models per
//     sample; the candidates of entry j are the models of its samples in sample order and
//     slot order, so over the whole call they are the models in (sample, slot) order.
//     add_slab takes the slabs' counts in order and appends, per model, the sample's index
//     within its entry and the slot (the tags the device writes beside the compacted
//     models, which the engine checks against these), and closes the offsets of every entry
//     whose samples have all been seen; finish closes the rest.
//   * cand_origin: a winner's candidate index within its entry back to (sample, slot).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../include/mp_draw.h"
#include "hypothesis_plan.h"

namespace mp {

// items[i].pair is the entry's position in the selection (the caller maps it to the set's
// pair), s0 the first sample's index within the entry, out its slab position
// first (nullable): entry k's samples are first[k], first[k] + 1, ... of its pair instead of
// 0, 1, ... (a later round of mp_ransac_adaptive_set)
inline void draw_items(int32_t np, const int64_t *soff, const int32_t *first, const HypSlab &s,
                       std::vector<DrawItem> &items) {
    items.clear();
    if (s.s0 >= s.s1 || np <= 0) return;
    int32_t k = (int32_t)(std::upper_bound(soff, soff + np + 1, s.s0 + soff[0]) - soff) - 1;
    int64_t m = s.s0;
    while (m < s.s1 && k < np) {
        const int64_t begin = soff[k] - soff[0];
        const int64_t end = std::min(s.s1, soff[k + 1] - soff[0]);
        for (int64_t a = m; a < end; a += kDrawItemSamples) {
            DrawItem it;
            it.pair = k;
            it.s0 = (int)(a - begin) + (first ? first[k] : 0);
            it.count = (int)std::min<int64_t>(kDrawItemSamples, end - a);
            it.out = (int)(a - s.s0);
            items.push_back(it);
        }
        m = std::max(m, end);
        ++k;
    }
}
inline void draw_items(int32_t np, const int64_t *soff, const HypSlab &s, std::vector<DrawItem> &items) {
    draw_items(np, soff, nullptr, s, items);
}

struct CandPlan {
    int32_t np = 0;
    const int64_t *soff = nullptr;
    int maxm = 0;
    std::vector<int64_t> moff;         // np + 1: entry j's candidates are moff[j] .. moff[j + 1] - 1
    std::vector<int32_t> sample, slot; // per candidate: the sample within its entry, the slot
    std::vector<int32_t> slab_pos;     // of the last add_slab: per model its slab position
    int64_t seen = 0;                  // samples taken so far
    int32_t open = 0;                  // the first entry whose offsets are not closed

    void begin(int32_t np_, const int64_t *soff_, int maxm_) {
        np = np_;
        soff = soff_;
        maxm = maxm_;
        moff.assign((size_t)np + 1, 0);
        sample.clear();
        slot.clear();
        slab_pos.clear();
        seen = 0;
        open = 0;
    }
    // the counts of the slab's samples (s.s1 - s.s0 values); slabs come in order without
    // gaps.  Returns the slab's number of models.
    int64_t add_slab(const HypSlab &s, const int32_t *counts) {
        if (s.s0 != seen || s.s1 < s.s0 || s.s1 > soff[np] - soff[0])
            throw std::logic_error("candidates: slabs out of order");
        slab_pos.clear();
        const int64_t before = (int64_t)sample.size();
        for (int64_t g = s.s0; g < s.s1; ++g) {
            // the entry that owns sample g; the entries before it are complete
            while (open < np && soff[open + 1] - soff[0] <= g) moff[(size_t)++open] = (int64_t)sample.size();
            const int32_t c = counts[g - s.s0];
            if (c < 0 || c > maxm)
                throw std::runtime_error("candidates: model count of sample " + std::to_string(g) + " out of range");
            for (int32_t i = 0; i < c; ++i) {
                sample.push_back((int32_t)(g - (soff[open] - soff[0])));
                slot.push_back(i);
                slab_pos.push_back((int32_t)(g - s.s0));
            }
        }
        seen = s.s1;
        return (int64_t)sample.size() - before;
    }
    void finish() {
        if (seen != soff[np] - soff[0]) throw std::logic_error("candidates: samples missing");
        while (open < np) moff[(size_t)++open] = (int64_t)sample.size();
    }
};

// candidate `index` (within entry j, as mp_select_set's best_index) of a finished plan
inline void cand_origin(const CandPlan &P, int32_t j, int32_t index, int32_t *sample, int32_t *slot) {
    if (j < 0 || j >= P.np || index < 0 || index >= P.moff[(size_t)j + 1] - P.moff[(size_t)j])
        throw std::logic_error("candidates: no such candidate");
    *sample = P.sample[(size_t)(P.moff[(size_t)j] + index)];
    *slot = P.slot[(size_t)(P.moff[(size_t)j] + index)];
}

} // namespace mp
