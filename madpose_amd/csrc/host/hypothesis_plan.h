// Slab and work-item planning of mp_hypothesize_batch: plain C++, no HIP, so the index
// arithmetic is checked on the CPU under a sanitizer (tests/hypothesis_plan_check.cpp).
//
// The pairs of a run (host/refine_plan.h) are resident at once; their samples, S in all,
// are numbered 0 .. S - 1 in pair order (pair k of the run owns soff[k] - soff[0] ..
// soff[k + 1] - soff[0]).  `sample_chunk` consecutive samples -- a slab -- are on the device
// at a time; a slab may cut through a pair's samples.  Inside a slab a sample has a
// position (its number minus the slab's first).  Per solver type (0 the MD solver, 1 the
// point solver) the slab has a list: the positions of the type's samples, pair by pair and
// ascending inside a pair -- so ascending overall.  A list is cut into work items, one
// workgroup each: up to `cap` consecutive list entries of one pair, never across a pair
// boundary.  The cap is the solve kernels' samples per workgroup.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../include/mp_types.h"

namespace mp {

constexpr int64_t kHypSlabSamples = 32768;             // samples per slab when sample_chunk == 0
constexpr int64_t kHypSlabSamplesMax = int64_t(1) << 17; // a larger sample_chunk is cut to this
constexpr int64_t kHypSamplesMax = int64_t(1) << 22;   // samples of one call

// samples per workgroup: the exact MD solver at R lanes per sample (64 / R; R = 2 shared
// focal, 4 otherwise), the 16-lane groups of the 5pt root stage and the 6pt pencil (4), one
// lane per sample of the 7pt root stage (64)
constexpr int hyp_md_cap(int v) { return v == kSF ? 32 : 16; }
constexpr int hyp_pt_cap(int v) { return v == kTF ? 64 : 4; }

struct HypSlab {
    int64_t s0, s1; // samples s0 .. s1 - 1 of the run
};

// S samples in slabs of sample_chunk (0: kHypSlabSamples; at most kHypSlabSamplesMax); none is empty
inline std::vector<HypSlab> hyp_slabs(int64_t S, int64_t sample_chunk) {
    const int64_t c = sample_chunk > 0 ? std::min(sample_chunk, kHypSlabSamplesMax) : kHypSlabSamples;
    std::vector<HypSlab> slabs;
    for (int64_t s = 0; s < S; s += c) slabs.push_back(HypSlab{s, std::min(S, s + c)});
    return slabs;
}

struct HypPlan {
    std::vector<int> list[2];      // per type: slab positions
    std::vector<HypItem> items[2]; // per type: `first` indexes list[type]
};

// The lists and work items of one slab.  soff: the np + 1 non-decreasing sample offsets of
// the run's pairs (any base: soff[0] is sample 0 of the run); types: the type (0 / 1) of
// every sample of the run, types[s] for sample s; cap[t]: samples per item of type t.
inline void hyp_items(int32_t np, const int64_t *soff, const int32_t *types, const HypSlab &s, const int cap[2],
                      HypPlan &plan) {
    for (int t = 0; t < 2; ++t) {
        plan.list[t].clear();
        plan.items[t].clear();
    }
    if (s.s0 >= s.s1 || np <= 0) return;
    // the pair that owns sample s0: the last k with soff[k] - soff[0] <= s0
    int32_t k = (int32_t)(std::upper_bound(soff, soff + np + 1, s.s0 + soff[0]) - soff) - 1;
    int64_t m = s.s0;
    while (m < s.s1 && k < np) {
        const int64_t end = std::min(s.s1, soff[k + 1] - soff[0]); // of this pair inside the slab
        int begin[2] = {(int)plan.list[0].size(), (int)plan.list[1].size()};
        for (int64_t a = m; a < end; ++a) plan.list[types[a] != 0 ? 1 : 0].push_back((int)(a - s.s0));
        for (int t = 0; t < 2; ++t) {
            const int stop = (int)plan.list[t].size();
            for (int a = begin[t]; a < stop; a += cap[t]) {
                HypItem it;
                it.pair = k;
                it.first = a;
                it.count = std::min(cap[t], stop - a);
                it.pad = 0;
                plan.items[t].push_back(it);
            }
        }
        m = std::max(m, end); // (end >= m: pair k owns m, or starts at it)
        ++k;
    }
}

} // namespace mp
