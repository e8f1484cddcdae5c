// The random subset of an inlier list that mp_lsq_fit_set's least-squares fits run on: one
// integer-only rule for host and device, so a subset's elements agree by construction (no
// floating point anywhere).  Uses mp_draw.h's philox4x32_10.
//
// An element is (t, i): list type t in {0, 1, 2} and correspondence index i < 2^28.  It belongs
// to an entry with the pair's index in the set `pair`, a stream < 2^31, a substream < 2^30 and
// the 64-bit seed.  Its key is the first two words of
//   philox4x32_10(i, (substream << 2) | t, pair, 0x80000000 | stream; seed low, seed high),
// word 0 the high half.  The set top bit of counter word 3 keeps these streams apart from the
// sampler's, whose word 3 is 0.
//
// Elements are ordered by (key & key_mask, t, i), lexicographically; key_mask is all ones
// everywhere but in the test hook, so ties are defined and can be tested.  The subset of size k
// of three ascending lists with M elements in all: everything when M <= k, otherwise the k
// smallest elements in that order -- again three ascending lists.
//
// subset_size: k from the entry's solver type s (0 MD, 1 point), the variant and the options'
// min_sample_multiplicator (mu) and non_min_sample_multiplier (nu), with k_md = 3 / 4 / 4, k_pt =
// 5 / 6 / 7, ss[0] = (k_md, k_md, 0), ss[1] = (0, 0, k_pt):
//   rule kSubsetLsq     LeastSquaresFit (Run::lsq_fit): skipped when any M_t < ss[s][t], otherwise
//                       k = mu * sum_t min(ss[s][t] * mu, M_t);
//   rule kSubsetNonmin  LocalOptimization's non-minimal sample (k_nonmin of Run::local_opt):
//                       k = max(35 calibrated / 36 otherwise, min(k_pt * nu, M / 2)), never skipped.
// All products in 64 bits, the result clamped to M.
#pragma once
#include "mp_draw.h"

#include <algorithm>
#include <vector>

namespace mp {

constexpr int kSubsetLsq = 0, kSubsetNonmin = 1;
constexpr uint32_t kSubsetIndexMax = 1u << 28;     // i below
constexpr uint32_t kSubsetStreamMax = 1u << 31;    // stream below
constexpr uint32_t kSubsetSubstreamMax = 1u << 30; // substream below
constexpr uint64_t kSubsetMaskAll = ~uint64_t(0);

// the counter words 1 and 3 of an element's Philox block
MP_HD uint32_t subset_word1(uint32_t substream, int t) { return (substream << 2) | (uint32_t)t; }
MP_HD uint32_t subset_word3(uint32_t stream) { return 0x80000000u | stream; }

MP_HD uint64_t subset_key(uint64_t seed, uint32_t pair, uint32_t stream, uint32_t substream, int t, uint32_t i) {
    uint32_t w[4];
    philox4x32_10(i, subset_word1(substream, t), pair, subset_word3(stream), (uint32_t)seed, (uint32_t)(seed >> 32),
                  w);
    return ((uint64_t)w[0] << 32) | w[1];
}

// the non-minimal sample size of the variant (v: 0 calibrated, 1 shared focal, 2 two focal)
constexpr int subset_nonmin_size(int v) { return v == kCal ? 35 : 36; }

// k of an entry (false: the rule skips it; *k = 0 then).  M[t]: the lengths of the three lists.
MP_HD bool subset_size(int rule, int s, int v, int mu, int nu, const int M[3], int64_t *k) {
    const int64_t total = (int64_t)M[0] + M[1] + M[2];
    const int k_md = draw_k_md(v), k_pt = draw_k_pt(v);
    int64_t r;
    *k = 0;
    if (rule == kSubsetNonmin) {
        const int64_t a = (int64_t)k_pt * nu, h = total / 2;
        const int64_t m = a < h ? a : h, f = subset_nonmin_size(v);
        r = f > m ? f : m;
    } else {
        const int ss[3] = {s == 0 ? k_md : 0, s == 0 ? k_md : 0, s == 0 ? 0 : k_pt};
        int64_t sum = 0;
        for (int t = 0; t < 3; ++t) {
            if (M[t] < ss[t]) return false;
            const int64_t a = (int64_t)ss[t] * mu;
            sum += a < M[t] ? a : (int64_t)M[t];
        }
        r = (int64_t)mu * sum;
    }
    if (r > total) r = total;
    if (r < 0) r = 0;
    *k = r;
    return true;
}

// The subset on the host: lists[t] the M[t] ascending indices of type t; out[t] receives the
// subset's ascending indices of type t.
inline void subset_select_host(const int *const lists[3], const int M[3], int64_t k, uint64_t seed, uint32_t pair,
                               uint32_t stream, uint32_t substream, uint64_t key_mask, std::vector<int> out[3]) {
    const int64_t total = (int64_t)M[0] + M[1] + M[2];
    for (int t = 0; t < 3; ++t) out[t].clear();
    if (k < 0) k = 0;
    if (total <= k) {
        for (int t = 0; t < 3; ++t) out[t].assign(lists[t], lists[t] + M[t]);
        return;
    }
    struct Elem {
        uint64_t key;
        int t, i;
    };
    std::vector<Elem> all;
    all.reserve((size_t)total);
    for (int t = 0; t < 3; ++t)
        for (int j = 0; j < M[t]; ++j)
            all.push_back(Elem{subset_key(seed, pair, stream, substream, t, (uint32_t)lists[t][j]) & key_mask, t,
                               lists[t][j]});
    auto less = [](const Elem &a, const Elem &b) {
        if (a.key != b.key) return a.key < b.key;
        if (a.t != b.t) return a.t < b.t;
        return a.i < b.i;
    };
    std::nth_element(all.begin(), all.begin() + k, all.end(), less);
    for (int64_t j = 0; j < k; ++j) out[all[(size_t)j].t].push_back(all[(size_t)j].i);
    for (int t = 0; t < 3; ++t) std::sort(out[t].begin(), out[t].end());
}

} // namespace mp
