// The termination rule of the adaptive mode of mp_ransac_adaptive_set: plain C++, no HIP, so
// it is checked on the CPU under a sanitizer (tests/ransac_stop_check.cpp) and against a
// restatement through mp_debug_ransac_required (tests/test_ransac_adaptive_cpu.py).
//
// The rule is the estimators' UpdateRANSACTerminationCriteria (engine.cpp Run::num_required /
// Run::termination) read on the running best of a pair: r[t] = counts[t] / n the inlier
// ratios of its three lists, ss[0] = (k_md, k_md, 0) and ss[1] = (0, 0, k_pt) the sample
// sizes per list of the MD and the point solver.  One deliberate difference: the required
// count is clamped to max_num_iterations_per_solver as a double, before any integer
// conversion (the estimator converts first, as its reference does; a ratio such as 2 / 700 on
// seven points gives more than 2^32 there).
//
// Samples go in rounds of `step` per pair up to `budget`: the checkpoints are
// m_k = min(k step, budget), and round k of a pair that has had `first` samples takes
// round_count(first, step, budget) more.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace mp {

constexpr int32_t kAdaptiveBudgetMax = 1 << 20; // samples a pair may get at most

struct StopOptions {
    double success_probability;
    uint32_t min_num_iterations, max_num_iterations_per_solver;
};

// req[s] for solver s (0 the MD solver, 1 the point solver) of a pair of n correspondences
// whose running best has the list lengths counts[0 .. 2] (null: no winner yet)
inline uint32_t required_samples(int s, int k_md, int k_pt, int64_t n, const int32_t *counts, const StopOptions &o) {
    const int ss[2][3] = {{k_md, k_md, 0}, {0, 0, k_pt}};
    double p_all = 1.0;
    for (int t = 0; t < 3; ++t) {
        const double r = (n > 0 && counts) ? (double)counts[t] / (double)n : 0.0;
        p_all *= std::pow(r, (double)ss[s][t]);
    }
    if (p_all <= 0.0) return o.max_num_iterations_per_solver;
    if (p_all >= 1.0) return o.min_num_iterations;
    const double p_bad = 1.0 - p_all;
    if (p_bad >= 0.99999999999999) return o.max_num_iterations_per_solver;
    const double it = std::ceil(std::log(1.0 - o.success_probability) / std::log(p_bad) + 0.5);
    // (in double: `it` may be above 2^32, -inf, or NaN; !(it < max) takes the bound for all but -inf)
    uint32_t r = o.max_num_iterations_per_solver;
    if (it < (double)o.max_num_iterations_per_solver) r = it > 0.0 ? (uint32_t)it : 0u;
    return std::max(o.min_num_iterations, r);
}

// The weighted rule (mp_ransac_weighted_stop_set): required_samples with r[t] = mass[t] / total,
// mass[t] the sum of the quantised confidences q_i over list t of the running best and total
// their sum W over the pair (both below 2^32, exact in double); mass null: no winner yet.  For
// a pair that is not weighted, mass = counts and total = n: the quotient above, the same bits.
// For equal weights q, (q c) / (q n) and c / n are correctly rounded quotients of one rational:
// the same bits again.
inline uint32_t required_samples_mass(int s, int k_md, int k_pt, uint32_t total, const uint32_t *mass,
                                      const StopOptions &o) {
    const int ss[2][3] = {{k_md, k_md, 0}, {0, 0, k_pt}};
    double p_all = 1.0;
    for (int t = 0; t < 3; ++t) {
        const double r = (total > 0 && mass) ? (double)mass[t] / (double)total : 0.0;
        p_all *= std::pow(r, (double)ss[s][t]);
    }
    if (p_all <= 0.0) return o.max_num_iterations_per_solver;
    if (p_all >= 1.0) return o.min_num_iterations;
    const double p_bad = 1.0 - p_all;
    if (p_bad >= 0.99999999999999) return o.max_num_iterations_per_solver;
    const double it = std::ceil(std::log(1.0 - o.success_probability) / std::log(p_bad) + 0.5);
    // (in double: `it` may be above 2^32, -inf, or NaN; !(it < max) takes the bound for all but -inf)
    uint32_t r = o.max_num_iterations_per_solver;
    if (it < (double)o.max_num_iterations_per_solver) r = it > 0.0 ? (uint32_t)it : 0u;
    return std::max(o.min_num_iterations, r);
}

// the mass of three inlier lists (idx[offsets[t] .. offsets[t + 1]), indices in 0 .. n - 1) under
// the table c[0 .. n]: the host form of kernels/inlier_mass.h's sums (uint32, wrapping only if
// a list repeats rows)
inline void inlier_mass_host(const uint32_t *cum, const int64_t offsets[4], const int32_t *idx, uint32_t mass[3]) {
    for (int t = 0; t < 3; ++t) {
        uint32_t m = 0u;
        for (int64_t j = offsets[t]; j < offsets[t + 1]; ++j) m += cum[idx[j] + 1] - cum[idx[j]];
        mass[t] = m;
    }
}

// the stop test after a round: drawn[s] samples of type s so far
inline bool stop_reached(const uint32_t req[2], const int64_t drawn[2]) {
    for (int s = 0; s < 2; ++s)
        if (drawn[s] > 0 && drawn[s] >= (int64_t)req[s]) return true;
    return false;
}

// the samples of the next round of a pair that has had `first` of at most `budget`
inline int32_t round_count(int32_t first, int32_t step, int32_t budget) {
    if (first >= budget) return 0;
    return std::min(step, budget - first);
}

} // namespace mp
