// The two-track bookkeeping of mp_ransac_lo_set (PairSet.ransac(step=, lo=)): plain C++ on
// plain numbers, no HIP, so it is checked on the CPU under a sanitizer
// (tests/ransac_lo_check.cpp) and against a Python restatement through
// mp_debug_ransac_lo_track (tests/test_ransac_lo_cpu.py).
//
// A pair keeps its minimal track (the running best of the strict-< walk over its minimal
// models, exactly mp_ransac_adaptive_set's) and beside it an overall best: the lowest score
// among the minimal bests and the models their local optimisations returned.  After a round
// in which the minimal best was replaced, in this order:
//   1. lo_take_minimal: the new minimal model becomes the overall best when its score is
//      strictly below the overall best's; lo_index = -1.
//   2. lo_take_refined: the new minimal model's local optimisation is counted (lo_runs), and
//      its result becomes the overall best when a round of it was accepted and its final
//      score is strictly below the overall best's; lo_index = that candidate, lo_accepted + 1.
// Equal scores and NaN scores replace nothing (every test is `a < b`).
#pragma once
#include <cfloat>
#include <cstdint>

namespace mp {

struct LoTrack {
    double score = DBL_MAX;           // the overall best's (DBL_MAX: none yet)
    int32_t counts[3] = {0, 0, 0};    // its three tight list lengths
    int32_t lo_index = -1;            // the candidate whose LO produced it; -1: a minimal model
    int32_t lo_runs = 0, lo_accepted = 0;
    int32_t source = 0;               // 0 none, 1 a minimal model, 2 an LO result
};

inline bool lo_take_minimal(LoTrack &T, double score, const int32_t counts[3]) {
    if (!(score < T.score)) return false;
    T.score = score;
    for (int t = 0; t < 3; ++t) T.counts[t] = counts[t];
    T.lo_index = -1;
    T.source = 1;
    return true;
}

inline bool lo_take_refined(LoTrack &T, int32_t candidate, int32_t rounds_accepted, double score_final,
                            const int32_t counts[3]) {
    ++T.lo_runs;
    if (rounds_accepted < 1 || !(score_final < T.score)) return false;
    T.score = score_final;
    for (int t = 0; t < 3; ++t) T.counts[t] = counts[t];
    T.lo_index = candidate;
    ++T.lo_accepted;
    T.source = 2;
    return true;
}

} // namespace mp
