// The LO steps of mp_ransac_lo_steps_set (PairSet.ransac(step=, lo=, lo_steps=S)) beside the
// two-track bookkeeping of host/ransac_lo_track.h: the thresholds' schedule, the packing of a
// stage into the subset's streams, and the offers of the steps' models to the overall best.
// Plain C++ on plain numbers, no HIP, checked on the CPU under a sanitizer
// (tests/lsq_subset_check.cpp).
//
// At a checkpoint, after ransac_lo_track.h's steps 1 and 2 for an entry whose minimal best was
// replaced (candidate c, solver type s), with a the model the relaxed refinement returned, Q =
// num_lsq_iterations and lambda = threshold_multiplier, step r = 0 .. S - 1 runs the stages
//   0        lsq_fit(a, factor 1, rule nonmin) -> m1; a status other than 1 ends the step
//   1        lsq_fit(m1, factor 1, rule lsq) -> m2
//   2 + i    lsq_fit(m(2+i), factor f_i, rule lsq) -> m(3+i), i = 0 .. Q - 1
//   finals   m(2+Q) of every live step, ranked by one select over the entry's finals
// with stream = c and substream = 256 r + q at stage q.  A stage whose status is not 1 passes
// its model on unchanged.  Every lsq_fit returns the score and tight counts of its input, so
// the stages 1 .. 1 + Q score m1 .. m(1+Q) for free; each is offered to the overall best with a
// strict <, stage-major (stage 1 for the steps in order, then stage 2, ...), and last the
// select's winner among the finals.  An accepted offer records the step r and the stage that
// produced the model: q - 1 for the model stage q scored, 2 + Q for a final.
#pragma once
#include <cstdint>

#include "ransac_lo_track.h"

namespace mp {

constexpr int kLoStepsMax = 64;          // lo_steps: 1 .. 64
constexpr int kLoStepStageStride = 256;  // substream = stride * step + stage
constexpr int kLoStepLsqIterMax = kLoStepStageStride - 2; // stages 0 .. 1 + Q below the stride

// f_i of the shrinking thresholds thr * f_i: lambda at i = 0 down to 1 at i = Q - 1, by exactly
// this expression (one product, one quotient, one difference)
inline double lo_step_factor(int i, int Q, double lambda) {
    if (Q < 2) return lambda;
    const double num = (double)i * (lambda - 1.0);
    const double q = num / (double)(Q - 1);
    return lambda - q;
}

inline int32_t lo_step_substream(int r, int q) { return (int32_t)(kLoStepStageStride * r + q); }

// what an entry's steps did (mp_ransac_lo_steps_info): the step and stage that gave the overall
// best (-1: it is not a step's model), the offers made and those accepted
struct LoStepTrack {
    int32_t lo_step = -1, lo_stage = -1;
    int32_t offers = 0, accepted = 0;
};
constexpr int32_t kLoSourceStep = 3; // LoTrack::source of a step's model

// the overall best was replaced by a minimal model or a relaxed refinement's result
inline void lo_step_clear(LoStepTrack &S) { S.lo_step = S.lo_stage = -1; }

// one offer: the model of step r that stage `stage` produced, of candidate c's LO
inline bool lo_step_offer(LoTrack &T, LoStepTrack &S, int32_t c, int32_t r, int32_t stage, double score,
                          const int32_t counts[3]) {
    ++S.offers;
    if (!(score < T.score)) return false;
    T.score = score;
    for (int t = 0; t < 3; ++t) T.counts[t] = counts[t];
    T.lo_index = c;
    T.source = kLoSourceStep;
    S.lo_step = r;
    S.lo_stage = stage;
    ++S.accepted;
    return true;
}

} // namespace mp
