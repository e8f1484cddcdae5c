// Chunk planning and packed device layout of mp_refine_batch: plain C++, no HIP, so the
// index arithmetic is checked on the CPU under a sanitizer (tests/refine_plan_check.cpp).
//
// The pairs of a call are split into runs of consecutive pairs; all pairs of a run are
// resident on the device at once.  With T = the run's correspondences and off_p = the
// correspondences of the run's pairs before pair p (n_p its own):
//   * doubles, one allocation of 12 T: the six uploaded rows (x0u x0v x1u x1v d0 d1) of
//     pair p at 6 off_p + k n_p, k = 0..5 -- the first 6 T doubles are one host staging
//     buffer and one copy -- and the six derived rows (r0 r1 a0 a1 b0 b1, written by the
//     pair preparation) at 6 T + 6 off_p + (k - 6) n_p, k = 6..11;
//   * inlier lists, two buffers of 3 T ints (the accepted model's lists and the
//     candidate's): list t of pair p at b 3 T + 3 off_p + t n_p -- inside a buffer the
//     layout of the caller's inlier_idx.
#pragma once
#include <cstdint>
#include <vector>

namespace mp {

constexpr int64_t kRefineRunCorr = int64_t(1) << 22; // correspondences per run when chunk == 0
constexpr int kRefineRows = 12;                      // doubles per correspondence (PairData)
constexpr int64_t kRefinePairMax = int64_t(1) << 28; // correspondences of one pair
// resident bytes of a run of T correspondences (12 doubles + 2 x 3 ints each); the
// default bound keeps it at 480 MiB, under 1 GiB with the per-pair records beside it
constexpr int64_t refine_run_bytes(int64_t T) { return T * (kRefineRows * 8 + 2 * 3 * 4); }
static_assert(refine_run_bytes(kRefineRunCorr) < (int64_t(1) << 30), "default run above 1 GiB");

struct RefineRun {
    int32_t p0, p1; // pairs p0 .. p1 - 1
    int64_t total;  // their correspondences
};

// offsets: num_pairs + 1 non-decreasing values.  chunk > 0: runs of `chunk` pairs;
// chunk == 0: as many pairs as fit `bound` correspondences, at least one (a pair larger
// than the bound runs alone).  Pairs of length zero join the run that is open.
inline std::vector<RefineRun> refine_plan(int32_t num_pairs, const int64_t *offsets, int64_t chunk,
                                          int64_t bound = kRefineRunCorr) {
    std::vector<RefineRun> runs;
    int32_t p = 0;
    while (p < num_pairs) {
        RefineRun r{p, p, 0};
        while (r.p1 < num_pairs) {
            const int64_t n = offsets[r.p1 + 1] - offsets[r.p1];
            if (chunk > 0) {
                if (r.p1 - r.p0 >= chunk) break;
            } else if (r.p1 > r.p0 && r.total + n > bound) {
                break;
            }
            r.total += n;
            ++r.p1;
        }
        runs.push_back(r);
        p = r.p1;
    }
    return runs;
}

// position (in doubles) of row k (0..11) of a pair in the run's allocation
inline int64_t refine_row(int64_t T, int64_t off_p, int64_t n_p, int k) {
    return k < 6 ? 6 * off_p + k * n_p : 6 * T + 6 * off_p + (k - 6) * n_p;
}
// position (in ints) of list t (0..2) of a pair in list buffer b (0, 1)
inline int64_t refine_list(int64_t T, int64_t off_p, int64_t n_p, int b, int t) {
    return b * 3 * T + 3 * off_p + t * n_p;
}

// the six uploaded rows of one pair into the staging buffer (stage: the run's 6 T
// doubles); x0, x1: n x 2 point-major
inline void refine_pack_pair(const double *x0, const double *x1, const double *d0, const double *d1, int64_t n,
                             int64_t off_p, double *stage) {
    double *s = stage + 6 * off_p;
    for (int64_t i = 0; i < n; ++i) {
        s[i] = x0[2 * i];
        s[n + i] = x0[2 * i + 1];
        s[2 * n + i] = x1[2 * i];
        s[3 * n + i] = x1[2 * i + 1];
        s[4 * n + i] = d0[i];
        s[5 * n + i] = d1[i];
    }
}

} // namespace mp
