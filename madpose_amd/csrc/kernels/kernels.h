// Host-side launch wrappers of the HIP kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "../host/ingest_plan.h"
#include "../host/pair_set_plan.h"
#include "../host/information_plan.h"
#include "../host/residuals_plan.h"
#include "../include/mp_draw.h"
#include "../include/mp_types.h"

namespace mp {

constexpr int kSampleStride = 8; // sample indices per iteration slot (max minimal sample = 7)

// r0/r1 = 1 / |K^-1 x| for the calibrated bearings; a0 .. b1 (nullable, calibrated):
// the rays' first two components, a = K0^-1 x0 and b = K1^-1 x1 (PairData::a0 .. b1)
hipError_t launch_prep_pair(hipStream_t s, const PairConst &C, const PairData &D, double *r0, double *r1,
                            double *a0 = nullptr, double *a1 = nullptr, double *b0 = nullptr, double *b1 = nullptr);

// launch_prep_pair for many resident calibrated pairs in one launch: one workgroup per
// item (host/pair_set_plan.h), rows 6 .. 11 of every listed pair (Ds[k].r0 .. b1) written
// with launch_prep_pair's bits.  Ds / Cs / items: device arrays.
hipError_t launch_prep_pairs(hipStream_t s, const PairData *Ds, const PairConst *Cs, const PrepItem *items,
                             int nitems);

// The device ingest (ingest_pairs.h; host/ingest_plan.h): rows 0 .. 5 of resident pairs from the
// caller's device arrays A.  launch_ingest_scale (shared / two focal): scale[k] = pair k's
// normalization scale, make_problem's bits (1 for an empty pair).  launch_ingest_rows: rows 0 .. 5
// of the items' correspondences (Ds[k].x0u .. d1) and stats[item]; scale: launch_ingest_scale's
// (not read for calibrated geometry).  Ps / Ds / items / scale / stats: device arrays.
hipError_t launch_ingest_scale(hipStream_t s, const IngestArgs &A, const IngestPair *Ps, int np, double *scale);
hipError_t launch_ingest_rows(hipStream_t s, const IngestArgs &A, const IngestItem *items, int nitems,
                              const IngestPair *Ps, const PairData *Ds, const double *scale, IngestStats *stats);

// MD minimal solver over the listed iterations (md_exact: R lanes per sample).
hipError_t launch_md_solve(hipStream_t s, const PairData &D, const PairConst &C, const int *list, int nlist,
                           const int *samples, Model *models, ScoreRec *recs, int *counts, int maxm);
// Workspace of the staged point solvers (per point sample: candidate roots and model
// slots).  cand: kPtCandStride doubles, slots / valid: kPtSlotStride entries.
constexpr int kPtCandStride = 96, kPtSlotStride = 32;
constexpr int kPtPenStride = 300; // shared focal: the 3 x 10 x 10 pencil of a sample (eig6.h)
struct PtWorkspace {
    double *cand;
    int *ncand;
    Model *slots;
    int *valid;
    double *pen; // kPtPenStride doubles per point sample (shared focal)
    // the two-stage exact MD solver's per-sample state (kMdWsStride doubles per MD sample,
    // structure of arrays with leading dimension md_ld >= the batch's MD samples) and root
    // counts; null: the one-stage kernel
    double *md_ws = nullptr;
    int *md_nr = nullptr;
    int md_ld = 0;
};
constexpr int kMdWsStride = 72; // doubles: the system (<= 62) + its roots (<= 8)
// The exact MD solver in two launches when W.md_ws is set and MADPOSE_MD_TWO_STAGE=2 (the
// setup with one lane per sample, then one lane per root); else launch_md_solve.  (The
// fused calibrated launch, launch_solve_fused, takes the two stages by default.)
hipError_t launch_md_solve_staged(hipStream_t s, const PairData &D, const PairConst &C, const int *list, int nlist,
                                  const int *samples, const PtWorkspace &W, Model *models, ScoreRec *recs,
                                  int *counts, int maxm);
// point minimal solver over the listed iterations (three launches, see kernels.hip;
// roots_done: the root stage ran in launch_solve_fused).
hipError_t launch_pt_solve(hipStream_t s, const PairData &D, const PairConst &C, const int *list, int nlist,
                           const int *samples, const PtWorkspace &W, Model *models, ScoreRec *recs, int *counts,
                           int maxm, bool roots_done = false);
// Calibrated, default MD solver at 4 lanes per sample (MADPOSE_SOLVE_FUSE=0 turns it
// off): the MD solver and the 5pt root stage in one launch, then the 5pt tails and
// compaction -- both solvers on one stream, no fork / join.
bool solve_fusable(const PairConst &C);
hipError_t launch_solve_fused(hipStream_t s, const PairData &D, const PairConst &C, const int *md_list, int nmd,
                              const int *pt_list, int npt, const int *samples, const PtWorkspace &W, Model *models,
                              ScoreRec *recs, int *counts, int maxm);
// scoring sweep: one workgroup per iteration, every model of the iteration scored
// over all correspondences; per-iteration argmin (first minimum wins) into res[b] with
// the screening bounds hi / lo and the kSlotAmbiguous / kSlotUncertain flags (each
// model's margin is ScoreRec::tie, mp_score.h score_margins).  best: the best
// minimal-model score before the batch (DBL_MAX: none yet); with non-negative weights a
// model whose partial sum minus its margin reaches best cannot win and is dropped early
// (exact early exit, kernels.hip ScoreBound), reporting DBL_MAX.  work (nullable): per
// iteration the (model, 256-correspondence trip) pairs evaluated.  rec (nullable): the
// record word of a batch that is cut at its first new best (kernels.hip ScoreBound),
// with epoch_hi = ~epoch, a value unique to the batch; published when hi < best without
// a flag.  rec_out (nullable, device-mapped host memory, nb Models): iterations whose lo
// is below best, or that are uncertain, write their best model (from models, nb x maxm)
// to rec_out[b].
hipError_t launch_score_batch(hipStream_t s, const PairData &D, const PairConst &C, const ScoreRec *recs,
                              const int *counts, int nb, int maxm, double *scores, IterResult *res, double best,
                              int *work, unsigned long long *rec = nullptr, unsigned epoch_hi = 0,
                              const Model *models = nullptr, Model *rec_out = nullptr, uint8_t *flags8 = nullptr,
                              IterResult *cand_out = nullptr);
// score_batch's per-correspondence errors (3 x n per model) and flags (n per model) of
// nm explicit models (test hook)
hipError_t launch_debug_terms(hipStream_t s, const PairData &D, const PairConst &C, const ScoreRec *recs, int nm,
                              double *err, int *flags);
// single-model sweep: per-point squared errors (3 x n, no gating) + gated MSAC score
hipError_t launch_sweep(hipStream_t s, const PairData &D, const PairConst &C, const ScoreRec *rec, double *err,
                        double *score);
// the estimator's point-solver root stage alone, C.variant kCal (5pt, 16-lane groups)
// or kSF (6pt, deflated eigenproblem, eig6.h; pen: kPtPenStride doubles per sample).
// cand: kPtCandStride doubles per sample (cal: 9 per essential matrix; sf: null-space
// basis N (27), then the positive roots u)
hipError_t launch_pt_roots(hipStream_t s, const PairData &D, const PairConst &C, const int *list, int nlist,
                           const int *samples, double *cand, int *ncand, double *pen = nullptr);
// scores of many explicit models (one workgroup per model) -- used by mp_score_models
hipError_t launch_score_models(hipStream_t s, const PairData &D, const PairConst &C, const ScoreRec *recs, int nm,
                               double *scores);

// standalone solvers (mp_solve_* C API): one sample, one thread
hipError_t launch_md_direct(hipStream_t s, int variant, int alt, const double *in /* x(3K) y(3K) dx(K) dy(K) */,
                            double *sols, int *nsols, Model *poses, int *nposes);
// (kind 0: cand / ncand are the root stage's workspace, kPtCandStride doubles and one int)
hipError_t launch_point_direct(hipStream_t s, int kind, const double *in, Model *poses, int *nposes, double *cand,
                               int *ncand);
// shared-focal 6pt poses from a root stage's output (cand: null space + roots of one
// sample, ncand: root count); in: the 6 + 6 normalized 2-D points
hipError_t launch_point_direct_6pt(hipStream_t s, const double *in, const double *cand, const int *ncand,
                                   Model *poses, int *nposes);

// The minimal solvers over many raw samples (solve_batch.h; mp_*_batch).  The outputs are
// zeroed by the caller; a sample's rows past its count are not written.
// MD solvers: in = the chunk as structure of arrays (host/solve_batch_pack.h pack_md_soa,
// leading dimension ld); pose false: sols = ns x 8 rows of width 4 / 5 / 6 (alt 0 only),
// pose true: poses = ns x 8 Models; counts = ns row counts.
hipError_t launch_sb_md(hipStream_t s, int variant, int alt, bool pose, const double *in, int ld, int ns, double *sols,
                        Model *poses, int *counts);
// 5pt: in = ns x 30 doubles (unit bearings of image 0, then image 1); cand / ncand: the root
// stage's workspace (kPtCandStride doubles and one int per sample); poses = ns x 16 Models
hipError_t launch_sb_pt5(hipStream_t s, const double *in, int ns, double *cand, int *ncand, Model *poses, int *counts);
// shared-focal 6pt poses from the root stage's output (launch_pt_roots on the chunk's
// pseudo-pair); in = ns x 24 doubles (normalized 2-D points of image 0, then image 1)
hipError_t launch_sb_pt6_poses(hipStream_t s, const double *in, int ns, const double *cand, const int *ncand,
                               Model *poses, int *counts);
// two-focal 7pt: in = 28 rows (structure of arrays, ld); Fws: 27 rows of workspace
hipError_t launch_sb_pt7(hipStream_t s, const double *in, int ld, int ns, double *Fws, Model *poses, int *counts);

// batched device LM: one workgroup per job; out[j] the refined model, status[j] 1
// refined, 0 no residuals, 2 infeasible constant block (unchanged)
hipError_t launch_lm_batch(hipStream_t s, const PairData &D, const PairConst &C, const LmJob *jobs, int njobs,
                           const int *idx, Model *out, int *status);
// one evaluation and one step of each job at its start model with radius[j] -- test hook
// (mp_debug_lm_system): sys[j] in the full layout, status[j] as above
hipError_t launch_lm_system(hipStream_t s, const PairData &D, const PairConst &C, const LmJob *jobs, int njobs,
                            const int *idx, const double *radius, LmSystem *sys, int *status);

// Many resident pairs per launch (refine_batch.h; mp_refine_batch).  Ds / Cs: one record
// per pair in device memory; variant: the pairs' common PairConst::variant.
// Sweep of item k = (pair, list buffer) with model record recs[k]: out[k] = the score as
// launch_score_models gives it and the lengths of the three ascending inlier lists (err <
// thr, errors as launch_sweep's), written to lists + buf * buf_stride + list_off[pair] +
// t * n.  One workgroup per item.
hipError_t launch_refine_sweep(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                               const RefineItem *items, const ScoreRec *recs, int nitems, const int64_t *list_off,
                               int *lists, int64_t buf_stride, RefineSweepOut *out);
// The same sweep with two thresholds per term in one pass: score and tight lists as above,
// and the relaxed lists err < thr * relax (ascending, the same layout) written to the item's
// other list buffer, (buf ^ 1) * buf_stride; out[k].relaxed their lengths.  Both buffers
// must exist.
hipError_t launch_refine_sweep_relaxed(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                                       const RefineItem *items, const ScoreRec *recs, int nitems,
                                       const int64_t *list_off, int *lists, int64_t buf_stride, double relax,
                                       RelaxedSweepOut *out);
// launch_lm_batch with job j on pair refs[j].pair, its block lists at idx + refs[j].idx_off
hipError_t launch_lm_pairs(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs, const LmJob *jobs,
                           const LmPairRef *refs, int njobs, const int *idx, Model *out, int *status);

// The weight mass of a model's inlier lists (inlier_mass.h; mp_inlier_mass_set).  One workgroup
// per item k = (pair, weighted) with model record recs[k]: out[k] = per term the sum of the
// quantised weights q_i = c[i + 1] - c[i] and the number of the rows with err < thr (errors as
// launch_refine_sweep's), c the pair's table at cum + tab_off[pair] (n + 1 entries), and total
// = c[n]; an item that is not weighted takes q_i = 1 and total = n and reads no table (cum and
// tab_off may be null when no item is weighted).  Nothing else is written.
hipError_t launch_inlier_mass(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                              const MassItem *items, const ScoreRec *recs, int nitems, const uint32_t *cum,
                              const int64_t *tab_off, MassOut *out);

// The errors and the inlier mask of every correspondence (residuals.h; mp_residuals_set).  One
// workgroup per item k (host/residuals_plan.h): rows first .. first + count - 1 of pair
// items[k].pair under the record recs[items[k].rec].  Row first + j of it: mask[row + j] = bit t
// set iff err_t < thr_t * factor (errors as launch_refine_sweep's), and, errors not null,
// errors[t * stride + row + j] = err_t; out[k] = the item's three inlier counts.  Nothing else
// is written.  mask / errors may be memory of the caller.
hipError_t launch_residuals(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                            const ResidItem *items, int nitems, const ScoreRec *recs, unsigned char *mask,
                            double *errors, int64_t stride, ResidCount *out);

// The Gauss-Newton system over a model's inliers and its inverse (information.h;
// mp_information_set).  launch_information: one workgroup per item k (host/information_plan.h;
// the items of launch_residuals), part[k] = the sums of the item's blocks under the record
// recs[items[k].rec] and the job jobs[items[k].rec], and its three inlier counts.
// launch_information_finish: one workgroup per entry j, the partials jobs[j].first_item ..
// + nitems - 1 added in that order, masked and inverted; row jobs[j].out_row of H (66 doubles a
// row), g (11), cost (1) and cov (121), each nullable and possibly memory of the caller, and
// recs[j].  Nothing else is written.
hipError_t launch_information(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                              const ResidItem *items, int nitems, const ScoreRec *recs, const InfoJob *jobs,
                              InfoPartial *part);
hipError_t launch_information_finish(hipStream_t s, int variant, const InfoJob *jobs, int nentries,
                                     const InfoPartial *part, double *H, double *g, double *cost, double *cov,
                                     InfoRecord *recs);

// ransac's results into the caller's device arrays (ransac_out.h; mp_ransac_out_set).
// launch_ransac_out: launch_residuals' items, rows and counts with the comparison err_t < thr_t
// itself; an item with rec == kResidFill (a pair without a winner) stores mask 0 and NaN errors,
// counts 0, and reads neither the pair nor a record.  launch_ransac_out_pairs: pairs[j] to row j
// of models (17 doubles), index and counts (3 ints), each nullable.  Nothing else is written.
hipError_t launch_ransac_out(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                             const ResidItem *items, int nitems, const ScoreRec *recs, unsigned char *mask,
                             double *errors, int64_t stride, ResidCount *out);
hipError_t launch_ransac_out_pairs(hipStream_t s, const RansacOutPair *pairs, int npairs, double *models, int *index,
                                   int *counts);

// Least-squares fits on random inlier subsets (lsq_subset.h; mp_lsq_fit_set).  One workgroup
// per entry; entry k's model record is recs[k], its outcome out[k], its workspace slice ws +
// entries[k].ws_off (6 * stride ints: the three wide lists, then the three subset lists, each
// `stride` = the pair's n apart).
// launch_lsq_sweep: the score as launch_score_models gives it, the tight counts err < thr and
// the wide ascending lists err < thr * entries[k].factor with their lengths.
hipError_t launch_lsq_sweep(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                            const LsqEntry *entries, const ScoreRec *recs, int nentries, int *ws, LsqOut *out);
// launch_lsq_subset: the subset (include/mp_subset.h) of the wide lists of lengths out[k].wide,
// its size by the entry's rule (or entries[k].k for rule -1): out[k].k (-1: skipped by the rule)
// and out[k].sub, the subset's list lengths.
hipError_t launch_lsq_subset(hipStream_t s, const LsqEntry *entries, int nentries, int *ws, LsqOut *out, int variant,
                             int mu, int nu, uint64_t seed, uint64_t key_mask);

// Ranking of candidates over the resident pairs (select_batch.h; mp_select_batch).
// Work item k = items[k].count (<= tile) candidates of pair items[k].pair with the records
// recs[items[k].rec ..]; candidate j of the item has position at = base + items[k].rec + j
// in the run: scores[at] = its score as launch_score_models gives it, counts[3 at + t] =
// the number of errors (launch_sweep's) below thr[t].  tile: 1, 2, 4 or 8.
hipError_t launch_select_score(hipStream_t s, int variant, int tile, const PairData *Ds, const PairConst *Cs,
                               const SelectItem *items, int nitems, const ScoreRec *recs, int64_t base,
                               double *scores, int *counts);
// out[k] = GetBestEstimatedModelId's walk over scores[moff[k] .. moff[k + 1]) (np pairs)
hipError_t launch_select_argmin(hipStream_t s, const int64_t *moff, int np, const double *scores, SelectBest *out);
// the walk started from prior[k] instead of DBL_MAX: out[k].index = -1 and out[k].score =
// prior[k] where no candidate is strictly below prior[k] (mp_ransac_adaptive_set)
hipError_t launch_select_argmin_seeded(hipStream_t s, const int64_t *moff, int np, const double *scores,
                                       const double *prior, SelectBest *out);

// The estimator's solve stages over explicit samples of the resident pairs
// (hypothesize_batch.h; mp_hypothesize_batch).  samples: the slab's sample indices
// (kSampleStride per slab position); md_list / pt_list: the slab positions of the two
// solver types, cut into the work items md_items / pt_items (host/hypothesis_plan.h); npt:
// the length of pt_list.  Sample at slab position b: its models to models[b * max_models
// ..] in the estimator's order, their number to counts[b]; slots past it are not written.
// W: cand / ncand / slots / valid / pen sized for npt point samples (md_ws unused).  The
// launch count does not depend on the number of pairs: 1 for the MD samples, 3 (calibrated,
// two focal) or 5 (shared focal) for the point samples.
hipError_t launch_hyp_solve(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                            const HypItem *md_items, int nmd_items, const int *md_list, const HypItem *pt_items,
                            int npt_items, const int *pt_list, int npt, const int *samples, const PtWorkspace &W,
                            Model *models, int *counts);

// The hand-over of a slab's models to select (hypothesize_batch.h; mp_candidates_set): after
// launch_hyp_solve on ns <= 131072 samples, base[b] = the models of the samples before b
// (ns + 1 ints, base[ns] the total), compact[base[b] + i] = model i of sample b, tags[2 m],
// tags[2 m + 1] = the slab position and slot of compact model m.  compact and tags are sized
// for ns * max_models(variant) models.  Two launches: the scan (one workgroup) and the gather.
hipError_t launch_hyp_compact(hipStream_t s, int variant, const Model *models, const int *counts, int ns, int *base,
                              Model *compact, int *tags);
// The device sampler (draw_batch.h; mp_draw_set): item k draws the samples items[k].s0 ..
// + count - 1 of pair items[k].pair (n = pair_n[pair]) by include/mp_draw.h draw_sample into
// samples[kSampleStride * (items[k].out + i) ..] and types[items[k].out + i].
hipError_t launch_draw_samples(hipStream_t s, int variant, const DrawItem *items, int nitems, const int *pair_n,
                               uint64_t seed, int point_share, int *samples, int *types);
// The confidence-weighted sampler (draw_weighted.h; include/mp_draw.h).  launch_draw_weights_table:
// one launch over the set's pairs; pair p given weights (given null: every pair) of n = pair_n[p]
// <= kDrawWeightMaxN values at weights + off[p] (dtype 0 float32, 1 float64) gets its table at cum +
// off[p] + p (n + 1 entries), pos[p] = #{q > 0} and total[p] = W; *bad_row (set to INT_MAX before)
// takes the lowest row of the set whose weight is refused.  launch_draw_samples_weighted:
// launch_draw_samples with, for the pairs whose weighted[pair] is not 0, draw_sample_weighted on
// the table at cum + cum_off[pair]; stage: tables of at most kDrawStageEntries entries are read
// through LDS (the bytes do not depend on it).
hipError_t launch_draw_weights_table(hipStream_t s, const void *weights, int dtype, const int64_t *off,
                                     const int *pair_n, const unsigned char *given, int num_pairs, uint32_t *cum,
                                     int *pos, uint32_t *total, int *bad_row);
hipError_t launch_draw_samples_weighted(hipStream_t s, int variant, const DrawItem *items, int nitems,
                                        const int *pair_n, const uint32_t *cum, const int64_t *cum_off,
                                        const unsigned char *weighted, bool stage, uint64_t seed, int point_share,
                                        int *samples, int *types);

// squared Bougnoux focals of k fundamental matrices (9 doubles each) into out (2 each)
hipError_t launch_bougnoux(hipStream_t s, const double *F, int64_t k, double *out);

// compute_pose_error of k pairs (R k x 9, t k x 3, T k x 16 row-major T_0to1; t_thres
// < 0: none) into err_t, err_R (degrees) and, when err_max is given, max(err_t, err_R)
hipError_t launch_pose_errors(hipStream_t s, int64_t k, const double *R, const double *t, const double *T,
                              double t_thres, double *err_t, double *err_R, double *err_max);

// pose AUC of k errors at nthr thresholds: rank sort into sorted (k doubles of
// scratch), then one workgroup per threshold
hipError_t launch_pose_auc(hipStream_t s, int64_t k, const double *e, double *sorted, int nthr, const double *thr,
                           double *aucs);

// estimate_scale_and_pose over n points (in = X(3n) Y(3n) W(n)), one thread
hipError_t launch_scale_and_pose(hipStream_t s, const double *in, int64_t n, Model *out);

// get_depths of num pairs in one launch (dtype 0 float32, 1 float64 maps): map p at
// maps + map_off[p] (dims[2p] x dims[2p+1]), size ratios fac[2p] (x), fac[2p+1] (y),
// its keypoints at pts[2 pt_off[p] ..], results at out[pt_off[p] ..]; total = pt_off[num]
hipError_t launch_get_depths(hipStream_t s, int dtype, const void *maps, const int64_t *map_off, const int64_t *dims,
                             const double *fac, const int64_t *pt_off, int32_t num, int64_t total, const double *pts,
                             void *out);

} // namespace mp
