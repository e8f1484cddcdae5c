// Host controller of the MI355X hybrid LO-MSAC estimator.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../include/mp_types.h"
#include "lm.h"

namespace mp {

struct RansacOptions {
    uint32_t min_num_iterations = 100, max_num_iterations = 10000, max_num_iterations_per_solver = 10000;
    double success_probability = 0.99;
    double squared_inlier_thresholds[2] = {1.0, 1.0};
    double data_type_weights[2] = {1.0, 1.0};
    uint32_t random_seed = 0;
    int num_lo_steps = 10;
    double threshold_multiplier = 1.4142135623730951;
    int num_lsq_iterations = 4, min_sample_multiplicator = 7, non_min_sample_multiplier = 3;
    int lo_starting_iterations = 50;
    bool final_least_squares = false, use_ours = false, use_4p4d = false;
};

struct EstimatorConfig {
    int solver_type = 0, score_type = 0, lo_type = 0;
    bool min_depth_constraint = true, use_shift = true;
    double ftol = 1e-6, gtol = 1e-8, ptol = 1e-6, max_iter = 25;
    bool nonmonotonic = true; // ceres_use_nonmonotonic_steps
};

struct Stats {
    uint32_t num_iterations_total = 0;
    uint32_t num_iterations_per_solver[2] = {0, 0};
    int best_num_inliers = 0;
    int best_solver_type = -1;
    double best_model_score = 0.0;
    double inlier_ratios[3] = {0, 0, 0};
    std::vector<int> inlier_indices[3];
    int number_lo_iterations = 0;
    uint64_t num_hypotheses = 0, num_lo_sweeps = 0;
    int num_batches = 0;
    double seconds_total = 0, seconds_lo = 0, seconds_gpu_wait = 0;
};

struct PairInput {
    int variant = kCal;
    int64_t n = 0;
    const double *x0 = nullptr, *x1 = nullptr, *d0 = nullptr, *d1 = nullptr;
    double min_depth[2] = {0, 0};
    double cam0[9] = {0}, cam1[9] = {0}; // K (CAL) or principal point (SF/TF)
};

// Runs the full estimator on one pair on `device`; throws std::runtime_error on HIP
// errors and std::invalid_argument on bad input.  The returned model is in user
// units (SF/TF focals multiplied back by the normalisation scale).
void estimate_pair(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int device, Model *out,
                   Stats *stats);

// Scores explicit models (problem units) on the device (mp_score_models).
void score_models(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, const Model *models,
                  int nm, double *scores, double *errors, int device, double *norm_scale);

// The engine's host LO sweep (host/lo_sweep.h) over explicit models (problem units):
// the errors and ScoreModel sums LO uses (mp_debug_lo_sweep, test hook; no device)
void lo_sweep_models(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, const Model *models,
                     int nm, double *scores, double *errors, double *fast_bounds = nullptr);

// score_batch's residuals of explicit models: errors nm x 3 x n, flags nm x n, taus nm x
// 3 (per-term bounds), ties nm (margins) -- mp_debug_score_terms, test hook
void debug_score_terms(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, const Model *models,
                       int nm, double *errors, int *flags, double *taus, double *ties, int device);

// score_margins of explicit models on the host, no device (mp_debug_score_margins, test
// hook): per model taus[3], wz0, wz1, wl, kg2, tie; per pair thr[3], w[3], the
// normalization scale, the Sampson loss scale, kstd
void debug_score_margins(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg,
                         const Model *models, int nm, double *per_model /* 8 nm */, double *per_pair /* 9 */);

// score_batch over explicit models (mp_debug_score_batch; test hook).  models: nb x
// max_models(variant) (problem units), counts[b] of them used per iteration.  flags: 1
// exact early exit against `best`, 2 record skip.  res_slot keeps kSlotAmbiguous /
// kSlotUncertain; res_hi_lo (nullable): hi, lo per iteration; model_ties (nullable, nb x
// max_models): the margins.
void debug_score_batch(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int nb,
                       const int *counts, const Model *models, double best, int flags, double *res_best,
                       int *res_slot, Model *rec_models, double *res_hi_lo, double *model_ties, int device);

// Batched device LM (mp_lm_refine_batch): problem j refines models[j] (problem units)
// over the residual blocks idx[offsets[3j] .. offsets[3j+1]) (reproj 0->1),
// [offsets[3j+1] .. offsets[3j+2]) (1->0), [offsets[3j+2] .. offsets[3j+3]) (Sampson),
// with the settings of LeastSquares (kinds[j] 0) or NonMinimalSolver (1).  status[j]:
// 1 refined, 0 no residuals, 2 infeasible constant block, 3 too few data (unchanged).
void lm_refine_batch_device(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int nprob,
                            const int32_t *kinds, const int64_t *offsets, const int32_t *idx, Model *models,
                            int32_t *status, int device);

void lm_refine_batch_host(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int nprob,
                          const int32_t *kinds, const int64_t *offsets, const int32_t *idx, Model *models,
                          int32_t *status);
// One evaluation and one step per problem -- test hook (mp_debug_lm_system; engine.cpp)
void lm_system_batch(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int nprob,
                     const int32_t *kinds, const int64_t *offsets, const int32_t *idx, const Model *models,
                     const double *radius, int where, const int64_t *ranges, LmSystem *out, int32_t *status,
                     int device);

// Device refinement of given models over many pairs (mp_refine_batch).  Pairs laid out
// as mp_estimate_batch's (offsets, 2 min depths and 9 / 2 camera values per pair); models:
// one per pair, in and out, user units.  Per pair and round: the inlier lists of the model
// (launch_sweep's errors below PairConst::thr), LeastSquares (kind 0 of
// lm_refine_batch_device) over them, the result accepted when the LM status is 1 and its
// score (score_models') is strictly lower; a pair stops at its first round without an
// accepted model, or after `rounds`.  A pair no round of which was accepted keeps its
// model's bytes.  Pairs run in resident runs of `chunk` pairs (0: host/refine_plan.h's
// default bound on a run's correspondences).  inlier_idx (nullable): as mp_estimate_batch.
struct RefineResult {
    double score_initial, score_final, norm_scale;
    int32_t rounds_run, rounds_accepted;
    int32_t lm_status; // of the last round run (0..3 as lm_refine_batch_device), -1: none ran
    int32_t num_inliers[3];
};
void refine_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                  const double *d0, const double *d1, const double *min_depth, const double *cam0, const double *cam1,
                  const RansacOptions &opts, const EstimatorConfig &cfg, int rounds, Model *models,
                  RefineResult *results, int32_t *inlier_idx, int64_t chunk, int device);

// Ranking of given candidate models over many pairs on the device (mp_select_batch).
// Pairs laid out as refine_batch's, without min_depth (no score depends on it); pair p's
// candidates are models[model_offsets[p] .. model_offsets[p + 1]), user units.  Per
// candidate: the score score_models gives for it in problem units (the record prepared on
// the host, the same bits) and the three counts of errors (score_models') below
// PairConst::thr -- scores[m] / counts[3 m + t] for m the candidate's index into models,
// both nullable.  Per pair: GetBestEstimatedModelId's walk (start at DBL_MAX, strict <)
// over its scores, and the winner's three ascending inlier lists as refine_batch forms
// them (inlier_idx, nullable, its layout).  Runs of `chunk` pairs as refine_batch; the
// records of `model_chunk` candidates (0: host/select_plan.h's default) are on the device
// at once.  Results depend on neither.
struct SelectResult {
    double best_score, norm_scale; // best_score DBL_MAX when no candidate won
    int32_t best_index;            // within the pair's candidates; -1: none
    int32_t num_inliers[3];        // the winner's lists
};
void select_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                  const double *d0, const double *d1, const double *cam0, const double *cam1,
                  const RansacOptions &opts, const EstimatorConfig &cfg, const int64_t *model_offsets,
                  const Model *models, double *scores, int32_t *counts, SelectResult *results, int32_t *inlier_idx,
                  int64_t chunk, int64_t model_chunk, int device);
// Measurement hooks of select_batch (mp_debug_select_tile, mp_debug_select_timing).
// select_tile_override: candidates per work item of the following calls (1, 2, 4, 8; 0:
// the built-in kSelectTile, the only size pinned to score_models' bits); returns the
// previous setting.  select_timing_last: the stage
// times of the last call made while profiling was enabled (profile_enable), every stage
// waited for, so nothing overlaps.
struct SelectTiming {
    double pairs_ms = 0;   // make_problem, the packed upload, the pair preparation
    double prepare_ms = 0; // host: the work items and prepare_score_rec of every slab
    double upload_ms = 0;  // records and items to the device
    double score_ms = 0;   // select_score
    double argmin_ms = 0;  // select_argmin and the copy back of its results (scores, counts)
    double winners_ms = 0; // the winners' records, refine_sweep, lists back
};
int select_tile_override(int tile);
SelectTiming select_timing_last();

// The estimators' sample models over many pairs (mp_hypothesize_batch).  Pairs laid out as
// refine_batch's; pair p's samples are sample_offsets[p] .. sample_offsets[p + 1] - 1 of
// sample_types (0 the MD solver, 1 the point solver) and sample_idx (8 slots per sample,
// indices within the pair; the first 3 / 4 read for type 0, the first 5 / 6 / 7 for type 1).
// Sample s: counts[s] models at models[s * max_models(variant) ..], the ones the
// estimator's MinimalSolver stage forms for that pair, solver type and sample (the exact MD
// solver with the min-depth filter; 5pt / 6pt / 7pt with depth tail, compaction and the
// shared-focal duplicate rule), in its order and to the bit, in user units (SF / TF: the
// focals times the pair's norm_scale); slots from counts[s] on are zero.  Supported: the
// variants 0 .. 2 with use_shift on and without use_ours / use_4p4d.  Runs of `chunk` pairs
// as refine_batch; `sample_chunk` samples (0: host/hypothesis_plan.h's default) are on the
// device at once.  Results depend on neither, nor on the other samples of the call.
// norm_scale (nullable): one per pair.  All arguments are checked before any device call.
void hypothesize_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                       const double *d0, const double *d1, const double *min_depth, const double *cam0,
                       const double *cam1, const RansacOptions &opts, const EstimatorConfig &cfg,
                       const int64_t *sample_offsets, const int32_t *sample_types, const int32_t *sample_idx,
                       Model *models, int32_t *counts, double *norm_scale, int64_t chunk, int64_t sample_chunk,
                       int device);
// Measurement hook (mp_debug_hypothesize_timing): the stage times of the last call made
// while profiling was enabled (profile_enable), every stage waited for.
struct HypTiming {
    double pairs_ms = 0;    // make_problem, the packed upload, the pair preparation
    double plan_ms = 0;     // host: lists, work items and the checked sample copy of every slab
    double upload_ms = 0;   // samples, lists and items to the device, the output's zeroing
    double solve_ms = 0;    // the solve launches
    double download_ms = 0; // models and counts back, the focals to user units
    double draw_ms = 0;     // device-drawn samples only (ransac_set with a budget): the sampler
    double compact_ms = 0;  // the compact output mode only: the scan and the gather
};
HypTiming hypothesize_timing_last();

// Pairs set up once and resident on one device until destroyed (mp_pair_set_*;
// host/resident_pairs.h): the setup refine_batch / select_batch / hypothesize_batch make per
// call -- make_problem, the packed upload, the pair records, the calibrated preparation --
// under the options and config given at creation.  All pairs are one resident range
// (at most host/pair_set_plan.h kPairSetMaxCorr correspondences).  refine_set / select_set /
// hypothesize_set run the batch entries' stage bodies on a selection of the set's pairs
// (pair_ids: num_sel distinct indices in any order, or null with num_sel = the pair count:
// all in order) and return the bytes the batch entry returns on those pairs' inputs in that
// order; per-pair arguments and results are indexed by position in the selection, and
// inlier_idx is the batch layout over the selected pairs.  A call leaves nothing in the set
// that a later call can see.  Calls on one set are serialised by its mutex; a context is
// leased per call.  Sets still live at process teardown are released before the pooled
// contexts go.  hypothesize_set: std::invalid_argument on a set whose variant or options
// hypothesize_batch rejects.
struct PairSet;
struct DrawWeights; // (below, with draw_set)
PairSet *pair_set_create(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                         const double *d0, const double *d1, const double *min_depth, const double *cam0,
                         const double *cam1, const RansacOptions &opts, const EstimatorConfig &cfg, int device);
// pair_set_create from arrays that are already on `device` (mp_pair_set_create_device;
// host/ingest_plan.h, kernels/ingest_pairs.h): the set is the one pair_set_create builds from
// the same numbers, bit for bit.  x0, x1: T x 2 interleaved pixels of type xy_type (0 float32,
// widened exactly, 1 float64).  The depth priors: d0, d1 (T values of depth_type), or num_maps
// maps (host table `maps` of device pointers, h x w row-major of map_type; map_dims num_maps x 4
// = h, w, image_h, image_w; map_ids num_pairs x 2 = the map of side 0 / 1 of each pair) looked
// up at the pair's keypoints with get_depths' arithmetic -- exactly one of the two.  The set's
// stream waits for an event recorded on producer_stream (a hipStream_t; null: the null stream)
// before its first read; the call returns after its own stream is synchronised and the inputs
// are neither written nor referenced afterwards.  std::invalid_argument before any launch or
// copy: what pair_set_create refuses, type codes outside {0, 1}, both or neither depth source,
// map ids outside the table, non-positive map or image sizes, and every device pointer that
// is not device memory of `device`, not aligned to its element type, or whose allocation
// (hipMemGetAddressRange) does not hold the bytes the kernels read.
struct DevicePairArrays {
    const void *x0 = nullptr, *x1 = nullptr;
    int xy_type = 1;
    const void *d0 = nullptr, *d1 = nullptr;
    int depth_type = 1;
    const void *const *maps = nullptr;
    int32_t num_maps = 0;
    int map_type = 0;
    const int64_t *map_dims = nullptr;
    const int32_t *map_ids = nullptr;
    void *producer_stream = nullptr;
};
PairSet *pair_set_create_device(int variant, int32_t num_pairs, const int64_t *offsets, const DevicePairArrays &in,
                                const double *min_depth, const double *cam0, const double *cam1,
                                const RansacOptions &opts, const EstimatorConfig &cfg, int device);
void pair_set_destroy(PairSet *set); // null: nothing
// resident_bytes: the rows (96 bytes per correspondence) and the list buffers allocated so
// far (12 bytes per correspondence each: none after creation or hypothesize_set, one after
// select_set, two after refine_set); the per-pair records are not counted
void pair_set_info(const PairSet *set, int32_t *variant, int32_t *num_pairs, int64_t *correspondences,
                   int64_t *resident_bytes, int32_t *device);
void pair_set_norm_scales(const PairSet *set, double *out);
// relax (mp_refine_relaxed_set): the first sweep also forms the lists under the thresholds
// times the options' threshold_multiplier, and round 0's size test and least-squares fit read
// those (the estimators' m_init); the candidate of round 0 is accepted as any other (LM status
// 1, score strictly below score_initial), rounds 1 onward and every returned count and list
// are the tight ones
void refine_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int rounds, Model *models,
                RefineResult *results, int32_t *inlier_idx, bool relax = false);
// lsq_fit_set (mp_lsq_fit_set): one least-squares fit per entry on a random subset of the
// entry's inliers -- LeastSquaresFit (rule 0, include/mp_subset.h kSubsetLsq) or the non-minimal
// fit of an LO step (rule 1, kSubsetNonmin) of the estimators' LocalOptimization.  Entry e is a
// model (user units, in and out) of pair pair_ids[e] (null: e; a pair MAY repeat) with solver
// type solver_types[e], threshold factor factors[e] and the subset streams streams[e] /
// substreams[e].  Per entry: the model's score (score_models' bits) and tight counts, the wide
// lists err < thr * factor and their lengths, the subset of include/mp_subset.h of them (size by
// the rule) with its lengths; when the rule skips the entry or the subset fails
// lm_refine_batch_device's size test, status 3 and the model's bytes kept; otherwise the device
// LM (kind 0 for rule 0, 1 for rule 1) on the subset from the model, status 1: its result,
// anything else: the input bytes.  subset_idx (nullable): refine's inlier_idx layout over the
// entries.  The pairs' list buffers are not touched and nothing stays in the set.
struct LsqFitResult {
    double score;
    int32_t num_inliers[3], num_wide[3], subset_sizes[3];
    int32_t status; // 0..3 as lm_refine_batch_device
};
void lsq_fit_set(PairSet *set, int32_t num_entries, const int32_t *pair_ids, const int32_t *solver_types,
                 const double *factors, int rule, uint64_t seed, const int32_t *streams, const int32_t *substreams,
                 Model *models, LsqFitResult *results, int32_t *subset_idx, int64_t entry_chunk);
// Test hooks.  subset_select_device (mp_debug_subset_select): lsq_subset_kernel on three given
// strictly ascending lists (idx[offsets[t] .. offsets[t + 1]), offsets[0] = 0) with the size k;
// the subset's lists to out_idx + offsets[t], their lengths to out_sizes.
// subset_select_host_hook (mp_debug_subset_select_host): the header's host form, no device.
// lsq_subset_size (mp_debug_lsq_subset_size): the size rule; returns 0 when it skips.
void subset_select_device(const int64_t *offsets, const int32_t *idx, int64_t k, uint64_t seed, int32_t pair,
                          int32_t stream, int32_t substream, uint64_t key_mask, int32_t *out_idx, int32_t *out_sizes,
                          int device);
void subset_select_host_hook(const int64_t *offsets, const int32_t *idx, int64_t k, uint64_t seed, int32_t pair,
                             int32_t stream, int32_t substream, uint64_t key_mask, int32_t *out_idx,
                             int32_t *out_sizes);
int lsq_subset_size(int rule, int solver_type, int variant, int mu, int nu, const int32_t *sizes, int64_t *k);
void select_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *model_offsets,
                const Model *models, double *scores, int32_t *counts, SelectResult *results, int32_t *inlier_idx,
                int64_t model_chunk);
void hypothesize_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *sample_offsets,
                     const int32_t *sample_types, const int32_t *sample_idx, Model *models, int32_t *counts,
                     int64_t sample_chunk);
// The fused budget entry and its parts on a pair set (mp_draw_set, mp_candidates_set /
// mp_candidates_fetch, mp_ransac_set); the selection as in the calls above.
// draw_set: `budget` samples per selected pair drawn on the device by include/mp_draw.h
// (counter (s, block, pair of the set, 0), key = seed), in hypothesize_set's form; a pair too
// small for the MD solver gets none (sample_counts[j] = 0 or budget; the offsets are their
// running sums).  point_share -1: draw_default_share of the set's solver_type.
// draw_host: one sample on the host (mp_debug_draw_host; no device): out[0] the type (-1: the
// pair is too small), out[1 .. 8] the slots, out[9] whether the ascending fill was needed.
// candidates_set: hypothesize_set's arguments; the models that exist, packed as select_set
// takes them, are kept in the set until candidates_fetch copies them out (with the
// num_sel + 1 offsets and, per model, its sample's index within the pair and its slot) and
// drops them; returns their number.  The bytes are hypothesize_set's for those slots.
// ransac_set: draw (sample_offsets null, budget >= 0; the samples never reach the host) or
// the given samples (budget -1) -> hypothesize_run in the compact mode -> select_run ->
// refine_run on the pairs with a winner (rounds >= 1), under one lock and one lease: the bytes
// of candidates_set -> select_set -> refine_set(pair_ids = the pairs with a winner).
struct RansacResult {
    double score_selected, score_initial, score_final, norm_scale;
    int32_t num_samples, num_candidates;
    int32_t best_candidate, best_sample, best_slot, best_type; // -1 without a winner
    int32_t rounds_run, rounds_accepted;
    int32_t lm_status; // as RefineResult; -1 without a winner or with rounds = 0
    int32_t num_inliers[3];
};
// Confidence-weighted sampling (mp_draw_weights_*, mp_draw_weighted_set, mp_ransac_weighted_set;
// the rule: include/mp_draw.h, the kernels: kernels/draw_weighted.h).  draw_weights_create: one
// launch builds the integer tables of the pairs given weights (given: num_pairs bytes, null: all;
// weights: one value per correspondence of the set in set order, dtype 0 float32 / 1 float64, on
// the host or -- on_device -- on the set's device, checked as pair_set_create_device checks its
// arrays and ordered after producer_stream by an event).  std::invalid_argument: a weight that
// is not finite in 0..1 (the lowest such row of the set is named), a pair above 65535
// correspondences given weights, and the sets hypothesize_set refuses.  The handle is immutable,
// belongs to `set` and lives outside it: draw_set / ransac_*_set with `weights` only read it, so a
// call still leaves nothing in the set.  A pair whose positive weights number fewer than its
// largest sample draws uniformly (weighted 0).  pair_set_destroy drops the handles' device
// arrays; such a handle is refused by every call and may still be destroyed.
// draw_weights_host / draw_weighted_host (mp_debug_*; no device): one pair's table (n + 1
// entries) and count of positive weights; one sample of a weighted pair, draw_host's out.
struct DrawWeights;
DrawWeights *draw_weights_create(PairSet *set, const void *weights, int dtype, bool on_device,
                                 const unsigned char *given, void *producer_stream);
void draw_weights_info(const DrawWeights *w, int32_t *weighted, int32_t *positive, uint32_t *total);
void draw_weights_destroy(DrawWeights *w); // null: nothing
void draw_weights_host(int64_t n, const void *weights, int dtype, uint32_t *cum, int32_t *positive);
void draw_weighted_host(int variant, int64_t n, const uint32_t *cum, uint64_t seed, int32_t point_share, int32_t pair,
                        int32_t s, int32_t *out);
// weights (here and in the ransac_*_set entries below; null: the uniform draw, today's launches)
void draw_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, uint64_t seed,
              int32_t point_share, int32_t *sample_types, int32_t *sample_idx, int32_t *sample_counts,
              const DrawWeights *weights = nullptr);
void draw_host(int variant, int64_t n, uint64_t seed, int32_t point_share, int32_t pair, int32_t s, int32_t *out);
int64_t candidates_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *sample_offsets,
                       const int32_t *sample_types, const int32_t *sample_idx, int64_t sample_chunk);
void candidates_fetch(PairSet *set, Model *models, int64_t *model_offsets, int32_t *cand_sample, int32_t *cand_slot);
struct RansacOut; // (below, at ransac_out_set)
void ransac_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, uint64_t seed,
                int32_t point_share, const int64_t *sample_offsets, const int32_t *sample_types,
                const int32_t *sample_idx, int32_t rounds, Model *models, RansacResult *results, int32_t *inlier_idx,
                int64_t sample_chunk, int64_t model_chunk, const DrawWeights *weights = nullptr,
                const RansacOut *out = nullptr);
// The weight mass of models' inlier lists and the weighted stopping rule (mp_inlier_mass_set,
// mp_ransac_weighted_stop_set; kernels/inlier_mass.h, host/ransac_stop.h required_samples_mass).
// q_i = c[i + 1] - c[i] are the quantised confidences of the handle's table of the pair and
// W = c[n] < 2^32 their sum.  For a model of a pair, L_t (t = 0..2) are the lists select
// returns for that single candidate (err_t < thr_t, ungated errors).  A weighted pair:
// mass[t] = the sum of q_i over L_t (uint32; distinct rows, so mass <= W) and total = W.  A
// pair that is not weighted (no weights given, or fallen back): mass[t] = |L_t|, total = n.
// count[t] = |L_t| always.
// inlier_mass_set: entry e is the model models[e] (user units) of pair pair_ids[e] (null: e);
// a pair MAY repeat, at most 2^24 entries; one upload, launch, copy and synchronise; nothing
// of the set is written.
// weighted_stop (the three adaptive entries below; needs weights): the termination rule of a
// weighted pair reads r[t] = mass[t] / total of its rule model -- the running best of
// ransac_adaptive_set, the overall best at the checkpoint's end of the lo bodies -- instead
// of counts[t] / n.  At a checkpoint, after the tracks are updated and before the rule is
// read, ONE mass run covers the still-active entries of weighted pairs whose rule model
// was replaced during that checkpoint; its counts must equal the track's (std::logic_error
// naming the pair otherwise).  Entries of pairs that are not weighted read their counts, the
// count rule's bits.  rule_mass[j] (nullable): what the rule last read for entry j; all zero
// with total = W or n for an entry that never had a winner.  Draws, walks, tracks, the final
// rounds and the result layout are untouched; with weighted_stop off no launch or byte of the
// call changes.  The device arrays of the stage are sized once for the selection.
constexpr int32_t kMassEntriesMax = 1 << 24;
struct InlierMass {
    uint32_t mass[3], total;
    int32_t count[3], weighted;
};
void inlier_mass_set(PairSet *set, const DrawWeights *weights, int32_t num_entries, const int32_t *pair_ids,
                     const Model *models, InlierMass *out);
// Test hooks, no device.  ransac_required_mass (mp_debug_ransac_required_mass): req[0], req[1] of
// the weighted rule on (total, mass[0 .. 2]); mass null: no winner.  inlier_mass_host_hook
// (mp_debug_inlier_mass_host): the masses of three strictly ascending lists under a table.
// inlier_mass_stats (mp_debug_inlier_mass_stats): the mass runs since the last reset and their
// summed host milliseconds (upload to synchronise).
void ransac_required_mass(int variant, uint32_t total, const uint32_t *mass, const RansacOptions &opts, uint32_t *req);
void inlier_mass_host_hook(int64_t n, const uint32_t *cum, const int64_t *offsets, const int32_t *idx, uint32_t *mass);
void inlier_mass_stats(int64_t *launches, double *ms, bool reset);
// The errors and inlier mask of every correspondence under given models (mp_residuals_set;
// kernels/residuals.h, host/residuals_plan.h).  Entry e is the model models[e] (user units) of
// pair pair_ids[e] (null: e; a pair MAY repeat) under the thresholds times factors[e] (null:
// 1.0).  row_offsets (num_entries + 1): entry e's rows; counts (3 per entry): its rows with
// err_t < thr_t * factor.  out.mask (R bytes, R = row_offsets[num_entries]): bit t of row i;
// out.errors (nullable; 3 R doubles, term-major): the ungated errors in problem units, the
// numbers compared.  on_device 0: host arrays, filled through a device scratch in runs whose
// size does not grow with R.  on_device 1: memory of the set's device, checked as
// pair_set_create_device checks its arrays (and that the two do not overlap) before any
// launch; the kernel writes into it directly, ordered after producer_stream (null: the null
// stream) by an event.  Returns after the library's stream is synchronised.  Nothing of the
// set is written.  std::invalid_argument before the device is touched: a null set, mask,
// row_offsets, counts or models; num_entries outside 0 .. 2^24; a pair outside the set; null
// pair_ids with num_entries != the pair count; a factor that is not finite and > 0.
struct ResidualsOut {
    void *mask = nullptr;
    void *errors = nullptr;
    int32_t on_device = 0, pad = 0;
    void *producer_stream = nullptr;
};
void residuals_set(PairSet *set, int32_t num_entries, const int32_t *pair_ids, const Model *models,
                   const double *factors, const ResidualsOut &out, int64_t *row_offsets, int32_t *counts);
// residuals_stats (mp_debug_residuals_stats): the kernel launches since the last reset and
// their summed device milliseconds (events around each launch; measured only while profiling
// is enabled).
void residuals_stats(int64_t *launches, double *ms, bool reset);
// The Gauss-Newton system of the estimators' cost over each model's inliers, and its inverse
// (mp_information_set; kernels/information.h, host/information_plan.h,
// include/mp_information.h).  Entries, pair_ids and factors as residuals_set.  Per entry e
// (model m on pair p): m to problem units as residuals_set takes it; row i is a block of type t
// iff bit t of residuals_set's mask is set for it (the same record, load_corr / eval_corr call
// and thr_t * factor product); gating and job flags are make_lm_job(P, cfg, sizes, .., nonminimal
// = false, m)'s (LO type, use_shift, the scale-only rule, w_sampson); the parameters are set up
// as lm_setup.inc sets them up (bounds and feasibility are not read: nothing is optimised).
// Row e of the outputs, all in problem units and in LmSystem's full 11-parameter layout:
// out.H (66: packed upper triangle of J^T J), out.g (11: J^T r), out.cost (sum r^2 / 2),
// out.cov (121: the inverse of H on the active set by info_covariance, zero elsewhere); each
// nullable.  entries[e] (always host memory): the active mask, pd (1 inverted, 0 an active
// H_aa or a pivot was not positive and finite: cov zero, -1 status 0: everything zero), status
// (1: at least one block), rows = 2 (n0 + n1) + n2 after gating, counts = residuals_set's.
// Every entry of g and H of an inactive parameter is exactly 0.0.  on_device / producer_stream
// as ResidualsOut: device outputs are checked (memory of the set's device, aligned, inside
// their allocations, pairwise disjoint) before any launch and written by the finishing kernel
// directly.  A result depends on its entry alone.  Nothing of the set is written.
// std::invalid_argument before the device is touched: residuals_set's cases (entries in place
// of row_offsets and counts), and overlapping device outputs.
struct InformationOut {
    void *H = nullptr, *g = nullptr, *cost = nullptr, *cov = nullptr;
    int32_t on_device = 0, pad = 0;
    void *producer_stream = nullptr;
};
struct InfoRecord; // (host/information_plan.h; == mp_information_entry)
void information_set(PairSet *set, int32_t num_entries, const int32_t *pair_ids, const Model *models,
                     const double *factors, const InformationOut &out, InfoRecord *entries);
// information_stats (mp_debug_information_stats): the runs since the last reset and the summed
// device milliseconds of the two kernel stages (events; measured only while profiling is
// enabled).
void information_stats(int64_t *launches, double *rows_ms, double *finish_ms, bool reset);
// ransac_adaptive_set (mp_ransac_adaptive_set): ransac_set's drawn mode with a per-pair
// number of samples.  Samples go through draw -> hypothesize_run -> select_run in rounds of
// `step` per still-active pair (checkpoints m_k = min(k step, budget)); select_run continues
// each pair's strict-< walk from its running best's score, so the running best is the winner
// of the walk over all its samples so far.  After a round a pair leaves when the estimators'
// termination rule (host/ransac_stop.h) holds on its running best's three counts and its
// samples per type (stopped[j] = 1) or when it has had `budget` samples (stopped[j] = 0).  One
// refine_run at the end.  Entry j's result equals, byte for byte, ransac_set(budget =
// results[j].num_samples, pair_ids = that pair).  Nothing grows with budget x pairs: types,
// counts and candidates are per round.  max_num_iterations is not read.
void ransac_adaptive_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                         uint64_t seed, int32_t point_share, int32_t rounds, Model *models, RansacResult *results,
                         int32_t *inlier_idx, int32_t *stopped, int64_t sample_chunk, int64_t model_chunk,
                         const DrawWeights *weights = nullptr, bool weighted_stop = false,
                         InlierMass *rule_mass = nullptr, const RansacOut *out = nullptr);
// ransac_lo_set (mp_ransac_lo_set): ransac_adaptive_set with the estimators' local
// optimisation prefix inside the rounds, two tracks per pair.  The minimal track is
// ransac_adaptive_set's in every bit (select_run is seeded with the minimal best's score).
// The overall best is the lowest score among the minimal bests and the models their LOs
// returned (host/ransac_lo_track.h): after a round's select, every entry whose minimal best
// was replaced (1) offers it to the overall best (strict <, select's counts) and (2) gets one
// LO -- a single refine_run(relax, lo_rounds) over all such entries -- whose result becomes
// the overall best when a round of it was accepted and its score is strictly lower.  The
// termination rule reads the overall best's counts; stop, continue and `stopped` are as in
// ransac_adaptive_set.  At the end one refine_run(rounds) on the overall bests.  In a result,
// score_selected, best_candidate / sample / slot / type describe the minimal track;
// score_initial, score_final, rounds_run, rounds_accepted, lm_status, num_inliers, the model
// and the lists the final refinement of the overall best (rounds = 0: the overall best as it
// stands, its lists select's or the ones its LO returned).  lo_info: one per entry.  The
// running bests are held in user units, so every LO start and the final refinement go through
// refine_run's unit change.  Nothing grows with budget x pairs; the LO's device arrays are
// sized once for the selection.
struct RansacLoInfo {
    int32_t lo_runs, lo_accepted; // LOs run; LOs that became the overall best
    int32_t lo_index;             // the candidate whose LO produced the overall best; -1: a minimal model (or none)
    int32_t pad;
};
void ransac_lo_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step, uint64_t seed,
                   int32_t point_share, int32_t rounds, int32_t lo_rounds, Model *models, RansacResult *results,
                   int32_t *inlier_idx, int32_t *stopped, RansacLoInfo *lo_info, int64_t sample_chunk,
                   int64_t model_chunk, const DrawWeights *weights = nullptr, bool weighted_stop = false,
                   InlierMass *rule_mass = nullptr, const RansacOut *out = nullptr);
// ransac_lo_steps_set (mp_ransac_lo_steps_set): ransac_lo_set with the num_lo_steps steps of the
// estimators' LocalOptimization after each local optimisation (host/ransac_lo_steps.h): lo_steps
// steps per entry whose minimal best was replaced, from the model the relaxed refinement
// returned; all steps of all such entries go through each stage in one lsq_fit_run (2 +
// num_lsq_iterations runs and one select per checkpoint), every intermediate model is offered
// to the overall best.  steps_info: one per entry.  With rounds = 0 the lists of an overall best
// that a step produced are select's for that model.
struct RansacLoStepsInfo {
    int32_t lo_step, lo_stage;              // the step and stage that gave the overall best; -1: no step did
    int32_t lo_step_offers, lo_step_accepted; // the steps' offers to the overall best; those accepted
};
void ransac_lo_steps_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                         uint64_t seed, int32_t point_share, int32_t rounds, int32_t lo_rounds, int32_t lo_steps,
                         Model *models, RansacResult *results, int32_t *inlier_idx, int32_t *stopped,
                         RansacLoInfo *lo_info, RansacLoStepsInfo *steps_info, int64_t sample_chunk,
                         int64_t model_chunk, const DrawWeights *weights = nullptr, bool weighted_stop = false,
                         InlierMass *rule_mass = nullptr, const RansacOut *out = nullptr);
// ransac's results into the caller's device arrays (mp_ransac_out_set; kernels/ransac_out.h,
// host/residuals_plan.h).  ransac_out_set takes the union of the arguments of the bodies above
// and runs the one they choose (weights nullable; step 0: ransac_set, its samples given or drawn;
// lo_rounds 0: ransac_adaptive_set; lo_steps 0: ransac_lo_set; else ransac_lo_steps_set), whose
// results and bytes are the body's own.  inlier_idx null: no list is copied back from the device;
// with a refinement to come the selection copies none either.  out (nullable; any subset of its
// arrays): memory of the set's device for the selection's R = out_off[num_sel] rows and num_sel
// pairs, checked before any launch as residuals_set checks its arrays, and pairwise disjoint.
// For entry j with a winner: models[j] = the returned model's bytes, index[j] = best_candidate,
// counts[j] = num_inliers; bit t of mask[out_off[j] + i] is set iff i is in the returned list t,
// and errors[t R + out_off[j] + i] is the squared error, in problem units, under the model those
// lists were swept from (refine_run's `swept`; rounds = 0: the selected candidate as select_run
// converts it), so (errors[t] < thr_t) == bit t on every row.  Without a winner: zeros, index -1,
// NaN errors.  Every element belonging to the selection is written once, by a kernel; the stage
// adds its items' counts per pair and throws std::logic_error when they differ from num_inliers.
// The library's stream waits for an event recorded on producer_stream before its first write.
// std::invalid_argument before any launch: errors without mask; outputs with lo_rounds >= 1 and
// rounds = 0 (the overall best's lists may be a local optimisation's, whose problem-unit model
// is not kept); lo_rounds / lo_steps without step; lo_steps without lo_rounds; weighted_stop
// without weights or step; samples with step or weights; and each body's own refusals.
struct RansacOut {
    void *mask = nullptr;    // uint8, R
    void *errors = nullptr;  // float64, 3 R, term-major; needs mask
    void *models = nullptr;  // float64, 17 num_sel
    void *index = nullptr;   // int32, num_sel
    void *counts = nullptr;  // int32, 3 num_sel
    void *producer_stream = nullptr;
    bool any() const { return mask || errors || models || index || counts; }
};
void ransac_out_set(PairSet *set, const DrawWeights *weights, int32_t num_sel, const int32_t *pair_ids, int32_t budget,
                    int32_t step, uint64_t seed, int32_t point_share, const int64_t *sample_offsets,
                    const int32_t *sample_types, const int32_t *sample_idx, int32_t rounds, int32_t lo_rounds,
                    int32_t lo_steps, bool weighted_stop, Model *models, RansacResult *results, int32_t *inlier_idx,
                    int32_t *stopped, RansacLoInfo *lo_info, RansacLoStepsInfo *steps_info, int64_t sample_chunk,
                    int64_t model_chunk, InlierMass *rule_mass, const RansacOut *out);
// ransac_out_stats (mp_debug_ransac_out_stats): the output stage's item launches since the last
// reset and their summed device milliseconds (measured only while profiling is enabled).
void ransac_out_stats(int64_t *launches, double *ms, bool reset);
// Test hook (mp_debug_ransac_lo_track; no device): host/ransac_lo_track.h walked over
// num_rounds rounds in each of which the minimal best was replaced (its score and counts,
// its candidate index, and its LO's rounds_accepted, score_final and counts).  score: the
// overall best's; out[0 .. 6]: its counts, lo_index, lo_runs, lo_accepted, source.
void ransac_lo_track(int32_t num_rounds, const double *min_score, const int32_t *min_counts, const int32_t *candidate,
                     const int32_t *lo_rounds_accepted, const double *lo_score, const int32_t *lo_counts,
                     double *score, int32_t *out);
// Test hooks.  ransac_required (mp_debug_ransac_required; no device): req[0], req[1] of the
// rule for a pair of n correspondences whose best has the list lengths counts[0 .. 2].
// select_argmin_direct (mp_debug_select_argmin): the argmin launch alone over given scores,
// seeded with prior (one per pair) or, prior null, the unseeded launch.
void ransac_required(int variant, int64_t n, const int32_t *counts, const RansacOptions &opts, uint32_t *req);
void select_argmin_direct(int32_t num_pairs, const int64_t *model_offsets, const double *scores, const double *prior,
                          int32_t *index, double *score, int device);
// Measurement hook (mp_debug_ransac_timing): the last ransac_set made while profiling was
// enabled; the stages' own splits are waited for, so nothing overlaps.
struct RansacTiming {
    double total_ms = 0, hypothesize_ms = 0, select_ms = 0, refine_ms = 0;
    double samples_ms = 0; // host, before the stages: the check of given samples, or the drawn samples' types
    HypTiming hyp;
    SelectTiming select;
    int64_t bytes_back = 0;  // copied back by the hypothesis stage
    int64_t bytes_slots = 0; // what the slot array and the counts would have been
};
RansacTiming ransac_timing_last();

// Test and measurement hooks (mp_debug_pair_set_prep, mp_debug_pair_set_rows).
// pair_set_prep_mode: how the following setups (sets and batch entries, process-wide) derive
// the calibrated rows: 0 one launch_prep_pairs, 1 one launch_prep_pair per pair; returns the
// previous mode.  pair_set_rows: rows 0 .. 11 of a pair (12 n doubles).
int pair_set_prep_mode(int mode);
void pair_set_rows(const PairSet *set, int32_t pair, double *out);
// mp_debug_pair_set_record: the data-dependent fields of the pair's device PairConst (copied
// back) and its normalization scale, host/ingest_plan.h pair_record_values' order.
// ingest_info: kIngestBlock, kIngestChunk, kIngestSpan.  device_extent: base and size of the
// allocation of `device` that holds ptr (hipMemGetAddressRange), as the ingest's checks see it.
void pair_set_record(const PairSet *set, int32_t pair, double *out);
void ingest_info(int32_t *out);
void device_extent(const void *ptr, int device, int64_t *out);

// Standalone solvers on the device (mp_solve_* / mp_relpose_5pt).
// alt: 0 default MD solver, 1 use_ours, 2 use_4p4d (two-focal)
int solve_md_direct(int variant, const double *x, const double *y, const double *dx, const double *dy, double *sols,
                    int max_sols, Model *poses, int max_poses, int *nposes, int device, int alt = 0);
// kind 0: relpose_5pt on unit bearings; 1: shared-focal 6pt; 2: two-focal 7pt +
// Bougnoux + recoverPose (normalized 2-D points).  Models before the depth fit.
int solve_point_direct(int kind, const double *x1, const double *x2, Model *poses, int max_poses, int device);
// root stage of the calibrated 5-point (variant 0) or shared-focal 6-point (variant 1)
// solver over ns samples of K = 5 / 6 normalized image points each (pts*: ns x K x 2);
// candidates into cand (ns x 96), counts into ncand
void debug_pt_roots(int variant, int64_t ns, const double *pts0, const double *pts1, double *cand, int *ncand,
                    int device);

// The standalone solvers over ns samples per call (mp_*_batch), in rounds of `chunk`
// samples (0: the default, host/solve_batch_pack.h) on one set of device buffers kept by
// the context.  Inputs sample-major, inside a sample the single-sample layout.
// solve_md_batch: pose false -> sols (ns x 8 rows of width 4 / 5 / 6, alt 0 only), pose
// true -> poses (ns x 8); relpose_batch: poses (ns x 16).  counts[s]: the sample's rows;
// the slots past it are zero.  Each row is the single-sample entry's to the bit.
void solve_md_batch(int variant, int alt, bool pose, int64_t ns, const double *x, const double *y, const double *dx,
                    const double *dy, double *sols, Model *poses, int32_t *counts, int64_t chunk, int device);
void relpose_batch(int kind, int64_t ns, const double *x0, const double *x1, Model *poses, int32_t *counts,
                   int64_t chunk, int device);

// estimate_scale_and_pose (src/solver.cpp:5-33) on the device; X, Y point-major n x 3
void scale_and_pose_direct(const double *X, const double *Y, const double *W, int64_t n, Model *out, int device);
// get_depths of num pairs on the device (see launch_get_depths); dims: num x 4
// (depth-map h, w, image h, w); host buffers in and out
// squared Bougnoux focals of k fundamental matrices (device kernel, mp_bougnoux_focals)
void bougnoux_batch(int64_t k, const double *F, double *out, int device);
// compute_pose_error of k pairs and the pose AUC of max(err_R, err_t) at nthr
// thresholds on the device (mp_pose_eval); host buffers in and out
void pose_eval_batch(int64_t k, const double *R, const double *t, const double *T, double t_thres, double *err_t,
                     double *err_R, int nthr, const double *thr, double *aucs, int device);
// the pose AUC of k given errors at nthr thresholds (mp_pose_auc)
void pose_auc_batch(int64_t k, const double *errors, int nthr, const double *thr, double *aucs, int device);
void get_depths_batch(int dtype, int32_t num, const void *maps, const int64_t *dims, const int64_t *pt_off,
                      const double *pts, void *out, int device);

int device_count();

// Per-kernel device timing of the estimator's batch launches, measured with HIP
// events on the engine's own stream (mp_profile_* C API).  Process-wide totals.
struct KernelProfile {
    uint64_t batches = 0;          // speculative batches timed
    uint64_t iterations = 0;       // minimal samples solved
    uint64_t hypotheses = 0;       // models scored by score_batch
    uint64_t correspondences = 0;  // sum over batches of (hypotheses x n)
    uint64_t sweeps = 0;           // single-model LO / termination sweeps
    double solve_ms = 0.0;         // md_solve + pt_solve
    double score_ms = 0.0;         // score_batch
    uint64_t lm_calls = 0;         // host LM solves inside LO
    double lm_wall_ms = 0.0;       // host wall time in the LM
    double sweep_wall_ms = 0.0;    // host wall time of single-model sweeps (incl. copies + sync)
    double sample_wall_ms = 0.0;   // host minimal-sample generation (incl. LO rewinds)
    double wait_wall_ms = 0.0;     // host wait for batch results
    double run_wall_ms = 0.0;      // whole estimator runs
    uint64_t lm_blocks = 0;        // residual blocks over all LM solves
    uint64_t lm_big_calls = 0;     // LM solves with >= kBigLM residual blocks
    double lm_big_wall_ms = 0.0;   // host wall time of those
    uint64_t model_trips = 0;      // score_batch (model, 256-correspondence trip) pairs evaluated
    uint64_t model_trips_full = 0; // ... and without the early exit (models x trips)
    uint64_t accepted = 0;         // hypotheses of the iterations the estimator consumed
    uint64_t scored = 0;           // hypotheses whose score_batch sweep ran (not record-skipped)
    uint64_t tie_checks = 0;       // iterations whose new-best decision needed reference-order re-scoring
};
constexpr size_t kBigLM = 1024;
void profile_enable(bool on);
void profile_reset();
KernelProfile profile_read();

} // namespace mp
