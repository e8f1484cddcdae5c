/* madpose_mi355x.h -- C ABI of the MI355X-native hybrid-RANSAC relative-pose engine.
 *
 * Drop-in boundary for kocurvik/madpose's Python estimator API.  Each entry point
 * replaces one binding of the reference's pybind11 module (src/bindings.cpp) and
 * keeps its argument meaning; the reference signatures are cited per function.
 * Plain pointers and sizes only.  All buffers are owned by the caller; inputs are
 * copied to device memory inside the call.  Calls are re-entrant per device.
 *
 * Return codes: MP_OK, MP_EINVAL (bad sizes/options), MP_EDEVICE (HIP error; text
 * via mp_last_error()).  There is no CPU fallback: without a usable MI355X device
 * every compute entry point returns MP_EDEVICE.
 */
#ifndef MADPOSE_MI355X_H
#define MADPOSE_MI355X_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MP_OK 0
#define MP_EINVAL 1
#define MP_EDEVICE 2

/* estimator variants */
#define MP_CALIBRATED 0   /* HybridEstimatePoseScaleOffset          */
#define MP_SHARED_FOCAL 1 /* HybridEstimatePoseScaleOffsetSharedFocal */
#define MP_TWO_FOCAL 2    /* HybridEstimatePoseScaleOffsetTwoFocal    */
#define MP_SCALE_ONLY 3   /* HybridEstimatePoseAndScale (K0/K1 as cam0/cam1, min_depth ignored) */

/* ExtendedHybridLORansacOptions (src/hybrid_ransac.h:17-25, src/bindings.cpp:78-95) */
typedef struct mp_ransac_options {
    double success_probability;
    double squared_inlier_thresholds[2]; /* [reprojection^2, epipolar^2] (user units) */
    double data_type_weights[2];         /* [reprojection, epipolar]                  */
    double threshold_multiplier;
    uint32_t min_num_iterations;
    uint32_t max_num_iterations;
    uint32_t max_num_iterations_per_solver;
    uint32_t random_seed;
    int32_t num_lo_steps;
    int32_t num_lsq_iterations;
    int32_t min_sample_multiplicator;
    int32_t non_min_sample_multiplier;
    int32_t lo_starting_iterations;
    int32_t final_least_squares;
    int32_t use_ours;
    int32_t use_4p4d;
} mp_ransac_options;

/* EstimatorConfig (src/estimator_config.h:7-33, src/bindings.cpp:99-109) */
typedef struct mp_estimator_config {
    double ceres_function_tolerance;
    double ceres_gradient_tolerance;
    double ceres_parameter_tolerance;
    double ceres_max_num_iterations;
    int32_t solver_type; /* 0 HYBRID, 1 EPI_ONLY, 2 MD_ONLY */
    int32_t score_type;
    int32_t lo_type;
    int32_t min_depth_constraint;
    int32_t use_shift;
    int32_t ceres_use_nonmonotonic_steps;
    int32_t ceres_num_threads;
    int32_t reserved;
} mp_estimator_config;

/* PoseScaleOffset{,SharedFocal,TwoFocal} (src/pose.h:7-56); R row-major, x1 = R x0 + t */
typedef struct mp_model {
    double R[9];
    double t[3];
    double scale, offset0, offset1;
    double focal0, focal1; /* SF: focal0 == focal1 == focal */
} mp_model;

/* HybridRansacStatistics (src/bindings.cpp:67-76) + engine counters */
typedef struct mp_stats {
    double best_model_score;
    double inlier_ratios[3];
    uint64_t num_hypotheses;       /* models scored by minimal-sample iterations */
    uint64_t num_lo_sweeps;        /* full 3N sweeps issued by LO / termination   */
    uint32_t num_iterations_total;
    uint32_t num_iterations_per_solver[2];
    int32_t best_num_inliers;
    int32_t best_solver_type;
    int32_t number_lo_iterations;
    int32_t num_inliers[3]; /* lengths of the three inlier lists */
    int32_t num_batches;     /* speculative GPU batches issued */
    double seconds_total, seconds_lo, seconds_gpu_wait;
} mp_stats;

/* Full estimator.  Replaces
 *   HybridEstimatePoseScaleOffset            (src/hybrid_pose_estimator.cpp:8-35, bindings.cpp:169-170)
 *   HybridEstimatePoseScaleOffsetSharedFocal (src/hybrid_pose_shared_focal_estimator.cpp:8-51, :171-172)
 *   HybridEstimatePoseScaleOffsetTwoFocal    (src/hybrid_pose_two_focal_estimator.cpp:34-75, :173-174)
 *   HybridEstimatePoseAndScale               (src/hybrid_pose_estimator.cpp:37-63, 297-442, :167-168)
 * x0, x1: n x 2 row-major pixels; d0, d1: n depth priors; min_depth[2];
 * cam0/cam1: K (9, row-major) for MP_CALIBRATED, principal point (2) otherwise.
 * inlier_idx: optional caller buffer of 3*n int32; list t starts at t*n and has
 * stats->num_inliers[t] entries (reproj0, reproj1, sampson). */
int mp_estimate(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                const double *min_depth, const double *cam0, const double *cam1, const mp_ransac_options *options,
                const mp_estimator_config *config, mp_model *out_model, mp_stats *out_stats, int32_t *inlier_idx,
                int device);

/* estimate_scale_and_pose(X, Y, W) (src/solver.cpp:5-33, binding src/bindings.cpp:156):
 * weighted Procrustes with scale, Y ~ scale R X + t; X, Y point-major n x 3. */
int mp_estimate_scale_and_pose(const double *X, const double *Y, const double *W, int64_t n, mp_model *out,
                               int device);

/* Many independent pairs in one call (pairs concatenated; offsets[p]..offsets[p+1]).
 * min_depth: 2 per pair; cams: 9 or 2 doubles per pair; inlier buffers per pair at
 * 3*offsets[p].  Pairs run concurrently on one device. */
int mp_estimate_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                      const double *d0, const double *d1, const double *min_depth, const double *cam0,
                      const double *cam1, const mp_ransac_options *options, const mp_estimator_config *config,
                      mp_model *out_models, mp_stats *out_stats, int32_t *inlier_idx, int device, int num_streams);

/* solve_scale_and_shift{,_shared_focal,_two_focal} (src/solver.cpp:35-480, bindings.cpp:157-161).
 * x_homo, y_homo: K homogeneous points stored point-major (3*K doubles: x,y,w per point),
 * K = 3 (cal) or 4 (sf/tf).  out: max_out rows of width 4/5/6; returns count (>=0) or -code. */
int mp_solve_scale_and_shift(int variant, const double *x_homo, const double *y_homo, const double *depth_x,
                             const double *depth_y, double *out, int max_out, int device);

/* solve_scale_shift_pose{,_shared_focal,_two_focal} (src/solver.cpp:482-534, 682-739, 986-1043,
 * wrappers 1408-1433, bindings.cpp:162-166).  Returns count or -code. */
int mp_solve_scale_shift_pose(int variant, const double *x_homo, const double *y_homo, const double *depth_x,
                              const double *depth_y, mp_model *out, int max_out, int device);

/* Option-gated alternates of the MD solvers (HybridLORansacOptions::use_ours / use_4p4d):
 * alt 1 = solve_scale_shift_pose{,_shared_focal,_two_focal}_ours (src/solver.cpp:623-680,
 * 818-984, 1045-1148), alt 2 = solve_scale_shift_pose_two_focal_4p4d (:1287-1406).
 * Same point layout as mp_solve_scale_shift_pose.  Returns count or -code. */
int mp_solve_scale_shift_pose_alt(int variant, int alt, const double *x_homo, const double *y_homo,
                                  const double *depth_x, const double *depth_y, mp_model *out, int max_out, int device);

/* Batched device sweep over one pair's correspondences (ScoreModel / GetInliers,
 * src/hybrid_ransac.h:265-349) for num_models models given in problem units.
 * Used by tests to check the scoring kernel directly.  scores: num_models;
 * errors (optional): num_models x 3 x n squared errors (is_for_inlier = true). */
int mp_score_models(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                    const double *cam0, const double *cam1, const mp_ransac_options *options,
                    const mp_estimator_config *config, const mp_model *models, int32_t num_models, double *scores,
                    double *errors, int device);

/* mp_debug_score_batch: the estimator's scoring kernel (score_batch) on explicit
 * model lists -- test hook.  models: num_iterations x M (M = 10 / 16 / 4 for the
 * calibrated / shared-focal / two-focal variant, problem units), counts[b] of them
 * used by iteration b.  best: the pre-batch best; flags: 1 the exact early exit
 * against it, 2 the record skip.  Outputs per iteration: res_best, res_slot (bit 16:
 * another model's screening interval reaches the best's; bit 17: a correspondence
 * outside the margins' cover was flagged), rec_models[b] (the mapped record model,
 * written when the iteration could hold a new best), res_hi_lo (nullable, 2 per
 * iteration: best + its margin, min over models of score - margin), model_ties
 * (nullable, num_iterations x M: each model's screening margin). */
int mp_debug_score_batch(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                         const double *d1, const double *cam0, const double *cam1, const mp_ransac_options *options,
                         const mp_estimator_config *config, int32_t num_iterations, const int32_t *counts,
                         const mp_model *models, double best, int32_t flags, double *res_best, int32_t *res_slot,
                         mp_model *rec_models, double *res_hi_lo, double *model_ties, int device);

/* mp_debug_score_terms: score_batch's residual evaluation of explicit models, per
 * correspondence -- test hook of the screening margins.  errors: num_models x 3 x n
 * (reprojection 0 -> 1, 1 -> 0, Sampson; the score kernel's own forms and gating);
 * flags: num_models x n (1: the correspondence lies outside the margins' cover); taus
 * (nullable): num_models x 3 per-term bounds; ties (nullable): each model's margin. */
int mp_debug_score_terms(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                         const double *d1, const double *cam0, const double *cam1, const mp_ransac_options *options,
                         const mp_estimator_config *config, const mp_model *models, int32_t num_models, double *errors,
                         int32_t *flags, double *taus, double *ties, int device);

/* mp_debug_score_margins: the screening margins of explicit models as the score kernel's
 * records carry them, formed on the host -- test hook, no device.  per_model: 8 per
 * model (the per-term bounds tau0, tau1, tau2; the gate windows wz0, wz1, wl; the Sampson
 * denominator floor kg2; the margin of the sum, tie).  per_pair (nullable, 9): the
 * thresholds (3) and weights (3) of the three terms after the estimators' option
 * transform, the normalization scale (1 for calibrated pairs), the Sampson loss scale,
 * and 1 if the calibrated ray form applies (upper-triangular intrinsics), else 0. */
int mp_debug_score_margins(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                           const double *d1, const double *cam0, const double *cam1,
                           const mp_ransac_options *options, const mp_estimator_config *config, const mp_model *models,
                           int32_t num_models, double *per_model, double *per_pair);

/* mp_debug_lo_sweep: the same models through the engine's host LO sweep
 * (madpose_amd/csrc/host/lo_sweep.h), the sweep LocalOptimization and
 * UpdateRANSACTerminationCriteria use (src/hybrid_ransac.h:265-349, 383-538): errors
 * and ScoreModel sums in the reference's operation order -- test hook, no device.
 * fast_bounds (nullable, 2 per model): the LO's fast sum of the same terms and its
 * bound on the distance to the reference-order sum (lo_sweep.h lo_sweep_fast). */
int mp_debug_lo_sweep(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                      const double *cam0, const double *cam1, const mp_ransac_options *options,
                      const mp_estimator_config *config, const mp_model *models, int32_t num_models, double *scores,
                      double *errors, double *fast_bounds);

/* get_depths (madpose/utils.py:4-22) for many pairs in one launch: pair p's depth map
 * (dims[4p] x dims[4p+1], row-major, float32 for dtype 0 or float64 for dtype 1) is
 * stored after the previous pairs' maps in depth_maps; dims[4p+2], dims[4p+3] are the
 * image height and width the keypoints refer to; its keypoints (x, y pairs, float64)
 * are keypoints[2 pt_offsets[p] .. 2 pt_offsets[p+1]) and the depths go to
 * out[pt_offsets[p] ..] (dtype of the maps).  Same rounding (half to even), clipping
 * and [y, x] lookup as the reference's numpy code, so results are bit-identical. */
int mp_get_depths(int dtype, int32_t num_pairs, const void *depth_maps, const int64_t *dims, const int64_t *pt_offsets,
                  const double *keypoints, void *out, int device);

/* Batched device Levenberg-Marquardt: the Ceres solves of the local
 * optimisation -- HybridPoseOptimizer* (src/optimizer.h:48-125, SF :265-369, TF
 * :383-499) over the cost functors of src/cost_functions.h:16-387, as called by
 * LeastSquares (kinds[j] = 0; src/hybrid_pose_estimator.cpp:263-295) or
 * NonMinimalSolver (1; :188-214) -- for num_problems problems on one pair, one device
 * workgroup each.  Problem j refines models[j] (in/out, problem units: SF/TF focals
 * divided by the pair's normalize_points scale) over the residual blocks
 * sample_idx[sample_offsets[3j] ..) (reprojection 0->1), [sample_offsets[3j+1] ..)
 * (1->0), [sample_offsets[3j+2] .. sample_offsets[3j+3]) (Sampson).  status[j]: 1
 * refined, 0 no residuals, 2 infeasible constant bounded block, 3 too few data for
 * the solver (model unchanged in cases 0, 2, 3).  Options and config as mp_estimate
 * (thresholds / weights / Ceres settings); min_depth may be NULL (zeros). */
int mp_lm_refine_batch(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                       const double *d1, const double *min_depth, const double *cam0, const double *cam1,
                       const mp_ransac_options *options, const mp_estimator_config *config, int32_t num_problems,
                       const int32_t *kinds, const int64_t *sample_offsets, const int32_t *sample_idx,
                       mp_model *models, int32_t *status, int device);

/* mp_debug_lm_refine_host: the same problems through the engine's host LM (the
 * default LO path) -- test hook, no device needed. */
int mp_debug_lm_refine_host(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                            const double *d1, const double *min_depth, const double *cam0, const double *cam1,
                            const mp_ransac_options *options, const mp_estimator_config *config, int32_t num_problems,
                            const int32_t *kinds, const int64_t *sample_offsets, const int32_t *sample_idx,
                            mp_model *models, int32_t *status);

/* mp_debug_lm_system: one evaluation and one step of the same problems at their start
 * models -- test hook of the LM's normal equations (tests/test_lm_system_*.py).  Pair,
 * options, config, kinds, sample_offsets and sample_idx as mp_lm_refine_batch (no size
 * rule: any lists); models[j] the point of evaluation, radius[j] the trust-region radius
 * of the step.  where: 0 the device (the production kernels' setup, evaluation and step
 * functions, one workgroup per problem), 1 / 2 the host's 4-wide (AVX2) / 8-wide (AVX-512)
 * residual evaluation called directly over the blocks block_ranges[2j] .. block_ranges[2j+1]
 * of the concatenated list (null or negative: all; the accumulators as they come), 3 the
 * host LM's evaluate() (the compacted system, inactive entries zero); the host's step on
 * the compacted system in all three.  where 2 without AVX-512 is MP_EINVAL.  Outputs per
 * problem in the full 11-parameter layout (rotation tangent 3, t 3, scale, offset0,
 * offset1, focal0, focal1; on the device entries past the variant's parameters are zero):
 * cost, g[11] = J^T r, H[66] = the packed upper triangle of J^T J, col[11] = 1 for an
 * active parameter, d[11] = the step (0 on inactive parameters), pd = 1 the damped system
 * was positive definite, 0 it was not (d = 0), -1 nothing was evaluated (status 0 or 2 as
 * mp_lm_refine_batch; everything else zero). */
int mp_debug_lm_system(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                       const double *min_depth, const double *cam0, const double *cam1,
                       const mp_ransac_options *options, const mp_estimator_config *config, int32_t num_problems,
                       const int32_t *kinds, const int64_t *sample_offsets, const int32_t *sample_idx,
                       const mp_model *models, const double *radius, int32_t where, const int64_t *block_ranges,
                       double *cost, double *g, double *H, int32_t *col, double *d, int32_t *pd, int32_t *status,
                       int device);

/* Device refinement of given poses over many pairs: for callers who have a pose already
 * (a previous frame, a regressor, another estimator, an earlier run with other
 * thresholds) and want it polished with the estimators' depth-aware cost.  The
 * reference does this inside its estimator: LeastSquaresFit with
 * use_all_solver_inliers (src/hybrid_ransac.h:406, 484-510) and the final least squares
 * with its score < best rule (:186-203).  Per pair, with the current model m of score s,
 * one round is:
 *   1. the three squared-error arrays of m (is_for_inlier = true: the errors
 *      mp_score_models returns);
 *   2. list t = the ascending indices i with err[t][i] < threshold t (strict; the
 *      thresholds after the estimators' option transform, for SF / TF in normalized units);
 *   3. the LeastSquares call (kind 0) of mp_lm_refine_batch on the three lists from m,
 *      with its size rule (status 3, model unchanged) and settings, on the device LM;
 *   4. the score of the result as mp_score_models gives it;
 *   5. status 1 and a strictly lower score: the model, its score and its lists are
 *      accepted and the next round starts from them; otherwise the pair stops and keeps
 *      what it had.
 * At most `rounds` rounds run (1..64); the first round's step 1 also gives
 * score_initial.  The reported lists and score are the accepted model's.  Models cross
 * this boundary in user units as the estimators return them (SF / TF focals are divided
 * by the pair's normalization scale on the way in and multiplied back on the way out;
 * results[p].norm_scale is that scale); a pair without an accepted round keeps its
 * model's bytes.  MP_SCALE_ONLY runs on the calibrated geometry as elsewhere.
 * Pair layout exactly as mp_estimate_batch (offsets, min_depth 2 per pair, cameras 9 or 2
 * per pair); inlier_idx (nullable): pair p at 3*offsets[p], list t at + t*n_p,
 * results[p].num_inliers[t] entries.  A pair with n = 0 is legal: score 0, empty lists,
 * status 3.  The pairs run in runs of `chunk` pairs whose data is resident on the device
 * at once, one sweep launch and one LM launch per round over all pairs still running
 * (chunk 0: as many pairs as hold MP_REFINE_RUN_CORRESPONDENCES correspondences, under
 * 1 GiB of device memory).  num_pairs == 0 returns MP_OK without touching the device;
 * negative counts, decreasing offsets, null required pointers, rounds outside 1..64,
 * chunk < 0, a bad variant or invalid options give MP_EINVAL before any device call. */
#define MP_REFINE_RUN_CORRESPONDENCES 4194304
typedef struct mp_refine_result {
    double score_initial, score_final, norm_scale;
    int32_t rounds_run, rounds_accepted;
    int32_t lm_status;      /* of the last round run: 0/1/2/3 as mp_lm_refine_batch; -1: no round ran */
    int32_t num_inliers[3]; /* lists of the returned model */
} mp_refine_result;
int mp_refine_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                    const double *d0, const double *d1, const double *min_depth, const double *cam0,
                    const double *cam1, const mp_ransac_options *options, const mp_estimator_config *config,
                    int32_t rounds, mp_model *models /* in/out, one per pair */, mp_refine_result *results,
                    int32_t *inlier_idx /* nullable */, int64_t chunk, int device);

/* Ranking of candidate poses over many pairs on the device: for callers who have several
 * poses per pair (from several depth models, a retrieval or localisation prior beside an
 * estimator, runs with other thresholds, the batched solvers) and need the one the
 * estimators' depth-aware MSAC cost prefers, with the correspondences it explains.  Pair
 * p has n_p correspondences and the candidates models[model_offsets[p] ..
 * model_offsets[p+1]), in user units as the estimators return them and as mp_refine_batch
 * takes them (SF / TF focals are divided once by the pair's normalization scale,
 * results[p].norm_scale, on the way in; MP_SCALE_ONLY runs on the calibrated geometry as
 * elsewhere).  For every candidate m (its index into models):
 *   1. scores[m] = the score mp_score_models returns for the same pair, options, config
 *      and the model in problem units, bit for bit;
 *   2. counts[3m + t], t = 0..2, = the number of i with err[t][i] < threshold t (strict;
 *      the is_for_inlier = true errors mp_score_models returns, the thresholds after the
 *      estimators' option transform): the length of the list mp_refine_batch would form.
 * Per pair:
 *   1. best_index by the reference's GetBestEstimatedModelId (src/hybrid_ransac.h:245-263):
 *      start at DBL_MAX, walk the candidates in order, take one only on a strict <.  Of
 *      equal scores the first wins; a NaN or infinite score never wins.  With no
 *      candidates, or none that wins: best_index -1, best_score DBL_MAX, counts 0, empty
 *      lists;
 *   2. the winner's three ascending inlier lists (rule 2 above) in mp_refine_batch's
 *      inlier_idx layout; they and best_score equal the lists and score_initial that
 *      mp_refine_batch reports for that model.
 * A pair with n = 0 is legal: every score is 0, so candidate 0 wins if there is one.  No
 * min_depth is taken: no score depends on it.  Pair layout, `chunk` and its default run
 * bound as mp_refine_batch.  model_chunk: the candidates whose score records are on the
 * device at once (0: MP_SELECT_SLAB_MODELS); a slab may cut through a pair's candidates.
 * Results depend on neither chunk nor model_chunk.  scores, counts and inlier_idx are
 * nullable.  num_pairs == 0 returns MP_OK without touching the device; negative counts,
 * decreasing or negative offsets or model_offsets, more than 2^28 candidates, null
 * required pointers (models too when there is a candidate), chunk < 0, model_chunk < 0, a
 * bad variant or invalid options give MP_EINVAL before any device call. */
#define MP_SELECT_SLAB_MODELS 65536
#define MP_SELECT_TILE 1 /* candidates per device work item */
typedef struct mp_select_result {
    double best_score, norm_scale;
    int32_t best_index;     /* within the pair's candidates; -1: none */
    int32_t num_inliers[3]; /* the winner's lists */
} mp_select_result;         /* 32 bytes */
int mp_select_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                    const double *d0, const double *d1, const double *cam0, const double *cam1,
                    const mp_ransac_options *options, const mp_estimator_config *config,
                    const int64_t *model_offsets, const mp_model *models,
                    double *scores /* nullable: one per candidate */, int32_t *counts /* nullable: 3 per candidate */,
                    mp_select_result *results, int32_t *inlier_idx /* nullable */, int64_t chunk,
                    int64_t model_chunk, int device);
/* Measurement hooks of mp_select_batch (tools/select_batch_bench.py).
 * mp_debug_select_tile: candidates per work item of the following calls (1, 2, 4 or 8; 0:
 * MP_SELECT_TILE); returns the previous setting, -1 for a bad value.  Only MP_SELECT_TILE
 * is pinned to mp_score_models' bits; another size may move a score in its last bits.
 * mp_debug_select_timing: six stage times in ms of the last call made
 * while profiling was enabled (mp_profile_enable) -- pair setup, host record preparation,
 * record upload, select_score, select_argmin with its copies back, the winners' sweep
 * with its copies back; every stage is waited for then, so nothing overlaps. */
int mp_debug_select_tile(int tile);
int mp_debug_select_timing(double *out_ms /* 6 */);

/* The estimators' sample models over many pairs: for explicit minimal samples, exactly the
 * models the estimator's MinimalSolver stage generates for them, one launch sequence for all
 * pairs, in the form mp_select_batch takes.  Pair layout, `chunk` and its default run bound
 * as mp_refine_batch.  Pair p's samples are s = sample_offsets[p] .. sample_offsets[p + 1] - 1:
 * sample_types[s] 0 (the MD solver) or 1 (the point solver), sample_idx[8 s ..] its indices
 * within the pair -- a type-0 sample reads its first 3 (calibrated) or 4, a type-1 sample
 * its first 5 (calibrated), 6 (shared focal) or 7 (two focal); the other slots are ignored.
 * Sample s gets counts[s] models in models[s * slots ..], slots = MP_HYPOTHESIZE_SLOTS_*
 * of the variant, in the estimator's order: the models the estimator puts in the
 * iteration's model slots for the same pair, options, config, solver type and sample (the
 * ones MADPOSE_MODEL_DUMP records), all 17 doubles bit for bit -- type 0 the exact MD
 * solver with the estimator's min-depth filter, type 1 5pt / 6pt / 7pt with pose recovery,
 * depth tail, compaction and the shared-focal duplicate rule.  Models leave in user units,
 * as mp_estimate returns them: for shared and two focal each focal is the problem-unit
 * focal times the pair's norm_scale (one IEEE product).  Slots from counts[s] on are zero.
 * Results depend on neither chunk nor sample_chunk (samples on the device at once; 0:
 * MP_HYPOTHESIZE_SLAB_SAMPLES, values above 131072 act as 131072), nor on the other pairs
 * or samples of the call.  norm_scale (nullable): one per pair.
 * Supported: MP_CALIBRATED, MP_SHARED_FOCAL, MP_TWO_FOCAL with use_shift on and without
 * use_ours / use_4p4d; MP_SCALE_ONLY, use_shift = 0 and the alternates give MP_EINVAL.
 * min_depth and min_depth_constraint are honoured.  Checked on the host before any device
 * call, MP_EINVAL: a bad variant, negative counts, decreasing or negative offsets or
 * sample_offsets, more than 2^22 samples, null required pointers, chunk < 0, sample_chunk
 * < 0, a type other than 0 or 1, a read index outside [0, n_p), a repeated index within a
 * sample, a sample on a pair too small for its solver.  num_pairs == 0, and zero samples
 * once the arguments are valid, return MP_OK without touching the device. */
#define MP_HYPOTHESIZE_SLAB_SAMPLES 32768
#define MP_HYPOTHESIZE_SLOTS_CALIBRATED 10
#define MP_HYPOTHESIZE_SLOTS_SHARED_FOCAL 16
#define MP_HYPOTHESIZE_SLOTS_TWO_FOCAL 4
int mp_hypothesize_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                         const double *d0, const double *d1, const double *min_depth, const double *cam0,
                         const double *cam1, const mp_ransac_options *options, const mp_estimator_config *config,
                         const int64_t *sample_offsets /* num_pairs + 1 */,
                         const int32_t *sample_types /* S: 0 the MD solver, 1 the point solver */,
                         const int32_t *sample_idx /* S x 8, indices within the pair; unused slots ignored */,
                         mp_model *models /* S x slots(variant) */, int32_t *counts /* S */,
                         double *norm_scale /* nullable, one per pair */, int64_t chunk, int64_t sample_chunk,
                         int device);
/* Measurement hook (tools/hypothesize_batch_bench.py): five stage times in ms of the last
 * mp_hypothesize_batch call made while profiling was enabled (mp_profile_enable) -- pair
 * setup, host planning, uploads, the solve launches, the copies back; every stage is waited
 * for then. */
int mp_debug_hypothesize_timing(double *out_ms /* 5 */);

/* Pair sets: pairs set up once and resident on one device, for callers who run the stages
 * mp_hypothesize_batch -> mp_select_batch -> mp_refine_batch (or any of them, several times)
 * over the same pairs.  Each batch entry sets its pairs up per call (the problem of every
 * pair, the packed upload, the pair records, the calibrated preparation); a set does it at
 * creation, and mp_hypothesize_set / mp_select_set / mp_refine_set are the same stages on
 * the resident pairs.
 * mp_pair_set_create: pair layout exactly as mp_refine_batch (offsets, min_depth 2 per pair,
 * cameras 9 or 2 per pair).  The thresholds, weights, score type, min_depth, use_shift and
 * the MD alternates live in the per-pair device records, so options and config belong to
 * the set, not to a call (copies are kept for the LM).  All pairs are one resident range on
 * `device`: at most MP_PAIR_SET_MAX_CORRESPONDENCES correspondences.  MP_EINVAL, checked
 * before any array but offsets is read and before the device is touched: a bad variant, a
 * negative count, null required pointers, negative or decreasing offsets, a pair above 2^28
 * or a total above the bound, invalid options.  num_pairs == 0 gives a valid empty set (no
 * device call).  mp_pair_set_destroy(NULL) is MP_OK.  Sets still open when the process ends
 * are released at library teardown.
 * mp_pair_set_info (every output nullable): resident_bytes = 96 per correspondence for the
 * rows, plus 12 per correspondence for each list buffer allocated so far -- none after
 * creation or mp_hypothesize_set, one after mp_select_set, two after mp_refine_set (120 per
 * correspondence then); the per-pair records (under 1 KiB a pair) are not counted.
 * Calls: pair_ids NULL = all pairs in order, num_sel must equal the set's pair count;
 * otherwise num_sel indices into the set in any order, each in range and at most once
 * (MP_EINVAL names the position).  Every per-pair argument and result is indexed by the
 * position j in the selection: models[j] / results[j], model_offsets / sample_offsets
 * (num_sel + 1 values) and what they index; inlier_idx (nullable) is the batch layout over
 * the selected pairs in selection order: entry j at 3 * (correspondences of the entries
 * before j), list t at + t * n_j.  Each call returns exactly the bytes its batch entry
 * returns on the selected pairs' inputs in that order with the set's options and config
 * (mp_select_batch takes no min_depth: no score depends on it).  mp_hypothesize_set gives
 * MP_EINVAL on a set whose variant or options mp_hypothesize_batch rejects (MP_SCALE_ONLY,
 * use_shift = 0, use_ours, use_4p4d); such a set can be selected on and refined.  The
 * normalization scales are mp_pair_set_norm_scales (one per pair of the set).
 * A call leaves nothing in the set that a later call can see: any order of calls gives
 * each call the bytes it gives on a fresh set.  Calls on one set are serialised; calls on
 * different sets are independent. */
typedef struct mp_pair_set mp_pair_set;
#define MP_PAIR_SET_MAX_CORRESPONDENCES 67108864 /* 2^26; 120 bytes resident each */
int mp_pair_set_create(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                       const double *d0, const double *d1, const double *min_depth, const double *cam0,
                       const double *cam1, const mp_ransac_options *options, const mp_estimator_config *config,
                       int device, mp_pair_set **out);
/* mp_pair_set_create_device: mp_pair_set_create from arrays that are already on `device` --
 * keypoints out of a matcher, depths out of a depth network.  The set is, bit for bit, the one
 * mp_pair_set_create builds from the same numbers (the screening magnitudes of calibrated
 * pairs to the last few bits; no result depends on them), so every stage returns the same
 * bytes on it.  Host arguments (variant, num_pairs, offsets, min_depth, cam0, cam1, options,
 * config, device) exactly as there.  Device arguments, in mp_device_pairs:
 *   x0, x1          T x 2 interleaved pixel coordinates (T = offsets[num_pairs]) of element
 *                   type xy_type: 0 float32 (every value widened to double exactly), 1 float64;
 *   d0, d1          T depth priors of element type depth_type -- or
 *   depth_maps      a HOST table of num_maps device pointers to contiguous row-major 2-D maps
 *                   of one element type map_type, with map_dims (host, num_maps x 4: h, w,
 *                   image_h, image_w as mp_get_depths takes them) and map_ids (host, num_pairs x
 *                   2: the map of side 0 / side 1 of each pair; a map may serve many pairs and
 *                   either side).  The prior of a correspondence is mp_get_depths' value for
 *                   the pair's keypoint: keypoint * (w / image_w, h / image_h) in double, rint,
 *                   clipped, [row, col].
 *   Exactly one depth source: d0 / d1 null with the maps, the map fields null / 0 with d0 / d1.
 *   producer_stream a hipStream_t (NULL: the device's null stream) on which the inputs are
 *                   produced: the library records an event on it and makes its own stream wait
 *                   for that event before the first read; the caller's stream is never
 *                   synchronised with the host.
 * The call returns after the library's own stream is synchronised; the inputs are not
 * referenced after it returns and are never written.  MP_EINVAL, all before any launch or
 * copy: everything mp_pair_set_create checks, type codes outside {0, 1}, both or neither
 * depth source, map ids outside 0 .. num_maps - 1, non-positive map or image sizes, and for
 * every device pointer: not device memory of `device` (hipPointerGetAttributes), not aligned
 * to its element type, or the bytes the kernels read not inside the allocation's address range
 * (hipMemGetAddressRange) -- the message names the argument.  The runtime knows allocations,
 * not tensors: an array carved out of a caching allocator's block (a PyTorch tensor) is bounded
 * by that BLOCK, so an array that is merely shorter than offsets[num_pairs] inside a larger block
 * is NOT refused here -- the caller's shapes are the caller's to check (PairSet.from_device checks
 * them).  The kernels assume element alignment only.  num_pairs == 0 gives a valid empty set without touching the device. */
typedef struct mp_device_pairs {
    const void *x0, *x1;
    int32_t xy_type;
    int32_t depth_type;
    const void *d0, *d1;
    const void *const *depth_maps;
    const int64_t *map_dims;
    const int32_t *map_ids;
    int32_t num_maps;
    int32_t map_type;
    void *producer_stream;
} mp_device_pairs;
int mp_pair_set_create_device(int variant, int32_t num_pairs, const int64_t *offsets, const mp_device_pairs *inputs,
                              const double *min_depth, const double *cam0, const double *cam1,
                              const mp_ransac_options *options, const mp_estimator_config *config, int device,
                              mp_pair_set **out);
int mp_pair_set_destroy(mp_pair_set *set);
int mp_pair_set_info(const mp_pair_set *set, int32_t *variant, int32_t *num_pairs, int64_t *correspondences,
                     int64_t *resident_bytes, int32_t *device);
int mp_pair_set_norm_scales(const mp_pair_set *set, double *out /* num_pairs */);
int mp_refine_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int rounds,
                  mp_model *models /* in/out, one per selected pair */, mp_refine_result *results,
                  int32_t *inlier_idx /* nullable */);
int mp_select_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *model_offsets,
                  const mp_model *models, double *scores /* nullable */, int32_t *counts /* nullable */,
                  mp_select_result *results, int32_t *inlier_idx /* nullable */, int64_t model_chunk);
int mp_hypothesize_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *sample_offsets,
                       const int32_t *sample_types, const int32_t *sample_idx, mp_model *models, int32_t *counts,
                       int64_t sample_chunk);
/* Fixed-budget RANSAC over a pair set in one call, and its two new parts.  Selection
 * (num_sel, pair_ids), per-entry indexing and the inlier_idx layout as the calls above; the
 * three entries give MP_EINVAL, before any device call, on the sets mp_hypothesize_set
 * refuses.
 *
 * mp_draw_set: `budget` minimal samples for every selected pair, drawn on the device, in the
 * form mp_hypothesize_set takes (8 slots per sample, unread slots 0).  sample_counts[j] is
 * budget, or 0 for a pair too small for the MD solver; entry j's samples start at the running
 * sum of the counts before it.  The generator is Philox4x32-10 (multipliers 0xD2511F53,
 * 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), key (seed low, seed high), counter
 * (s, block, pair, 0): s the sample's index within the pair, pair the pair's index in the set
 * (not its position in the selection: a subset draws what the whole set draws for its pairs),
 * block = 0, 1, ...; the sample's words are the blocks' four outputs in order.  For a pair
 * of n correspondences, k_md = 3 (calibrated) or 4, k_pt = 5 / 6 / 7: word 0 gives the type, 1
 * (point solver) iff (w0 >> 24) < point_share and n >= k_pt; from word 1 on each word w
 * proposes (uint64(w) * n) >> 32 and slot a takes the next proposal that differs from the
 * slots before it; after MP_DRAW_BLOCKS blocks the open slots take the smallest unused
 * indices in ascending order.  point_share 0 .. 256; -1: the set's solver_type decides (128
 * hybrid, 256 point solver only, 0 MD solver only).  The code is integer-only and shared by
 * host and device (mp_debug_draw_host: one sample on the host, no device; out[0] the type or
 * -1 for n < k_md, out[1 .. 8] the slots, out[9] 1 if the ascending fill was used).
 * MP_EINVAL also: budget < 0, num_sel x budget > 2^22, point_share outside -1 .. 256, null
 * outputs.
 *
 * mp_candidates_set / mp_candidates_fetch: mp_hypothesize_set's arguments and checks, but
 * only the models that exist come back, packed as mp_select_set takes them.  The number of
 * models is not known beforehand, so the result takes two calls: mp_candidates_set runs the
 * stage, keeps the result in the set and reports num_models; the caller allocates and
 * mp_candidates_fetch copies out models (num_models), model_offsets (num_sel + 1) and, per
 * model, cand_sample (its sample's index within the pair) and cand_slot, then drops the
 * result (a second fetch, or one without a result, is MP_EINVAL; a new mp_candidates_set or
 * mp_pair_set_destroy drops an unfetched one).  The kept result is read by no other call.
 * Entry j's models are those of its samples in sample order and slot order, with the bytes
 * mp_hypothesize_set gives those slots (user units).  On the device the slab's counts are
 * scanned and the models gathered, so counts, models and tags are all that is copied back.
 *
 * mp_ransac_set: draw -> hypothesize -> compact -> select -> refine on the resident pairs.
 * Either budget >= 0 with sample_offsets / sample_types / sample_idx NULL (samples drawn as
 * mp_draw_set draws them; they never reach the host), or budget -1 with the three given
 * (mp_hypothesize_set's form and checks).  rounds 0 .. 64; 0 stops after the selection.
 * Per selected pair: models[j] (user units; all zero without a winner) and results[j].
 * The call equals, byte for byte, mp_candidates_set on the samples -> mp_select_set on its
 * output -> mp_refine_set(rounds) on the winners with pair_ids = the pairs that have one:
 * best_candidate / score_selected / norm_scale are mp_select_result's best_index / best_score
 * / norm_scale; best_sample / best_slot / best_type the winner's origin (-1 without one);
 * score_initial .. num_inliers mp_refine_result's -- for a pair without a winner or with
 * rounds = 0: lm_status -1, rounds_run 0, score_initial = score_final = score_selected and
 * the selection's lists.  inlier_idx (nullable): entries past num_inliers[t] are unspecified.
 * A call leaves nothing a later call can see.  MP_EINVAL also: rounds outside 0 .. 64,
 * negative sample_chunk / model_chunk, both or neither of budget and samples, and the draw's
 * refusals. */
#define MP_DRAW_BLOCKS 16
#define MP_DRAW_POINT_SHARE_MAX 256
typedef struct mp_ransac_result {
    double score_selected, score_initial, score_final, norm_scale;
    int32_t num_samples, num_candidates;
    int32_t best_candidate, best_sample, best_slot, best_type;
    int32_t rounds_run, rounds_accepted, lm_status;
    int32_t num_inliers[3];
} mp_ransac_result; /* 80 bytes */
int mp_draw_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, uint64_t seed,
                int32_t point_share, int32_t *sample_types /* num_sel*budget */,
                int32_t *sample_idx /* num_sel*budget*8 */, int32_t *sample_counts /* num_sel */);
int mp_debug_draw_host(int variant, int64_t n, uint64_t seed, int32_t point_share, int32_t pair, int32_t s,
                       int32_t *out /* 10 */);
int mp_candidates_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *sample_offsets,
                      const int32_t *sample_types, const int32_t *sample_idx, int64_t sample_chunk,
                      int64_t *num_models);
int mp_candidates_fetch(mp_pair_set *set, mp_model *models, int64_t *model_offsets, int32_t *cand_sample,
                        int32_t *cand_slot);
int mp_ransac_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, uint64_t seed,
                  int32_t point_share, const int64_t *sample_offsets, const int32_t *sample_types,
                  const int32_t *sample_idx, int32_t rounds, mp_model *models /* num_sel */,
                  mp_ransac_result *results /* num_sel */, int32_t *inlier_idx /* nullable */, int64_t sample_chunk,
                  int64_t model_chunk);
/* mp_ransac_adaptive_set: mp_ransac_set's drawn mode with a per-pair number of samples.  Pair
 * p's samples are s = 0, 1, 2, ... as mp_draw_set defines them (seed, point_share, the pair's
 * index in the set).  They go through draw -> hypothesize -> compact -> select in rounds of
 * `step` per still-active pair; the checkpoints are m_k = min(k step, budget).  A pair's
 * running best is the strict-< walk over all its candidates so far (the device continues the
 * walk from the running best's score, so a later round replaces it only with a strictly lower
 * score).  After round k a pair stops when the estimators' termination rule holds: with c[t]
 * the three list lengths of the running best, r[t] = c[t] / n (0 for n = 0 or without a
 * winner), ss[0] = (k_md, k_md, 0), ss[1] = (0, 0, k_pt) and d[s] the number of the pair's
 * samples 0 .. m_k - 1 of type s, req[s] is: p_all = prod_t pow(r[t], ss[s][t]); p_all <= 0
 * gives max_num_iterations_per_solver, p_all >= 1 min_num_iterations; p_bad = 1 - p_all >=
 * 0.99999999999999 gives max_num_iterations_per_solver; otherwise it = ceil(log(1 -
 * success_probability) / log(p_bad) + 0.5), clamped as a double (not it <
 * max_num_iterations_per_solver gives that bound); last max(min_num_iterations, value)
 * (mp_debug_ransac_required: req[0], req[1] on the host, no device).  The pair stops if d[s] >
 * 0 and d[s] >= req[s] for s = 0 or 1 (stopped[j] = 1), or at m_k = budget (stopped[j] = 0).
 * A pair too small for the MD solver gets no samples (num_samples 0, stopped 0).
 * max_num_iterations is not read.  The pairs with a winner are refined once at the end
 * (rounds 0 .. 64).  results[j].num_samples is the pair's m, and every field of models[j],
 * results[j] and the pair's lists equals, byte for byte, mp_ransac_set(budget = m, the same
 * seed, point_share and rounds, pair_ids = that pair).  Nothing on host or device grows with
 * budget x pairs.  MP_EINVAL also: step < 1, budget < 0 or > 2^20, num_sel x min(step,
 * budget) > 2^22, rounds outside 0 .. 64, negative sample_chunk / model_chunk, point_share
 * outside -1 .. 256, and the sets mp_hypothesize_set refuses.
 * mp_debug_select_argmin (test hook): the argmin launch alone over given scores (pair k's at
 * model_offsets[k] .. model_offsets[k + 1] - 1, offsets from 0); prior NULL: the launch of
 * mp_select_set (the walk from DBL_MAX; without a winner index -1, score DBL_MAX); prior given
 * (one per pair): the walk from prior[k]; no candidate strictly below it: index -1 and score
 * prior[k]'s bits. */
int mp_ransac_adaptive_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                           uint64_t seed, int32_t point_share, int32_t rounds, mp_model *models /* num_sel */,
                           mp_ransac_result *results /* num_sel */, int32_t *inlier_idx /* nullable */,
                           int32_t *stopped /* num_sel, nullable */, int64_t sample_chunk, int64_t model_chunk);
int mp_debug_ransac_required(int variant, int64_t n, const int32_t counts[3], const mp_ransac_options *options,
                             uint32_t req[2]);
int mp_debug_select_argmin(int32_t num_pairs, const int64_t *model_offsets, const double *scores,
                           const double *prior /* nullable */, int32_t *index, double *score, int device);
/* mp_refine_relaxed_set: mp_refine_set's arguments and checks, with the estimators' first
 * local-optimisation fit (LocalOptimization's m_init) as round 0.  The first sweep forms, in
 * one pass, the tight lists err < thr and the relaxed lists err < thr * threshold_multiplier
 * (the options of the set; one double product).  Round 0's size test and its least-squares fit
 * read the relaxed lists; its candidate is accepted as any round's is (LM status 1, score
 * strictly below score_initial).  Rounds 1 onward read the accepted model's tight lists, as
 * mp_refine_set's do, and a pair stops at its first round without an accepted model.
 * score_initial, num_inliers and the returned lists are tight ones throughout.  With
 * threshold_multiplier 1 the call returns mp_refine_set's bytes.
 *
 * mp_ransac_lo_set: mp_ransac_adaptive_set with that fit inside the rounds.  A pair keeps two
 * tracks.  The minimal track -- score_selected, best_candidate / best_sample / best_slot /
 * best_type, num_samples, num_candidates -- is mp_ransac_adaptive_set's in every bit: at m
 * samples it is mp_ransac_set(budget = m, rounds = 0)'s.  The overall best starts empty.  After
 * a round in which the pair's minimal best was replaced, in this order: (1) the new minimal
 * model becomes the overall best if its score is strictly below the overall best's (lo_index
 * -1); (2) the new minimal model gets one local optimisation, mp_refine_relaxed_set with
 * lo_rounds rounds (lo_runs + 1) -- one call covers all such pairs of the round -- and its
 * result becomes the overall best if a round of it was accepted and its score_final is
 * strictly below the overall best's (lo_index = that candidate, lo_accepted + 1).  The
 * termination rule of mp_ransac_adaptive_set then reads the overall best's three counts;
 * stopping, continuing and stopped[j] are unchanged.  At the end the overall bests are refined
 * once (rounds 0 .. 64): models[j], score_initial, score_final, rounds_run, rounds_accepted,
 * lm_status, num_inliers and the lists describe that refinement; with rounds = 0 they are the
 * overall best as it stands (score_initial = score_final its score; its lists the selection's
 * if it is a minimal model, else the ones its local optimisation returned).  The running
 * bests are kept in user units.  Not done: the num_lo_steps non-minimal samples and the
 * shrinking-threshold loop of LocalOptimization; lo_starting_iterations is not read; a best
 * replaced twice within one round gets one local optimisation, at the checkpoint.  Nothing on
 * host or device grows with budget x pairs.  MP_EINVAL: mp_ransac_adaptive_set's, lo_rounds
 * outside 1 .. 64, null lo_info. */
typedef struct mp_ransac_lo_info {
    int32_t lo_runs, lo_accepted; /* local optimisations run / that became the overall best */
    int32_t lo_index;             /* the candidate whose LO gave the overall best; -1: a minimal model, or none */
    int32_t pad;
} mp_ransac_lo_info; /* 16 bytes */
int mp_refine_relaxed_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int rounds,
                          mp_model *models /* in/out, one per selected pair */, mp_refine_result *results,
                          int32_t *inlier_idx /* nullable */);
int mp_ransac_lo_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                     uint64_t seed, int32_t point_share, int32_t rounds, int32_t lo_rounds,
                     mp_model *models /* num_sel */, mp_ransac_result *results /* num_sel */,
                     int32_t *inlier_idx /* nullable */, int32_t *stopped /* num_sel, nullable */,
                     mp_ransac_lo_info *lo_info /* num_sel */, int64_t sample_chunk, int64_t model_chunk);
/* Test hook (no device): the two-track bookkeeping walked over num_rounds rounds in each of
 * which the minimal best was replaced -- its score, counts (3 per round) and candidate index,
 * and its local optimisation's rounds_accepted, score_final and counts.  score: the overall
 * best's (DBL_MAX: none); out[0 .. 2] its counts, out[3] lo_index, out[4] lo_runs, out[5]
 * lo_accepted, out[6] 0 none / 1 a minimal model / 2 a local optimisation's result. */
int mp_debug_ransac_lo_track(int32_t num_rounds, const double *min_score, const int32_t *min_counts,
                             const int32_t *candidate, const int32_t *lo_rounds_accepted, const double *lo_score,
                             const int32_t *lo_counts, double *score, int32_t *out /* 7 */);
/* mp_lsq_fit_set: one least-squares fit per entry on a random subset of the entry's inliers --
 * LeastSquaresFit (rule MP_LSQ_RULE_LSQ) or the non-minimal fit of a local-optimisation step
 * (MP_LSQ_RULE_NONMIN) of the estimators' LocalOptimization.  Entry e: models[e] (user units,
 * in and out) of pair pair_ids[e] (NULL: pair e, num_entries = the pair count) -- a pair MAY
 * occur in any number of entries; every entry has its own workspace slice and the pairs' list
 * buffers are not touched -- with solver type solver_types[e] (0 MD, 1 point), threshold factor
 * factors[e] (> 0, finite) and the subset streams streams[e] (0 .. 2^31 - 1), substreams[e]
 * (0 .. 2^30 - 1).  Per entry:
 *   1. the model goes to problem units as mp_refine_set takes it;
 *   2. one sweep: score (mp_score_models' bits), num_inliers[t] = #(err_t < thr_t) and the wide
 *      ascending lists err_t < thr_t * factor (one double product) of lengths num_wide[t] = M_t;
 *   3. the size k.  With k_md = 3 / 4 / 4, k_pt = 5 / 6 / 7 (calibrated and scale only / shared /
 *      two focal), ss = (k_md, k_md, 0) for solver type 0 and (0, 0, k_pt) for 1, mu =
 *      min_sample_multiplicator, nu = non_min_sample_multiplier and M = sum M_t --
 *      MP_LSQ_RULE_LSQ: any M_t < ss_t skips the entry, else k = mu * sum_t min(ss_t * mu, M_t);
 *      MP_LSQ_RULE_NONMIN: k = max(35 calibrated / 36 otherwise, min(k_pt * nu, M / 2)), no skip;
 *      64-bit products, clamped to M;
 *   4. the subset: every element when M <= k, else the k smallest elements (t, i) in the order
 *      (key, t, i), key = words 0 (high) and 1 of Philox4x32-10 with the counter (i, (substream
 *      << 2) | t, pair index in the set, 0x80000000 | stream) and the key (seed low, seed high);
 *      again three ascending lists, of lengths subset_sizes[t] = z_t (0 when the rule skipped);
 *   5. mp_lm_refine_batch's size test on z: (z_0 < k_md && z_1 < k_md) || z_2 < k_pt;
 *   6. either skip: status 3, the model's bytes unchanged;
 *   7. otherwise mp_lm_refine_batch's problem on the three subset lists from the model, kind 0
 *      (rule lsq) or 1 (rule nonmin), on the device LM: status 1 returns its model in user units
 *      as mp_refine_set returns them, any other status the input bytes.
 * subset_idx (nullable): mp_refine_set's inlier_idx layout over the entries (entry e's list t at
 * 3 * (n of the entries before e) + t * n_e).  Entries run in runs whose wide lists total at
 * most 2^26 ints (a run of one entry is always allowed); entry_chunk > 0 also bounds a run's
 * entries; results depend on neither, nor on the other entries.  Two synchronisations per run.
 * Variants 0 .. 3.  MP_EINVAL: null set; negative or more than 2^24 entries; rule not 0 / 1; a
 * pair id outside the set; NULL pair_ids with num_entries != the pair count; a solver type,
 * factor, stream or substream outside its range; negative entry_chunk; null arrays. */
#define MP_LSQ_RULE_LSQ 0
#define MP_LSQ_RULE_NONMIN 1
typedef struct mp_lsq_fit_result {
    double score;            /* of the input model */
    int32_t num_inliers[3];  /* its tight counts */
    int32_t num_wide[3];     /* the lengths of the wide lists */
    int32_t subset_sizes[3]; /* the lengths of the subset's lists */
    int32_t status;          /* 0 .. 3 as mp_lm_refine_batch */
} mp_lsq_fit_result; /* 48 bytes */
int mp_lsq_fit_set(mp_pair_set *set, int32_t num_entries, const int32_t *pair_ids /* nullable */,
                   const int32_t *solver_types, const double *factors, int rule, uint64_t seed,
                   const int32_t *streams, const int32_t *substreams, mp_model *models /* in/out */,
                   mp_lsq_fit_result *results, int32_t *subset_idx /* nullable */, int64_t entry_chunk);
/* Test hooks of the subset rule.  mp_debug_subset_select: the device kernel on three strictly
 * ascending lists idx[offsets[t] .. offsets[t + 1]) (offsets[0] = 0, indices below 2^28) with
 * the size k and the order (key & key_mask, t, i); the subset's list t to out_idx + offsets[t],
 * its length to out_sizes[t].  Needs no pair set.  mp_debug_subset_select_host: the same through
 * the host form of the rule (no device).  mp_debug_lsq_subset_size: the size rule of step 3 for
 * the list lengths sizes[3]; *run = 0 when the rule skips the entry (*k = 0 then). */
int mp_debug_subset_select(const int64_t offsets[4], const int32_t *idx, int64_t k, uint64_t seed, int32_t pair,
                           int32_t stream, int32_t substream, uint64_t key_mask, int32_t *out_idx,
                           int32_t out_sizes[3], int device);
int mp_debug_subset_select_host(const int64_t offsets[4], const int32_t *idx, int64_t k, uint64_t seed, int32_t pair,
                                int32_t stream, int32_t substream, uint64_t key_mask, int32_t *out_idx,
                                int32_t out_sizes[3]);
int mp_debug_lsq_subset_size(int rule, int solver_type, int variant, int32_t min_sample_multiplicator,
                             int32_t non_min_sample_multiplier, const int32_t sizes[3], int64_t *k, int32_t *run);
/* mp_ransac_lo_steps_set: mp_ransac_lo_set with the num_lo_steps steps of LocalOptimization
 * after each local optimisation.  At a checkpoint, an entry whose minimal best was replaced
 * (candidate c, solver type s) first does mp_ransac_lo_set's steps (1) and (2).  Then, with a
 * the model step (2)'s mp_refine_relaxed_set returned (the minimal model's bytes if no round
 * was accepted), Q = num_lsq_iterations (0 .. 254), lambda = threshold_multiplier and f_i =
 * lambda - i * (lambda - 1) / (Q - 1) (Q >= 2; f_0 = lambda for Q = 1), step r = 0 .. lo_steps - 1
 * runs the stages, each an mp_lsq_fit_set entry with stream = c, substream = 256 r + q:
 *   q = 0:      (a, s, factor 1, MP_LSQ_RULE_NONMIN) -> m1; a status other than 1 ends the step;
 *   q = 1:      (m1, s, factor 1, MP_LSQ_RULE_LSQ) -> m2;
 *   q = 2 + i:  (m(2+i), s, factor f_i, MP_LSQ_RULE_LSQ) -> m(3+i), i = 0 .. Q - 1; a stage whose
 *               status is not 1 passes its model on unchanged;
 *   finals:     m(2+Q) of the entry's live steps, ranked by one mp_select_set in step order.
 * All steps of all such entries go through a stage in one run: 2 + Q runs and one select per
 * checkpoint.  A stage returns the score and counts of its input, so stages 1 .. 1 + Q score
 * m1 .. m(1+Q); each is offered to the overall best (strict <), stage-major and in step order
 * inside a stage, then the select's winner among the finals.  An accepted offer sets the
 * overall best's score, model and counts, lo_index = c, lo_step = r and lo_stage = the stage
 * that produced the model (q - 1 for the model stage q scored; 2 + Q for a final).  A later
 * minimal model or local optimisation that becomes the overall best sets lo_step = lo_stage =
 * -1 again.  The rule, the end of the call and the units are mp_ransac_lo_set's; with rounds =
 * 0 the lists of an overall best that a step produced are mp_select_set's for that one model.
 * MP_EINVAL: mp_ransac_lo_set's, lo_steps outside 1 .. 64, null steps_info, num_lsq_iterations
 * outside 0 .. 254. */
typedef struct mp_ransac_lo_steps_info {
    int32_t lo_step, lo_stage;                /* the step and stage that gave the overall best; -1: none */
    int32_t lo_step_offers, lo_step_accepted; /* the steps' offers / those that became the overall best */
} mp_ransac_lo_steps_info; /* 16 bytes */
int mp_ransac_lo_steps_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                           uint64_t seed, int32_t point_share, int32_t rounds, int32_t lo_rounds, int32_t lo_steps,
                           mp_model *models /* num_sel */, mp_ransac_result *results /* num_sel */,
                           int32_t *inlier_idx /* nullable */, int32_t *stopped /* num_sel, nullable */,
                           mp_ransac_lo_info *lo_info /* num_sel */, mp_ransac_lo_steps_info *steps_info /* num_sel */,
                           int64_t sample_chunk, int64_t model_chunk);
/* Confidence-weighted sampling: mp_draw_set's and mp_ransac_*_set's samples drawn by a weight per
 * correspondence (a matcher's confidence) instead of uniformly.  Every entry here is additive; the
 * entries above and their bytes are unchanged.
 *
 * The rule, for a pair of n correspondences given weights w_i (float32 is widened exactly):
 * valid weights are finite and 0 <= w_i <= 1; q_i = min(65535, floor(w_i * 65536)) as uint32 (a
 * product with a power of two: exact); q_i = 0 masks correspondence i; c[0] = 0, c[i + 1] = c[i] +
 * q_i in uint32, W = c[n]; n <= MP_DRAW_WEIGHT_MAX_N, so W < 2^32.  With k_max = k_pt if n >= k_pt
 * else k_md, the pair is weighted iff #{q_i > 0} >= k_max; a pair given weights with fewer draws by
 * mp_draw_set's uniform rule and is reported as not weighted.  For a weighted pair the type comes
 * from word 0 as before; from word 1 on each word w proposes t = (uint64(w) * W) >> 32 and then the
 * unique i with c[i] <= t < c[i + 1]; slot a takes the next proposal that differs from the slots
 * before it; after MP_DRAW_BLOCKS blocks the open slots take the smallest unused indices with q_i >
 * 0 in ascending order.  Counter, key and block order are mp_draw_set's, and the pair is still the
 * pair's index in the set.  Integer-only, one function for host and device.  If all q_i are equal
 * and positive the proposals are mp_draw_set's, so equal weights reproduce the uniform draw byte
 * for byte.  The termination rule of the adaptive modes is unchanged: it reads the count ratios of
 * the best model's lists, which under informative weights is conservative (it never stops earlier
 * than it does without weights).
 *
 * mp_draw_weights_create: the tables of one set, built by one device launch.  weights: one value
 * per correspondence of the set, concatenated in set order (dtype 0 float32, 1 float64), on the
 * host (on_device 0) or on the set's device (on_device 1: checked as mp_pair_set_create_device
 * checks its arrays; the build is ordered after producer_stream, a hipStream_t or NULL for the null
 * stream, by an event, and the array is not read after the call returns).  given (nullable: every
 * pair): num_pairs bytes, 0 = this pair draws uniformly and its rows of `weights` are ignored.
 * MP_EINVAL: a null set or output, a dtype outside {0, 1}, a weight that is NaN, infinite, negative
 * or above 1 (the message names the lowest such row of the set), a pair of more than
 * MP_DRAW_WEIGHT_MAX_N correspondences given weights (pass given = 0 for it), and the sets
 * mp_hypothesize_set refuses.  The handle belongs to its set, is immutable and lives outside the
 * set: any number of calls may share it and a call still leaves nothing in the set that a later
 * call can see.  mp_draw_weights_info: per pair, whether it is weighted (0 / 1), #{q_i > 0} and W
 * (0 for the pairs not given weights); each output nullable.  mp_pair_set_destroy invalidates the
 * set's handles (their device memory goes with the set): every later use of one is MP_EINVAL, and
 * mp_draw_weights_destroy on it is still MP_OK.  mp_draw_weights_destroy(NULL) is MP_OK.
 *
 * mp_draw_weighted_set: mp_draw_set with the handle.  mp_ransac_weighted_set: one entry over
 * mp_ransac_set's drawn mode (step 0; lo_rounds and lo_steps must be 0), mp_ransac_adaptive_set
 * (step >= 1, lo_rounds 0), mp_ransac_lo_set (lo_rounds >= 1, lo_steps 0) and
 * mp_ransac_lo_steps_set (lo_steps >= 1); stopped, lo_info and steps_info as the entry chosen
 * takes them (unused ones may be NULL).  Each runs that entry's own checks and returns its
 * MP_EINVALs, and its documented identities hold with the weighted draw in place of the uniform
 * one.  MP_EINVAL also: a NULL handle, one of another set, one whose set was destroyed.
 *
 * mp_debug_draw_weights_host (no device): the table cum[0 .. n] and #{q_i > 0} of n weights, n <=
 * MP_DRAW_WEIGHT_MAX_N.  mp_debug_draw_weighted_host (no device): one sample of a weighted pair
 * from its table (MP_EINVAL if the table does not rise by 0 .. 65535 per entry from 0 or has fewer
 * than k_max rises); out as mp_debug_draw_host's.  MP_DRAW_STAGE_ENTRIES: the device sampler reads
 * a table of at most that many entries (n + 1) through LDS, larger ones from global memory. */
#define MP_DRAW_WEIGHT_MAX_N 65535
#define MP_DRAW_STAGE_ENTRIES 4096
typedef struct mp_draw_weights mp_draw_weights;
int mp_draw_weights_create(mp_pair_set *set, const void *weights, int32_t dtype, int32_t on_device,
                           const uint8_t *given /* num_pairs, nullable */, void *producer_stream,
                           mp_draw_weights **out);
int mp_draw_weights_info(const mp_draw_weights *handle, int32_t *weighted /* num_pairs, nullable */,
                         int32_t *positive /* num_pairs, nullable */, uint32_t *total /* num_pairs, nullable */);
int mp_draw_weights_destroy(mp_draw_weights *handle);
int mp_draw_weighted_set(mp_pair_set *set, const mp_draw_weights *handle, int32_t num_sel, const int32_t *pair_ids,
                         int32_t budget, uint64_t seed, int32_t point_share, int32_t *sample_types,
                         int32_t *sample_idx, int32_t *sample_counts);
int mp_ransac_weighted_set(mp_pair_set *set, const mp_draw_weights *handle, int32_t num_sel, const int32_t *pair_ids,
                           int32_t budget, int32_t step /* 0: fixed budget */, uint64_t seed, int32_t point_share,
                           int32_t rounds, int32_t lo_rounds /* 0: none */, int32_t lo_steps /* 0: none */,
                           mp_model *models /* num_sel */, mp_ransac_result *results /* num_sel */,
                           int32_t *inlier_idx /* nullable */, int32_t *stopped /* num_sel, nullable */,
                           mp_ransac_lo_info *lo_info, mp_ransac_lo_steps_info *steps_info, int64_t sample_chunk,
                           int64_t model_chunk);
int mp_debug_draw_weights_host(int64_t n, const void *weights, int32_t dtype, uint32_t *cum /* n + 1 */,
                               int32_t *positive);
int mp_debug_draw_weighted_host(int variant, int64_t n, const uint32_t *cum /* n + 1 */, uint64_t seed,
                                int32_t point_share, int32_t pair, int32_t s, int32_t *out /* 10 */);
/* The weighted stopping rule: the adaptive modes stop a weighted pair on the weight mass of its
 * best model's inlier lists instead of their count ratios.  Every entry here is additive; the
 * entries above, mp_ransac_weighted_set included, and their bytes are unchanged.
 *
 * The rule, for pair p of n correspondences and a handle: q_i = c[i + 1] - c[i] from the handle's
 * table of that pair and W = c[n] < 2^32.  For a model m of the pair, L_t(m), t = 0..2, are the
 * three inlier lists mp_select_set returns for the single candidate m (err_t < thr_t on the
 * ungated errors).  If the handle reports the pair as weighted: mass[t] = sum of q_i over L_t as
 * uint32 (distinct rows, so mass[t] <= W) and total = W.  If not (it was given no weights, or it
 * fell back to the uniform draw): mass[t] = |L_t| and total = n.  count[t] = |L_t| in both cases.
 * The weighted rule is the termination rule above with r[t] = (double)mass[t] / (double)total, and
 * 0 when total = 0 or there is no winner; the exponents, the three bounds, ceil(log(1 - sp) /
 * log(p_bad) + 0.5), the clamp in double, max(min_num_iterations, .) and the stop test are
 * unchanged (mp_debug_ransac_required_mass: req[0], req[1] on the host, no device; mass NULL: no
 * winner; MP_EINVAL for a mass above total).  Consequences: a pair that is not weighted gets
 * mass / total = c / n, the count rule's bits; if all q_i = q > 0, (q c) / (q n) and c / n are
 * correctly rounded quotients of one rational with operands exact in double, the same bits, so
 * equal weights reproduce the count rule's stop points and, with the identity above, the
 * unweighted call byte for byte.  There is NO promise of "never later": a list made mostly of
 * low-confidence rows has a mass ratio below its count ratio.  Sampling without replacement and
 * the fill are ignored, as the count rule ignores them.
 *
 * mp_inlier_mass_set: one record per entry e = (pair pair_ids[e] (NULL: e), models[e] in user
 * units) from one launch of one workgroup per entry: integer sums only, so the record does not
 * depend on the reduction order.  A pair may occur in any number of entries (no list buffer of
 * the set is written); at most 2^24 entries; a call leaves nothing a later call can see.
 * MP_EINVAL: a null set, a handle that is NULL, of another set or whose set was destroyed, a
 * negative or too large num_entries, a pair outside the set, num_entries above num_pairs with
 * pair_ids NULL.  A model with a NaN entry has empty lists (mass and count 0).
 *
 * mp_ransac_weighted_stop_set: mp_ransac_weighted_set with the weighted rule.  It needs step >= 1
 * (MP_EINVAL) and a live handle of this set; otherwise it runs the chosen body's own checks and
 * returns that body's own MP_EINVALs.  At every checkpoint, after the tracks are updated and
 * before the rule is read, ONE launch computes the records of the still-active entries of weighted
 * pairs whose rule model -- the minimal best with lo_rounds 0, the overall best at the
 * checkpoint's end otherwise -- was replaced during that checkpoint.  Its counts must equal the
 * track's: a mismatch is an internal error (MP_EDEVICE, the message names the pair), never a silent stop or
 * continuation.
 * Entries of pairs that are not weighted read their counts.  rule_mass[j] (nullable): what the
 * rule last read for entry j, all zero with total = W or n when the entry never had a winner.
 * Unchanged: stopped, num_samples, the minimal track, the final rounds, the units, pair_ids
 * subsets (the table goes by the pair's index in the set), sample_chunk / model_chunk, and the
 * bound that nothing grows with budget x pairs.  Entry j still equals, byte for byte, the
 * fixed-budget identity of the body chosen at budget = results[j].num_samples.
 *
 * mp_debug_inlier_mass_host (no device): mass[0 .. 2] of three strictly ascending lists
 * idx[offsets[t] .. offsets[t + 1]) (offsets[0] = 0, indices in 0 .. n - 1) under the table
 * cum[0 .. n], n <= MP_DRAW_WEIGHT_MAX_N.  mp_debug_inlier_mass_stats: the launches of the mass
 * stage since the last reset and their summed host milliseconds, upload to synchronise (each
 * output nullable; reset != 0 clears both after reading). */
typedef struct mp_inlier_mass {
    uint32_t mass[3], total;
    int32_t count[3], weighted;
} mp_inlier_mass; /* 32 bytes */
int mp_inlier_mass_set(mp_pair_set *set, const mp_draw_weights *handle, int32_t num_entries,
                       const int32_t *pair_ids /* nullable: pair e */, const mp_model *models /* num_entries */,
                       mp_inlier_mass *out /* num_entries */);
int mp_ransac_weighted_stop_set(mp_pair_set *set, const mp_draw_weights *handle, int32_t num_sel,
                                const int32_t *pair_ids, int32_t budget, int32_t step /* >= 1 */, uint64_t seed,
                                int32_t point_share, int32_t rounds, int32_t lo_rounds /* 0: none */,
                                int32_t lo_steps /* 0: none */, mp_model *models /* num_sel */,
                                mp_ransac_result *results /* num_sel */, int32_t *inlier_idx /* nullable */,
                                int32_t *stopped /* num_sel, nullable */, mp_ransac_lo_info *lo_info,
                                mp_ransac_lo_steps_info *steps_info, int64_t sample_chunk, int64_t model_chunk,
                                mp_inlier_mass *rule_mass /* num_sel, nullable */);
int mp_debug_ransac_required_mass(int variant, uint32_t total, const uint32_t mass[3] /* nullable: no winner */,
                                  const mp_ransac_options *options, uint32_t req[2]);
int mp_debug_inlier_mass_host(int64_t n, const uint32_t *cum /* n + 1 */, const int64_t offsets[4],
                              const int32_t *idx, uint32_t mass[3]);
int mp_debug_inlier_mass_stats(int64_t *launches /* nullable */, double *ms /* nullable */, int32_t reset);
/* Per-correspondence errors and inlier masks: what a model does to every correspondence of a
 * resident pair.  The entry is additive; the entries above and their bytes are unchanged.
 *
 * mp_residuals_set: entry e = (pair pair_ids[e] (NULL: e), models[e] in user units, converted as
 * every set stage converts them, factors[e] (NULL: 1.0)).  A pair may occur in any number of
 * entries; at most 2^24 entries.  row_offsets[e] = the correspondences of the entries before e
 * and R = row_offsets[num_entries]; entry e owns rows row_offsets[e] .. row_offsets[e + 1] - 1 of
 * the outputs.  For row i of entry e, with err_t (t = 0: depth-aware reprojection 0 -> 1, 1: the
 * same 1 -> 0, 2: Sampson) the squared errors every stage compares with the thresholds -- ungated:
 * no score type replaces a term -- and thr_t the pair's thresholds:
 *   mask[row_offsets[e] + i]: bit t set iff err_t < thr_t * factors[e], the product formed once in
 *     double as mp_refine_relaxed_set and mp_lsq_fit_set form theirs (factor 1.0: thr_t itself);
 *     bits 3 .. 7 zero; a NaN error is not an inlier, so a model with a NaN entry has mask 0;
 *   errors[t * R + row_offsets[e] + i] = err_t (errors nullable; term-major (3, R) float64);
 *   counts[3 e + t] = the rows of entry e with bit t set.
 * With factor 1.0, bit t of row i is set iff i is in list t of mp_select_set for that single
 * candidate, and counts are the list lengths.  The errors are in problem units: for the focal
 * variants these are coordinates divided by the pair's normalization scale s
 * (mp_pair_set_norm_scales), so s * s * err_t is in squared pixels; the library does not multiply.
 * The MSAC score is not returned (mp_select_set returns it).  The call does not hypothesize, so
 * every variant 0 .. 3 and every use_shift / MD solver setting is supported.
 *
 * Outputs: on_device 0 -- host arrays, filled through a device scratch in runs whose size does
 * not grow with R.  on_device 1 -- memory of the set's device, checked before any launch as
 * mp_pair_set_create_device checks its arrays (device memory of that device, errors aligned to 8
 * bytes, the bytes inside the allocation's address range) and that the two ranges do not
 * overlap; the kernel writes into it directly (no staging copy) and only into those R bytes and
 * 3 R doubles.  The library's stream waits for an event recorded on producer_stream (a
 * hipStream_t; NULL: the null stream) before its first write; the host does not wait for that
 * stream.  The call returns after the library's own stream is synchronised.  It leaves nothing in
 * the set that a later call can see.
 * MP_EINVAL, before the device is touched: a NULL set, out, mask, row_offsets or counts; NULL
 * models with num_entries > 0; num_entries negative or above 2^24; a pair outside the set;
 * pair_ids NULL with num_entries != num_pairs; a factor that is not finite and > 0.
 * mp_debug_residuals_stats: the stage's kernel launches since the last reset and, measured while
 * profiling is enabled (mp_profile_enable), their summed device milliseconds. */
typedef struct mp_residuals_out {
    void *mask;            /* uint8, R bytes */
    void *errors;          /* nullable; float64, 3 * R, term-major */
    int32_t on_device;     /* 0: host arrays; 1: device memory of the set's device */
    int32_t pad;
    void *producer_stream; /* on_device only; NULL: the null stream */
} mp_residuals_out;
int mp_residuals_set(mp_pair_set *set, int32_t num_entries, const int32_t *pair_ids /* nullable: pair e */,
                     const mp_model *models /* user units */, const double *factors /* nullable: 1.0 */,
                     const mp_residuals_out *out, int64_t *row_offsets /* num_entries + 1 */,
                     int32_t *counts /* 3 * num_entries */);
int mp_debug_residuals_stats(int64_t *launches /* nullable */, double *ms /* nullable */, int32_t reset);
/* Per-entry information and covariance: how well a pair's correspondences determine a model.
 * The entry is additive; the entries above and their bytes are unchanged.
 *
 * mp_information_set: entries, pair_ids, models and factors as mp_residuals_set takes them (a pair
 * may occur in any number of entries; at most 2^24 entries; every variant 0 .. 3).  For entry e
 * (model m on pair p), m goes to problem units as every set stage converts it.  Row i of the pair
 * is a residual block of type t (0: depth-aware reprojection 0 -> 1, two residuals; 1: the same
 * 1 -> 0, two residuals; 2: Sampson, one residual) iff bit t of mp_residuals_set's mask is set for
 * it under factors[e].  The LO type gates block types as in the local optimisation (LO_type 1: no
 * reprojection blocks, 2: no Sampson blocks), and use_shift, the scale-only rule and the Sampson
 * weight are those of the job mp_refine_set would run on these lists.  With J the Jacobian of the
 * remaining residuals r at m over the 11 parameters (rotation tangent 3, t 3, scale, offset0,
 * offset1, focal0, focal1 -- the layout of mp_debug_lm_system), row e of the outputs is
 *   H[66 e ..]    the packed upper triangle of J^T J, (a, b), a <= b, at 11 a - a (a - 1) / 2 + b - a;
 *   g[11 e ..]    J^T r;
 *   cost[e]       sum r^2 / 2;
 *   cov[121 e ..] the inverse of H on the active parameters, row-major 11 x 11, zero on the rows
 *                 and columns of inactive ones: with D_a = 1 / sqrt(H_aa), A = D H D is factored
 *                 once by Cholesky and column k is D (A^-1 e_k) D_k from the two triangular solves;
 * each array nullable (cov NULL skips the inverse's stores), and entries[e] (always host memory):
 *   col[a]     1: parameter a is active (6 pose parameters whenever a block exists; scale with a
 *              block of type 1; offset0 / offset1 with a block of type 0 / 1 and use_shift; the
 *              focals the variant has);
 *   status     1: at least one block after gating, else 0;
 *   pd         1: the factorisation completed; 0: an active H_aa or a pivot was not positive and
 *              finite (cov is all zero); -1: status 0 (H, g, cost, cov and col are all zero);
 *   rows       2 (n0 + n1) + n2 over the gated block counts;
 *   counts[t]  the rows with bit t set, before gating: mp_residuals_set's counts.
 * Every entry of g and H that belongs to an inactive parameter is exactly 0.0.  A model with a NaN
 * entry has no blocks.  pd = 1 says only that the factorisation completed: it does not detect an
 * ill-conditioned system (with Sampson blocks alone |t| is a gauge and its pivot is rounding
 * noise); gauges are not handled here.
 *
 * Units: everything is in problem units, like mp_residuals_set's errors.  Residuals are pixels
 * for variants 0 and 3 and pixels / s for the focal variants, s the pair's normalization scale
 * (mp_pair_set_norm_scales); a focal parameter is the user's focal / s.  So cov is the covariance
 * under unit-variance residuals in those units; for a focal's row and column multiply by s per
 * index (cov[f][f] by s * s), and the a-posteriori variance factor is 2 cost / (rows - n), n the
 * number of active parameters.  The library does not multiply.
 *
 * Outputs: on_device 0 -- host arrays, filled through a device scratch in runs of bounded size.
 * on_device 1 -- memory of the set's device, checked before any launch as mp_residuals_set checks
 * its outputs (device memory of that device, aligned to 8 bytes, the bytes inside the allocation's
 * address range, the given ranges pairwise disjoint); the finishing kernel writes row e of each
 * directly and nothing else.  producer_stream and the return are mp_residuals_set's.  A result
 * depends on its entry alone: not on the other entries, the runs, or the output kind.  The call
 * leaves nothing in the set that a later call can see.
 * MP_EINVAL, before the device is touched: a NULL set, out or entries (num_entries > 0); NULL
 * models with num_entries > 0; num_entries negative or above 2^24; a pair outside the set;
 * pair_ids NULL with num_entries != num_pairs; a factor that is not finite and > 0; device outputs
 * that overlap.
 * mp_debug_information_finish: the finishing arithmetic alone, on the host (no device): H and g
 * are masked in place by col (exact zeros on inactive entries), cov = the inverse as above, *pd 1
 * or 0.  mp_debug_information_stats: the stage's runs since the last reset and, measured while
 * profiling is enabled, the summed device milliseconds of its two kernels. */
typedef struct mp_information_out {
    void *H;               /* nullable; float64, 66 per entry */
    void *g;               /* nullable; float64, 11 per entry */
    void *cost;            /* nullable; float64, 1 per entry */
    void *cov;             /* nullable; float64, 121 per entry */
    int32_t on_device;     /* 0: host arrays; 1: device memory of the set's device */
    int32_t pad;
    void *producer_stream; /* on_device only; NULL: the null stream */
} mp_information_out;
typedef struct mp_information_entry {
    int32_t col[11];
    int32_t pd, status, rows;
    int32_t counts[3];
} mp_information_entry;
int mp_information_set(mp_pair_set *set, int32_t num_entries, const int32_t *pair_ids /* nullable: pair e */,
                       const mp_model *models /* user units */, const double *factors /* nullable: 1.0 */,
                       const mp_information_out *out, mp_information_entry *entries /* num_entries */);
int mp_debug_information_finish(double H[66], double g[11], const int32_t col[11], double cov[121], int32_t *pd);
int mp_debug_information_stats(int64_t *launches /* nullable */, double *rows_ms /* nullable */,
                               double *finish_ms /* nullable */, int32_t reset);
/* RANSAC results into the caller's device arrays.  The entry is additive; the six ransac entries
 * above and their bytes are unchanged.
 *
 * mp_ransac_out_set takes the union of their arguments and runs the body they choose: handle
 * (nullable: the uniform draw); step 0: mp_ransac_set's fixed budget, its samples drawn (budget >=
 * 0, sample_* NULL) or given (budget -1); step >= 1: the adaptive rounds, with lo_rounds (0: none)
 * and lo_steps (0: none; needs lo_rounds) as mp_ransac_lo_set / mp_ransac_lo_steps_set take them;
 * weighted_stop != 0: mp_ransac_weighted_stop_set's rule (needs handle and step >= 1).  stopped,
 * lo_info, steps_info and rule_mass are the chosen body's (lo_info is needed with lo_rounds,
 * steps_info with lo_steps; the others are nullable).  models and results are what that body
 * returns, byte for byte.  inlier_idx is nullable: NULL copies no index list back from the device.
 * Where a refinement follows (rounds >= 1) the selection's lists are not copied back at all, as
 * every winner's lists are written again by the refinement.
 *
 * out (nullable; each of its five arrays nullable): memory of the set's device.  With ns = num_sel
 * and offs[j] the correspondences of the selected pairs before entry j, R = offs[ns]:
 *   models[17 j ..]: the bytes of models[j];  index[j] = results[j].best_candidate;
 *   counts[3 j + t] = results[j].num_inliers[t];
 *   mask[offs[j] + i]: bit t set iff i is in the returned list t of entry j; bits 3 .. 7 zero;
 *   errors[t R + offs[j] + i]: the squared error err_t of row i, in problem units (see
 *     mp_residuals_set), under the model the returned lists were formed from, kept in problem
 *     units by the library -- so (errors[t R + row] < thr_t) == bit t of mask[row] on every row, in
 *     every variant and after any number of rounds, which mp_residuals_set on the returned model
 *     cannot promise for a refined focal model (it divides the returned focal by the
 *     normalization scale again).  errors needs mask.
 * For an entry without a winner (best_candidate -1), or without a correspondence: mask rows 0,
 * error rows NaN, models row zeros, index -1, counts 0.  Every element of every given array that
 * belongs to the selection is written exactly once per call, by a kernel (no copy into and no
 * memset on the caller's memory), and nothing outside it.  Before any launch each array is checked
 * as mp_residuals_set checks its device outputs (device memory of the set's device; errors and
 * models aligned to 8 bytes, index and counts to 4; the bytes inside the allocation's address
 * range, the byte counts overflow-checked) and the five ranges must be pairwise disjoint.  The
 * library's stream waits for an event recorded on producer_stream (NULL: the null stream) before
 * its first write; the host does not wait for that stream.  The call returns after the library's
 * own stream is synchronised.  The output stage sums its per-item counts per pair and compares
 * them with num_inliers: a difference is an internal error (MP_EDEVICE).
 * MP_EINVAL, before the device is touched: a NULL set; errors without mask; any output array
 * together with lo_rounds >= 1 and rounds = 0 -- without final rounds the overall best's lists may
 * be those a local optimisation returned, and its model in problem units is not kept --; negative
 * step, lo_rounds or lo_steps; lo_rounds or lo_steps with step 0; lo_steps without lo_rounds;
 * weighted_stop without handle or step; given samples with step >= 1 or with handle; and the
 * chosen body's own refusals.
 * mp_debug_ransac_out_stats: the output stage's row launches since the last reset and, measured
 * while profiling is enabled (mp_profile_enable), their summed device milliseconds. */
typedef struct mp_ransac_out {
    void *mask;            /* nullable; uint8, R bytes */
    void *errors;          /* nullable; float64, 3 * R, term-major; needs mask */
    void *models;          /* nullable; float64, 17 * num_sel */
    void *index;           /* nullable; int32, num_sel */
    void *counts;          /* nullable; int32, 3 * num_sel */
    void *producer_stream; /* NULL: the null stream */
} mp_ransac_out; /* 48 bytes */
int mp_ransac_out_set(mp_pair_set *set, const mp_draw_weights *handle /* nullable */, int32_t num_sel,
                      const int32_t *pair_ids, int32_t budget, int32_t step /* 0: a fixed budget */, uint64_t seed,
                      int32_t point_share, const int64_t *sample_offsets /* nullable */,
                      const int32_t *sample_types /* nullable */, const int32_t *sample_idx /* nullable */,
                      int32_t rounds, int32_t lo_rounds /* 0: none */, int32_t lo_steps /* 0: none */,
                      int32_t weighted_stop, mp_model *models /* num_sel */, mp_ransac_result *results /* num_sel */,
                      int32_t *inlier_idx /* nullable: no lists */, int32_t *stopped /* num_sel, nullable */,
                      mp_ransac_lo_info *lo_info, mp_ransac_lo_steps_info *steps_info, int64_t sample_chunk,
                      int64_t model_chunk, mp_inlier_mass *rule_mass /* num_sel, nullable */,
                      const mp_ransac_out *out /* nullable */);
int mp_debug_ransac_out_stats(int64_t *launches /* nullable */, double *ms /* nullable */, int32_t reset);
/* Measurement hook (tools/ransac_set_bench.py): the last mp_ransac_set made while profiling
 * was enabled (mp_profile_enable), every stage waited for -- ms: the call, its hypothesis /
 * select / refine stages; of the hypothesis stage: host planning, the sampler, uploads, the
 * solve launches, scan + gather, copies back; of the selection: record preparation, upload,
 * scoring, argmin, winners' sweep; then the bytes the hypothesis stage copied back and the
 * bytes of the slot array and counts it replaces; last, ms again, the host work on the samples
 * before the stages (inside the call's time): the check of given samples, or the types of
 * the drawn ones. */
#define MP_RANSAC_TIMING_VALUES 18
int mp_debug_ransac_timing(double *out /* MP_RANSAC_TIMING_VALUES */);

/* Test and measurement hooks.  mp_debug_pair_set_prep: how the pair setups that follow (of
 * sets and of the batch entries; process-wide) derive the calibrated rows -- 0: one launch
 * over all pairs, 1: one launch per pair, the form before; the rows are equal bit for bit.
 * MP_EINVAL for another mode.  mp_debug_pair_set_rows: the twelve device rows of one pair
 * (x0u x0v x1u x1v d0 d1 r0 r1 a0 a1 b0 b1, n doubles each; rows 6 .. 11 are written for
 * calibrated and scale-only sets only). */
int mp_debug_pair_set_prep(int mode);
int mp_debug_pair_set_rows(const mp_pair_set *set, int32_t pair, double *out /* 12 n */);
/* mp_debug_pair_set_record: the data-dependent fields of one pair's device record (copied back
 * from the device) -- [0..2] thr, [3..5] w, [6] loss_scale, [7] tie_scale, [8] the
 * normalization scale, [9..19] ea eap exi eb ebp exj ed0 ed1 ex0 ex1 eab2, then the margin
 * constants [20..21] s2, [22..23] U, [24..25] c0, [26..27] c1, [28] tau2, [29] fixed.
 * mp_debug_ingest_info: the trip lengths of mp_pair_set_create_device's kernels -- the
 * workgroup size, the chunk length of the staged sum of the normalization scale, the
 * correspondences of one work item.  mp_debug_device_extent: base address and size of the
 * allocation of `device` that holds ptr, as the device pointers' range check sees it. */
#define MP_PAIR_RECORD_VALUES 30
#define MP_INGEST_INFO_VALUES 3
int mp_debug_pair_set_record(const mp_pair_set *set, int32_t pair, double *out /* MP_PAIR_RECORD_VALUES */);
int mp_debug_ingest_info(int32_t *out /* MP_INGEST_INFO_VALUES */);
int mp_debug_device_extent(const void *ptr, int device, int64_t *out /* 2 */);

/* bougnoux_focals (src/hybrid_pose_two_focal_estimator.cpp:11-32; numpy twin
 * madpose/utils.py:25-56 bougnoux_numpy with p1 = p2 = 0): squared focal lengths
 * (f0^2, f1^2) of k fundamental matrices F (k x 9, row-major) into out (k x 2), on
 * the device with the same code the two-focal 7-point tail runs. */
int mp_bougnoux_focals(int64_t k, const double *F, double *out, int device);

/* compute_pose_error (madpose/utils.py:59-78) of k estimated poses against their
 * ground truth on the device, and the pose AUC of the evaluation the reference's
 * README reports (ScanNet-1500 AUC@5/10/20, README.md:18-181):
 * R: k x 9 row-major, t: k x 3, T_0to1: k x 16 (row-major 4x4); t_thres < 0 means
 * none (else err_t = 0 where |t_gt| < t_thres).  err_t, err_R: k degrees each.  When
 * nthr > 0, aucs[b] = area under the recall curve of max(err_R, err_t) up to
 * thresholds[b], divided by it (trapezoid rule, NaN errors sorted last; the
 * SuperGlue-style pose_auc of madpose_amd/utils.py); k = 0 gives NaN. */
int mp_pose_eval(int64_t k, const double *R, const double *t, const double *T_0to1, double t_thres, double *err_t,
                 double *err_R, int32_t nthr, const double *thresholds, double *aucs, int device);
/* The same pose AUC over k given errors (degrees; e.g. max(err_R, err_t) gathered
 * from many ranks): aucs[b] for thresholds[b], b < nthr. */
int mp_pose_auc(int64_t k, const double *errors, int32_t nthr, const double *thresholds, double *aucs, int device);

/* Point minimal solver (PoseLib relpose_5pt, src/hybrid_pose_estimator.cpp:134) on unit bearings
 * (5 points, point-major 3 doubles each).  Returns count or -code. */
int mp_relpose_5pt(const double *x1, const double *x2, mp_model *out, int max_out, int device);
/* mp_debug_pt5_roots: the engine's batched root stage of the calibrated 5-point
 * solver (the part of PoseLib relpose_5pt before pose recovery) over ns samples of
 * five normalized image points (pts0, pts1: ns x 5 x 2, identity intrinsics).
 * impl must be 1 (one 16-lane group per sample, the estimator's stage).  cand: ns x 96
 * doubles, 9 per essential matrix (ascending roots); ncand: ns counts.  Test hook. */
int mp_debug_pt5_roots(int impl, int64_t ns, const double *pts0, const double *pts1, double *cand, int32_t *ncand,
                       int device);
/* mp_debug_pt_roots: the same for variant 0 (calibrated 5-point, impl 1, as above) or
 * 1 (shared-focal 6-point, impl 3: the root stage of PoseLib relpose_6pt_shared_focal
 * as called at src/hybrid_pose_shared_focal_estimator.cpp:87, by the deflated
 * eigenproblem the estimator runs; pts0/pts1: ns x 6 x 2 normalized points; cand per
 * sample: the 3x9 epipolar null-space basis N, then the positive roots u = f^2 of the
 * degree-15 focal polynomial, ascending), or 2 (two-focal 7-point, impl 1: the root stage of
 * PoseLib relpose_7pt as called at src/hybrid_pose_two_focal_estimator.cpp:116; pts0/pts1: ns x 7
 * x 2 normalized points; cand per sample: the unit-norm fundamental matrices, 9 doubles each,
 * in root order).  Other impl values return MP_EINVAL.  Test hook. */
int mp_debug_pt_roots(int variant, int impl, int64_t ns, const double *pts0, const double *pts1, double *cand,
                      int32_t *ncand, int device);

/* Point minimal solvers of the uncalibrated estimators on 2-D points in the
 * estimators' normalized pixel frame ((x - pp) / s, point-major, 2 doubles each),
 * bearings formed as at src/hybrid_pose_shared_focal_estimator.cpp:79-84:
 *   6pt: PoseLib relpose_6pt_shared_focal (:87); out.focal0 = out.focal1 = f.
 *   7pt: PoseLib relpose_7pt + bougnoux_focals + cv::recoverPose
 *        (src/hybrid_pose_two_focal_estimator.cpp:116-146); out.focal0/1 = f0/f1.
 * Models are returned before the depth fit (scale 1, offsets 0).  Returns count or -code. */
int mp_relpose_6pt_shared_focal(const double *x0, const double *x1, mp_model *out, int max_out, int device);
int mp_relpose_7pt_two_focal(const double *x0, const double *x1, mp_model *out, int max_out, int device);

/* The standalone solvers over ns samples per call.  Inputs are sample-major and inside
 * a sample exactly the single-sample layout: x_homo / y_homo ns x K x 3 (K = 3
 * calibrated, 4 otherwise), depths ns x K; mp_relpose_batch kind 0 (5pt): unit bearings
 * ns x 5 x 3, kind 1 / 2 (6pt shared focal / 7pt two focal): normalized 2-D points ns x 6
 * x 2 / ns x 7 x 2.  Outputs: mp_solve_scale_and_shift_batch ns x 8 rows of width 4 / 5 /
 * 6, mp_solve_scale_shift_pose_batch ns x 8 models (alt 0: the default solvers, 1 / 2 as
 * mp_solve_scale_shift_pose_alt), mp_relpose_batch ns x 16 models, within a sample in the
 * single-sample entry's order; counts[s] = that entry's return value for sample s (at
 * most the slot count), the slots from counts[s] on are zero.  Every row equals the
 * single-sample entry's result bit for bit.  The batch runs in rounds of `chunk` samples
 * on one set of device buffers (chunk bounds their size; 0 = MP_SOLVE_BATCH_CHUNK).
 * ns == 0 returns MP_OK without touching the device; ns < 0 or ns > 2^22, null pointers,
 * a bad variant / alt / kind or chunk < 0 give MP_EINVAL.  Returns MP_OK or a code. */
#define MP_SOLVE_BATCH_CHUNK 32768
int mp_solve_scale_and_shift_batch(int variant, int64_t ns, const double *x_homo, const double *y_homo,
                                   const double *depth_x, const double *depth_y, double *out, int32_t *counts,
                                   int64_t chunk, int device);
int mp_solve_scale_shift_pose_batch(int variant, int alt, int64_t ns, const double *x_homo, const double *y_homo,
                                    const double *depth_x, const double *depth_y, mp_model *out, int32_t *counts,
                                    int64_t chunk, int device);
int mp_relpose_batch(int kind, int64_t ns, const double *x0, const double *x1, mp_model *out, int32_t *counts,
                     int64_t chunk, int device);

/* Test hooks for the host-side random streams (no device needed).
 * mp_debug_random_stream: kind 0 raw mt19937 words, 1 uniform_int(a, b),
 * 2 uniform_real(0, b), 3 uniform_int(i % 300, 300 + i % 17) for i = 0..count-1.
 * mp_debug_iteration_stream: the solver-type / minimal-sample sequence the engine
 * replays (SelectMinimalSolver + HybridUniformSampling, src/hybrid_ransac.h:64,
 * 98-109); idx holds 8 slots per iteration (unused slots -1). */
int mp_debug_random_stream(int kind, uint32_t seed, int32_t a, int32_t b, int32_t count, double *out);
int mp_debug_iteration_stream(int variant, int32_t n, uint32_t seed, int32_t solver_type, int32_t iterations,
                              int32_t *types, int32_t *idx);

/* Device timing of the estimator's batch kernels (engine-internal; no reference
 * counterpart).  Durations come from HIP events recorded on the engine's stream
 * around each launch and are process-wide totals since the last reset. */
typedef struct mp_kernel_profile {
    uint64_t batches;         /* speculative batches timed                  */
    uint64_t iterations;      /* minimal samples solved                     */
    uint64_t hypotheses;      /* models scored by the score_batch kernel    */
    uint64_t correspondences; /* sum of hypotheses x n over timed batches   */
    uint64_t sweeps;          /* single-model LO / termination sweeps       */
    double solve_ms;          /* md_solve + pt_solve kernels                */
    double score_ms;          /* score_batch kernel                         */
    uint64_t lm_calls;        /* host LM solves inside LO                   */
    double lm_wall_ms;        /* host wall time spent in the LM             */
    double sweep_wall_ms;     /* host wall time of LO sweeps (incl. copies) */
    double sample_wall_ms;    /* host minimal-sample generation + rewinds   */
    double wait_wall_ms;      /* host wait for speculative batch results    */
    double run_wall_ms;       /* whole estimator runs                       */
    uint64_t lm_blocks;       /* residual blocks over all LM solves         */
    uint64_t lm_big_calls;    /* LM solves with >= 1024 residual blocks     */
    double lm_big_wall_ms;    /* host wall time of those                    */
    uint64_t model_trips;     /* score_batch: (model, 256-correspondence trip)
                                 pairs evaluated (early exit stops short)     */
    uint64_t model_trips_full;/* the same without the early exit            */
    uint64_t accepted;        /* hypotheses of the iterations the estimator
                                 consumed (the rest was speculative)          */
    uint64_t scored;          /* hypotheses whose score_batch sweep ran (the
                                 record skip drops iterations past a batch's
                                 first new best; `hypotheses` counts them)     */
    uint64_t tie_checks;      /* iterations whose new-best decision was re-scored
                                 in the reference's order (near ties)         */
} mp_kernel_profile;
int mp_profile_enable(int on);
int mp_profile_reset(void);
int mp_profile_read(mp_kernel_profile *out);

const char *mp_last_error(void);

/* The host LM pool's spin-before-block in microseconds (engine-internal): the
 * MADPOSE_LO_SPIN environment value, else 300, or 0 when the process's CPU affinity
 * share holds fewer than 12 CPUs per rank of LOCAL_WORLD_SIZE. */
int mp_lo_spin_us(void);
int mp_device_count(void);
const char *mp_version(void);

#ifdef __cplusplus
}
#endif
#endif
