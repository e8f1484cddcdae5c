// extern "C" boundary: include/madpose_mi355x.h
#include <atomic>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/madpose_mi355x.h"
#include "host/engine.h"
#include "include/mp_subset.h"
#include "host/hypothesis_plan.h"
#include "host/information_plan.h"
#include "host/ingest_plan.h"
#include "host/pair_set_plan.h"
#include "host/rng.h"
#include "host/select_plan.h"
#include "include/mp_draw.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

mp::RansacOptions to_opts(const mp_ransac_options *o) {
    mp::RansacOptions r;
    r.success_probability = o->success_probability;
    r.squared_inlier_thresholds[0] = o->squared_inlier_thresholds[0];
    r.squared_inlier_thresholds[1] = o->squared_inlier_thresholds[1];
    r.data_type_weights[0] = o->data_type_weights[0];
    r.data_type_weights[1] = o->data_type_weights[1];
    r.threshold_multiplier = o->threshold_multiplier;
    r.min_num_iterations = o->min_num_iterations;
    r.max_num_iterations = o->max_num_iterations;
    r.max_num_iterations_per_solver = o->max_num_iterations_per_solver;
    r.random_seed = o->random_seed;
    r.num_lo_steps = o->num_lo_steps;
    r.num_lsq_iterations = o->num_lsq_iterations;
    r.min_sample_multiplicator = o->min_sample_multiplicator;
    r.non_min_sample_multiplier = o->non_min_sample_multiplier;
    r.lo_starting_iterations = o->lo_starting_iterations;
    r.final_least_squares = o->final_least_squares != 0;
    r.use_ours = o->use_ours != 0;
    r.use_4p4d = o->use_4p4d != 0;
    return r;
}

mp::EstimatorConfig to_cfg(const mp_estimator_config *c) {
    mp::EstimatorConfig r;
    if (!c) return r;
    r.solver_type = c->solver_type;
    r.score_type = c->score_type;
    r.lo_type = c->lo_type;
    r.min_depth_constraint = c->min_depth_constraint != 0;
    r.use_shift = c->use_shift != 0;
    r.ftol = c->ceres_function_tolerance;
    r.gtol = c->ceres_gradient_tolerance;
    r.ptol = c->ceres_parameter_tolerance;
    r.max_iter = c->ceres_max_num_iterations;
    r.nonmonotonic = c->ceres_use_nonmonotonic_steps != 0;
    return r;
}

void to_model(const mp::Model &m, mp_model *o) {
    static_assert(sizeof(mp::Model) == sizeof(mp_model), "model layout");
    std::memcpy(o, &m, sizeof(mp_model));
}

void fill_stats(const mp::Stats &S, int64_t n, mp_stats *o, int32_t *inlier_idx) {
    std::memset(o, 0, sizeof(*o));
    o->best_model_score = S.best_model_score;
    for (int t = 0; t < 3; ++t) {
        o->inlier_ratios[t] = S.inlier_ratios[t];
        o->num_inliers[t] = (int32_t)S.inlier_indices[t].size();
        if (inlier_idx)
            for (size_t k = 0; k < S.inlier_indices[t].size(); ++k) inlier_idx[t * n + (int64_t)k] = S.inlier_indices[t][k];
    }
    o->num_hypotheses = S.num_hypotheses;
    o->num_lo_sweeps = S.num_lo_sweeps;
    o->num_iterations_total = S.num_iterations_total;
    o->num_iterations_per_solver[0] = S.num_iterations_per_solver[0];
    o->num_iterations_per_solver[1] = S.num_iterations_per_solver[1];
    o->best_num_inliers = S.best_num_inliers;
    o->best_solver_type = S.best_solver_type;
    o->number_lo_iterations = S.number_lo_iterations;
    o->num_batches = S.num_batches;
    o->seconds_total = S.seconds_total;
    o->seconds_lo = S.seconds_lo;
    o->seconds_gpu_wait = S.seconds_gpu_wait;
}

mp::PairInput make_input(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                         const double *d1, const double *min_depth, const double *cam0, const double *cam1) {
    mp::PairInput in;
    in.variant = variant;
    in.n = n;
    in.x0 = x0;
    in.x1 = x1;
    in.d0 = d0;
    in.d1 = d1;
    if (min_depth) {
        in.min_depth[0] = min_depth[0];
        in.min_depth[1] = min_depth[1];
    }
    const int nc = (variant == MP_CALIBRATED || variant == MP_SCALE_ONLY) ? 9 : 2;
    if (!cam0 || !cam1) throw std::invalid_argument("camera parameters missing");
    std::memcpy(in.cam0, cam0, sizeof(double) * nc);
    std::memcpy(in.cam1, cam1, sizeof(double) * nc);
    return in;
}

template <class F> int guarded(F f) {
    try {
        return f();
    } catch (const std::invalid_argument &e) {
        return fail(MP_EINVAL, e.what());
    } catch (const std::exception &e) {
        return fail(MP_EDEVICE, e.what());
    } catch (...) {
        return fail(MP_EDEVICE, "unknown error");
    }
}

} // namespace

extern "C" {

int mp_estimate(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                const double *min_depth, const double *cam0, const double *cam1, const mp_ransac_options *options,
                const mp_estimator_config *config, mp_model *out_model, mp_stats *out_stats, int32_t *inlier_idx,
                int device) {
    return guarded([&]() {
        if (!options || !out_model || !out_stats) throw std::invalid_argument("null options / outputs");
        mp::PairInput in = make_input(variant, n, x0, x1, d0, d1, min_depth, cam0, cam1);
        mp::Model m;
        mp::Stats S;
        mp::estimate_pair(in, to_opts(options), to_cfg(config), device, &m, &S);
        to_model(m, out_model);
        fill_stats(S, n, out_stats, inlier_idx);
        return MP_OK;
    });
}

int mp_estimate_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                      const double *d0, const double *d1, const double *min_depth, const double *cam0,
                      const double *cam1, const mp_ransac_options *options, const mp_estimator_config *config,
                      mp_model *out_models, mp_stats *out_stats, int32_t *inlier_idx, int device, int num_streams) {
    return guarded([&]() {
        if (num_pairs < 0 || !offsets || !options || !out_models || !out_stats)
            throw std::invalid_argument("bad batch arguments");
        const int nc = (variant == MP_CALIBRATED || variant == MP_SCALE_ONLY) ? 9 : 2;
        const mp::RansacOptions opts = to_opts(options);
        const mp::EstimatorConfig cfg = to_cfg(config);
        std::atomic<int> next(0);
        std::vector<std::string> errors(num_pairs);
        std::vector<int> codes(num_pairs, MP_OK);
        auto worker = [&]() {
            for (;;) {
                const int p = next.fetch_add(1);
                if (p >= num_pairs) break;
                const int64_t o = offsets[p], n = offsets[p + 1] - offsets[p];
                try {
                    mp::PairInput in = make_input(variant, n, x0 + 2 * o, x1 + 2 * o, d0 + o, d1 + o,
                                                  min_depth + 2 * p, cam0 + nc * p, cam1 + nc * p);
                    mp::Model m;
                    mp::Stats S;
                    mp::estimate_pair(in, opts, cfg, device, &m, &S);
                    to_model(m, &out_models[p]);
                    fill_stats(S, n, &out_stats[p], inlier_idx ? inlier_idx + 3 * o : nullptr);
                } catch (const std::invalid_argument &e) {
                    codes[p] = MP_EINVAL;
                    errors[p] = e.what();
                } catch (const std::exception &e) {
                    codes[p] = MP_EDEVICE;
                    errors[p] = e.what();
                }
            }
        };
        const int nt = std::max(1, std::min(num_streams, std::max(num_pairs, 1)));
        std::vector<std::thread> threads;
        for (int t = 0; t < nt; ++t) threads.emplace_back(worker);
        for (auto &t : threads) t.join();
        for (int p = 0; p < num_pairs; ++p)
            if (codes[p] != MP_OK) return fail(codes[p], "pair " + std::to_string(p) + ": " + errors[p]);
        return MP_OK;
    });
}

int mp_refine_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                    const double *d0, const double *d1, const double *min_depth, const double *cam0,
                    const double *cam1, const mp_ransac_options *options, const mp_estimator_config *config,
                    int32_t rounds, mp_model *models, mp_refine_result *results, int32_t *inlier_idx, int64_t chunk,
                    int device) {
    return guarded([&]() {
        static_assert(sizeof(mp::Model) == sizeof(mp_model), "model layout");
        static_assert(sizeof(mp::RefineResult) == sizeof(mp_refine_result), "refine result layout");
        if (!options) throw std::invalid_argument("null options");
        mp::refine_batch(variant, num_pairs, offsets, x0, x1, d0, d1, min_depth, cam0, cam1, to_opts(options),
                         to_cfg(config), rounds, reinterpret_cast<mp::Model *>(models),
                         reinterpret_cast<mp::RefineResult *>(results), inlier_idx, chunk, device);
        return MP_OK;
    });
}

int mp_select_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                    const double *d0, const double *d1, const double *cam0, const double *cam1,
                    const mp_ransac_options *options, const mp_estimator_config *config,
                    const int64_t *model_offsets, const mp_model *models, double *scores, int32_t *counts,
                    mp_select_result *results, int32_t *inlier_idx, int64_t chunk, int64_t model_chunk, int device) {
    return guarded([&]() {
        static_assert(sizeof(mp::Model) == sizeof(mp_model), "model layout");
        static_assert(sizeof(mp::SelectResult) == sizeof(mp_select_result) && sizeof(mp_select_result) == 32,
                      "select result layout");
        static_assert(mp::kSelectSlabModels == MP_SELECT_SLAB_MODELS && mp::kSelectTile == MP_SELECT_TILE,
                      "select constants");
        if (!options) throw std::invalid_argument("null options");
        mp::select_batch(variant, num_pairs, offsets, x0, x1, d0, d1, cam0, cam1, to_opts(options), to_cfg(config),
                         model_offsets, reinterpret_cast<const mp::Model *>(models), scores, counts,
                         reinterpret_cast<mp::SelectResult *>(results), inlier_idx, chunk, model_chunk, device);
        return MP_OK;
    });
}

int mp_debug_select_tile(int tile) {
    int prev = -1;
    const int r = guarded([&]() {
        prev = mp::select_tile_override(tile);
        return MP_OK;
    });
    return r == MP_OK ? prev : -1;
}

int mp_debug_select_timing(double *out_ms) {
    return guarded([&]() {
        if (!out_ms) throw std::invalid_argument("null output");
        const mp::SelectTiming t = mp::select_timing_last();
        out_ms[0] = t.pairs_ms;
        out_ms[1] = t.prepare_ms;
        out_ms[2] = t.upload_ms;
        out_ms[3] = t.score_ms;
        out_ms[4] = t.argmin_ms;
        out_ms[5] = t.winners_ms;
        return MP_OK;
    });
}

int mp_hypothesize_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                         const double *d0, const double *d1, const double *min_depth, const double *cam0,
                         const double *cam1, const mp_ransac_options *options, const mp_estimator_config *config,
                         const int64_t *sample_offsets, const int32_t *sample_types, const int32_t *sample_idx,
                         mp_model *models, int32_t *counts, double *norm_scale, int64_t chunk, int64_t sample_chunk,
                         int device) {
    return guarded([&]() {
        static_assert(sizeof(mp::Model) == sizeof(mp_model), "model layout");
        static_assert(mp::kHypSlabSamples == MP_HYPOTHESIZE_SLAB_SAMPLES &&
                          mp::kMaxModelsCal == MP_HYPOTHESIZE_SLOTS_CALIBRATED &&
                          mp::kMaxModelsSF == MP_HYPOTHESIZE_SLOTS_SHARED_FOCAL &&
                          mp::kMaxModelsTF == MP_HYPOTHESIZE_SLOTS_TWO_FOCAL,
                      "hypothesize constants");
        if (!options) throw std::invalid_argument("null options");
        mp::hypothesize_batch(variant, num_pairs, offsets, x0, x1, d0, d1, min_depth, cam0, cam1, to_opts(options),
                              to_cfg(config), sample_offsets, sample_types, sample_idx,
                              reinterpret_cast<mp::Model *>(models), counts, norm_scale, chunk, sample_chunk, device);
        return MP_OK;
    });
}

int mp_debug_hypothesize_timing(double *out_ms) {
    return guarded([&]() {
        if (!out_ms) throw std::invalid_argument("null output");
        const mp::HypTiming t = mp::hypothesize_timing_last();
        out_ms[0] = t.pairs_ms;
        out_ms[1] = t.plan_ms;
        out_ms[2] = t.upload_ms;
        out_ms[3] = t.solve_ms;
        out_ms[4] = t.download_ms;
        return MP_OK;
    });
}

int mp_pair_set_create(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                       const double *d0, const double *d1, const double *min_depth, const double *cam0,
                       const double *cam1, const mp_ransac_options *options, const mp_estimator_config *config,
                       int device, mp_pair_set **out) {
    return guarded([&]() {
        static_assert(mp::kPairSetMaxCorr == MP_PAIR_SET_MAX_CORRESPONDENCES, "pair set constants");
        if (!out) throw std::invalid_argument("null output");
        *out = nullptr;
        if (!options) throw std::invalid_argument("null options");
        *out = reinterpret_cast<mp_pair_set *>(mp::pair_set_create(variant, num_pairs, offsets, x0, x1, d0, d1,
                                                                   min_depth, cam0, cam1, to_opts(options),
                                                                   to_cfg(config), device));
        return MP_OK;
    });
}

int mp_pair_set_create_device(int variant, int32_t num_pairs, const int64_t *offsets, const mp_device_pairs *inputs,
                              const double *min_depth, const double *cam0, const double *cam1,
                              const mp_ransac_options *options, const mp_estimator_config *config, int device,
                              mp_pair_set **out) {
    return guarded([&]() {
        static_assert(mp::kPairRecordValues == MP_PAIR_RECORD_VALUES, "pair record constants");
        if (!out) throw std::invalid_argument("null output");
        *out = nullptr;
        if (!options) throw std::invalid_argument("null options");
        mp::DevicePairArrays in;
        if (inputs) {
            in.x0 = inputs->x0;
            in.x1 = inputs->x1;
            in.xy_type = inputs->xy_type;
            in.d0 = inputs->d0;
            in.d1 = inputs->d1;
            in.depth_type = inputs->depth_type;
            in.maps = inputs->depth_maps;
            in.num_maps = inputs->num_maps;
            in.map_type = inputs->map_type;
            in.map_dims = inputs->map_dims;
            in.map_ids = inputs->map_ids;
            in.producer_stream = inputs->producer_stream;
        } else if (num_pairs > 0) {
            throw std::invalid_argument("null inputs");
        }
        *out = reinterpret_cast<mp_pair_set *>(mp::pair_set_create_device(variant, num_pairs, offsets, in, min_depth,
                                                                          cam0, cam1, to_opts(options),
                                                                          to_cfg(config), device));
        return MP_OK;
    });
}

int mp_pair_set_destroy(mp_pair_set *set) {
    return guarded([&]() {
        mp::pair_set_destroy(reinterpret_cast<mp::PairSet *>(set));
        return MP_OK;
    });
}

int mp_pair_set_info(const mp_pair_set *set, int32_t *variant, int32_t *num_pairs, int64_t *correspondences,
                     int64_t *resident_bytes, int32_t *device) {
    return guarded([&]() {
        mp::pair_set_info(reinterpret_cast<const mp::PairSet *>(set), variant, num_pairs, correspondences,
                          resident_bytes, device);
        return MP_OK;
    });
}

int mp_pair_set_norm_scales(const mp_pair_set *set, double *out) {
    return guarded([&]() {
        mp::pair_set_norm_scales(reinterpret_cast<const mp::PairSet *>(set), out);
        return MP_OK;
    });
}

int mp_refine_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int rounds, mp_model *models,
                  mp_refine_result *results, int32_t *inlier_idx) {
    return guarded([&]() {
        mp::refine_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, rounds,
                       reinterpret_cast<mp::Model *>(models), reinterpret_cast<mp::RefineResult *>(results),
                       inlier_idx);
        return MP_OK;
    });
}

int mp_select_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *model_offsets,
                  const mp_model *models, double *scores, int32_t *counts, mp_select_result *results,
                  int32_t *inlier_idx, int64_t model_chunk) {
    return guarded([&]() {
        mp::select_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, model_offsets,
                       reinterpret_cast<const mp::Model *>(models), scores, counts,
                       reinterpret_cast<mp::SelectResult *>(results), inlier_idx, model_chunk);
        return MP_OK;
    });
}

int mp_hypothesize_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *sample_offsets,
                       const int32_t *sample_types, const int32_t *sample_idx, mp_model *models, int32_t *counts,
                       int64_t sample_chunk) {
    return guarded([&]() {
        mp::hypothesize_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, sample_offsets, sample_types,
                            sample_idx, reinterpret_cast<mp::Model *>(models), counts, sample_chunk);
        return MP_OK;
    });
}

int mp_draw_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, uint64_t seed,
                int32_t point_share, int32_t *sample_types, int32_t *sample_idx, int32_t *sample_counts) {
    return guarded([&]() {
        mp::draw_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, budget, seed, point_share, sample_types,
                     sample_idx, sample_counts);
        return MP_OK;
    });
}

int mp_debug_draw_host(int variant, int64_t n, uint64_t seed, int32_t point_share, int32_t pair, int32_t s,
                       int32_t *out) {
    return guarded([&]() {
        mp::draw_host(variant, n, seed, point_share, pair, s, out);
        return MP_OK;
    });
}

int mp_candidates_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *sample_offsets,
                      const int32_t *sample_types, const int32_t *sample_idx, int64_t sample_chunk,
                      int64_t *num_models) {
    return guarded([&]() {
        if (!num_models) throw std::invalid_argument("null num_models");
        *num_models = 0;
        *num_models = mp::candidates_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, sample_offsets,
                                         sample_types, sample_idx, sample_chunk);
        return MP_OK;
    });
}

int mp_candidates_fetch(mp_pair_set *set, mp_model *models, int64_t *model_offsets, int32_t *cand_sample,
                        int32_t *cand_slot) {
    return guarded([&]() {
        mp::candidates_fetch(reinterpret_cast<mp::PairSet *>(set), reinterpret_cast<mp::Model *>(models), model_offsets,
                             cand_sample, cand_slot);
        return MP_OK;
    });
}

int mp_ransac_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, uint64_t seed,
                  int32_t point_share, const int64_t *sample_offsets, const int32_t *sample_types,
                  const int32_t *sample_idx, int32_t rounds, mp_model *models, mp_ransac_result *results,
                  int32_t *inlier_idx, int64_t sample_chunk, int64_t model_chunk) {
    return guarded([&]() {
        static_assert(sizeof(mp::RansacResult) == sizeof(mp_ransac_result), "ransac result layout");
        static_assert(mp::kDrawShareMax == MP_DRAW_POINT_SHARE_MAX && mp::kDrawBlocks == MP_DRAW_BLOCKS,
                      "draw constants");
        mp::ransac_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, budget, seed, point_share,
                       sample_offsets, sample_types, sample_idx, rounds, reinterpret_cast<mp::Model *>(models),
                       reinterpret_cast<mp::RansacResult *>(results), inlier_idx, sample_chunk, model_chunk);
        return MP_OK;
    });
}

int mp_ransac_adaptive_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                           uint64_t seed, int32_t point_share, int32_t rounds, mp_model *models,
                           mp_ransac_result *results, int32_t *inlier_idx, int32_t *stopped, int64_t sample_chunk,
                           int64_t model_chunk) {
    return guarded([&]() {
        mp::ransac_adaptive_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, budget, step, seed,
                                point_share, rounds, reinterpret_cast<mp::Model *>(models),
                                reinterpret_cast<mp::RansacResult *>(results), inlier_idx, stopped, sample_chunk,
                                model_chunk);
        return MP_OK;
    });
}

int mp_refine_relaxed_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int rounds, mp_model *models,
                          mp_refine_result *results, int32_t *inlier_idx) {
    return guarded([&]() {
        mp::refine_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, rounds,
                       reinterpret_cast<mp::Model *>(models), reinterpret_cast<mp::RefineResult *>(results),
                       inlier_idx, true);
        return MP_OK;
    });
}

int mp_ransac_lo_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                     uint64_t seed, int32_t point_share, int32_t rounds, int32_t lo_rounds, mp_model *models,
                     mp_ransac_result *results, int32_t *inlier_idx, int32_t *stopped, mp_ransac_lo_info *lo_info,
                     int64_t sample_chunk, int64_t model_chunk) {
    return guarded([&]() {
        static_assert(sizeof(mp::RansacLoInfo) == sizeof(mp_ransac_lo_info) && sizeof(mp_ransac_lo_info) == 16,
                      "lo info layout");
        mp::ransac_lo_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, budget, step, seed, point_share,
                          rounds, lo_rounds, reinterpret_cast<mp::Model *>(models),
                          reinterpret_cast<mp::RansacResult *>(results), inlier_idx, stopped,
                          reinterpret_cast<mp::RansacLoInfo *>(lo_info), sample_chunk, model_chunk);
        return MP_OK;
    });
}

int mp_lsq_fit_set(mp_pair_set *set, int32_t num_entries, const int32_t *pair_ids, const int32_t *solver_types,
                   const double *factors, int rule, uint64_t seed, const int32_t *streams, const int32_t *substreams,
                   mp_model *models, mp_lsq_fit_result *results, int32_t *subset_idx, int64_t entry_chunk) {
    return guarded([&]() {
        static_assert(sizeof(mp::LsqFitResult) == sizeof(mp_lsq_fit_result) && sizeof(mp_lsq_fit_result) == 48,
                      "lsq fit result layout");
        static_assert(mp::kSubsetLsq == MP_LSQ_RULE_LSQ && mp::kSubsetNonmin == MP_LSQ_RULE_NONMIN, "lsq rules");
        mp::lsq_fit_set(reinterpret_cast<mp::PairSet *>(set), num_entries, pair_ids, solver_types, factors, rule, seed,
                        streams, substreams, reinterpret_cast<mp::Model *>(models),
                        reinterpret_cast<mp::LsqFitResult *>(results), subset_idx, entry_chunk);
        return MP_OK;
    });
}

int mp_debug_subset_select(const int64_t offsets[4], const int32_t *idx, int64_t k, uint64_t seed, int32_t pair,
                           int32_t stream, int32_t substream, uint64_t key_mask, int32_t *out_idx,
                           int32_t out_sizes[3], int device) {
    return guarded([&]() {
        mp::subset_select_device(offsets, idx, k, seed, pair, stream, substream, key_mask, out_idx, out_sizes, device);
        return MP_OK;
    });
}

int mp_debug_subset_select_host(const int64_t offsets[4], const int32_t *idx, int64_t k, uint64_t seed, int32_t pair,
                                int32_t stream, int32_t substream, uint64_t key_mask, int32_t *out_idx,
                                int32_t out_sizes[3]) {
    return guarded([&]() {
        mp::subset_select_host_hook(offsets, idx, k, seed, pair, stream, substream, key_mask, out_idx, out_sizes);
        return MP_OK;
    });
}

int mp_debug_lsq_subset_size(int rule, int solver_type, int variant, int32_t min_sample_multiplicator,
                             int32_t non_min_sample_multiplier, const int32_t sizes[3], int64_t *k, int32_t *run) {
    return guarded([&]() {
        if (!run) throw std::invalid_argument("null run");
        *run = mp::lsq_subset_size(rule, solver_type, variant, min_sample_multiplicator, non_min_sample_multiplier,
                                   sizes, k);
        return MP_OK;
    });
}

int mp_ransac_lo_steps_set(mp_pair_set *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                           uint64_t seed, int32_t point_share, int32_t rounds, int32_t lo_rounds, int32_t lo_steps,
                           mp_model *models, mp_ransac_result *results, int32_t *inlier_idx, int32_t *stopped,
                           mp_ransac_lo_info *lo_info, mp_ransac_lo_steps_info *steps_info, int64_t sample_chunk,
                           int64_t model_chunk) {
    return guarded([&]() {
        static_assert(sizeof(mp::RansacLoStepsInfo) == sizeof(mp_ransac_lo_steps_info) &&
                          sizeof(mp_ransac_lo_steps_info) == 16,
                      "lo steps info layout");
        mp::ransac_lo_steps_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, budget, step, seed,
                                point_share, rounds, lo_rounds, lo_steps, reinterpret_cast<mp::Model *>(models),
                                reinterpret_cast<mp::RansacResult *>(results), inlier_idx, stopped,
                                reinterpret_cast<mp::RansacLoInfo *>(lo_info),
                                reinterpret_cast<mp::RansacLoStepsInfo *>(steps_info), sample_chunk, model_chunk);
        return MP_OK;
    });
}

int mp_draw_weights_create(mp_pair_set *set, const void *weights, int32_t dtype, int32_t on_device,
                           const uint8_t *given, void *producer_stream, mp_draw_weights **out) {
    return guarded([&]() {
        static_assert(mp::kDrawWeightMaxN == MP_DRAW_WEIGHT_MAX_N && mp::kDrawStageEntries == MP_DRAW_STAGE_ENTRIES,
                      "weighted draw constants");
        if (!out) throw std::invalid_argument("null output handle");
        *out = nullptr;
        *out = reinterpret_cast<mp_draw_weights *>(mp::draw_weights_create(
            reinterpret_cast<mp::PairSet *>(set), weights, dtype, on_device != 0, given, producer_stream));
        return MP_OK;
    });
}

int mp_draw_weights_info(const mp_draw_weights *handle, int32_t *weighted, int32_t *positive, uint32_t *total) {
    return guarded([&]() {
        mp::draw_weights_info(reinterpret_cast<const mp::DrawWeights *>(handle), weighted, positive, total);
        return MP_OK;
    });
}

int mp_draw_weights_destroy(mp_draw_weights *handle) {
    return guarded([&]() {
        mp::draw_weights_destroy(reinterpret_cast<mp::DrawWeights *>(handle));
        return MP_OK;
    });
}

int mp_draw_weighted_set(mp_pair_set *set, const mp_draw_weights *handle, int32_t num_sel, const int32_t *pair_ids,
                         int32_t budget, uint64_t seed, int32_t point_share, int32_t *sample_types,
                         int32_t *sample_idx, int32_t *sample_counts) {
    return guarded([&]() {
        if (!set) throw std::invalid_argument("null pair set");
        if (!handle) throw std::invalid_argument("null draw weights");
        mp::draw_set(reinterpret_cast<mp::PairSet *>(set), num_sel, pair_ids, budget, seed, point_share, sample_types,
                     sample_idx, sample_counts, reinterpret_cast<const mp::DrawWeights *>(handle));
        return MP_OK;
    });
}

int mp_ransac_weighted_set(mp_pair_set *set, const mp_draw_weights *handle, int32_t num_sel, const int32_t *pair_ids,
                           int32_t budget, int32_t step, uint64_t seed, int32_t point_share, int32_t rounds,
                           int32_t lo_rounds, int32_t lo_steps, mp_model *models, mp_ransac_result *results,
                           int32_t *inlier_idx, int32_t *stopped, mp_ransac_lo_info *lo_info,
                           mp_ransac_lo_steps_info *steps_info, int64_t sample_chunk, int64_t model_chunk) {
    return guarded([&]() {
        if (!set) throw std::invalid_argument("null pair set");
        if (!handle) throw std::invalid_argument("null draw weights");
        mp::PairSet *S = reinterpret_cast<mp::PairSet *>(set);
        const mp::DrawWeights *W = reinterpret_cast<const mp::DrawWeights *>(handle);
        mp::Model *M = reinterpret_cast<mp::Model *>(models);
        mp::RansacResult *Q = reinterpret_cast<mp::RansacResult *>(results);
        mp::RansacLoInfo *LI = reinterpret_cast<mp::RansacLoInfo *>(lo_info);
        if (step == 0 && (lo_rounds != 0 || lo_steps != 0))
            throw std::invalid_argument("lo_rounds and lo_steps need step: they run inside the adaptive rounds");
        if (lo_rounds == 0 && lo_steps != 0) throw std::invalid_argument("lo_steps needs lo_rounds");
        if (step == 0)
            mp::ransac_set(S, num_sel, pair_ids, budget, seed, point_share, nullptr, nullptr, nullptr, rounds, M, Q,
                           inlier_idx, sample_chunk, model_chunk, W);
        else if (lo_rounds == 0)
            mp::ransac_adaptive_set(S, num_sel, pair_ids, budget, step, seed, point_share, rounds, M, Q, inlier_idx,
                                    stopped, sample_chunk, model_chunk, W);
        else if (lo_steps == 0)
            mp::ransac_lo_set(S, num_sel, pair_ids, budget, step, seed, point_share, rounds, lo_rounds, M, Q, inlier_idx,
                              stopped, LI, sample_chunk, model_chunk, W);
        else
            mp::ransac_lo_steps_set(S, num_sel, pair_ids, budget, step, seed, point_share, rounds, lo_rounds, lo_steps, M,
                                    Q, inlier_idx, stopped, LI, reinterpret_cast<mp::RansacLoStepsInfo *>(steps_info),
                                    sample_chunk, model_chunk, W);
        return MP_OK;
    });
}

int mp_inlier_mass_set(mp_pair_set *set, const mp_draw_weights *handle, int32_t num_entries, const int32_t *pair_ids,
                       const mp_model *models, mp_inlier_mass *out) {
    return guarded([&]() {
        static_assert(sizeof(mp::InlierMass) == sizeof(mp_inlier_mass) && sizeof(mp_inlier_mass) == 32,
                      "inlier mass layout");
        if (!set) throw std::invalid_argument("null pair set");
        if (!handle) throw std::invalid_argument("null draw weights");
        mp::inlier_mass_set(reinterpret_cast<mp::PairSet *>(set), reinterpret_cast<const mp::DrawWeights *>(handle),
                            num_entries, pair_ids, reinterpret_cast<const mp::Model *>(models),
                            reinterpret_cast<mp::InlierMass *>(out));
        return MP_OK;
    });
}

int mp_ransac_weighted_stop_set(mp_pair_set *set, const mp_draw_weights *handle, int32_t num_sel,
                                const int32_t *pair_ids, int32_t budget, int32_t step, uint64_t seed,
                                int32_t point_share, int32_t rounds, int32_t lo_rounds, int32_t lo_steps,
                                mp_model *models, mp_ransac_result *results, int32_t *inlier_idx, int32_t *stopped,
                                mp_ransac_lo_info *lo_info, mp_ransac_lo_steps_info *steps_info, int64_t sample_chunk,
                                int64_t model_chunk, mp_inlier_mass *rule_mass) {
    return guarded([&]() {
        if (!set) throw std::invalid_argument("null pair set");
        if (!handle) throw std::invalid_argument("null draw weights");
        mp::PairSet *S = reinterpret_cast<mp::PairSet *>(set);
        const mp::DrawWeights *W = reinterpret_cast<const mp::DrawWeights *>(handle);
        mp::Model *M = reinterpret_cast<mp::Model *>(models);
        mp::RansacResult *Q = reinterpret_cast<mp::RansacResult *>(results);
        mp::RansacLoInfo *LI = reinterpret_cast<mp::RansacLoInfo *>(lo_info);
        mp::InlierMass *RM = reinterpret_cast<mp::InlierMass *>(rule_mass);
        if (step < 1) throw std::invalid_argument("the weighted stop needs step >= 1: the rule is read at checkpoints");
        if (lo_rounds == 0 && lo_steps != 0) throw std::invalid_argument("lo_steps needs lo_rounds");
        if (lo_rounds == 0)
            mp::ransac_adaptive_set(S, num_sel, pair_ids, budget, step, seed, point_share, rounds, M, Q, inlier_idx,
                                    stopped, sample_chunk, model_chunk, W, true, RM);
        else if (lo_steps == 0)
            mp::ransac_lo_set(S, num_sel, pair_ids, budget, step, seed, point_share, rounds, lo_rounds, M, Q, inlier_idx,
                              stopped, LI, sample_chunk, model_chunk, W, true, RM);
        else
            mp::ransac_lo_steps_set(S, num_sel, pair_ids, budget, step, seed, point_share, rounds, lo_rounds, lo_steps, M,
                                    Q, inlier_idx, stopped, LI, reinterpret_cast<mp::RansacLoStepsInfo *>(steps_info),
                                    sample_chunk, model_chunk, W, true, RM);
        return MP_OK;
    });
}

int mp_debug_ransac_required_mass(int variant, uint32_t total, const uint32_t mass[3], const mp_ransac_options *options,
                                  uint32_t req[2]) {
    return guarded([&]() {
        if (!options) throw std::invalid_argument("null options");
        mp::ransac_required_mass(variant, total, mass, to_opts(options), req);
        return MP_OK;
    });
}

int mp_debug_inlier_mass_host(int64_t n, const uint32_t *cum, const int64_t offsets[4], const int32_t *idx,
                              uint32_t mass[3]) {
    return guarded([&]() {
        mp::inlier_mass_host_hook(n, cum, offsets, idx, mass);
        return MP_OK;
    });
}

int mp_debug_inlier_mass_stats(int64_t *launches, double *ms, int32_t reset) {
    return guarded([&]() {
        mp::inlier_mass_stats(launches, ms, reset != 0);
        return MP_OK;
    });
}

int mp_residuals_set(mp_pair_set *set, int32_t num_entries, const int32_t *pair_ids, const mp_model *models,
                     const double *factors, const mp_residuals_out *out, int64_t *row_offsets, int32_t *counts) {
    return guarded([&]() {
        if (!set) throw std::invalid_argument("null pair set");
        if (!out) throw std::invalid_argument("null out");
        mp::ResidualsOut O;
        O.mask = out->mask;
        O.errors = out->errors;
        O.on_device = out->on_device;
        O.producer_stream = out->producer_stream;
        mp::residuals_set(reinterpret_cast<mp::PairSet *>(set), num_entries, pair_ids,
                          reinterpret_cast<const mp::Model *>(models), factors, O, row_offsets, counts);
        return MP_OK;
    });
}

int mp_ransac_out_set(mp_pair_set *set, const mp_draw_weights *handle, int32_t num_sel, const int32_t *pair_ids,
                      int32_t budget, int32_t step, uint64_t seed, int32_t point_share, const int64_t *sample_offsets,
                      const int32_t *sample_types, const int32_t *sample_idx, int32_t rounds, int32_t lo_rounds,
                      int32_t lo_steps, int32_t weighted_stop, mp_model *models, mp_ransac_result *results,
                      int32_t *inlier_idx, int32_t *stopped, mp_ransac_lo_info *lo_info,
                      mp_ransac_lo_steps_info *steps_info, int64_t sample_chunk, int64_t model_chunk,
                      mp_inlier_mass *rule_mass, const mp_ransac_out *out) {
    return guarded([&]() {
        static_assert(sizeof(mp_ransac_out) == 6 * sizeof(void *) && offsetof(mp_ransac_out, errors) == sizeof(void *) &&
                          offsetof(mp_ransac_out, models) == 2 * sizeof(void *) &&
                          offsetof(mp_ransac_out, index) == 3 * sizeof(void *) &&
                          offsetof(mp_ransac_out, counts) == 4 * sizeof(void *) &&
                          offsetof(mp_ransac_out, producer_stream) == 5 * sizeof(void *),
                      "ransac out layout");
        if (!set) throw std::invalid_argument("null pair set");
        mp::RansacOut O;
        if (out) {
            O.mask = out->mask;
            O.errors = out->errors;
            O.models = out->models;
            O.index = out->index;
            O.counts = out->counts;
            O.producer_stream = out->producer_stream;
        }
        mp::ransac_out_set(reinterpret_cast<mp::PairSet *>(set), reinterpret_cast<const mp::DrawWeights *>(handle),
                           num_sel, pair_ids, budget, step, seed, point_share, sample_offsets, sample_types, sample_idx,
                           rounds, lo_rounds, lo_steps, weighted_stop != 0, reinterpret_cast<mp::Model *>(models),
                           reinterpret_cast<mp::RansacResult *>(results), inlier_idx, stopped,
                           reinterpret_cast<mp::RansacLoInfo *>(lo_info),
                           reinterpret_cast<mp::RansacLoStepsInfo *>(steps_info), sample_chunk, model_chunk,
                           reinterpret_cast<mp::InlierMass *>(rule_mass), &O);
        return MP_OK;
    });
}

int mp_debug_ransac_out_stats(int64_t *launches, double *ms, int32_t reset) {
    return guarded([&]() {
        mp::ransac_out_stats(launches, ms, reset != 0);
        return MP_OK;
    });
}

int mp_debug_residuals_stats(int64_t *launches, double *ms, int32_t reset) {
    return guarded([&]() {
        mp::residuals_stats(launches, ms, reset != 0);
        return MP_OK;
    });
}

int mp_information_set(mp_pair_set *set, int32_t num_entries, const int32_t *pair_ids, const mp_model *models,
                       const double *factors, const mp_information_out *out, mp_information_entry *entries) {
    return guarded([&]() {
        static_assert(sizeof(mp_information_entry) == sizeof(mp::InfoRecord) &&
                          offsetof(mp_information_entry, pd) == offsetof(mp::InfoRecord, pd) &&
                          offsetof(mp_information_entry, status) == offsetof(mp::InfoRecord, status) &&
                          offsetof(mp_information_entry, rows) == offsetof(mp::InfoRecord, rows) &&
                          offsetof(mp_information_entry, counts) == offsetof(mp::InfoRecord, counts),
                      "information entry layout");
        if (!set) throw std::invalid_argument("null pair set");
        if (!out) throw std::invalid_argument("null out");
        mp::InformationOut O;
        O.H = out->H;
        O.g = out->g;
        O.cost = out->cost;
        O.cov = out->cov;
        O.on_device = out->on_device;
        O.producer_stream = out->producer_stream;
        mp::information_set(reinterpret_cast<mp::PairSet *>(set), num_entries, pair_ids,
                            reinterpret_cast<const mp::Model *>(models), factors, O,
                            reinterpret_cast<mp::InfoRecord *>(entries));
        return MP_OK;
    });
}

int mp_debug_information_finish(double H[66], double g[11], const int32_t col[11], double cov[121], int32_t *pd) {
    return guarded([&]() {
        if (!H || !g || !col || !cov || !pd) throw std::invalid_argument("null argument");
        int c[mp::kInfoN];
        for (int a = 0; a < mp::kInfoN; ++a) c[a] = col[a] != 0 ? 1 : 0;
        mp::info_mask(H, g, c);
        *pd = mp::info_covariance(H, c, cov);
        return MP_OK;
    });
}

int mp_debug_information_stats(int64_t *launches, double *rows_ms, double *finish_ms, int32_t reset) {
    return guarded([&]() {
        mp::information_stats(launches, rows_ms, finish_ms, reset != 0);
        return MP_OK;
    });
}

int mp_debug_draw_weights_host(int64_t n, const void *weights, int32_t dtype, uint32_t *cum, int32_t *positive) {
    return guarded([&]() {
        mp::draw_weights_host(n, weights, dtype, cum, positive);
        return MP_OK;
    });
}

int mp_debug_draw_weighted_host(int variant, int64_t n, const uint32_t *cum, uint64_t seed, int32_t point_share,
                                int32_t pair, int32_t s, int32_t *out) {
    return guarded([&]() {
        mp::draw_weighted_host(variant, n, cum, seed, point_share, pair, s, out);
        return MP_OK;
    });
}

int mp_debug_ransac_lo_track(int32_t num_rounds, const double *min_score, const int32_t *min_counts,
                             const int32_t *candidate, const int32_t *lo_rounds_accepted, const double *lo_score,
                             const int32_t *lo_counts, double *score, int32_t *out) {
    return guarded([&]() {
        mp::ransac_lo_track(num_rounds, min_score, min_counts, candidate, lo_rounds_accepted, lo_score, lo_counts, score,
                            out);
        return MP_OK;
    });
}

int mp_debug_ransac_required(int variant, int64_t n, const int32_t counts[3], const mp_ransac_options *options,
                             uint32_t req[2]) {
    return guarded([&]() {
        if (!options) throw std::invalid_argument("null options");
        mp::ransac_required(variant, n, counts, to_opts(options), req);
        return MP_OK;
    });
}

int mp_debug_select_argmin(int32_t num_pairs, const int64_t *model_offsets, const double *scores, const double *prior,
                           int32_t *index, double *score, int device) {
    return guarded([&]() {
        mp::select_argmin_direct(num_pairs, model_offsets, scores, prior, index, score, device);
        return MP_OK;
    });
}

int mp_debug_ransac_timing(double *out_ms) {
    return guarded([&]() {
        if (!out_ms) throw std::invalid_argument("null output");
        const mp::RansacTiming t = mp::ransac_timing_last();
        const double v[MP_RANSAC_TIMING_VALUES] = {
            t.total_ms,       t.hypothesize_ms,  t.select_ms,         t.refine_ms,        t.hyp.plan_ms,
            t.hyp.draw_ms,    t.hyp.upload_ms,   t.hyp.solve_ms,      t.hyp.compact_ms,   t.hyp.download_ms,
            t.select.prepare_ms, t.select.upload_ms, t.select.score_ms, t.select.argmin_ms, t.select.winners_ms,
            (double)t.bytes_back, (double)t.bytes_slots, t.samples_ms};
        for (int i = 0; i < MP_RANSAC_TIMING_VALUES; ++i) out_ms[i] = v[i];
        return MP_OK;
    });
}

int mp_debug_pair_set_prep(int mode) {
    return guarded([&]() {
        mp::pair_set_prep_mode(mode);
        return MP_OK;
    });
}

int mp_debug_pair_set_rows(const mp_pair_set *set, int32_t pair, double *out) {
    return guarded([&]() {
        mp::pair_set_rows(reinterpret_cast<const mp::PairSet *>(set), pair, out);
        return MP_OK;
    });
}

int mp_debug_pair_set_record(const mp_pair_set *set, int32_t pair, double *out) {
    return guarded([&]() {
        mp::pair_set_record(reinterpret_cast<const mp::PairSet *>(set), pair, out);
        return MP_OK;
    });
}

int mp_debug_ingest_info(int32_t *out) {
    return guarded([&]() {
        mp::ingest_info(out);
        return MP_OK;
    });
}

int mp_debug_device_extent(const void *ptr, int device, int64_t *out) {
    return guarded([&]() {
        mp::device_extent(ptr, device, out);
        return MP_OK;
    });
}

int mp_get_depths(int dtype, int32_t num_pairs, const void *depth_maps, const int64_t *dims, const int64_t *pt_offsets,
                  const double *keypoints, void *out, int device) {
    return guarded([&]() {
        if (num_pairs < 0 || (num_pairs > 0 && (!depth_maps || !dims || !pt_offsets || !out)))
            throw std::invalid_argument("bad get_depths arguments");
        mp::get_depths_batch(dtype, num_pairs, depth_maps, dims, pt_offsets, keypoints, out, device);
        return MP_OK;
    });
}

int mp_bougnoux_focals(int64_t k, const double *F, double *out, int device) {
    return guarded([&]() {
        if (k < 0 || (k > 0 && (!F || !out))) throw std::invalid_argument("bad bougnoux arguments");
        mp::bougnoux_batch(k, F, out, device);
        return MP_OK;
    });
}

int mp_pose_eval(int64_t k, const double *R, const double *t, const double *T_0to1, double t_thres, double *err_t,
                 double *err_R, int32_t nthr, const double *thresholds, double *aucs, int device) {
    return guarded([&]() {
        if (k < 0 || nthr < 0 || (k > 0 && (!R || !t || !T_0to1 || !err_t || !err_R)) ||
            (nthr > 0 && (!thresholds || !aucs)))
            throw std::invalid_argument("bad pose_eval arguments");
        for (int b = 0; b < nthr; ++b)
            if (!(thresholds[b] > 0.0)) throw std::invalid_argument("AUC thresholds must be positive");
        mp::pose_eval_batch(k, R, t, T_0to1, t_thres, err_t, err_R, nthr, thresholds, aucs, device);
        return MP_OK;
    });
}

int mp_pose_auc(int64_t k, const double *errors, int32_t nthr, const double *thresholds, double *aucs, int device) {
    return guarded([&]() {
        if (k < 0 || nthr < 0 || (k > 0 && !errors) || (nthr > 0 && (!thresholds || !aucs)))
            throw std::invalid_argument("bad pose_auc arguments");
        for (int b = 0; b < nthr; ++b)
            if (!(thresholds[b] > 0.0)) throw std::invalid_argument("AUC thresholds must be positive");
        mp::pose_auc_batch(k, errors, nthr, thresholds, aucs, device);
        return MP_OK;
    });
}

int mp_estimate_scale_and_pose(const double *X, const double *Y, const double *W, int64_t n, mp_model *out,
                               int device) {
    return guarded([&]() {
        if (!X || !Y || !W || !out || n < 1) throw std::invalid_argument("bad arguments");
        mp::Model m;
        mp::scale_and_pose_direct(X, Y, W, n, &m, device);
        to_model(m, out);
        return MP_OK;
    });
}

int mp_solve_scale_and_shift(int variant, const double *x_homo, const double *y_homo, const double *depth_x,
                             const double *depth_y, double *out, int max_out, int device) {
    int r = guarded([&]() {
        if (variant < 0 || variant > 2) throw std::invalid_argument("bad variant");
        mp::Model poses[8];
        int np = 0;
        int n = mp::solve_md_direct(variant, x_homo, y_homo, depth_x, depth_y, out, max_out, poses, 8, &np, device);
        return -(n + 1000); // encode count through the guard
    });
    return r <= -1000 ? -(r + 1000) : -r;
}

int mp_solve_scale_shift_pose(int variant, const double *x_homo, const double *y_homo, const double *depth_x,
                              const double *depth_y, mp_model *out, int max_out, int device) {
    int r = guarded([&]() {
        if (variant < 0 || variant > 2) throw std::invalid_argument("bad variant");
        double sols[48];
        mp::Model poses[8];
        int np = 0;
        mp::solve_md_direct(variant, x_homo, y_homo, depth_x, depth_y, sols, 8, poses, 8, &np, device);
        for (int i = 0; i < std::min(np, max_out); ++i) to_model(poses[i], &out[i]);
        return -(np + 1000);
    });
    return r <= -1000 ? -(r + 1000) : -r;
}

int mp_solve_scale_shift_pose_alt(int variant, int alt, const double *x_homo, const double *y_homo,
                                  const double *depth_x, const double *depth_y, mp_model *out, int max_out, int device) {
    int r = guarded([&]() {
        if (variant < 0 || variant > 2) throw std::invalid_argument("bad variant");
        if (alt < 1 || alt > 2 || (alt == 2 && variant != 2))
            throw std::invalid_argument("alt must be 1 (use_ours) or 2 (use_4p4d, two-focal only)");
        double sols[48];
        mp::Model poses[8];
        int np = 0;
        mp::solve_md_direct(variant, x_homo, y_homo, depth_x, depth_y, sols, 8, poses, 8, &np, device, alt);
        for (int i = 0; i < std::min(np, max_out); ++i) to_model(poses[i], &out[i]);
        return -(np + 1000);
    });
    return r <= -1000 ? -(r + 1000) : -r;
}

int mp_solve_scale_and_shift_batch(int variant, int64_t ns, const double *x_homo, const double *y_homo,
                                   const double *depth_x, const double *depth_y, double *out, int32_t *counts,
                                   int64_t chunk, int device) {
    return guarded([&]() {
        mp::solve_md_batch(variant, 0, false, ns, x_homo, y_homo, depth_x, depth_y, out, nullptr, counts, chunk, device);
        return MP_OK;
    });
}

int mp_solve_scale_shift_pose_batch(int variant, int alt, int64_t ns, const double *x_homo, const double *y_homo,
                                    const double *depth_x, const double *depth_y, mp_model *out, int32_t *counts,
                                    int64_t chunk, int device) {
    return guarded([&]() {
        static_assert(sizeof(mp::Model) == sizeof(mp_model), "model layout");
        mp::solve_md_batch(variant, alt, true, ns, x_homo, y_homo, depth_x, depth_y, nullptr,
                           reinterpret_cast<mp::Model *>(out), counts, chunk, device);
        return MP_OK;
    });
}

int mp_relpose_batch(int kind, int64_t ns, const double *x0, const double *x1, mp_model *out, int32_t *counts,
                     int64_t chunk, int device) {
    return guarded([&]() {
        mp::relpose_batch(kind, ns, x0, x1, reinterpret_cast<mp::Model *>(out), counts, chunk, device);
        return MP_OK;
    });
}

extern "C++" {
namespace {
// the shared argument handling of mp_score_models and mp_debug_lo_sweep: `sweep`
// receives the pair, the converted options and the models
template <class F>
int with_models(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                const double *cam0, const double *cam1, const mp_ransac_options *options,
                const mp_estimator_config *config, const mp_model *models, int32_t num_models, double *scores,
                F &&sweep) {
    return guarded([&]() {
        if (!options || !models || !scores || num_models < 0) throw std::invalid_argument("bad arguments");
        const double md[2] = {0.0, 0.0};
        mp::PairInput in = make_input(variant, n, x0, x1, d0, d1, md, cam0, cam1);
        std::vector<mp::Model> ms(num_models);
        std::memcpy(ms.data(), models, sizeof(mp_model) * num_models);
        sweep(in, to_opts(options), to_cfg(config), ms);
        return MP_OK;
    });
}
} // namespace
} // extern "C++"

int mp_score_models(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                    const double *cam0, const double *cam1, const mp_ransac_options *options,
                    const mp_estimator_config *config, const mp_model *models, int32_t num_models, double *scores,
                    double *errors, int device) {
    return with_models(variant, n, x0, x1, d0, d1, cam0, cam1, options, config, models, num_models, scores,
                       [&](const mp::PairInput &in, const mp::RansacOptions &o, const mp::EstimatorConfig &c,
                           std::vector<mp::Model> &ms) {
                           mp::score_models(in, o, c, ms.data(), num_models, scores, errors, device, nullptr);
                       });
}

int mp_debug_score_batch(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                         const double *d1, const double *cam0, const double *cam1, const mp_ransac_options *options,
                         const mp_estimator_config *config, int32_t num_iterations, const int32_t *counts,
                         const mp_model *models, double best, int32_t flags, double *res_best, int32_t *res_slot,
                         mp_model *rec_models, double *res_hi_lo, double *model_ties, int device) {
    return guarded([&]() {
        if (!options || !counts || !models || !res_best || !res_slot || num_iterations <= 0)
            throw std::invalid_argument("bad arguments");
        const double md[2] = {0.0, 0.0};
        mp::PairInput in = make_input(variant, n, x0, x1, d0, d1, md, cam0, cam1);
        const int maxm = mp::max_models(variant == 3 ? 0 : variant);
        std::vector<mp::Model> ms((size_t)num_iterations * maxm), rm(num_iterations);
        std::memcpy(ms.data(), models, sizeof(mp_model) * ms.size());
        mp::debug_score_batch(in, to_opts(options), to_cfg(config), num_iterations, counts, ms.data(), best, flags,
                              res_best, res_slot, rm.data(), res_hi_lo, model_ties, device);
        if (rec_models)
            for (int b = 0; b < num_iterations; ++b) to_model(rm[b], &rec_models[b]);
        return MP_OK;
    });
}

int mp_debug_score_terms(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                         const double *d1, const double *cam0, const double *cam1, const mp_ransac_options *options,
                         const mp_estimator_config *config, const mp_model *models, int32_t num_models, double *errors,
                         int32_t *flags, double *taus, double *ties, int device) {
    return guarded([&]() {
        if (!options || !models || !errors || !flags || num_models < 0) throw std::invalid_argument("bad arguments");
        const double md[2] = {0.0, 0.0};
        mp::PairInput in = make_input(variant, n, x0, x1, d0, d1, md, cam0, cam1);
        std::vector<mp::Model> ms(num_models);
        std::memcpy(ms.data(), models, sizeof(mp_model) * num_models);
        mp::debug_score_terms(in, to_opts(options), to_cfg(config), ms.data(), num_models, errors, flags, taus, ties,
                              device);
        return MP_OK;
    });
}

int mp_debug_score_margins(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                           const double *d1, const double *cam0, const double *cam1,
                           const mp_ransac_options *options, const mp_estimator_config *config, const mp_model *models,
                           int32_t num_models, double *per_model, double *per_pair) {
    return guarded([&]() {
        if (!options || !models || !per_model || num_models < 0) throw std::invalid_argument("bad arguments");
        const double md[2] = {0.0, 0.0};
        mp::PairInput in = make_input(variant, n, x0, x1, d0, d1, md, cam0, cam1);
        std::vector<mp::Model> ms(num_models);
        std::memcpy(ms.data(), models, sizeof(mp_model) * num_models);
        mp::debug_score_margins(in, to_opts(options), to_cfg(config), ms.data(), num_models, per_model, per_pair);
        return MP_OK;
    });
}

int mp_debug_lo_sweep(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                      const double *cam0, const double *cam1, const mp_ransac_options *options,
                      const mp_estimator_config *config, const mp_model *models, int32_t num_models, double *scores,
                      double *errors, double *fast_bounds) {
    return with_models(variant, n, x0, x1, d0, d1, cam0, cam1, options, config, models, num_models, scores,
                       [&](const mp::PairInput &in, const mp::RansacOptions &o, const mp::EstimatorConfig &c,
                           std::vector<mp::Model> &ms) {
                           mp::lo_sweep_models(in, o, c, ms.data(), num_models, scores, errors, fast_bounds);
                       });
}

extern "C++" {
namespace {
// the shared argument handling of mp_lm_refine_batch and mp_debug_lm_refine_host
template <class F>
int with_lm_problems(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                     const double *min_depth, const double *cam0, const double *cam1,
                     const mp_ransac_options *options, const mp_estimator_config *config, int32_t num_problems,
                     const int64_t *sample_offsets, const int32_t *sample_idx, mp_model *models, int32_t *status,
                     F &&refine) {
    return guarded([&]() {
        if (!options || num_problems < 0 || (num_problems > 0 && (!sample_offsets || !models || !status)))
            throw std::invalid_argument("bad arguments");
        if (num_problems > 0 && sample_offsets[3 * num_problems] > 0 && !sample_idx)
            throw std::invalid_argument("null sample indices");
        const double md0[2] = {0.0, 0.0};
        mp::PairInput in = make_input(variant, n, x0, x1, d0, d1, min_depth ? min_depth : md0, cam0, cam1);
        std::vector<mp::Model> ms(num_problems);
        std::memcpy(ms.data(), models, sizeof(mp_model) * num_problems);
        refine(in, to_opts(options), to_cfg(config), ms);
        for (int j = 0; j < num_problems; ++j) to_model(ms[j], &models[j]);
        return MP_OK;
    });
}
} // namespace
} // extern "C++"

int mp_lm_refine_batch(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                       const double *d1, const double *min_depth, const double *cam0, const double *cam1,
                       const mp_ransac_options *options, const mp_estimator_config *config, int32_t num_problems,
                       const int32_t *kinds, const int64_t *sample_offsets, const int32_t *sample_idx,
                       mp_model *models, int32_t *status, int device) {
    return with_lm_problems(variant, n, x0, x1, d0, d1, min_depth, cam0, cam1, options, config, num_problems,
                            sample_offsets, sample_idx, models, status,
                            [&](const mp::PairInput &in, const mp::RansacOptions &o, const mp::EstimatorConfig &c,
                                std::vector<mp::Model> &ms) {
                                mp::lm_refine_batch_device(in, o, c, num_problems, kinds, sample_offsets, sample_idx,
                                                           ms.data(), status, device);
                            });
}

int mp_debug_lm_refine_host(int variant, int64_t n, const double *x0, const double *x1, const double *d0,
                            const double *d1, const double *min_depth, const double *cam0, const double *cam1,
                            const mp_ransac_options *options, const mp_estimator_config *config, int32_t num_problems,
                            const int32_t *kinds, const int64_t *sample_offsets, const int32_t *sample_idx,
                            mp_model *models, int32_t *status) {
    return with_lm_problems(variant, n, x0, x1, d0, d1, min_depth, cam0, cam1, options, config, num_problems,
                            sample_offsets, sample_idx, models, status,
                            [&](const mp::PairInput &in, const mp::RansacOptions &o, const mp::EstimatorConfig &c,
                                std::vector<mp::Model> &ms) {
                                mp::lm_refine_batch_host(in, o, c, num_problems, kinds, sample_offsets, sample_idx,
                                                         ms.data(), status);
                            });
}

int mp_debug_lm_system(int variant, int64_t n, const double *x0, const double *x1, const double *d0, const double *d1,
                       const double *min_depth, const double *cam0, const double *cam1,
                       const mp_ransac_options *options, const mp_estimator_config *config, int32_t num_problems,
                       const int32_t *kinds, const int64_t *sample_offsets, const int32_t *sample_idx,
                       const mp_model *models, const double *radius, int32_t where, const int64_t *block_ranges,
                       double *cost, double *g, double *H, int32_t *col, double *d, int32_t *pd, int32_t *status,
                       int device) {
    return guarded([&]() {
        if (!options || num_problems < 0 ||
            (num_problems > 0 && (!sample_offsets || !models || !radius || !cost || !g || !H || !col || !d || !pd ||
                                  !status)))
            throw std::invalid_argument("bad arguments");
        if (num_problems > 0 && sample_offsets[3 * num_problems] > 0 && !sample_idx)
            throw std::invalid_argument("null sample indices");
        const double md0[2] = {0.0, 0.0};
        mp::PairInput in = make_input(variant, n, x0, x1, d0, d1, min_depth ? min_depth : md0, cam0, cam1);
        std::vector<mp::Model> ms(num_problems);
        if (num_problems > 0) std::memcpy(ms.data(), models, sizeof(mp_model) * num_problems);
        std::vector<mp::LmSystem> sys(num_problems);
        mp::lm_system_batch(in, to_opts(options), to_cfg(config), num_problems, kinds, sample_offsets, sample_idx,
                            ms.data(), radius, where, block_ranges, sys.data(), status, device);
        for (int j = 0; j < num_problems; ++j) {
            cost[j] = sys[j].cost;
            std::memcpy(g + 11 * j, sys[j].g, sizeof(sys[j].g));
            std::memcpy(H + 66 * j, sys[j].H, sizeof(sys[j].H));
            std::memcpy(d + 11 * j, sys[j].d, sizeof(sys[j].d));
            for (int a = 0; a < 11; ++a) col[11 * j + a] = sys[j].col[a];
            pd[j] = sys[j].pd;
        }
        return MP_OK;
    });
}

static int point_direct(int kind, const double *x1, const double *x2, mp_model *out, int max_out, int device) {
    if (!x1 || !x2 || (max_out > 0 && !out)) return -fail(MP_EINVAL, "null argument");
    int r = guarded([&]() {
        mp::Model poses[16];
        int np = mp::solve_point_direct(kind, x1, x2, poses, 16, device);
        for (int i = 0; i < std::min(np, max_out); ++i) to_model(poses[i], &out[i]);
        return -(np + 1000);
    });
    return r <= -1000 ? -(r + 1000) : -r;
}

int mp_debug_pt_roots(int variant, int impl, int64_t ns, const double *pts0, const double *pts1, double *cand,
                      int32_t *ncand, int device) {
    if (!pts0 || !pts1 || !cand || !ncand) return fail(MP_EINVAL, "null pointer");
    // impl names the estimator's root stage: 1 for the 5-point (16-lane groups), 3 for
    // the 6-point (deflated eigenproblem), 1 for the 7-point (lane per sample); the
    // round-2 alternates left the library
    if ((variant == 0 && impl != 1) || (variant == 1 && impl != 3) || (variant == 2 && impl != 1) || variant < 0 ||
        variant > 2)
        return fail(MP_EINVAL, "impl must be 1 (5-point group stage, 7-point) or 3 (6-point eigen stage)");
    return guarded([&] {
        mp::debug_pt_roots(variant, ns, pts0, pts1, cand, ncand, device);
        return MP_OK;
    });
}

int mp_debug_pt5_roots(int impl, int64_t ns, const double *pts0, const double *pts1, double *cand, int32_t *ncand,
                       int device) {
    return mp_debug_pt_roots(0, impl, ns, pts0, pts1, cand, ncand, device);
}

int mp_relpose_5pt(const double *x1, const double *x2, mp_model *out, int max_out, int device) {
    return point_direct(0, x1, x2, out, max_out, device);
}

int mp_relpose_6pt_shared_focal(const double *x0, const double *x1, mp_model *out, int max_out, int device) {
    return point_direct(1, x0, x1, out, max_out, device);
}

int mp_relpose_7pt_two_focal(const double *x0, const double *x1, mp_model *out, int max_out, int device) {
    return point_direct(2, x0, x1, out, max_out, device);
}

int mp_debug_random_stream(int kind, uint32_t seed, int32_t a, int32_t b, int32_t count, double *out) {
    if (!out || count < 0) return fail(MP_EINVAL, "bad arguments");
    mp::Mt19937 g(seed);
    for (int i = 0; i < count; ++i) {
        if (kind == 0)
            out[i] = (double)g();
        else if (kind == 1)
            out[i] = (double)mp::uniform_int(g, a, b);
        else if (kind == 2)
            out[i] = mp::uniform_real(g, 0.0, (double)b);
        else if (kind == 3)
            out[i] = (double)mp::uniform_int(g, i % 300, 300 + (i % 17));
        else
            return fail(MP_EINVAL, "bad kind");
    }
    return MP_OK;
}

int mp_debug_iteration_stream(int variant, int32_t n, uint32_t seed, int32_t solver_type, int32_t iterations,
                              int32_t *types, int32_t *idx) {
    if (!types || !idx || iterations < 0 || n <= 0 || variant < 0 || variant > 2)
        return fail(MP_EINVAL, "bad arguments");
    mp::IterationStream rs;
    const int kmd = variant == MP_CALIBRATED ? 3 : 4;
    const int kpt = variant == MP_CALIBRATED ? 5 : (variant == MP_SHARED_FOCAL ? 6 : 7);
    const int ss[2][3] = {{kmd, kmd, 0}, {0, 0, kpt}};
    for (int s = 0; s < 2; ++s)
        for (int t = 0; t < 3; ++t) {
            rs.ss[s][t] = ss[s][t];
            if (ss[s][t] > n) rs.prior[s] = 0.0;
        }
    if (solver_type == 1) rs.prior[0] = 0.0;
    if (solver_type == 2) rs.prior[1] = 0.0;
    rs.n = n;
    rs.seed(seed);
    for (int k = 0; k < iterations; ++k) {
        int tmp[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
        types[k] = rs.next(tmp);
        for (int j = 0; j < 8; ++j) idx[8 * k + j] = tmp[j];
    }
    return MP_OK;
}

int mp_profile_enable(int on) {
    mp::profile_enable(on != 0);
    return MP_OK;
}
int mp_profile_reset(void) {
    mp::profile_reset();
    return MP_OK;
}
int mp_profile_read(mp_kernel_profile *out) {
    if (!out) return MP_EINVAL;
    const mp::KernelProfile p = mp::profile_read();
    out->batches = p.batches;
    out->iterations = p.iterations;
    out->hypotheses = p.hypotheses;
    out->correspondences = p.correspondences;
    out->sweeps = p.sweeps;
    out->solve_ms = p.solve_ms;
    out->score_ms = p.score_ms;
    out->lm_calls = p.lm_calls;
    out->lm_wall_ms = p.lm_wall_ms;
    out->sweep_wall_ms = p.sweep_wall_ms;
    out->sample_wall_ms = p.sample_wall_ms;
    out->wait_wall_ms = p.wait_wall_ms;
    out->run_wall_ms = p.run_wall_ms;
    out->lm_blocks = p.lm_blocks;
    out->lm_big_calls = p.lm_big_calls;
    out->lm_big_wall_ms = p.lm_big_wall_ms;
    out->model_trips = p.model_trips;
    out->model_trips_full = p.model_trips_full;
    out->accepted = p.accepted;
    out->scored = p.scored;
    out->tie_checks = p.tie_checks;
    return MP_OK;
}

const char *mp_last_error(void) { return g_last_error.c_str(); }

int mp_device_count(void) { return mp::device_count(); }

int mp_lo_spin_us(void) { return mp::lo_spin_us(); }

const char *mp_version(void) { return "madpose-mi355x 0.1.0 (gfx950)"; }

} // extern "C"
