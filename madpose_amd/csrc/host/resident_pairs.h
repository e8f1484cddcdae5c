// The resident pairs of a run: the setup shared by refine_batch, select_batch,
// hypothesize_batch and the pair set (mp_pair_set_*).  A fragment of engine.cpp, included
// there once after Problem / make_problem and DevArray: not a stand-alone header.
//
// For a range of np pairs with T correspondences it owns
//   * the 12 T doubles of host/refine_plan.h's layout (refine_row): rows 0 .. 5 uploaded,
//     rows 6 .. 11 derived on the device (calibrated pairs; the other variants read none),
//   * the device PairData[] / PairConst[] records and list_off[],
//   * the list buffers of refine_list, allocated on first use (lists()): hypothesize needs
//     none, select one (3 T ints), refine both (6 T ints, one allocation, halves 3 T apart),
//   * the host copies a stage needs after the inputs are gone: Ch, norm_scale, off, n, and
//     the Problems without their host point arrays (make_lm_job reads the rest).
// Nothing here depends on a call: the lists are scratch that every call rewrites before it
// reads (a sweep writes a pair's lists and returns their lengths), so a ResidentPairs has no
// state a later call could see.
//
// Setup: make_problem and the packing run on up to kPairSetupThreads host threads (each
// pair is independent and writes its own slice; the pool never follows the machine's CPU
// count), the 6 T doubles are staged in one pageable vector and go up in one copy (a
// page-locked staging buffer was measured and did not pay for its allocation),
// and the calibrated rows are derived by one launch_prep_pairs (pair_set_prep_mode 1: one launch_prep_pair per pair, the
// form before; the rows are equal bit for bit, tests/test_pair_set_gpu.py).
#pragma once

// (inside namespace mp, as engine.cpp includes it)
namespace {

constexpr int kPairSetupThreads = 8;              // host threads of make_problem + packing
constexpr int64_t kPairSetupPerThread = 1 << 15;  // correspondences a thread is started for
std::atomic<int> g_pair_set_prep{0};              // 0: one launch, 1: one per pair (pair_set_prep_mode)

// The data-independent part of make_problem, restated for the device ingest (statement for
// statement; make_problem itself keeps its bytes): everything of the Problem that does not
// depend on the correspondences.  What depends on them -- thr, w, the magnitudes, tie_scale,
// the margin constants, the Sampson weight, the scale -- is host/ingest_plan.h ingest_finish.
// min_depth nullable (zeros); cam0, cam1: the pair's 9 or 2 values.
void ingest_static(Problem &P, int variant, int64_t n, const double *min_depth, const double *cam0,
                   const double *cam1, const RansacOptions &o, const EstimatorConfig &cfg) {
#pragma clang fp contract(off)
    PairConst &C = P.C;
    std::memset(&C, 0, sizeof(C));
    C.scale_only = variant == kScaleOnly ? 1 : 0;
    C.variant = C.scale_only ? kCal : variant;
    C.n = (int)n;
    C.score_type = cfg.score_type;
    C.min_depth_constraint = cfg.min_depth_constraint ? 1 : 0;
    C.use_shift = cfg.use_shift ? 1 : 0;
    C.md_alt = C.scale_only ? 0 : (o.use_ours ? 1 : ((o.use_4p4d && variant == kTF) ? 2 : 0));
    C.min_depth[0] = min_depth ? min_depth[0] : 0.0;
    C.min_depth[1] = min_depth ? min_depth[1] : 0.0;
    HostPair &H = P.H;
    H.variant = C.variant;
    H.n = (int)n;
    H.min_depth[0] = C.min_depth[0];
    H.min_depth[1] = C.min_depth[1];
    if (C.variant == kCal) {
        std::memcpy(C.K0, cam0, sizeof(C.K0));
        std::memcpy(C.K1, cam1, sizeof(C.K1));
        inv3(C.K0, C.K0i);
        inv3(C.K1, C.K1i);
        const double s = 1.0 / (C.K0[0] + C.K0[4]) + 1.0 / (C.K1[0] + C.K1[4]);
        C.loss_scale = 1.0 / (s * s);
        auto tri = [](const double *K) { return K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0; };
        C.kstd = (tri(C.K0) && tri(C.K1) && tri(C.K0i) && tri(C.K1i)) ? 1 : 0;
    } else {
        for (int i = 0; i < 9; ++i) C.K0[i] = C.K1[i] = C.K0i[i] = C.K1i[i] = (i % 4 == 0) ? 1.0 : 0.0;
        C.loss_scale = 1.0;
    }
    std::memcpy(H.K0, C.K0, sizeof(H.K0));
    std::memcpy(H.K1, C.K1, sizeof(H.K1));
    std::memcpy(H.K0i, C.K0i, sizeof(H.K0i));
    std::memcpy(H.K1i, C.K1i, sizeof(H.K1i));
    P.norm_scale = 1.0;
}

// A device pointer of the ingest, before anything reads it: device memory of `device`, aligned
// to its element type, and `bytes` bytes from it inside its allocation's address range
// (host/ingest_plan.h ingest_extent_error).  std::invalid_argument naming the argument.
// (an address the runtime has never seen is what a tensor of a SECOND HIP runtime in the process
// looks like: a PyTorch-ROCm wheel loads its own libamdhip64 unless it was imported first)
const char *const kOtherRuntimeHint =
    " (if it belongs to PyTorch: import torch before the first call into this library, so that both use one HIP "
    "runtime -- INTEGRATION.md)";
void check_device_array(const char *name, const void *p, int64_t bytes, int64_t elem, int device) {
    const std::string who = std::string("device array ") + name;
    if (!p) throw std::invalid_argument(who + " is null");
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        throw std::invalid_argument(who + " is not memory this library's HIP runtime knows" + kOtherRuntimeHint);
    }
    if (at.type != hipMemoryTypeDevice)
        throw std::invalid_argument(who + " is not device memory" +
                                    (at.type == hipMemoryTypeUnregistered ? kOtherRuntimeHint : ""));
    if (at.device != device)
        throw std::invalid_argument(who + " is on device " + std::to_string(at.device) + ", the set on device " +
                                    std::to_string(device));
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess) {
        (void)hipGetLastError();
        throw std::invalid_argument(who + " has no allocation range");
    }
    if (const char *why = ingest_extent_error((uint64_t)(uintptr_t)p, (uint64_t)(uintptr_t)base, (uint64_t)size, bytes, elem))
        throw std::invalid_argument(who + " " + why);
}

struct ResidentPairs {
    int variant = 0; // the caller's (kScaleOnly kept)
    int v = 0;       // the kernels' (kScaleOnly runs on the calibrated geometry)
    int np = 0;
    int64_t T = 0;
    std::vector<int64_t> n, off, list_off;
    std::vector<Problem> Ps; // host point arrays dropped
    std::vector<PairConst> Ch;
    std::vector<PairData> Dh;
    std::vector<double> norm_scale;
    DevArray<double> d_data;
    DevArray<PairData> d_D;
    DevArray<PairConst> d_C;
    DevArray<int64_t> d_list_off;

    // offsets: np + 1 values into x0 .. d1 (the range's first pair at offsets[0]); min_depth
    // (nullable: zeros), cam0, cam1: the range's first pair at index 0
    ResidentPairs(hipStream_t stream, int variant_, int32_t np_, const int64_t *offsets, const double *x0,
                  const double *x1, const double *d0, const double *d1, const double *min_depth, const double *cam0,
                  const double *cam1, const RansacOptions &opts, const EstimatorConfig &cfg)
        : variant(variant_), v(variant_ == kScaleOnly ? kCal : variant_), np(np_), T(offsets[np_] - offsets[0]),
          n(np_), off(np_), list_off(np_), Ps(np_), Ch(np_), Dh(np_), norm_scale(np_),
          d_data((size_t)kRefineRows * (size_t)(offsets[np_] - offsets[0])), d_D(np_), d_C(np_), d_list_off(np_) {
        const int nc = (variant == kCal || variant == kScaleOnly) ? 9 : 2;
        // (pageable staging: a page-locked buffer of 6 T doubles costs more to allocate per
        // setup than its faster copy gives back)
        std::vector<double> vec_stage(6 * (size_t)T);
        double *stage = vec_stage.data();
        for (int k = 0; k < np; ++k) {
            n[k] = offsets[k + 1] - offsets[k];
            off[k] = offsets[k] - offsets[0];
            list_off[k] = 3 * off[k];
        }
        // pairs k0 .. k1 - 1: the problem, its slice of the staging buffer, its records
        auto setup = [&](int k0, int k1) {
            for (int k = k0; k < k1; ++k) {
                const int64_t o = offsets[k];
                PairInput in;
                in.variant = variant;
                in.n = n[k];
                in.x0 = x0 + 2 * o;
                in.x1 = x1 + 2 * o;
                in.d0 = d0 + o;
                in.d1 = d1 + o;
                if (min_depth) {
                    in.min_depth[0] = min_depth[2 * (size_t)k];
                    in.min_depth[1] = min_depth[2 * (size_t)k + 1];
                }
                std::memcpy(in.cam0, cam0 + (size_t)nc * k, sizeof(double) * nc);
                std::memcpy(in.cam1, cam1 + (size_t)nc * k, sizeof(double) * nc);
                Problem &P = Ps[k];
                P = make_problem(in, opts, cfg);
                refine_pack_pair(P.H.x0.data(), P.H.x1.data(), P.H.d0.data(), P.H.d1.data(), n[k], off[k], stage);
                // (the host copies are not needed again: every stage runs on the device)
                P.H.x0 = std::vector<double>();
                P.H.x1 = std::vector<double>();
                P.H.d0 = std::vector<double>();
                P.H.d1 = std::vector<double>();
                wire_rows(k);
                Ch[k] = P.C;
                norm_scale[k] = P.norm_scale;
            }
        };
        // contiguous blocks of pairs with about equal correspondences; the first block on
        // this thread.  A pair's results do not depend on the block it falls in.
        // (MADPOSE_PAIR_SETUP_THREADS: fewer threads, for the A/B of tools/pair_set_bench.py)
        const int64_t max_thr = env_int("MADPOSE_PAIR_SETUP_THREADS", kPairSetupThreads, 1, kPairSetupThreads);
        const int nthr =
            (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(max_thr, np), T / kPairSetupPerThread));
        if (nthr <= 1) {
            setup(0, np);
        } else {
            std::vector<int> cut(nthr + 1, np);
            cut[0] = 0;
            for (int t = 1, k = 0; t < nthr; ++t) {
                while (k < np && off[k] < T * t / nthr) ++k;
                cut[t] = k;
            }
            std::vector<std::exception_ptr> errs(nthr);
            std::vector<std::thread> threads;
            auto guarded_setup = [&](int t) {
                try {
                    setup(cut[t], cut[t + 1]);
                } catch (...) {
                    errs[t] = std::current_exception();
                }
            };
            for (int t = 1; t < nthr; ++t) threads.emplace_back(guarded_setup, t);
            guarded_setup(0);
            for (auto &t : threads) t.join();
            for (auto &e : errs)
                if (e) std::rethrow_exception(e);
        }
        if (T > 0) MP_HIP(hipMemcpyAsync(d_data.p, stage, sizeof(double) * 6 * (size_t)T, hipMemcpyHostToDevice, stream));
        if (np > 0) {
            MP_HIP(hipMemcpyAsync(d_D.p, Dh.data(), sizeof(PairData) * np, hipMemcpyHostToDevice, stream));
            MP_HIP(hipMemcpyAsync(d_C.p, Ch.data(), sizeof(PairConst) * np, hipMemcpyHostToDevice, stream));
            MP_HIP(hipMemcpyAsync(d_list_off.p, list_off.data(), sizeof(int64_t) * np, hipMemcpyHostToDevice, stream));
        }
        // pair preparation (the calibrated bearings and rays; the other variants read none)
        prepare_rows(stream);
        // (the staging buffer dies here)
    }

    // The same pairs from arrays that are already on the device (engine.h DevicePairArrays,
    // checked by pair_set_create_device but for the device pointers; host/ingest_plan.h,
    // kernels/ingest_pairs.h).  Before the launches: the data-independent part of every
    // record (ingest_static: make_problem's, restated) and the device pointers' checks.  The
    // kernels write rows 0 .. 5 and the items' statistics; the scales and the statistics (a few
    // dozen bytes a pair) come back, ingest_finish completes the records as make_problem does,
    // and the tail is the first constructor's: records and list offsets up, the calibrated rows
    // by launch_prep_pairs.  Every field, row and record equals the first constructor's on the
    // same numbers (the seven ray maxima of calibrated pairs to the last few bits: the host
    // forms them with its compiler's contraction; tests/test_pair_set_ingest_gpu.py).
    ResidentPairs(hipStream_t stream, int device, int variant_, int32_t np_, const int64_t *offsets,
                  const DevicePairArrays &in, const double *min_depth, const double *cam0, const double *cam1,
                  const RansacOptions &opts, const EstimatorConfig &cfg)
        : variant(variant_), v(variant_ == kScaleOnly ? kCal : variant_), np(np_), T(offsets[np_] - offsets[0]),
          n(np_), off(np_), list_off(np_), Ps(np_), Ch(np_), Dh(np_), norm_scale(np_),
          d_data((size_t)kRefineRows * (size_t)(offsets[np_] - offsets[0])), d_D(np_), d_C(np_), d_list_off(np_) {
        const int nc = (variant == kCal || variant == kScaleOnly) ? 9 : 2;
        const bool cal = v == kCal, use_maps = in.maps != nullptr;
        std::vector<IngestPair> Ih((size_t)np);
        for (int k = 0; k < np; ++k) {
            n[k] = offsets[k + 1] - offsets[k];
            off[k] = offsets[k] - offsets[0];
            list_off[k] = 3 * off[k];
            Problem &P = Ps[k];
            ingest_static(P, variant, n[k], min_depth ? min_depth + 2 * (size_t)k : nullptr, cam0 + (size_t)nc * k,
                          cam1 + (size_t)nc * k, opts, cfg);
            IngestPair &I = Ih[(size_t)k];
            std::memset(&I, 0, sizeof(I));
            I.off = offsets[k];
            I.n = (int)n[k];
            if (cal) {
                std::memcpy(I.cam0, P.C.K0i, sizeof(I.cam0));
                std::memcpy(I.cam1, P.C.K1i, sizeof(I.cam1));
            } else {
                std::memcpy(I.cam0, cam0 + (size_t)nc * k, sizeof(double) * 2);
                std::memcpy(I.cam1, cam1 + (size_t)nc * k, sizeof(double) * 2);
            }
            for (int s = 0; s < 2 && use_maps; ++s) {
                const int32_t m = in.map_ids[2 * (size_t)k + s];
                const int64_t *dm = in.map_dims + 4 * (size_t)m;
                I.map[s] = in.maps[m];
                I.h[s] = dm[0];
                I.w[s] = dm[1];
                I.fx[s] = (double)dm[1] / (double)dm[3]; // get_depths_batch's factors
                I.fy[s] = (double)dm[0] / (double)dm[2];
            }
            wire_rows(k);
        }
        std::vector<IngestItem> items;
        std::vector<int64_t> first_item;
        ingest_items(np, n.data(), items, first_item);
        // (pairs without correspondences: no item, zero statistics, scale 1 as make_problem's)
        std::vector<IngestStats> stats(items.size());
        std::vector<double> scale((size_t)np, 1.0);
        if (T > 0) {
            // ---- every device pointer, before any launch or copy ----
            const int64_t xe = in.xy_type ? 8 : 4, de = in.depth_type ? 8 : 4, me = in.map_type ? 8 : 4;
            check_device_array("x0", in.x0, ingest_bytes(offsets[np], 2, xe), xe, device);
            check_device_array("x1", in.x1, ingest_bytes(offsets[np], 2, xe), xe, device);
            if (use_maps) {
                for (int32_t m = 0; m < in.num_maps; ++m)
                    check_device_array(("depth_maps[" + std::to_string(m) + "]").c_str(), in.maps[m],
                                       ingest_bytes(in.map_dims[4 * (size_t)m], in.map_dims[4 * (size_t)m + 1], me), me,
                                       device);
            } else {
                check_device_array("d0", in.d0, ingest_bytes(offsets[np], 1, de), de, device);
                check_device_array("d1", in.d1, ingest_bytes(offsets[np], 1, de), de, device);
            }
            // ---- the producer's work first: an event on its stream, no host wait ----
            struct Event { // (destroyed after this block's synchronise, or on its way out)
                hipEvent_t ev = nullptr;
                ~Event() {
                    if (ev) (void)hipEventDestroy(ev);
                }
            } produced;
            MP_HIP(hipEventCreateWithFlags(&produced.ev, hipEventDisableTiming));
            MP_HIP(hipEventRecord(produced.ev, static_cast<hipStream_t>(in.producer_stream)));
            MP_HIP(hipStreamWaitEvent(stream, produced.ev, 0));
            IngestArgs A;
            A.x0 = in.x0;
            A.x1 = in.x1;
            A.d0 = use_maps ? nullptr : in.d0;
            A.d1 = use_maps ? nullptr : in.d1;
            A.xtype = in.xy_type;
            A.dtype = in.depth_type;
            A.mtype = in.map_type;
            A.cal = cal ? 1 : 0;
            DevArray<IngestPair> d_I((size_t)np);
            DevArray<IngestItem> d_items(items.size());
            DevArray<IngestStats> d_stats(items.size());
            DevArray<double> d_scale((size_t)np);
            MP_HIP(hipMemcpyAsync(d_I.p, Ih.data(), sizeof(IngestPair) * np, hipMemcpyHostToDevice, stream));
            MP_HIP(hipMemcpyAsync(d_items.p, items.data(), sizeof(IngestItem) * items.size(), hipMemcpyHostToDevice,
                                  stream));
            MP_HIP(hipMemcpyAsync(d_D.p, Dh.data(), sizeof(PairData) * np, hipMemcpyHostToDevice, stream));
            if (!cal) MP_HIP(launch_ingest_scale(stream, A, d_I.p, np, d_scale.p));
            MP_HIP(launch_ingest_rows(stream, A, d_items.p, (int)items.size(), d_I.p, d_D.p, cal ? nullptr : d_scale.p,
                                      d_stats.p));
            MP_HIP(hipMemcpyAsync(stats.data(), d_stats.p, sizeof(IngestStats) * items.size(), hipMemcpyDeviceToHost,
                                  stream));
            if (!cal)
                MP_HIP(hipMemcpyAsync(scale.data(), d_scale.p, sizeof(double) * np, hipMemcpyDeviceToHost, stream));
            MP_HIP(hipStreamSynchronize(stream)); // (the caller's arrays are not read after this)
        } else if (np > 0) {
            MP_HIP(hipMemcpyAsync(d_D.p, Dh.data(), sizeof(PairData) * np, hipMemcpyHostToDevice, stream));
        }
        // ---- the records, finished from the statistics ----
        const double tie = env_real("MADPOSE_TIE_SCALE", 1.0, 1.0, 1e300);
        for (int k = 0; k < np; ++k) {
            IngestStats S;
            std::memset(&S, 0, sizeof(S));
            for (int64_t j = first_item[(size_t)k]; j < first_item[(size_t)k + 1]; ++j) ingest_merge(S, stats[(size_t)j]);
            Problem &P = Ps[k];
            P.norm_scale = cal ? 1.0 : scale[(size_t)k];
            P.H.sampson_squared_weight =
                ingest_finish(P.C, S, P.norm_scale, opts.squared_inlier_thresholds[0], opts.squared_inlier_thresholds[1],
                              opts.data_type_weights[0], opts.data_type_weights[1], tie);
            Ch[k] = P.C;
            norm_scale[k] = P.norm_scale;
        }
        if (np > 0) {
            MP_HIP(hipMemcpyAsync(d_C.p, Ch.data(), sizeof(PairConst) * np, hipMemcpyHostToDevice, stream));
            MP_HIP(hipMemcpyAsync(d_list_off.p, list_off.data(), sizeof(int64_t) * np, hipMemcpyHostToDevice, stream));
        }
        prepare_rows(stream);
    }

    // the list buffers: nbuf (1, 2) buffers of 3 T ints, buffer b at lists + b 3 T.  Per-call
    // scratch: growing from one buffer to two keeps no contents.
    int *lists(int nbuf) {
        if (nbuf > lists_nbuf_) {
            d_lists_.reset(); // (free first: a set may be close to the device's memory)
            d_lists_.reset(new DevArray<int>((size_t)nbuf * 3 * (size_t)T));
            lists_nbuf_ = nbuf;
        }
        return d_lists_->p;
    }
    // bytes per correspondence held on the device: the rows and the list buffers there are
    int64_t resident_bytes() const { return T * (kRefineRows * 8 + lists_nbuf_ * 3 * 4); }

  private:
    // pair k's PairData: the twelve rows of refine_row's layout in the set's allocation
    void wire_rows(int k) {
        const double *rows[kRefineRows];
        for (int r = 0; r < kRefineRows; ++r) rows[r] = d_data.p + refine_row(T, off[k], n[k], r);
        PairData &D = Dh[k];
        D.x0u = rows[0];
        D.x0v = rows[1];
        D.x1u = rows[2];
        D.x1v = rows[3];
        D.d0 = rows[4];
        D.d1 = rows[5];
        D.r0 = rows[6];
        D.r1 = rows[7];
        D.a0 = rows[8];
        D.a1 = rows[9];
        D.b0 = rows[10];
        D.b1 = rows[11];
    }
    // The end of both constructors, after the records and rows 0 .. 5 are on the device: rows
    // 6 .. 11 of calibrated geometry (one launch_prep_pairs; pair_set_prep_mode 1: one
    // launch_prep_pair per pair), then the stream is waited for.
    void prepare_rows(hipStream_t stream) {
        std::unique_ptr<DevArray<PrepItem>> d_items;
        std::vector<PrepItem> items;
        if (v == kCal && T > 0) {
            if (g_pair_set_prep.load() == 0) {
                prep_items(np, n.data(), items);
                d_items.reset(new DevArray<PrepItem>(items.size()));
                MP_HIP(hipMemcpyAsync(d_items->p, items.data(), sizeof(PrepItem) * items.size(), hipMemcpyHostToDevice,
                                      stream));
                MP_HIP(launch_prep_pairs(stream, d_D.p, d_C.p, d_items->p, (int)items.size()));
            } else {
                for (int k = 0; k < np; ++k) {
                    auto row = [&](int r) { return d_data.p + refine_row(T, off[k], n[k], r); };
                    MP_HIP(launch_prep_pair(stream, Ch[k], Dh[k], row(6), row(7), row(8), row(9), row(10), row(11)));
                }
            }
        }
        // (the items die here)
        MP_HIP(hipStreamSynchronize(stream));
    }
    std::unique_ptr<DevArray<int>> d_lists_;
    int lists_nbuf_ = 0;
};

// The pairs a call runs on: positions 0 .. n - 1, entry j the pair (*this)[j] of the
// ResidentPairs (ids null: all pairs in order).  Checked by check_selection before.
struct PairSel {
    int n;
    const int32_t *ids;
    int operator[](int j) const { return ids ? ids[j] : j; }
};

} // namespace
