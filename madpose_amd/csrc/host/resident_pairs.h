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
        // (the staging buffers and the items die here)
        MP_HIP(hipStreamSynchronize(stream));
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
