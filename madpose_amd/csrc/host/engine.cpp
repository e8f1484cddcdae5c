// Host controller of the MI355X hybrid LO-MSAC estimator.
//
// Semantics follow HybridLOMSAC::EstimateModel (src/hybrid_ransac.h:38-206) step for
// step; the difference is WHERE the work runs.  The reference draws one minimal
// sample, solves it and scores its models over all 3N residuals before drawing the
// next.  Here the controller replays the reference's two random streams
// (sampler mt19937, solver-selection/LO mt19937, both seeded with random_seed) to
// generate a *speculative batch* of B iterations, assuming no local optimisation
// happens inside the batch; the GPU solves every sample and scores every model of
// the batch in one pass; the host then scans the per-iteration best scores in
// order, reproducing the sequential decisions exactly.  The only event that
// invalidates the rest of a batch is an LO run (it consumes the selection stream);
// the controller then rewinds both streams to the end of that iteration, runs LO
// and starts the next batch there.  New-best events before lo_starting_iterations
// do not consume randomness and do not cut the batch.  Results are therefore
// independent of the batch size (tests/test_engine_gpu.py checks this).
//
// Local optimisation stays on the host (north star); its full-data sweeps
// (ScoreModel / GetInliers) run on the GPU through the single-model sweep kernel.
#include <fcntl.h>
#include <immintrin.h>
#include <signal.h>
#include <unistd.h>
#include "engine.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>

#include "../include/mp_draw_weights.h"
#include "../include/mp_score.h"
#include "../kernels/kernels.h"
#include "batch_draw.h"
#include "candidates_plan.h"
#include "env.h"
#include "hypothesis_plan.h"
#include "lo_sweep.h"
#include "lsq_fit_plan.h"
#include "pair_set_plan.h"
#include "ransac_lo_steps.h"
#include "ransac_lo_track.h"
#include "ransac_stop.h"
#include "refine_plan.h"
#include "select_plan.h"
#include "rng.h"
#include "solve_batch_pack.h"

namespace mp {

// kCompactLut[m]: the lane numbers of the set bits of the 4-bit mask m, ascending
// (inliers(): AVX2 stream compaction of the error rows)
alignas(16) static const int32_t kCompactLut[16][4] = {
    {0, 0, 0, 0}, {0, 0, 0, 0}, {1, 0, 0, 0}, {0, 1, 0, 0}, {2, 0, 0, 0}, {0, 2, 0, 0}, {1, 2, 0, 0}, {0, 1, 2, 0},
    {3, 0, 0, 0}, {0, 3, 0, 0}, {1, 3, 0, 0}, {0, 1, 3, 0}, {2, 3, 0, 0}, {0, 2, 3, 0}, {1, 2, 3, 0}, {0, 1, 2, 3}};

#define MP_HIP(expr)                                                                                                    \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr);               \
    } while (0)

namespace {

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a) { return std::chrono::duration<double>(Clock::now() - a).count(); }

const double kMax = DBL_MAX;

// Minimal-sample batches and their drawing: batch_draw.h.  MADPOSE_SAMPLER_TWO_PASS=0
// keeps the draw-by-draw loop for hybrid batches too, MADPOSE_SAMPLER_SIMD=0 the scalar
// two passes (A/B; identical draws).
int sampler_mode() {
    static const int mode = [] {
        if (!env_flag("MADPOSE_SAMPLER_TWO_PASS", true)) return 0;
        return env_flag("MADPOSE_SAMPLER_SIMD", true) ? 2 : 1;
    }();
    return mode;
}

// Background sampler: draws the next speculative batch while the current one is on
// the GPU and the host replays it / runs LO.  The batch is kept only if the current
// one neither triggers LO nor terminates, so the worker can be told to give up.
class Sampler {
  public:
    Sampler() : th_([this] { loop(); }) {}
    ~Sampler() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_ = true;
            abort_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    // starts drawing B iterations from `from` into *g (the caller must not touch *g
    // or the slot memory until finish()/cancel() returned); `after` runs on the worker
    // once the batch is drawn (the post-LO speculation launches it on the GPU there)
    // chain (nullable): a second batch for the same job -- once *g is drawn (and `after`
    // ran), chain->B more iterations are drawn from where it ended into chain->g (the
    // post-LO speculation's successor, drawn while the LO runs; only drawn: host work)
    struct Chain {
        Batch *g;
        uint32_t B;
        int slot;
        int *smp;
    };
    void start(const IterationStream &from, Batch *g, uint32_t B, int slot, int *smp,
               std::function<void()> after = nullptr, const Chain *chain = nullptr) {
        std::unique_lock<std::mutex> lk(mu_);
        if (busy_) { // a chained batch nobody asked for (chained()) is still being drawn
            abort_ = true;
            done_cv_.wait(lk, [this] { return !busy_; });
        }
        g2_ = chain ? chain->g : nullptr;
        B2_ = chain ? chain->B : 0;
        slot2_ = chain ? chain->slot : 0;
        smp2_ = chain ? chain->smp : nullptr;
        ok2_ = false;
        after_ = std::move(after);
        err_ = nullptr;
        rs_ = from;
        g_ = g;
        B_ = B;
        slot_ = slot;
        smp_ = smp;
        abort_ = false;
        busy_ = busy1_ = true;
        ok_ = false;
        ++gen_;
        cv_.notify_all();
    }
    // after finish(): waits for the chained batch (the rest of the job); whether it was
    // drawn, *rs the stream state after it
    bool chained(IterationStream *rs) {
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [this] { return !busy_; });
        if (ok2_) *rs = rs2_;
        return ok2_;
    }
    // waits for the batch (not for a chained one: that is drawn on while the caller reads
    // this one, until chained(), cancel() or the next start()); on success *rs is the
    // stream state after it
    bool finish(IterationStream *rs) {
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [this] { return !busy1_; });
        if (err_) std::rethrow_exception(err_);
        if (ok_) *rs = rs1_;
        return ok_;
    }
    void cancel() {
        abort_ = true;
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [this] { return !busy_; });
    }

  private:
    void loop() {
        uint64_t seen = 0;
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return quit_ || gen_ != seen; });
            if (quit_) return;
            seen = gen_;
            lk.unlock();
            const bool ok = draw_batch(rs_, *g_, B_, slot_, smp_, &abort_, sampler_mode());
            std::exception_ptr err;
            if (ok && after_) {
                try {
                    after_();
                } catch (...) {
                    err = std::current_exception();
                }
            }
            Batch *const g2 = g2_; // (set with the job, under the lock)
            lk.lock();
            rs1_ = rs_;
            err_ = err;
            ok_ = ok;
            busy1_ = false; // finish() returns here: the chained batch is drawn after it
            ok2_ = false;
            const bool go2 = ok && !err && g2;
            if (!go2) busy_ = false;
            done_cv_.notify_all();
            if (!go2) continue;
            lk.unlock();
            IterationStream r2 = rs_;
            const bool ok2 = draw_batch(r2, *g2, B2_, slot2_, smp2_, &abort_, sampler_mode());
            lk.lock();
            rs2_ = r2;
            ok2_ = ok2;
            busy_ = false;
            done_cv_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    IterationStream rs_;
    Batch *g_ = nullptr;
    uint32_t B_ = 0;
    int slot_ = 0;
    int *smp_ = nullptr;
    std::function<void()> after_;
    Batch *g2_ = nullptr;
    uint32_t B2_ = 0;
    int slot2_ = 0;
    int *smp2_ = nullptr;
    IterationStream rs1_, rs2_; // the streams after the batch / after the chained one
    bool ok2_ = false;
    std::exception_ptr err_;
    std::atomic<bool> abort_{false};
    bool busy_ = false, busy1_ = false, ok_ = false, quit_ = false; // busy1_: the first batch is drawing
    uint64_t gen_ = 0;
    std::thread th_;
};

// ---------------------------------------------------------------------------
// Device resources of one LO lane (the estimator thread or an LO worker): a stream and
// the staging of the opt-in device LM (MADPOSE_DEVICE_LM).  The LO sweeps themselves
// run on the lane's own core (host/lo_sweep.h).
struct SweepSlot {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    // device-LM staging: job + index lists up, model + status down
    int64_t lm_cap = 0;
    char *h_lm = nullptr, *d_lm = nullptr;
    hipEvent_t lm_done = nullptr; // blocking-sync event: the waiting thread sleeps

    void ensure_lm(int64_t nidx) {
        if (!stream) {
            MP_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            own_stream = true;
        }
        if (!lm_done) MP_HIP(hipEventCreateWithFlags(&lm_done, hipEventBlockingSync | hipEventDisableTiming));
        if (nidx <= lm_cap) return;
        if (h_lm) hipHostFree(h_lm);
        if (d_lm) hipFree(d_lm);
        h_lm = d_lm = nullptr;
        lm_cap = 0;
        const size_t bytes = lm_bytes(nidx);
        MP_HIP(hipHostMalloc(&h_lm, bytes, hipHostMallocDefault));
        MP_HIP(hipMalloc(&d_lm, bytes));
        lm_cap = nidx;
    }
    // layout: LmJob | Model out | int status | pad | int idx[nidx]
    static size_t lm_bytes(int64_t nidx) { return 512 + sizeof(int) * (size_t)nidx; }
};

int active_runs(int device);

// Worker threads for the parallel LO steps: run(n, f) calls f(job, lane) for jobs
// 0..n-1, lane 0 being the calling thread and lanes 1..size-1 the workers.  While the
// estimator has its device to itself, the workers spin (with pause, bounded by
// lo_spin_us() as the LM pool's) before they block, and so does the caller at the
// join: a futex wake-up per worker per LO delayed the steps of each LO by ~30 us
// (steps phase 230 us for a 200 us longest step, profiles/r04/lotab).  With other
// estimators on the device they block at once (their threads share the CPUs).
// MADPOSE_LO_WORKER_SPIN=0 turns the spinning off.
class LoWorkers {
  public:
    LoWorkers(int lanes, int device) : device_(device) {
        // microseconds (MADPOSE_LO_WORKER_SPIN; 0: block at once); default 2000 -- the
        // LO runs of a pair come ~0.3-1 ms apart, so a shorter spin sleeps through the
        // gap -- or 0 where the LM pool does not spin either (a small CPU share per rank)
        spin_ns_ = 1000ll * env_int("MADPOSE_LO_WORKER_SPIN", lo_spin_us() > 0 ? 2000 : 0, 0, 1000000);
        for (int i = 1; i < lanes; ++i) th_.emplace_back([this, i] { loop(i); });
    }
    ~LoWorkers() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            quit_.store(true);
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    int lanes() const { return (int)th_.size() + 1; }
    void run(int n, const std::function<void(int, int)> &f) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            f_ = &f;
            n_ = n;
            next_.store(0);
            active_.store((int)th_.size());
            err_ = nullptr;
            gen_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
        work(0);
        if (!spin_until([this] { return active_.load(std::memory_order_acquire) == 0; })) {
            std::unique_lock<std::mutex> lk(mu_);
            done_cv_.wait(lk, [this] { return active_.load(std::memory_order_acquire) == 0; });
        }
        f_ = nullptr;
        if (err_) std::rethrow_exception(err_);
    }

  private:
    // polls ready() with pause for at most spin_ns_ (none with other estimators on the
    // device); true once it held
    template <class F> bool spin_until(const F &ready) const {
        if (spin_ns_ <= 0 || active_runs(device_) > 1) return ready();
        const auto t0 = Clock::now();
        for (int k = 0;; ++k) {
            if (ready()) return true;
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
            if ((k & 63) == 63 &&
                std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t0).count() > spin_ns_)
                return ready();
        }
    }
    void work(int lane) {
        for (int k; (k = next_.fetch_add(1)) < n_;) {
            try {
                (*f_)(k, lane);
            } catch (...) {
                std::lock_guard<std::mutex> lk(err_mu_);
                if (!err_) err_ = std::current_exception();
            }
        }
    }
    void loop(int lane) {
        uint64_t seen = 0;
        for (;;) {
            if (!spin_until([&] { return quit_.load() || gen_.load(std::memory_order_acquire) != seen; })) {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return quit_.load() || gen_.load(std::memory_order_acquire) != seen; });
            }
            {
                std::lock_guard<std::mutex> lk(mu_); // (pairs with run()'s publication)
                if (quit_.load()) return;
                seen = gen_.load(std::memory_order_relaxed);
            }
            work(lane);
            if (active_.fetch_sub(1, std::memory_order_acq_rel) == 1) {
                std::lock_guard<std::mutex> lk(mu_);
                done_cv_.notify_one();
            }
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_, err_mu_;
    std::condition_variable cv_, done_cv_;
    const std::function<void(int, int)> *f_ = nullptr;
    int n_ = 0;
    std::atomic<int> active_{0};
    std::atomic<int> next_{0};
    std::atomic<uint64_t> gen_{0};
    std::atomic<bool> quit_{false};
    std::exception_ptr err_;
    int device_ = 0;
    long long spin_ns_ = 0;
};

constexpr int kLoLanes = 12; // most concurrent LO steps (and sweep slots) per context

// concurrent LO steps of one estimator (MADPOSE_LO_LANES, 1..kLoLanes): the default
// is 4 lanes; see DESIGN.md §8 for the measurements behind it
inline int lo_lanes_setting() {
    static const int v = [] {
        return (int)env_int("MADPOSE_LO_LANES", 4, 1, kLoLanes);
    }();
    return v;
}

// ---------------------------------------------------------------------------
// Device context: stream + cached buffers (one per device and concurrent caller)
//
// The per-batch buffers come in two slots (BatchBufs), the slot of a batch being the
// host sample slot it was drawn into: the next batch is drawn into the other slot while
// this one is on the GPU, and the post-LO speculation is launched from there while the
// host still works on this one's results (Run::run).
struct BatchBufs {
    int *d_counts = nullptr;
    IterResult *d_res = nullptr;
    int *d_work = nullptr, *h_work = nullptr; // score_batch's evaluated (model, trip) pairs per iteration
    // the walk's inputs (ScoreBound::flags8 / cand_out): one byte per iteration (model
    // count | 0x80 for a possible new best), copied back; the IterResults of the marked
    // iterations, written by score_batch into mapped memory
    uint8_t *d_flags8 = nullptr, *h_flags8 = nullptr;
    IterResult *h_cand = nullptr, *d_cand = nullptr;

    Model *d_models = nullptr;
    ScoreRec *d_recs = nullptr;
    double *d_scores = nullptr;
    // score_batch writes the models of the iterations that beat the pre-batch best here
    // (mapped pinned memory, one slot per iteration of the batch)
    Model *h_recmodel = nullptr, *d_recmodel = nullptr;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr}; // solve start / score start / score end
    hipEvent_t ev_fork = nullptr, ev_join = nullptr; // MD side stream fork / join
    hipEvent_t ev_h2d = nullptr;                    // the batch's samples have been copied
    hipEvent_t ev_solved = nullptr;                 // the batch's solver kernels are done
    hipEvent_t ev_done = nullptr;                   // the batch's results are on the host
    // each slot's batches run on the slot's stream from the slot's sample buffer; a
    // batch waits for the other slot's ev_solved before it solves (the point solvers'
    // workspace and the MD side stream are shared)
    hipStream_t stream = nullptr;
    int *d_samples = nullptr;
    unsigned epoch_hi = 0;                          // ~epoch of the batch last launched here
    bool h2d_pending = false;                       // launched, ev_h2d not yet waited for
};

struct DeviceCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t cap_n = 0;
    int cap_b = 0, cap_m = 0;
    double *d_pair = nullptr; // 12 arrays of cap_n (PairData)
    // score_batch's record word (kernels.hip ScoreBound::rec) and the batch epoch
    unsigned long long *d_recword = nullptr;
    uint32_t epoch = 0;
    BatchBufs bb[2];
    ScoreRec *d_rec1 = nullptr;
    double *d_err = nullptr, *d_score1 = nullptr;
    // staged point-solver workspace (kernels.h PtWorkspace)
    double *d_pt_cand = nullptr, *d_pt_pen = nullptr;
    int *d_pt_ncand = nullptr, *d_pt_valid = nullptr;
    Model *d_pt_slots = nullptr;
    // the two-stage exact MD solver's per-sample state (kernels.h kMdWsStride, SoA, ld cap_b)
    double *d_md_ws = nullptr;
    int *d_md_nr = nullptr;
    // device resources of the LO lanes (lane 0: the estimator thread)
    SweepSlot sweep_slot[kLoLanes];
    std::unique_ptr<LoWorkers> lo_workers; // created on first parallel LO
    // pinned host mirrors
    int *h_samples = nullptr; // two slots of 9 * max_batch ints
    double *h_err = nullptr, *h_score1 = nullptr;
    ScoreRec *h_rec1 = nullptr;
    Model *h_model1 = nullptr;
    // the MD solver runs on md_stream, concurrently with the point-solver stages; host
    // reads of a finished batch's device data go through copy_stream (the main stream
    // may already hold the next batch)
    hipStream_t md_stream = nullptr, copy_stream = nullptr;
    std::unique_ptr<Sampler> sampler;               // created on first use
    // one block for the rounds of the batched minimal solvers (solve_md_batch,
    // relpose_batch), grown on demand and kept with the context; not sized by ensure()
    char *d_solve = nullptr;
    size_t solve_cap = 0;
    char *solve_block(size_t bytes) {
        if (bytes > solve_cap) {
            MP_HIP(hipStreamSynchronize(stream));
            if (d_solve) MP_HIP(hipFree(d_solve));
            d_solve = nullptr;
            solve_cap = 0;
            MP_HIP(hipMalloc(&d_solve, bytes));
            solve_cap = bytes;
        }
        return d_solve;
    }

    void free_all() {
        hipSetDevice(device);
        for (void *p : {(void *)d_pair, (void *)bb[0].d_samples, (void *)bb[1].d_samples, (void *)d_recword, (void *)d_rec1, (void *)d_err,
                        (void *)d_score1, (void *)d_pt_cand, (void *)d_pt_pen, (void *)d_pt_ncand, (void *)d_pt_valid,
                        (void *)d_pt_slots, (void *)d_md_ws, (void *)d_md_nr})
            if (p) hipFree(p);
        for (void *p : {(void *)h_samples, (void *)h_err, (void *)h_score1, (void *)h_rec1, (void *)h_model1})
            if (p) hipHostFree(p);
        for (BatchBufs &q : bb) {
            for (void *p : {(void *)q.d_counts, (void *)q.d_res, (void *)q.d_work, (void *)q.d_models,
                            (void *)q.d_recs, (void *)q.d_scores, (void *)q.d_flags8})
                if (p) hipFree(p);
            for (void *p : {(void *)q.h_flags8, (void *)q.h_cand, (void *)q.h_work, (void *)q.h_recmodel})
                if (p) hipHostFree(p);
            q.d_counts = q.d_work = q.h_work = nullptr;
            q.d_res = q.h_cand = q.d_cand = nullptr;
            q.d_flags8 = q.h_flags8 = nullptr;
            q.d_models = q.h_recmodel = q.d_recmodel = nullptr;
            q.d_recs = nullptr;
            q.d_scores = nullptr;
            q.h2d_pending = false;
        }
        d_pair = d_err = d_score1 = nullptr;
        bb[0].d_samples = bb[1].d_samples = nullptr;
        d_recword = nullptr;
        d_rec1 = nullptr;
        d_pt_cand = d_pt_pen = nullptr;
        d_pt_ncand = d_pt_valid = nullptr;
        d_pt_slots = nullptr;
        d_md_ws = nullptr;
        d_md_nr = nullptr;
        h_samples = nullptr;
        h_err = h_score1 = nullptr;
        h_rec1 = nullptr;
        h_model1 = nullptr;
        cap_n = 0;
        cap_b = cap_m = 0;
    }

    void ensure(int64_t n, int B, int M) {
        if (n <= cap_n && B <= cap_b && M <= cap_m) return;
        const int64_t nn = std::max<int64_t>(std::max<int64_t>(n, cap_n), 64);
        const int bb_ = std::max(B, cap_b), mm = std::max(M, cap_m);
        MP_HIP(hipSetDevice(device));
        MP_HIP(hipDeviceSynchronize()); // (a batch of an unwound run may still use the old buffers)
        free_all();
        MP_HIP(hipMalloc(&d_pair, sizeof(double) * 12 * nn));
        MP_HIP(hipMalloc(&d_err, sizeof(double) * 3 * nn));
        for (BatchBufs &q : bb) MP_HIP(hipMalloc(&q.d_samples, sizeof(int) * 9 * bb_));
        MP_HIP(hipMalloc(&d_recword, sizeof(unsigned long long)));
        MP_HIP(hipMemset(d_recword, 0xff, sizeof(unsigned long long)));
        for (BatchBufs &q : bb) {
            MP_HIP(hipMalloc(&q.d_counts, sizeof(int) * bb_));
            MP_HIP(hipMalloc(&q.d_res, sizeof(IterResult) * bb_));
            MP_HIP(hipMalloc(&q.d_work, sizeof(int) * bb_));
            MP_HIP(hipMalloc(&q.d_models, sizeof(Model) * (size_t)bb_ * mm));
            MP_HIP(hipMalloc(&q.d_recs, sizeof(ScoreRec) * (size_t)bb_ * mm));
            MP_HIP(hipMalloc(&q.d_scores, sizeof(double) * (size_t)bb_ * mm));
            // (score_batch writes a byte per iteration to device memory and one copy
            // brings them over; writing every workgroup's result to mapped host memory
            // made the kernel 51 -> 63 us per cal launch, profiles/r05/r5j -- only the
            // few marked iterations write theirs there)
            MP_HIP(hipMalloc(&q.d_flags8, (size_t)bb_));
            MP_HIP(hipHostMalloc(&q.h_flags8, (size_t)bb_, hipHostMallocDefault));
            MP_HIP(hipHostMalloc(&q.h_cand, sizeof(IterResult) * bb_, hipHostMallocMapped | hipHostMallocCoherent));
            MP_HIP(hipHostGetDevicePointer((void **)&q.d_cand, q.h_cand, 0));
            MP_HIP(hipHostMalloc(&q.h_work, sizeof(int) * bb_, hipHostMallocDefault));
            MP_HIP(hipHostMalloc(&q.h_recmodel, sizeof(Model) * (size_t)bb_,
                                 hipHostMallocMapped | hipHostMallocCoherent));
            MP_HIP(hipHostGetDevicePointer((void **)&q.d_recmodel, q.h_recmodel, 0));
        }
        MP_HIP(hipMalloc(&d_rec1, sizeof(ScoreRec) * 64));
        MP_HIP(hipMalloc(&d_pt_cand, sizeof(double) * (size_t)bb_ * kPtCandStride));
        // (the pencil workspace of the shared-focal root stage; a stub elsewhere)
        MP_HIP(hipMalloc(&d_pt_pen, sizeof(double) * (mm == kMaxModelsSF ? (size_t)bb_ * kPtPenStride : 1)));
        MP_HIP(hipMalloc(&d_pt_ncand, sizeof(int) * (size_t)bb_));
        MP_HIP(hipMalloc(&d_pt_valid, sizeof(int) * (size_t)bb_ * kPtSlotStride));
        MP_HIP(hipMalloc(&d_pt_slots, sizeof(Model) * (size_t)bb_ * kPtSlotStride));
        MP_HIP(hipMalloc(&d_md_ws, sizeof(double) * (size_t)bb_ * kMdWsStride));
        MP_HIP(hipMalloc(&d_md_nr, sizeof(int) * (size_t)bb_));
        MP_HIP(hipMalloc(&d_score1, sizeof(double) * 64));
        // two slots each: the next batch is generated while the current one is in flight
        MP_HIP(hipHostMalloc(&h_samples, sizeof(int) * 2 * 9 * bb_, hipHostMallocDefault));
        MP_HIP(hipHostMalloc(&h_err, sizeof(double) * 3 * nn, hipHostMallocDefault));
        MP_HIP(hipHostMalloc(&h_score1, sizeof(double) * 64, hipHostMallocDefault));
        MP_HIP(hipHostMalloc(&h_rec1, sizeof(ScoreRec) * 64, hipHostMallocDefault));
        MP_HIP(hipHostMalloc(&h_model1, sizeof(Model) * 64, hipHostMallocDefault));
        cap_n = nn;
        cap_b = bb_;
        cap_m = mm;
    }
};

std::mutex g_pool_mu;
std::vector<DeviceCtx *> g_pool;

// Process teardown: the pooled (idle) contexts' host threads -- each context's sampler
// and LO workers -- are stopped and joined before the HIP runtime's own teardown (this
// library's static destructors run first: it is loaded after libamdhip64).  A context
// leased by an estimator still running at exit is not in the pool and is left alone.
// The device buffers are not freed: the process is ending.
struct PoolReaper {
    ~PoolReaper() {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (DeviceCtx *c : g_pool) {
            c->sampler.reset();
            c->lo_workers.reset();
        }
    }
} g_pool_reaper;

// The live pair sets (mp_pair_set_create .. destroy).  At process teardown the sets still
// open are released while the HIP runtime is alive and before the pooled contexts go
// (g_set_reaper is defined after g_pool_reaper, so it is destroyed first): a process that
// exits with a set open exits cleanly.
std::mutex g_sets_mu;
std::vector<PairSet *> g_sets;
// the live confidence-weight handles (mp_draw_weights_create .. destroy), of every set
std::mutex g_weights_mu;
std::vector<DrawWeights *> g_weights;
void release_live_sets();
struct SetReaper {
    ~SetReaper() { release_live_sets(); }
} g_set_reaper;

// MADPOSE_SEGV_MAPS (diagnostic, presence): on SIGSEGV / SIGBUS write the fault address
// and /proc/self/maps to stderr, then hand the signal to the handler installed before
// (a profiler's stack printer, or the default action).  Async-signal-safe: open / read /
// write only.
struct sigaction g_old_segv, g_old_bus;
void segv_maps_handler(int sig, siginfo_t *si, void *uc) {
    char buf[4096];
    static const char hex[] = "0123456789abcdef";
    int k = 0;
    const char *hdr = "[madpose] fault address 0x";
    while (*hdr) buf[k++] = *hdr++;
    const unsigned long long a = (unsigned long long)(uintptr_t)(si ? si->si_addr : nullptr);
    for (int sh = 60; sh >= 0; sh -= 4) buf[k++] = hex[(a >> sh) & 15];
    const char *tail = ", /proc/self/maps:\n";
    while (*tail) buf[k++] = *tail++;
    ssize_t w = write(2, buf, (size_t)k);
    const int fd = open("/proc/self/maps", O_RDONLY);
    if (fd >= 0) {
        ssize_t r;
        while ((r = read(fd, buf, sizeof(buf))) > 0) w = write(2, buf, (size_t)r);
        close(fd);
    }
    (void)w;
    const struct sigaction &old = sig == SIGBUS ? g_old_bus : g_old_segv;
    if (old.sa_flags & SA_SIGINFO) {
        old.sa_sigaction(sig, si, uc);
    } else if (old.sa_handler != SIG_IGN && old.sa_handler != SIG_DFL) {
        old.sa_handler(sig);
    } else {
        signal(sig, SIG_DFL);
        raise(sig);
    }
}
void install_segv_maps() {
    static std::once_flag once;
    std::call_once(once, [] {
        if (!std::getenv("MADPOSE_SEGV_MAPS")) return;
        struct sigaction sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.sa_sigaction = segv_maps_handler;
        sa.sa_flags = SA_SIGINFO;
        sigemptyset(&sa.sa_mask);
        sigaction(SIGSEGV, &sa, &g_old_segv);
        sigaction(SIGBUS, &sa, &g_old_bus);
    });
}

std::atomic<bool> g_prof_on{false};
std::mutex g_prof_mu;
KernelProfile g_prof;

// estimators running on each device (leases held): the LO workers spin for their jobs
// only while one estimator has the device to itself (LoWorkers::spin_until)
constexpr int kMaxDevices = 64;
std::atomic<int> g_active_runs[kMaxDevices];
int active_runs(int device) {
    return device >= 0 && device < kMaxDevices ? g_active_runs[device].load(std::memory_order_relaxed) : 1;
}

struct CtxLease {
    DeviceCtx *c = nullptr;
    explicit CtxLease(int device) {
        install_segv_maps();
        {
            std::lock_guard<std::mutex> lk(g_pool_mu);
            for (size_t i = 0; i < g_pool.size(); ++i)
                if (g_pool[i]->device == device) {
                    c = g_pool[i];
                    g_pool.erase(g_pool.begin() + i);
                    break;
                }
        }
        if (!c) {
            int cnt = 0;
            if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
                throw std::runtime_error("no HIP device available (MI355X required; there is no CPU fallback)");
            if (device < 0 || device >= cnt) throw std::invalid_argument("device index out of range");
            c = new DeviceCtx();
            c->device = device;
            MP_HIP(hipSetDevice(device));
            MP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
            MP_HIP(hipStreamCreateWithFlags(&c->md_stream, hipStreamNonBlocking));
            MP_HIP(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
            c->bb[0].stream = c->stream;
            MP_HIP(hipStreamCreateWithFlags(&c->bb[1].stream, hipStreamNonBlocking));
            for (BatchBufs &q : c->bb) {
                for (auto &e : q.ev) MP_HIP(hipEventCreate(&e));
                MP_HIP(hipEventCreateWithFlags(&q.ev_solved, hipEventDisableTiming));
                MP_HIP(hipEventCreateWithFlags(&q.ev_fork, hipEventDisableTiming));
                MP_HIP(hipEventCreateWithFlags(&q.ev_join, hipEventDisableTiming));
                MP_HIP(hipEventCreateWithFlags(&q.ev_h2d, hipEventDisableTiming));
                MP_HIP(hipEventCreateWithFlags(&q.ev_done, hipEventDisableTiming));
            }
        }
        MP_HIP(hipSetDevice(device));
        if (device < kMaxDevices) g_active_runs[device].fetch_add(1, std::memory_order_relaxed);
    }
    ~CtxLease() {
        if (c->device < kMaxDevices) g_active_runs[c->device].fetch_sub(1, std::memory_order_relaxed);
        std::lock_guard<std::mutex> lk(g_pool_mu);
        g_pool.push_back(c);
    }
};

// ---------------------------------------------------------------------------
void inv3(const double *K, double *Ki) {
    // no FMA contraction: the calibrated rays K^-1 x the MD solvers see are the oracle's
    // (oracle/src/estimator.cpp inv3, mv3) to the bit
#pragma clang fp contract(off)
    const double d = K[0] * (K[4] * K[8] - K[5] * K[7]) - K[1] * (K[3] * K[8] - K[5] * K[6]) +
                     K[2] * (K[3] * K[7] - K[4] * K[6]);
    Ki[0] = (K[4] * K[8] - K[5] * K[7]) / d;
    Ki[1] = (K[2] * K[7] - K[1] * K[8]) / d;
    Ki[2] = (K[1] * K[5] - K[2] * K[4]) / d;
    Ki[3] = (K[5] * K[6] - K[3] * K[8]) / d;
    Ki[4] = (K[0] * K[8] - K[2] * K[6]) / d;
    Ki[5] = (K[2] * K[3] - K[0] * K[5]) / d;
    Ki[6] = (K[3] * K[7] - K[4] * K[6]) / d;
    Ki[7] = (K[1] * K[6] - K[0] * K[7]) / d;
    Ki[8] = (K[0] * K[4] - K[1] * K[3]) / d;
}

// Problem setup shared by every entry point: the option transform to three data
// types (src/hybrid_pose_estimator.cpp:13-23) and, for SF/TF, pp-centring plus
// PoseLib normalize_points(..., true, false, true) (..shared..cpp:14-25).
struct Problem {
    PairConst C;
    HostPair H;
    double norm_scale = 1.0;
};

// Ceres settings of one LeastSquares / NonMinimalSolver call (the flags of
// Run::least_squares; src/hybrid_pose_estimator.cpp:203, 281 and the SF/TF analogues)
LmJob make_lm_job(const Problem &P, const EstimatorConfig &cfg, const int *sizes, int off, bool nonminimal,
                  const Model &m) {
    LmJob J;
    std::memset(&J, 0, sizeof(J));
    const bool use_reproj = cfg.lo_type != 1, use_sampson = cfg.lo_type != 2;
    const int v = P.C.variant;
    J.off0 = off;
    J.n0 = use_reproj ? sizes[0] : 0;
    J.off1 = off + sizes[0];
    J.n1 = use_reproj ? sizes[1] : 0;
    J.off2 = off + sizes[0] + sizes[1];
    J.n2 = use_sampson ? sizes[2] : 0;
    J.use_shift = (v == kCal || (v == kSF && nonminimal)) ? cfg.use_shift : 1;
    J.min_depth_constraint = cfg.min_depth_constraint;
    if (P.C.scale_only) { // HybridPoseOptimizerScaleOnly: offsets constant, unbounded
        J.use_shift = 0;
        J.min_depth_constraint = 0;
    }
    J.w_sampson = v == kCal ? std::sqrt(P.H.sampson_squared_weight) /
                                  (1.0 / (P.C.K0[0] + P.C.K0[4]) + 1.0 / (P.C.K1[0] + P.C.K1[4]))
                            : std::sqrt(P.H.sampson_squared_weight);
    J.ftol = cfg.ftol;
    J.gtol = cfg.gtol;
    J.ptol = cfg.ptol;
    J.max_iter = (int)cfg.max_iter;
    J.nonmonotonic = cfg.nonmonotonic ? 1 : 0;
    J.m = m;
    return J;
}

// The pair's magnitudes behind the screening margins (PairConst::ea.., mp_score.h
// score_margins): maxima of the rays' absolute sums, depths and coordinates.
void pair_magnitudes(PairConst &C, const HostPair &H) {
    const bool cal = C.variant == kCal;
    double ea = 0, eap = 0, exi = 0, eb = 0, ebp = 0, exj = 0, ed0 = 0, ed1 = 0, ex0 = 0, ex1 = 0, eab2 = 0;
    for (int i = 0; i < H.n; ++i) {
        const double u0 = H.x0[2 * i], v0 = H.x0[2 * i + 1], u1 = H.x1[2 * i], v1 = H.x1[2 * i + 1];
        ex0 = std::max(ex0, std::max(std::fabs(u0), std::fabs(v0)));
        ex1 = std::max(ex1, std::max(std::fabs(u1), std::fabs(v1)));
        ed0 = std::max(ed0, std::fabs(H.d0[i]));
        ed1 = std::max(ed1, std::fabs(H.d1[i]));
        if (cal) {
            auto ray = [](const double *Ki, double u, double v, double *abs1, double *absp, double *xi) {
                double a[3], p = 0.0;
                for (int j = 0; j < 3; ++j) {
                    a[j] = Ki[3 * j] * u + Ki[3 * j + 1] * v + Ki[3 * j + 2];
                    p += std::fabs(Ki[3 * j] * u) + std::fabs(Ki[3 * j + 1] * v) + std::fabs(Ki[3 * j + 2]);
                }
                *abs1 = std::max(*abs1, std::fabs(a[0]) + std::fabs(a[1]) + std::fabs(a[2]));
                *absp = std::max(*absp, p);
                *xi = std::max(*xi, p / (std::fabs(a[0]) + std::fabs(a[1]) + 1.0));
            };
            ray(C.K0i, u0, v0, &ea, &eap, &exi);
            ray(C.K1i, u1, v1, &eb, &ebp, &exj);
            const double a0 = C.K0i[0] * u0 + C.K0i[1] * v0 + C.K0i[2], a1 = C.K0i[3] * u0 + C.K0i[4] * v0 + C.K0i[5];
            const double b0 = C.K1i[0] * u1 + C.K1i[1] * v1 + C.K1i[2], b1 = C.K1i[3] * u1 + C.K1i[4] * v1 + C.K1i[5];
            const double ab = (std::fabs(a0) + std::fabs(a1) + 1.0) * (std::fabs(b0) + std::fabs(b1) + 1.0);
            eab2 = std::max(eab2, ab * ab);
        } else {
            ea = std::max(ea, std::fabs(u0) + std::fabs(v0));
            eb = std::max(eb, std::fabs(u1) + std::fabs(v1));
            const double ab = (std::fabs(u0) + std::fabs(v0) + 1.0) * (std::fabs(u1) + std::fabs(v1) + 1.0);
            eab2 = std::max(eab2, ab * ab);
        }
    }
    if (!cal) {
        eap = ea;
        ebp = eb;
    }
    // (a non-finite coordinate or depth turns screening off: make_problem)
    C.ea = ea * (1 + 1e-12);
    C.eap = eap * (1 + 1e-12);
    C.exi = exi * (1 + 1e-12);
    C.eb = eb * (1 + 1e-12);
    C.ebp = ebp * (1 + 1e-12);
    C.exj = exj * (1 + 1e-12);
    C.ed0 = ed0;
    C.ed1 = ed1;
    C.ex0 = ex0;
    C.ex1 = ex1;
    C.eab2 = eab2 * (1 + 1e-12);
}

Problem make_problem(const PairInput &in, const RansacOptions &o, const EstimatorConfig &cfg) {
    // no FMA contraction: the normalization scale (and with it every normalized
    // coordinate the MD solvers see) is the oracle's to the bit (estimator.cpp:88-103)
#pragma clang fp contract(off)
    Problem P;
    const int n = (int)in.n;
    PairConst &C = P.C;
    std::memset(&C, 0, sizeof(C));
    // the scale-only estimator runs on the calibrated geometry (src/hybrid_pose_estimator.h:110-134)
    C.scale_only = in.variant == kScaleOnly ? 1 : 0;
    C.variant = C.scale_only ? kCal : in.variant;
    C.n = n;
    C.score_type = cfg.score_type;
    C.min_depth_constraint = cfg.min_depth_constraint ? 1 : 0;
    C.use_shift = cfg.use_shift ? 1 : 0;
    // option-gated MD alternates (src/hybrid_pose_estimator.cpp:75-78, ..shared..cpp:62-65,
    // ..two..cpp:87-94); use_ours wins over use_4p4d, 4p4d exists for two-focal only
    C.md_alt = C.scale_only ? 0 : (o.use_ours ? 1 : ((o.use_4p4d && in.variant == kTF) ? 2 : 0));
    C.min_depth[0] = in.min_depth[0];
    C.min_depth[1] = in.min_depth[1];
    HostPair &H = P.H;
    H.variant = C.variant;
    H.n = n;
    H.x0.resize(2 * n);
    H.x1.resize(2 * n);
    H.d0.assign(in.d0, in.d0 + n);
    H.d1.assign(in.d1, in.d1 + n);
    H.min_depth[0] = in.min_depth[0];
    H.min_depth[1] = in.min_depth[1];
    double thr0 = o.squared_inlier_thresholds[0], thr1 = o.squared_inlier_thresholds[1];
    if (C.variant == kCal) {
        std::memcpy(C.K0, in.cam0, sizeof(C.K0));
        std::memcpy(C.K1, in.cam1, sizeof(C.K1));
        inv3(C.K0, C.K0i);
        inv3(C.K1, C.K1i);
        std::memcpy(H.x0.data(), in.x0, sizeof(double) * 2 * n);
        std::memcpy(H.x1.data(), in.x1, sizeof(double) * 2 * n);
        const double s = 1.0 / (C.K0[0] + C.K0[4]) + 1.0 / (C.K1[0] + C.K1[4]);
        C.loss_scale = 1.0 / (s * s);
        // upper-triangular intrinsics with unit last row: the score kernels' ray form
        auto tri = [](const double *K) { return K[3] == 0.0 && K[6] == 0.0 && K[7] == 0.0 && K[8] == 1.0; };
        C.kstd = (tri(C.K0) && tri(C.K1) && tri(C.K0i) && tri(C.K1i)) ? 1 : 0;
    } else {
        double scale = 0.0;
        for (int i = 0; i < n; ++i) {
            const double a0 = in.x0[2 * i] - in.cam0[0], a1 = in.x0[2 * i + 1] - in.cam0[1];
            const double b0 = in.x1[2 * i] - in.cam1[0], b1 = in.x1[2 * i + 1] - in.cam1[1];
            H.x0[2 * i] = a0;
            H.x0[2 * i + 1] = a1;
            H.x1[2 * i] = b0;
            H.x1[2 * i + 1] = b1;
            // (two accumulations per correspondence, as PoseLib's normalize_points and the
            // oracle: the scale, hence every normalized coordinate, to the bit)
            scale += std::sqrt(a0 * a0 + a1 * a1);
            scale += std::sqrt(b0 * b0 + b1 * b1);
        }
        scale = (n > 0) ? scale / (std::sqrt(2.0) * n) : 1.0;
        for (int i = 0; i < 2 * n; ++i) {
            H.x0[i] /= scale;
            H.x1[i] /= scale;
        }
        P.norm_scale = scale;
        thr0 /= scale * scale;
        thr1 /= scale * scale;
        for (int i = 0; i < 9; ++i) C.K0[i] = C.K1[i] = C.K0i[i] = C.K1i[i] = (i % 4 == 0) ? 1.0 : 0.0;
        C.loss_scale = 1.0;
    }
    pair_magnitudes(C, H);
    {
        C.tie_scale = env_real("MADPOSE_TIE_SCALE", 1.0, 1.0, 1e300);
        // a non-finite coordinate or depth: no screening at all (every margin infinite;
        // the score kernel's residuals could be NaN where no gate flags them)
        bool finite = true;
        for (int i = 0; i < 2 * n && finite; ++i) finite = std::isfinite(H.x0[i]) && std::isfinite(H.x1[i]);
        for (int i = 0; i < n && finite; ++i) finite = std::isfinite(H.d0[i]) && std::isfinite(H.d1[i]);
        if (!finite) C.tie_scale = std::numeric_limits<double>::infinity();
    }
    std::memcpy(H.K0, C.K0, sizeof(H.K0));
    std::memcpy(H.K1, C.K1, sizeof(H.K1));
    std::memcpy(H.K0i, C.K0i, sizeof(H.K0i));
    std::memcpy(H.K1i, C.K1i, sizeof(H.K1i));
    const double w0 = o.data_type_weights[0];
    // data_type_weights_[1] *= 2 * thr0 / thr1 (src/hybrid_pose_estimator.cpp:16-17)
    const double ws = o.data_type_weights[1] * (2 * thr0 / thr1);
    H.sampson_squared_weight = ws;
    C.thr[0] = C.thr[1] = thr0;
    C.thr[2] = thr1;
    C.w[0] = C.w[1] = w0;
    C.w[2] = ws;
    margin_consts(C);
    return P;
}

void upload_pair(DeviceCtx &X, const Problem &P, PairData *D) {
    const int64_t n = P.C.n;
    double *base = X.d_pair;
    const int64_t cn = X.cap_n;
    // one upload: the six arrays packed at stride n on the host, placed at their device
    // stride cap_n by one 2-D copy (the pooled context's cap_n is the high-water mark of
    // the pairs it has seen: a small pair after a large one moves 6 n doubles, not 6 cap_n)
    if (n > cn) throw std::logic_error("upload_pair: pair larger than the device buffers");
    std::vector<double> soa(6 * (size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        soa[i] = P.H.x0[2 * i];
        soa[n + i] = P.H.x0[2 * i + 1];
        soa[2 * n + i] = P.H.x1[2 * i];
        soa[3 * n + i] = P.H.x1[2 * i + 1];
        soa[4 * n + i] = P.H.d0[i];
        soa[5 * n + i] = P.H.d1[i];
    }
    if (n > 0)
        MP_HIP(hipMemcpy2DAsync(base, sizeof(double) * (size_t)cn, soa.data(), sizeof(double) * (size_t)n,
                                sizeof(double) * (size_t)n, 6, hipMemcpyHostToDevice, X.stream));
    D->x0u = base;
    D->x0v = base + cn;
    D->x1u = base + 2 * cn;
    D->x1v = base + 3 * cn;
    D->d0 = base + 4 * cn;
    D->d1 = base + 5 * cn;
    D->r0 = base + 6 * cn;
    D->r1 = base + 7 * cn;
    D->a0 = base + 8 * cn;
    D->a1 = base + 9 * cn;
    D->b0 = base + 10 * cn;
    D->b1 = base + 11 * cn;
    MP_HIP(launch_prep_pair(X.stream, P.C, *D, base + 6 * cn, base + 7 * cn, base + 8 * cn, base + 9 * cn,
                            base + 10 * cn, base + 11 * cn));
    // the staging vector dies here: make the copies complete first
    MP_HIP(hipStreamSynchronize(X.stream));
}

// ---------------------------------------------------------------------------
// The estimator run (one pair)
class Run {
  public:
    Run(DeviceCtx &X, const Problem &P, const RansacOptions &o, const EstimatorConfig &cfg)
        : X_(X), P_(P), o_(o), cfg_(cfg), n_(P.C.n), variant_(P.C.variant), maxm_(max_models(P.C.variant)) {
        const int kmd = variant_ == kCal ? 3 : 4;
        const int kpt = variant_ == kCal ? 5 : (variant_ == kSF ? 6 : 7);
        ss_[0][0] = kmd;
        ss_[0][1] = kmd;
        ss_[0][2] = 0;
        ss_[1][0] = 0;
        ss_[1][1] = 0;
        ss_[1][2] = kpt;
        min_sample_size_ = kpt;
        non_min_sample_size_ = variant_ == kCal ? 35 : 36;
        thr_[0] = P.C.thr[0];
        thr_[1] = P.C.thr[1];
        thr_[2] = P.C.thr[2];
        w_[0] = P.C.w[0];
        w_[1] = P.C.w[1];
        w_[2] = P.C.w[2];
        max_batch_ = (int)env_int("MADPOSE_MAX_BATCH", 32768, 1, 1 << 22);
        // (1024: the solver kernels cost about the same at 128 and at 1024 samples, so a
        // short run -- the ScanNet stand-in's 1000 iterations -- takes fewer round trips:
        // 903 / 982 / 998 pairs/s at 128 / 512 / 1000 on one box, profiles/r03/s6)
        // calibrated: 4096 since the post-LO speculation runs beside the LO (§2 step 6): a
        // bigger speculative batch costs no wait and covers more iterations per LO cycle,
        // 4.31 -> 4.07 ms per pair (2048: 4.19; profiles/r05/min_batch); shared focal
        // neutral at 2048 (9.94 -> 9.97 ms)
        min_batch_ = (int)env_int("MADPOSE_MIN_BATCH", variant_ == kCal ? 4096 : 1024, 1, 1 << 22);
        min_batch_ = std::min(min_batch_, max_batch_);
        // growth 1 for every variant: round 4 ran the shared focal at 2 (fewer, larger
        // batches for its latency-bound chain: 11.48 -> 10.97-11.20 ms, profiles/r04/gab2)
        // at 1.49 solved per accepted hypothesis; with the round-5 host the difference is
        // 10.62 (1.33) against 10.39 ms (1.42), 1.5: 10.50 (1.38), 3 x 60 pairs on one
        // box (profiles/r05/r5sg).  For cal, 0.5 and the waste it saves cost more round
        // trips than they save work (r04 gab)
        growth_ = env_real("MADPOSE_BATCH_GROWTH", 1.0, 0.01, 1e6);
        trace_ = std::getenv("MADPOSE_TRACE") != nullptr;
    }

    void run(Model *best, Stats *S);

  private:
    DeviceCtx &X_;
    const Problem &P_;
    const RansacOptions &o_;
    const EstimatorConfig &cfg_;
    const int n_, variant_, maxm_;
    int ss_[2][3];
    int min_sample_size_, non_min_sample_size_;
    double thr_[3], w_[3];
    int max_batch_, min_batch_;
    double growth_; // batch = growth_ x iterations so far (MADPOSE_BATCH_GROWTH)
    bool trace_ = false;
    // New bests are decided on reference-order sums (exact_score); score_batch's sums
    // screen with per-model margins (ScoreRec::tie, mp_score.h score_margins: |device
    // sum - reference-order sum| <= tie unless the iteration is flagged uncertain), see
    // the walk in run().  MADPOSE_TIE_SCALE multiplies every margin (tests force the
    // resolution path with a large factor).
    uint64_t tie_checks_ = 0;
    // MADPOSE_COUNT_DUMP=<file>: one line per walked iteration (iteration, solver type,
    // model count, the solver's sample) -- a diagnostic (tools/diag_counts.py)
    FILE *count_dump_ = nullptr;
    // MADPOSE_MODEL_DUMP=<file>: per walked iteration (int32 iteration, int32 model count,
    // the models as 17 doubles each, problem units) -- the oracle replays them
    // (ORACLE_MODEL_REPLAY, oracle/src/ransac.cpp) to separate the selection logic from
    // the solvers' rounding (tests/test_ties_gpu.py)
    FILE *model_dump_ = nullptr;
    // MADPOSE_TIMELINE=k (or k-m): the k-th estimator run of the process (0-based) prints its
    // timeline to stderr at the end -- one line per event, microseconds since the run
    // started: launch begin/end (B), wait begin/end, LO begin / prefix end / end, resolve
    // and exact-score calls, sampler joins -- a diagnostic of the critical path
    struct Timeline {
        bool on = false;
        long run = 0;
        Clock::time_point t0;
        struct Ev {
            double us;
            const char *what;
            long a;
        };
        std::vector<Ev> ev;
        std::mutex mu; // (the sampler thread launches speculative batches)
        void mark(const char *what, long a = 0) {
            if (!on) return;
            std::lock_guard<std::mutex> lk(mu);
            ev.push_back({1e6 * std::chrono::duration<double>(Clock::now() - t0).count(), what, a});
        }
    } tl_;
    PairData D_;
    Stats *S_ = nullptr;
    IterationStream rs_; // sampler + selection/LO streams
    double sample_s_ = 0.0;

    // --- GPU sweeps ---
    // One issuer of single-model sweeps (the estimator thread, or an LO worker during
    // parallel LO steps) with the cache of its last result; `sel` is the
    // selection/LO random stream the issuer draws from.
    struct Lane {
        SweepSlot *slot = nullptr;
        Mt19937 *sel = nullptr;
        Model model;
        bool valid = false;
        double fast = 0.0, bound = 0.0; // the fast sum and its distance bound (lo_sweep_fast)
        bool exact_valid = false;
        double score = 0.0;              // the reference-order sum, once taken
        const double *err = nullptr; // the buffer holding the last result
        std::vector<double> herr;    // host sweeps' errors (3 x n)
        uint64_t count = 0;
        double t[3] = {0, 0, 0}; // -, sweep, - seconds (MADPOSE_SWEEP_TIMING)
    };
    Lane lanes_[kLoLanes]; // lanes_[0]: the estimator thread
    // LO phase seconds (MADPOSE_LO_TIMING): serial prefix, steps phase, LO count, sum of
    // step times, longest step, step-0 time
    // + step 0's non-minimal fit and score, other steps' fit; step 0's first lsq_fit and
    // lsq iterations, the other steps' (mean)
    double lo_t_[14] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double lo_seg_[3] = {0, 0, 0}; // steps phase: before, during and after the parallel run
    bool lo_parallel_ = true;
    const bool early_hook_ = [] {
        return env_flag("MADPOSE_LO_EARLY_HOOK", true);
    }();

    // LO sweeps run on the issuing thread's core (host/lo_sweep.h): the reference's
    // residual operations and ScoreModel order, bit-identical to the oracle; a lane
    // keeps its last result (LO asks for the same model's score and inliers in turn)
    LoSweepData hsw_;
    // the errors of m (and its fast sum), cached per lane
    const double *sweep(Lane &L, const Model &m) {
        if (L.valid && std::memcmp(&m, &L.model, sizeof(Model)) == 0) return L.err;
        auto t_sw = Clock::now();
        if (L.herr.size() < 3 * (size_t)n_) L.herr.resize(3 * (size_t)n_);
        lo_sweep_fast(P_.C, hsw_, m, L.herr.data(), &L.fast, &L.bound);
        L.err = L.herr.data();
        L.model = m;
        L.valid = true;
        L.exact_valid = false;
        L.count++;
        const double dt = secs(t_sw);
        L.t[1] += dt;
        if (g_prof_on.load(std::memory_order_relaxed)) {
            std::lock_guard<std::mutex> lk(g_prof_mu);
            g_prof.sweeps += 1;
            g_prof.sweep_wall_ms += 1e3 * dt;
        }
        return L.err;
    }
    // ScoreModel's reference-order sum of m
    double score(Lane &L, const Model &m) {
        sweep(L, m);
        if (!L.exact_valid) {
            L.score = lo_ordered_score(P_.C, L.err, n_);
            L.exact_valid = true;
        }
        return L.score;
    }
    // Whether m's reference-order score could be below b: false when the fast sum
    // decides it cannot (fast - bound >= b); otherwise the reference-order score in *e
    // (the caller compares it).  UpdateBestModel needs the exact sum only then.
    bool score_below(Lane &L, const Model &m, double b, double *e) {
        sweep(L, m);
        if (!L.exact_valid && L.fast - L.bound >= b) return false;
        *e = score(L, m);
        return true;
    }
    int inliers(Lane &L, const Model &m, const double *thr, std::vector<int> out[3]) {
        const double *e = sweep(L, m);
        // Branch-free compaction: whether a correspondence is an inlier is close to a
        // coin flip along the index, so a conditional push_back mispredicts about every
        // other element (measured on the build host, 3 x 2000 errors at ~50 % inliers:
        // 17.8 us branchy, 5.5 us branch-free scalar).  AVX2: four errors per compare,
        // the lanes below the threshold appended as one 4-index store through a table of
        // the 16 masks (7.1-7.9 -> 3.1 us per 3 x 2000 on the build container).  Same
        // lists (ascending indices).
        int c = 0;
        const __m128i step = _mm_set1_epi32(4);
        for (int t = 0; t < 3; ++t) {
            std::vector<int> &o = out[t];
            o.resize(n_ + 4);
            int *w = o.data(), k = 0, i = 0;
            const double *et = e + (size_t)t * n_;
            const double th = thr[t];
            const __m256d tv = _mm256_set1_pd(th);
            __m128i base = _mm_setzero_si128();
            for (; i + 4 <= n_; i += 4) {
                const int msk = _mm256_movemask_pd(_mm256_cmp_pd(_mm256_loadu_pd(et + i), tv, _CMP_LT_OQ));
                _mm_storeu_si128((__m128i *)(w + k),
                                 _mm_add_epi32(_mm_load_si128((const __m128i *)kCompactLut[msk]), base));
                k += __builtin_popcount((unsigned)msk);
                base = _mm_add_epi32(base, step);
            }
            for (; i < n_; ++i) {
                w[k] = i;
                k += et[i] < th;
            }
            o.resize(k);
            c += k;
        }
        return c;
    }

    static void update_best(double sc, const Model &m, int st, double *best_sc, Model *best, int *best_st) {
        if (sc < *best_sc) {
            *best_sc = sc;
            *best = m;
            *best_st = st;
        }
    }

    uint32_t num_required(int s) const {
        double p_all = 1.0;
        for (int t = 0; t < 3; ++t) p_all *= std::pow(S_->inlier_ratios[t], (double)ss_[s][t]);
        if (p_all <= 0.0) return o_.max_num_iterations_per_solver;
        if (p_all >= 1.0) return o_.min_num_iterations;
        const double p_bad = 1.0 - p_all;
        if (p_bad >= 0.99999999999999) return o_.max_num_iterations_per_solver;
        const double it = std::ceil(std::log(1.0 - o_.success_probability) / std::log(p_bad) + 0.5);
        uint32_t r = std::min((uint32_t)it, o_.max_num_iterations_per_solver);
        return std::max(o_.min_num_iterations, r);
    }

    // UpdateRANSACTerminationCriteria (src/hybrid_ransac.h:351-378)
    void termination(const Model &m, uint32_t *max_per) {
        // after an LO the new best was usually swept last by the LO lane that recorded it:
        // its cached errors give the same inliers as a fresh sweep (the workers are idle
        // between LOs, so their lanes are read here without a race)
        Lane *L = &lanes_[0];
        for (Lane &c : lanes_)
            if (c.valid && std::memcmp(&m, &c.model, sizeof(Model)) == 0) {
                L = &c;
                break;
            }
        S_->best_num_inliers = inliers(*L, m, thr_, S_->inlier_indices);
        for (int t = 0; t < 3; ++t)
            S_->inlier_ratios[t] = n_ > 0 ? (double)S_->inlier_indices[t].size() / (double)n_ : 0.0;
        for (int s = 0; s < 2; ++s) max_per[s] = num_required(s);
    }

    // --- LO (src/hybrid_ransac.h:383-538) ---
    // The batched device LM (kernels/lm_device.h) on the lane's stream instead of the
    // host LM (MADPOSE_DEVICE_LM=1).  The issuing thread sleeps on a blocking-sync event
    // meanwhile, which frees its core for other pairs in flight (estimate_batch).
    bool device_lm_ = false;
    void least_squares_device(Lane &L, const std::vector<int> sample[3], Model *m, bool nonminimal) {
        SweepSlot &sl = *L.slot;
        const int sz[3] = {(int)sample[0].size(), (int)sample[1].size(), (int)sample[2].size()};
        const int64_t nidx = (int64_t)sz[0] + sz[1] + sz[2];
        sl.ensure_lm(nidx);
        constexpr size_t kJob = 0, kOut = 256, kSt = 448, kIdx = 512;
        static_assert(sizeof(LmJob) <= kOut && kOut + sizeof(Model) <= kSt, "LM staging layout");
        const LmJob J = make_lm_job(P_, cfg_, sz, 0, nonminimal, *m);
        std::memcpy(sl.h_lm + kJob, &J, sizeof(J));
        int *hi = (int *)(sl.h_lm + kIdx);
        for (int t = 0, o = 0; t < 3; ++t) {
            std::memcpy(hi + o, sample[t].data(), sizeof(int) * sz[t]);
            o += sz[t];
        }
        MP_HIP(hipMemcpyAsync(sl.d_lm, sl.h_lm, kIdx + sizeof(int) * (size_t)nidx, hipMemcpyHostToDevice, sl.stream));
        MP_HIP(launch_lm_batch(sl.stream, D_, P_.C, (const LmJob *)(sl.d_lm + kJob), 1, (const int *)(sl.d_lm + kIdx),
                               (Model *)(sl.d_lm + kOut), (int *)(sl.d_lm + kSt)));
        MP_HIP(hipMemcpyAsync(sl.h_lm + kOut, sl.d_lm + kOut, kIdx - kOut, hipMemcpyDeviceToHost, sl.stream));
        MP_HIP(hipEventRecord(sl.lm_done, sl.stream));
        MP_HIP(hipEventSynchronize(sl.lm_done));
        std::memcpy(m, sl.h_lm + kOut, sizeof(Model));
    }

    void least_squares(Lane &L, const std::vector<int> sample[3], Model *m, bool nonminimal) {
        const int kmd = variant_ == kCal ? 3 : 4;
        if (((int)sample[0].size() < kmd && (int)sample[1].size() < kmd) || (int)sample[2].size() < min_sample_size_)
            return;
        if (device_lm_) {
            auto t_lm = Clock::now();
            least_squares_device(L, sample, m, nonminimal);
            if (g_prof_on.load(std::memory_order_relaxed)) {
                std::lock_guard<std::mutex> lk(g_prof_mu);
                g_prof.lm_calls += 1;
                g_prof.lm_wall_ms += 1e3 * secs(t_lm);
            }
            return;
        }
        LMSettings S;
        S.use_reproj = cfg_.lo_type != 1;
        S.use_sampson = cfg_.lo_type != 2;
        // use_shift is forwarded by the calibrated estimator (NonMinimalSolver and
        // LeastSquares) and by the shared-focal NonMinimalSolver only.
        S.use_shift = (variant_ == kCal || (variant_ == kSF && nonminimal)) ? cfg_.use_shift : true;
        S.min_depth_constraint = cfg_.min_depth_constraint;
        if (P_.C.scale_only) { // HybridPoseOptimizerScaleOnly: offsets constant, unbounded
            S.use_shift = false;
            S.min_depth_constraint = false;
        }
        S.w_sampson = variant_ == kCal ? std::sqrt(P_.H.sampson_squared_weight) /
                                             (1.0 / (P_.C.K0[0] + P_.C.K0[4]) + 1.0 / (P_.C.K1[0] + P_.C.K1[4]))
                                       : std::sqrt(P_.H.sampson_squared_weight);
        S.ftol = cfg_.ftol;
        S.gtol = cfg_.gtol;
        S.ptol = cfg_.ptol;
        S.max_iter = (int)cfg_.max_iter;
        S.nonmonotonic = cfg_.nonmonotonic;
        auto t_lm = Clock::now();
        lm_refine(P_.H, sample, S, m);
        if (lo_timing_) {
            const size_t nb = (S.use_reproj ? sample[0].size() + sample[1].size() : 0) +
                              (S.use_sampson ? sample[2].size() : 0);
            if (nb >= kBigLM) {
                std::lock_guard<std::mutex> lk(lm_stat_mu_);
                lm_stat_[0] += 1.0;
                lm_stat_[1] += lm_last_evals;
                lm_stat_[2] += secs(t_lm);
                lm_stat_[3] += (double)nb;
            }
        }
        if (g_prof_on.load(std::memory_order_relaxed)) {
            const double dt = secs(t_lm);
            const size_t nb = (S.use_reproj ? sample[0].size() + sample[1].size() : 0) +
                              (S.use_sampson ? sample[2].size() : 0);
            std::lock_guard<std::mutex> lk(g_prof_mu);
            g_prof.lm_calls += 1;
            g_prof.lm_wall_ms += 1e3 * dt;
            g_prof.lm_blocks += nb;
            if (nb >= kBigLM) {
                g_prof.lm_big_calls += 1;
                g_prof.lm_big_wall_ms += 1e3 * dt;
            }
        }
    }

    // all: indices idx + t * n (t < 3, shuffled, so the type is random along the list);
    // branch-free like inliers()
    static void split(const std::vector<int> &all, int n, std::vector<int> out[3]) {
        const size_t m = all.size();
        for (int t = 0; t < 3; ++t) out[t].resize(m);
        int *w0 = out[0].data(), *w1 = out[1].data(), *w2 = out[2].data();
        int k0 = 0, k1 = 0, k2 = 0;
        for (size_t i = 0; i < m; ++i) {
            const int idx = all[i];
            const int t = (idx >= n) + (idx >= 2 * n);
            const int v = idx - t * n;
            w0[k0] = v;
            w1[k1] = v;
            w2[k2] = v;
            k0 += t == 0;
            k1 += t == 1;
            k2 += t == 2;
        }
        out[0].resize(k0);
        out[1].resize(k1);
        out[2].resize(k2);
    }
    static void shuffle_resize(Mt19937 &sel, int k, std::vector<int> *v) {
        const int n = (int)v->size();
        if (n <= k) return;
        for (int i = 0; i < k; ++i) std::swap((*v)[i], (*v)[uniform_int(sel, i, n - 1)]);
        v->resize(k);
    }
    // draws of one lsq_fit when every data type has enough inliers (the usual case)
    int lsq_fit_draws(int st) const {
        int k = 0;
        for (int t = 0; t < 3; ++t) k += ss_[st][t] * o_.min_sample_multiplicator;
        return k * o_.min_sample_multiplicator;
    }

    void lsq_fit(Lane &L, const double *thr, int st, Model *m, bool use_all) {
        std::vector<int> inl[3];
        inliers(L, *m, thr, inl);
        int k[3];
        for (int t = 0; t < 3; ++t) {
            if ((int)inl[t].size() < ss_[st][t]) return;
            k[t] = std::min(ss_[st][t] * o_.min_sample_multiplicator, (int)inl[t].size());
        }
        if (use_all) {
            least_squares(L, inl, m, false);
            return;
        }
        const int total = (k[0] + k[1] + k[2]) * o_.min_sample_multiplicator;
        std::vector<int> all;
        all.reserve(inl[0].size() + inl[1].size() + inl[2].size());
        for (int t = 0; t < 3; ++t)
            for (int idx : inl[t]) all.push_back(idx + t * n_);
        shuffle_resize(*L.sel, total, &all);
        std::vector<int> smp[3];
        split(all, n_, smp);
        least_squares(L, smp, m, false);
    }

    // The non-minimal sample of an LO step is unusable (NonMinimalSolver returns 0,
    // or Solve() sees no residuals): the step is skipped without drawing.
    bool step_skipped(const std::vector<int> &sample_all) const {
        // (the sizes split() would give, counted without building the lists: this runs
        // on the estimator thread before the parallel steps start)
        int cnt[3] = {0, 0, 0};
        for (const int idx : sample_all) cnt[(idx >= n_) + (idx >= 2 * n_)]++;
        const int kmd = variant_ == kCal ? 3 : 4;
        if ((cnt[0] < kmd && cnt[1] < kmd) || cnt[2] < min_sample_size_) return true;
        const size_t nres = (cfg_.lo_type != 1 ? (size_t)cnt[0] + cnt[1] : 0) + (cfg_.lo_type != 2 ? (size_t)cnt[2] : 0);
        return nres == 0;
    }
    struct StepOut {
        std::vector<std::pair<double, Model>> updates; // the step's update_best calls, in order
        Mt19937 sel;                                   // LO stream after the step
        double nonmin_s = 0.0, score_s = 0.0;          // MADPOSE_LO_TIMING: non-minimal fit, its score,
        double lsq_s = 0.0, iter_s = 0.0;              // the first lsq_fit, the lsq iterations
    };
    // One LO step (the loop body of src/hybrid_ransac.h:435-470) from m_init on the
    // non-minimal sample `sample_all`, drawing from *L.sel.
    // The step's update_best calls are applied after all steps, in step order, so a
    // score can update the best only if it is below b0 (the best when the steps start:
    // later bests are lower) and below every score this step recorded before it; scores
    // the fast sum puts at or above that are not recorded (score_below).
    void lo_step(Lane &L, int st, const std::vector<int> &sample_all, const Model &m_init, const double *thr,
                 const double *upd, double b0, StepOut &out) {
        out.updates.clear();
        if (step_skipped(sample_all)) return;
        double b = b0;
        auto record = [&](const Model &mm) {
            double e;
            if (score_below(L, mm, b, &e)) {
                out.updates.emplace_back(e, mm);
                b = std::min(b, e);
            }
        };
        Model m = m_init;
        std::vector<int> smp[3];
        split(sample_all, n_, smp);
        auto t_nm = Clock::now();
        least_squares(L, smp, &m, true);
        out.nonmin_s = secs(t_nm);
        auto t_sc = Clock::now();
        record(m);
        out.score_s = secs(t_sc);
        auto t_l = Clock::now();
        lsq_fit(L, thr_, st, &m, false);
        out.lsq_s = secs(t_l);
        double cur[3] = {thr[0], thr[1], thr[2]};
        auto t_it = Clock::now();
        for (int i = 0; i < o_.num_lsq_iterations; ++i) {
            lsq_fit(L, cur, st, &m, false);
            record(m);
            for (int t = 0; t < 3; ++t) cur[t] -= upd[t];
        }
        out.iter_s = secs(t_it);
    }

    // LocalOptimization (src/hybrid_ransac.h:383-470).  The steps depend on each
    // other only through the LO random stream, and each step draws a predictable
    // number of values (lsq_fit_draws per lsq_fit) unless an lsq_fit finds too few
    // inliers or a draw is rejected.  So the steps run concurrently on kLoLanes
    // threads from the stream positions they would start at; afterwards every
    // step's end position is checked against the next step's start, steps after a
    // mismatch are recomputed in order, and the steps' update_best calls are applied
    // in step order -- the result is the serial one in every case.
    // predicted(sel): called once the LO stream's end state is predicted (parallel
    // steps), before the steps run -- the estimator speculates the next batch on it.
    void local_opt(int st, Model *best_min, double *best_min_score, int *best_st,
                   const std::function<void(const Mt19937 &)> &predicted = nullptr) {
        auto t0 = Clock::now();
        Lane &L0 = lanes_[0];
        double thr[3], upd[3];
        for (int t = 0; t < 3; ++t) {
            upd[t] = (o_.threshold_multiplier - 1.0) * thr_[t] / (int)(o_.num_lsq_iterations - 1);
            thr[t] = thr_[t] * o_.threshold_multiplier;
        }
        // Early hook (MADPOSE_LO_EARLY_HOOK=0 turns it off): the stream's end is predicted
        // before the serial prefix, so the speculative batch is on the GPU while the prefix
        // runs.  The prefix's shuffle draws k_nonmin values when the base inlier set is
        // larger -- k_nonmin = max(non_min_sample_size, min(min_sample_size x multiplier,
        // |base| / 2)) is that constant whenever |base| / 2 reaches the product (always for
        // the default options: 35 >= 15) -- and every step draws per_step unless it is
        // skipped.  Any other outcome ends the LO elsewhere and the speculation is
        // discarded (the caller compares the draw counts), as for the late prediction.
        bool hooked = false;
        const int R_steps = o_.num_lo_steps;
        if (predicted && early_hook_ && lo_parallel_ && R_steps > 1) {
            const uint64_t per_step = (uint64_t)(1 + o_.num_lsq_iterations) * (uint64_t)lsq_fit_draws(st);
            const int k_pred = std::max(non_min_sample_size_, min_sample_size_ * o_.non_min_sample_multiplier);
            Mt19937 e = rs_.sel;
            e.discard((uint64_t)k_pred + (uint64_t)R_steps * per_step);
            predicted(e);
            hooked = true;
        }
        Model m_init = *best_min;
        lsq_fit(L0, thr, st, &m_init, true);
        double sc;
        if (score_below(L0, m_init, *best_min_score, &sc)) update_best(sc, m_init, st, best_min_score, best_min, best_st);
        const double b0 = *best_min_score; // (the steps' scores are decided against it, lo_step)
        std::vector<int> base[3];
        inliers(L0, m_init, thr_, base);
        std::vector<int> base_all;
        for (int t = 0; t < 3; ++t)
            for (int idx : base[t]) base_all.push_back(idx + t * n_);
        const int k_nonmin = std::max(non_min_sample_size_,
                                      std::min(min_sample_size_ * o_.non_min_sample_multiplier, (int)base_all.size() / 2));
        const int R = o_.num_lo_steps;
        lo_t_[0] += secs(t0); // serial prefix: initial fit, score, base inliers
        tl_.mark("lo_prefix_end", (long)base_all.size());
        auto t_steps = Clock::now();
        if (R > 0) {
            // step 0 solves on base_all as it is and then shuffles it down to
            // k_nonmin; later steps shuffle nothing (it is that size already) and all
            // solve on the shuffled sample (:439-440)
            const std::vector<int> sample0 = base_all;
            shuffle_resize(rs_.sel, k_nonmin, &base_all);
            const std::vector<int> &sample1 = base_all;
            std::vector<StepOut> outs(R);
            int first_serial = 0; // steps [first_serial, R) still to run in order
            Mt19937 sel = rs_.sel;
            if (lo_parallel_ && R > 1) {
                std::vector<uint64_t> start(R);
                uint64_t pos = sel.draws();
                const uint64_t per_step = (uint64_t)(1 + o_.num_lsq_iterations) * (uint64_t)lsq_fit_draws(st);
                const bool skip0 = step_skipped(sample0), skip1 = R > 1 && step_skipped(sample1);
                for (int r = 0; r < R; ++r) {
                    start[r] = pos;
                    if (!(r == 0 ? skip0 : skip1)) pos += per_step;
                }
                const Mt19937 base_sel = sel;
                // the speculation hook runs as job 1, beside the steps: step 0 (the
                // longest, on all base inliers) starts at once, and the lane that takes
                // the hook takes a short step after it (the hook may wait for the
                // sampler thread to give up the draw it cancels)
                Mt19937 end = base_sel;
                const bool hook_job = predicted && !hooked && X_.lo_workers->lanes() > 1;
                if (predicted && !hooked) {
                    end.discard(pos - base_sel.draws());
                    if (!hook_job) predicted(end);
                }
                std::vector<double> step_s(R, 0.0);
                const auto t_run = Clock::now();
                lo_seg_[0] += std::chrono::duration<double>(t_run - t_steps).count();
                X_.lo_workers->run(R + (hook_job ? 1 : 0), [&](int job, int lane) {
                    if (hook_job && job == 1) {
                        auto th = Clock::now();
                        if (lane != 0) MP_HIP(hipSetDevice(X_.device));
                        predicted(end);
                        lo_seg_[2] += secs(th);
                        return;
                    }
                    const int r = hook_job && job > 1 ? job - 1 : job;
                    auto ts = Clock::now();
                    if (lane != 0) MP_HIP(hipSetDevice(X_.device));
                    Mt19937 my = base_sel;
                    my.discard(start[r] - base_sel.draws());
                    Lane &L = lanes_[lane];
                    L.sel = &my;
                    lo_step(L, st, r == 0 ? sample0 : sample1, m_init, thr, upd, b0, outs[r]);
                    L.sel = lane == 0 ? &rs_.sel : nullptr;
                    outs[r].sel = my;
                    step_s[r] = secs(ts);
                });
                lo_seg_[1] += secs(t_run);
                for (int r = 0; r < R; ++r) {
                    lo_t_[3] += step_s[r];
                    lo_t_[4] = std::max(lo_t_[4], step_s[r]);
                }
                lo_t_[5] += step_s[0];
                lo_t_[6] += outs[0].nonmin_s;
                lo_t_[7] += outs[0].score_s;
                for (int r = 1; r < R; ++r) lo_t_[8] += outs[r].nonmin_s / (R - 1);
                lo_t_[9] += outs[0].lsq_s;
                lo_t_[10] += outs[0].iter_s;
                for (int r = 1; r < R; ++r) {
                    lo_t_[11] += outs[r].lsq_s / (R - 1);
                    lo_t_[12] += outs[r].iter_s / (R - 1);
                }
                // steps 0..r are right while each one ended where the next one started
                first_serial = R;
                for (int r = 0; r + 1 < R; ++r)
                    if (outs[r].sel.draws() != start[r + 1]) {
                        first_serial = r + 1;
                        break;
                    }
                sel = outs[first_serial - 1].sel;
                if (trace_ && first_serial < R)
                    std::fprintf(stderr, "[engine] LO step %d started off its predicted draw; recomputing\n",
                                 first_serial);
            }
            lo_t_[13] += R - first_serial; // steps recomputed in order
            for (int r = first_serial; r < R; ++r) {
                L0.sel = &sel;
                lo_step(L0, st, r == 0 ? sample0 : sample1, m_init, thr, upd, b0, outs[r]);
                L0.sel = &rs_.sel;
            }
            rs_.sel = sel;
            for (int r = 0; r < R; ++r)
                for (const auto &u : outs[r].updates) update_best(u.first, u.second, st, best_min_score, best_min, best_st);
        }
        lo_t_[1] += secs(t_steps);
        lo_t_[2] += 1.0;
        S_->seconds_lo += secs(t0);
    }

    // --- minimal-sample batches (host) ---
    // Batches drawn on this thread (at the start, after LO or a cut batch) are sized so
    // drawing them costs about one batch round trip on the GPU: cheap solvers get short
    // synchronous batches (the worker draws the long ones), expensive ones long.
    double draw_s_per_it_ = 40e-9, batch_s_ = 1e-3; // running estimates
    uint32_t sync_batch(uint32_t want) const {
        const double b = batch_s_ / std::max(draw_s_per_it_, 1e-9);
        return std::min<uint32_t>(want, (uint32_t)std::max<double>(min_batch_, std::min<double>(b, 1e9)));
    }
    int *slot_ptr(int slot) const { return X_.h_samples + (size_t)slot * 9 * max_batch_; }
    // slot_ptr for a draw or an upload of B iterations, bounds-checked on the host: slot s
    // spans [9 s max_batch_, 9 (s + 1) max_batch_) of the 2 x 9 cap_b ints of h_samples
    // (every draw into and upload from a slot is range-checked)
    int *slot_for(int slot, uint32_t B) const {
        if (slot < 0 || slot > 1 || B > (uint32_t)max_batch_ || max_batch_ > X_.cap_b || !X_.h_samples)
            throw std::logic_error("sample slot out of range: slot " + std::to_string(slot) + ", B " +
                                   std::to_string(B) + ", max_batch " + std::to_string(max_batch_) + ", cap_b " +
                                   std::to_string(X_.cap_b));
        return slot_ptr(slot);
    }
    void generate(Batch &g, uint32_t B, int slot) {
        auto t0 = Clock::now();
        draw_batch(rs_, g, B, slot, slot_for(slot, B), nullptr, sampler_mode());
        sample_s_ += secs(t0);
    }
    // both streams to the end of iteration j of batch g
    void rewind(const Batch &g, uint32_t j) {
        auto t0 = Clock::now();
        const uint32_t k = j / kSnap;
        rs_ = g.snaps[k];
        int scratch[8];
        for (uint32_t r = k * kSnap; r <= j; ++r) rs_.next(scratch);
        sample_s_ += secs(t0);
    }

    // Solves and scores batch g on the GPU (asynchronous, X_.stream): sample upload,
    // MD solver on the side stream, the point-solver stages, score_batch, and the
    // per-iteration best scores / slots / model counts back to pinned host memory.
    // best: best_min_model_score when the batch starts (the scoring's early exit).
    bool batch_prof_[2] = {false, false};
    double launch_s_ = 0.0; // main-thread time in launch_batch (MADPOSE_LO_TIMING)
    int launch_n_ = 0;
    // big LM solves (>= kBigLM blocks) under MADPOSE_LO_TIMING: count, evaluations,
    // seconds, blocks
    const bool lo_timing_ = std::getenv("MADPOSE_LO_TIMING") != nullptr;
    std::mutex lm_stat_mu_;
    double lm_stat_[4] = {0, 0, 0, 0};
    // the fused MD + 5pt launches up to this batch size (MADPOSE_SOLVE_FUSE_MAX; default:
    // every batch).  Round 5's one-stage fused kernel (216 VGPRs, two waves per SIMD) cost
    // the 5pt root stage its third wave on big batches (cal 5.62 always fused -> 5.46 ms
    // up to 8192, profiles/r05/r5o); the two-stage form (md_setup_pt5 + md_root_tail5)
    // runs the big batches faster than the MD side stream beside the point chain: cal
    // gpu_solve 2.10 -> 2.02 ms, 3.99 -> 3.90 ms per pair (5 same-box A/B pairs,
    // profiles/r06/fuse_all)
    const int64_t fuse_max_ = [] {
        return (int64_t)env_int("MADPOSE_SOLVE_FUSE_MAX", 1ll << 40, 0, 1ll << 40);
    }();

    // cut_on_record: the batch lies at or past lo_starting_iterations, so its first new
    // best runs LO and cuts it; score_batch then skips the iterations behind a record.
    //
    // Threading: one thread at a time calls this for a run.  The estimator thread
    // launches every batch but one kind, the post-LO speculation, which the sampler
    // thread launches (the `after` of its job, Run::run speculation_hook) between
    // Sampler::start() and the matching finish() / cancel().  The estimator thread spends
    // that span inside local_opt, which launches no batch (its hook only starts the job),
    // and on the few lines from there to the join (join_speculation), and it returns from
    // finish() / cancel() only once `after` has returned.  The
    // sampler's mutex orders the two threads at both ends, so X_.epoch, batch_prof_ and
    // the BatchBufs fields written here (epoch_hi, h2d_pending, the events) need no
    // atomics.  (tl_ takes its own lock: the LO's marks come from the other thread.)
    void launch_batch(const Batch &g, double best, bool cut_on_record) {
        const uint32_t B = g.B;
        const int nmd = g.nmd, npt = g.npt;
        BatchBufs &Q = X_.bb[g.slot];
        const BatchBufs &O = X_.bb[g.slot ^ 1];
        hipStream_t s = Q.stream;
        const bool prof = g_prof_on.load(std::memory_order_relaxed);
        batch_prof_[g.slot] = prof;
        const PairData &D = D_;
        // one upload: samples, then the MD list and the (descending) point list
        MP_HIP(hipMemcpyAsync(Q.d_samples, slot_for(g.slot, B), sizeof(int) * 9 * (size_t)B, hipMemcpyHostToDevice, s));
        tl_.mark("  h2d");
        MP_HIP(hipEventRecord(Q.ev_h2d, s));
        Q.h2d_pending = true;
        const int *d_md_list = Q.d_samples + 8 * (size_t)B, *d_pt_list = d_md_list + nmd;
        // (the other slot's batch may still be solving: the solvers' workspace is shared)
        MP_HIP(hipStreamWaitEvent(s, O.ev_solved, 0));
        if (prof) MP_HIP(hipEventRecord(Q.ev[0], s));
        // MD iterations on the side stream, point iterations on the main one (they
        // write disjoint model slots); scoring waits for both -- or, calibrated, both in
        // one launch on the main stream (launch_solve_fused)
        const PtWorkspace W{X_.d_pt_cand, X_.d_pt_ncand, X_.d_pt_slots, X_.d_pt_valid, X_.d_pt_pen,
                            X_.d_md_ws,   X_.d_md_nr,   X_.cap_b};
        const bool fused = solve_fusable(P_.C) && (int64_t)B <= fuse_max_;
        if (fused) {
            MP_HIP(launch_solve_fused(s, D, P_.C, d_md_list, nmd, d_pt_list, npt, Q.d_samples, W, Q.d_models,
                                      Q.d_recs, Q.d_counts, maxm_));
            tl_.mark("  solve_launched");
        } else {
            if (nmd > 0) {
                MP_HIP(hipEventRecord(Q.ev_fork, s));
                MP_HIP(hipStreamWaitEvent(X_.md_stream, Q.ev_fork, 0));
                MP_HIP(launch_md_solve_staged(X_.md_stream, D, P_.C, d_md_list, nmd, Q.d_samples, W, Q.d_models,
                                              Q.d_recs, Q.d_counts, maxm_));
                MP_HIP(hipEventRecord(Q.ev_join, X_.md_stream));
            }
            MP_HIP(launch_pt_solve(s, D, P_.C, d_pt_list, npt, Q.d_samples, W, Q.d_models, Q.d_recs, Q.d_counts,
                                   maxm_));
            if (nmd > 0) MP_HIP(hipStreamWaitEvent(s, Q.ev_join, 0));
        }
        MP_HIP(hipEventRecord(Q.ev_solved, s));
        if (prof) MP_HIP(hipEventRecord(Q.ev[1], s));
        const unsigned epoch_hi = ~(++X_.epoch);
        Q.epoch_hi = epoch_hi;
        MP_HIP(launch_score_batch(s, D, P_.C, Q.d_recs, Q.d_counts, (int)B, maxm_, Q.d_scores, Q.d_res, best,
                                  prof ? Q.d_work : nullptr, cut_on_record ? X_.d_recword : nullptr, epoch_hi,
                                  Q.d_models, Q.d_recmodel, Q.d_flags8, Q.d_cand));
        tl_.mark("  score_launched");
        if (prof) MP_HIP(hipEventRecord(Q.ev[2], s));
        MP_HIP(hipMemcpyAsync(Q.h_flags8, Q.d_flags8, (size_t)B, hipMemcpyDeviceToHost, s));
        if (prof) MP_HIP(hipMemcpyAsync(Q.h_work, Q.d_work, sizeof(int) * B, hipMemcpyDeviceToHost, s));
        MP_HIP(hipEventRecord(Q.ev_done, s));
    }
    // every batch launched from this run has finished (both slots' streams and the MD
    // side stream)
    void drain_batches() {
        for (const BatchBufs &q : X_.bb) MP_HIP(hipStreamSynchronize(q.stream));
        MP_HIP(hipStreamSynchronize(X_.md_stream));
    }
    // before host sample slot `slot` is redrawn: the last batch launched from it must
    // have been copied to the device (a run that an exception unwound leaves its batches
    // queued; otherwise the batch has been waited for or drained by then)
    void slot_free(int slot) {
        BatchBufs &Q = X_.bb[slot];
        if (Q.h2d_pending) {
            MP_HIP(hipEventSynchronize(Q.ev_h2d));
            Q.h2d_pending = false;
        }
    }

    // Reference-order score of a model (host/lo_sweep.h), on lane 0: the LO that follows
    // a new best starts with a sweep of the same model and finds it cached.
    double exact_score(const Model &m) { return score(lanes_[0], m); }

    // Iteration j of the last batch could hold a new best but it is not certain which of
    // its models wins in the reference order: its best's interval [S - T, S + T] reaches
    // another model's (kSlotAmbiguous), best_min_score lies inside it, or the iteration
    // is uncertain (a flagged correspondence: no margin holds, every model is a
    // contender).  Re-score the contenders in the reference's order and take the first
    // minimum (GetBestEstimatedModelId, src/hybrid_ransac.h:245-263); a model whose lower
    // bound S - T exceeds the smallest upper bound of the iteration cannot be the
    // reference's winner.  Rare (tests/test_ties_gpu.py forces it).
    void resolve_tie(const BatchBufs &Q, uint32_t j, Model *out, double *out_score) {
        const int nm = Q.h_cand[j].count;
        const bool uncertain = (Q.h_cand[j].slot & kSlotUncertain) != 0;
        std::vector<double> dsc(nm);
        std::vector<Model> ms(nm);
        std::vector<ScoreRec> rc(nm);
        // (the batch is complete; the main stream may already hold the next one)
        MP_HIP(hipMemcpyAsync(dsc.data(), Q.d_scores + (size_t)j * maxm_, sizeof(double) * nm,
                              hipMemcpyDeviceToHost, X_.copy_stream));
        MP_HIP(hipMemcpyAsync(ms.data(), Q.d_models + (size_t)j * maxm_, sizeof(Model) * nm, hipMemcpyDeviceToHost,
                              X_.copy_stream));
        MP_HIP(hipMemcpyAsync(rc.data(), Q.d_recs + (size_t)j * maxm_, sizeof(ScoreRec) * nm, hipMemcpyDeviceToHost,
                              X_.copy_stream));
        MP_HIP(hipStreamSynchronize(X_.copy_stream));
        double hi_min = kMax; // the smallest upper bound of a model's reference-order score
        for (int m = 0; m < nm; ++m)
            if (dsc[m] < kMax) hi_min = std::min(hi_min, dsc[m] + rc[m].tie);
        *out_score = kMax;
        for (int m = 0; m < nm; ++m) {
            // (a model the exit killed reports DBL_MAX: its reference sum reached the
            // pre-batch best, it cannot win)
            if (!uncertain && (!(dsc[m] < kMax) || dsc[m] - rc[m].tie > hi_min)) continue;
            const double e = exact_score(ms[m]);
            if (e < *out_score) { // strict '<': the first minimum wins
                *out_score = e;
                *out = ms[m];
            }
        }
        ++tie_checks_;
    }

    // the model of a new best: score_batch wrote it to the mapped record slot of its
    // iteration (the batch's stream has been synchronized)
    Model fetch_model(const BatchBufs &Q, int b) { return Q.h_recmodel[b]; }
};

void Run::run(Model *best, Stats *S) {
    auto t_start = Clock::now();
    const char *dump_path = std::getenv("MADPOSE_COUNT_DUMP");
    std::unique_ptr<FILE, int (*)(FILE *)> dump(dump_path ? std::fopen(dump_path, "w") : nullptr, &std::fclose);
    count_dump_ = dump.get();
    const char *mdump_path = std::getenv("MADPOSE_MODEL_DUMP");
    std::unique_ptr<FILE, int (*)(FILE *)> mdump(mdump_path ? std::fopen(mdump_path, "wb") : nullptr, &std::fclose);
    model_dump_ = mdump.get();
    {
        static std::atomic<long> runs{0};
        const long r = runs.fetch_add(1);
        const char *e = std::getenv("MADPOSE_TIMELINE");
        long lo = -1, hi = -1; // "k" or "k-m"
        if (e) {
            int used = 0;
            const int k = std::sscanf(e, "%ld%n-%ld%n", &lo, &used, &hi, &used);
            if (k < 1 || e[used] != '\0' || lo < 0 || (k == 2 && hi < lo)) env_reject("MADPOSE_TIMELINE", e, "expected k or k-m");
            if (k < 2) hi = lo;
        }
        tl_.on = e && r >= lo && r <= hi;
        tl_.run = r;
        tl_.t0 = t_start;
    }
    S_ = S;
    *S = Stats();
    S->best_model_score = kMax;
    std::memset(best, 0, sizeof(Model));
    best->scale = 1.0;
    best->focal0 = best->focal1 = 1.0;
    double *prior = rs_.prior;
    if (cfg_.solver_type == 1) prior[0] = 0.0;
    if (cfg_.solver_type == 2) prior[1] = 0.0;
    for (int s = 0; s < 2; ++s)
        for (int t = 0; t < 3; ++t) {
            rs_.ss[s][t] = ss_[s][t];
            if (ss_[s][t] > n_) prior[s] = 0.0;
        }
    if (prior[0] <= 0.0 && prior[1] <= 0.0) { // VerifyData failed
        S->seconds_total = secs(t_start);
        return;
    }
    X_.ensure(n_, max_batch_, maxm_);
    if (!X_.sampler) X_.sampler.reset(new Sampler());
    lanes_[0].slot = &X_.sweep_slot[0];
    lanes_[0].sel = &rs_.sel;
    {
        lo_parallel_ = env_flag("MADPOSE_LO_PARALLEL", true) && o_.num_lo_steps > 1;
        device_lm_ = env_flag("MADPOSE_DEVICE_LM", false);
    }
    if (lo_parallel_) {
        const int nl = lo_lanes_setting();
        if (!X_.lo_workers || X_.lo_workers->lanes() != nl) X_.lo_workers.reset(new LoWorkers(nl, X_.device));
        for (int l = 1; l < nl; ++l) lanes_[l].slot = &X_.sweep_slot[l];
    }
    upload_pair(X_, P_, &D_);
    lo_sweep_prepare(P_.C, P_.H.x0.data(), P_.H.x1.data(), P_.H.d0.data(), P_.H.d1.data(), &hsw_);
    rs_.n = n_;
    rs_.seed(o_.random_seed);

    const uint32_t max_total = std::max(o_.max_num_iterations, o_.min_num_iterations);
    uint32_t max_per[2];
    max_per[0] = max_per[1] = std::max(o_.max_num_iterations_per_solver, o_.min_num_iterations);
    const uint32_t lo_start = (uint32_t)o_.lo_starting_iterations;
    Model best_min;
    std::memset(&best_min, 0, sizeof(best_min));
    double best_min_score = kMax;

    uint32_t it = 0;
    bool done = false;
    int bcur = min_batch_;
    // batch size at position `at`: the solver kernels are latency-bound (cost ~flat
    // up to tens of thousands of samples) and new bests -- the only thing that cuts
    // a batch -- thin out like records of an iid sequence, so speculate on a window
    // proportional to the position in the stream; batches stop at lo_start.
    auto batch_size = [&](uint32_t at, uint32_t want) {
        uint32_t B = std::min<uint32_t>(want, max_total - at);
        if (at < lo_start) B = std::min<uint32_t>(B, lo_start - at);
        // the loop stops once a solver type reaches its (termination-adjusted) cap:
        // iterations past the expected stop would be scored for nothing.  Expected
        // stop of type st from here: its remaining count over its selection share
        // (+10 % and a few iterations of slack; a short batch only costs a round trip).
        const double ps = prior[0] + prior[1];
        double cap = 1e18;
        for (int st = 0; st < 2; ++st) {
            if (prior[st] <= 0.0) continue;
            const double share = prior[st] / ps;
            const double left = (double)max_per[st] - (double)S->num_iterations_per_solver[st] -
                                share * (double)(at > it ? at - it : 0);
            cap = std::min(cap, std::max(0.0, left) / share * 1.1 + 32.0);
        }
        if (cap < (double)B) B = std::max<uint32_t>(1, (uint32_t)cap);
        return B;
    };
    // speculation window at `at`: growth_ x at iterations, clamped to [min, max]
    auto grow = [&](uint32_t at) {
        return (uint32_t)std::min<double>((double)max_batch_, std::max<double>((double)min_batch_, growth_ * at));
    };
    Batch gen[2];
    // the worker may be drawing into gen[] when an exception unwinds this frame
    struct CancelOnExit {
        Sampler *s;
        ~CancelOnExit() { s->cancel(); }
    } cancel_on_exit{X_.sampler.get()};
    int cur = 0;
    bool have_next = false; // gen[cur] already holds the batch starting at `it`
    bool launched = false;  // ... and it is already on the GPU (post-LO speculation)
    // Post-LO speculation (MADPOSE_LO_SPECULATE=0 disables): the batch after an LO
    // depends on the LO only through the selection stream's end state, which the
    // parallel LO predicts before its steps run.  The sampler draws that batch from the
    // predicted state and launches it while the steps run; it is kept if the LO ends
    // exactly there (else discarded), so results never depend on the speculation.
    const bool speculate = [] {
        return env_flag("MADPOSE_LO_SPECULATE", true);
    }();
    // Chained speculation (MADPOSE_LO_CHAIN=0 disables): the sampler job of the post-LO
    // batch (at `at`, Bs iterations, in `slot`) also draws the batch after it into the
    // other slot, whose batch -- the one that led to the LO -- is spent; if the
    // speculative batch comes next and leads to no LO, that one is next and is already
    // drawn when the host has read the speculative batch.
    const bool chain_on = [] {
        return env_flag("MADPOSE_LO_CHAIN", true);
    }();
    // gen[cur ^ 1] holds (or the sampler is still drawing, until chained()) the batch
    // of chain_B iterations from chain_at on
    bool chain_ready = false;
    uint32_t chain_at = 0, chain_B = 0;
    // One post-LO speculation: what the hook started, read once local_opt has returned
    struct Speculation {
        bool on = false;    // the sampler holds (and launches) the post-LO batch
        uint64_t draws = 0; // ... for an LO that leaves the selection stream at this draw count
        bool chain = false; // ... and then draws the batch after it: chain_B iterations from chain_at
        uint32_t chain_at = 0, chain_B = 0;
    };
    // The hook that local_opt calls with the predicted end of the selection stream, for
    // an LO after which iteration `at` comes next.  It runs on the estimator thread or on
    // an LO worker beside the steps, always inside local_opt, so it gets
    // copies of the loop state it reads -- the streams as rewound (the LO draws only from
    // its own copies of the selection stream and writes rs_ after LoWorkers::run has
    // returned), the free slot, the pre-LO best (LO leaves best_min_model_score alone,
    // src/hybrid_ransac.h:149-155) -- and writes only *sp.  sampler_busy: the sampler is
    // drawing the batch that would have come next without the LO.
    auto speculation_hook = [&](uint32_t at, bool sampler_busy, Speculation *sp) {
        const IterationStream rs_at_lo = rs_;
        const int slot = cur ^ 1;
        const double bound = best_min_score;
        Batch *const gs = &gen[slot];
        return [this, rs_at_lo, slot, bound, gs, at, sampler_busy, sp, max_total, speculate, chain_on, lo_start, &gen,
                &grow, &batch_size](const Mt19937 &sel_end) {
            if (!speculate || at >= max_total) return;
            if (sampler_busy) X_.sampler->cancel();
            IterationStream from = rs_at_lo;
            from.sel = sel_end;
            slot_free(slot);
            const uint32_t Bs = batch_size(at, sync_batch(grow(at)));
            // the chained batch goes into the other slot: its batch, the one that led to
            // the LO, is spent
            Sampler::Chain ch;
            const uint32_t at2 = at + Bs;
            const uint32_t B2 = chain_on && at2 < max_total && at2 != lo_start ? batch_size(at2, grow(at2)) : 0;
            if (B2 > 0) {
                slot_free(slot ^ 1);
                ch = Sampler::Chain{&gen[slot ^ 1], B2, slot ^ 1, slot_for(slot ^ 1, B2)};
            }
            sp->chain = B2 > 0;
            sp->chain_at = at2;
            sp->chain_B = B2;
            X_.sampler->start(from, gs, Bs, slot, slot_for(slot, Bs),
                              [this, gs, bound, at, lo_start] {
                                  // the sampler thread is not bound to the estimator's
                                  // device by itself
                                  MP_HIP(hipSetDevice(X_.device));
                                  launch_batch(*gs, bound, at >= lo_start);
                              },
                              sp->chain ? &ch : nullptr);
            sp->on = true;
            sp->draws = sel_end.draws();
        };
    };
    // after that LO: the speculative batch comes next if the LO ended where predicted
    // (and the run goes on: `keep`); else it is discarded
    auto join_speculation = [&](const Speculation &sp, bool keep) {
        have_next = false;
        if (keep && rs_.sel.draws() == sp.draws) {
            tl_.mark("join_spec");
            have_next = X_.sampler->finish(&rs_);
            tl_.mark("joined", have_next ? 1 : 0);
            if (have_next) {
                cur ^= 1;
                launched = true;
                chain_ready = sp.chain; // (still drawing, maybe: chained() below)
                chain_at = sp.chain_at;
                chain_B = sp.chain_B;
            }
        } else {
            X_.sampler->cancel();
            drain_batches(); // a launched speculation drains
        }
    };
    while (it < max_total && !done) {
        if (it == lo_start && best_min_score < kMax) {
            ++S->number_lo_iterations;
            // post-LO speculation as after the LOs of the walk below (the sampler is idle:
            // batches stop at lo_start)
            Speculation sp;
            tl_.mark("lo", (long)it);
            local_opt(S->best_solver_type, best, &S->best_model_score, &S->best_solver_type,
                      speculation_hook(it, false, &sp));
            tl_.mark("lo_end", sp.on ? 1 : 0);
            termination(*best, max_per);
            if (sp.on) join_speculation(sp, true);
        }
        // (drawn here only at the start and after LO / a cut batch: kept short so the
        // GPU starts early and the worker draws the big ones)
        if (!have_next) {
            auto t0 = Clock::now();
            tl_.mark("draw");
            slot_free(cur);
            generate(gen[cur], batch_size(it, sync_batch((uint32_t)bcur)), cur);
            if (gen[cur].B >= 256) draw_s_per_it_ = 0.5 * draw_s_per_it_ + 0.5 * secs(t0) / gen[cur].B;
        }
        auto t_batch = Clock::now();
        const Batch &g = gen[cur];
        const uint32_t B = g.B;
        if (!launched) {
            auto tl = Clock::now();
            tl_.mark("launch", (long)g.B);
            launch_batch(g, best_min_score, it >= lo_start);
            tl_.mark("launched");
            launch_s_ += secs(tl);
            ++launch_n_;
        } else {
            tl_.mark("prelaunched", (long)g.B);
        }
        launched = false;
        BatchBufs &Q = X_.bb[g.slot];
        const bool prof = batch_prof_[g.slot];
        // While the batch is in flight, the sampler thread draws the next one into the
        // other slot.  It is kept if this batch neither triggers LO nor terminates (both
        // rewind the streams); never across lo_start, where an LO runs before the next
        // batch.
        const uint32_t it_next = it + B;
        const uint32_t Bn0 = (it_next < max_total && it_next != lo_start)
                                 ? batch_size(it_next, grow(it_next))
                                 : 0;
        // the chained batch, when it starts where the next one does
        const bool use_chain = chain_ready && Bn0 > 0 && it_next == chain_at;
        if (chain_ready && !use_chain) X_.sampler->cancel(); // (not the next batch)
        chain_ready = false;
        const uint32_t Bn = use_chain ? chain_B : Bn0;
        if (Bn > 0 && !use_chain) {
            slot_free(cur ^ 1);
            X_.sampler->start(rs_, &gen[cur ^ 1], Bn, cur ^ 1, slot_for(cur ^ 1, Bn));
        }
        auto tw = Clock::now();
        tl_.mark("wait", (long)it);
        MP_HIP(hipEventSynchronize(Q.ev_done));
        tl_.mark("ready");
        S->seconds_gpu_wait += secs(tw);
        batch_s_ = 0.5 * batch_s_ + 0.5 * secs(t_batch);
        S->num_batches++;
        if (prof) {
            float ms_solve = 0.f, ms_score = 0.f;
            MP_HIP(hipEventElapsedTime(&ms_solve, Q.ev[0], Q.ev[1]));
            MP_HIP(hipEventElapsedTime(&ms_score, Q.ev[1], Q.ev[2]));
            tl_.mark("solve_us", (long)(1000.f * ms_solve));
            tl_.mark("score_us", (long)(1000.f * ms_score));
            uint64_t h = 0, trips = 0, scored = 0;
            for (uint32_t q = 0; q < B; ++q) {
                // (record-skipped iterations report their partial trips negated)
                const int c = Q.h_flags8[q] & 0x7f;
                h += (uint64_t)c;
                trips += (uint64_t)std::abs(Q.h_work[q]);
                if (Q.h_work[q] > 0) scored += (uint64_t)c;
            }
            std::lock_guard<std::mutex> lk(g_prof_mu);
            g_prof.model_trips += trips;
            g_prof.model_trips_full += h * (uint64_t)((n_ + 255) / 256);
            g_prof.batches += 1;
            g_prof.iterations += B;
            g_prof.hypotheses += h;
            g_prof.scored += scored;
            g_prof.correspondences += h * (uint64_t)n_;
            g_prof.solve_ms += ms_solve;
            g_prof.score_ms += ms_score;
        }

        std::vector<Model> dumped;
        if (model_dump_) {
            dumped.resize((size_t)B * maxm_);
            MP_HIP(hipMemcpyAsync(dumped.data(), Q.d_models, sizeof(Model) * dumped.size(), hipMemcpyDeviceToHost,
                                  X_.copy_stream));
            MP_HIP(hipStreamSynchronize(X_.copy_stream));
        }
        bool invalidated = false;
        Speculation sp; // (on: the sampler holds the post-LO speculation, not the Bn batch)
        uint32_t j = 0;
        const bool dumping = model_dump_ || count_dump_;
        for (; j < B; ++j) {
            // 64 iterations at a time while nothing happens in them: none marked, not
            // lo_starting_iterations, no solver type reaching its cap (the counts only
            // grow, so a cap reached inside the block is reached at its end)
            while (!dumping && j + 64 <= B && !(lo_start >= it + j && lo_start < it + j + 64)) {
                const uint8_t *f = Q.h_flags8 + j, *ty = g.types.data() + j;
                unsigned mk = 0, n1 = 0, hy = 0;
                for (int k = 0; k < 64; ++k) {
                    mk |= f[k];
                    n1 += ty[k];
                    hy += f[k] & 0x7fu;
                }
                const uint32_t n0 = 64 - n1;
                if ((mk & 0x80u) || S->num_iterations_per_solver[0] + n0 >= max_per[0] ||
                    S->num_iterations_per_solver[1] + n1 >= max_per[1])
                    break;
                S->num_iterations_per_solver[0] += n0;
                S->num_iterations_per_solver[1] += n1;
                S->num_hypotheses += hy;
                j += 64;
            }
            if (j >= B) break;
            const uint32_t iter = it + j;
            const int st = g.types[j];
            S->num_iterations_per_solver[st] += 1;
            const int nm = Q.h_flags8[j] & 0x7f;
            S->num_hypotheses += (uint64_t)nm;
            if (model_dump_) {
                const int32_t hdr[2] = {(int32_t)iter, (int32_t)nm};
                std::fwrite(hdr, sizeof(hdr), 1, model_dump_);
                std::fwrite(dumped.data() + (size_t)j * maxm_, sizeof(Model), (size_t)nm, model_dump_);
            }
            if (count_dump_) {
                const int *smp = slot_ptr(g.slot) + 8 * (size_t)j;
                std::fprintf(count_dump_, "%u %d %d", iter, st, nm);
                for (int q = 0; q < (st == 0 ? ss_[0][0] : ss_[1][2]); ++q) std::fprintf(count_dump_, " %d", smp[q]);
                std::fprintf(count_dump_, "\n");
            }
            bool lo_here = false;
            if (nm > 0) {
                // The device sums screen; the decision is taken on reference-order sums
                // (exact_score) -- see resolve_tie.  `maybe`: the iteration could hold a new
                // best (some model's lower bound is below the running best, or no bound
                // holds); `certain`: it does, and its best model is the reference's winner.
                // Unmarked iterations (flag byte without 0x80) cannot: their lo is at or
                // above the pre-batch best, which bounds the running best from above.
                const bool marked = (Q.h_flags8[j] & 0x80) != 0;
                const IterResult &res = Q.h_cand[j]; // (valid when marked)
                const double bl = marked ? res.best : kMax;
                const int raw = marked ? res.slot : 0;
                const bool uncertain = (raw & kSlotUncertain) != 0;
                const bool maybe = marked && (uncertain || (best_min_score == kMax ? bl < kMax : res.lo < best_min_score));
                if (maybe || iter == lo_start) {
                    bool new_best = false;
                    if (maybe) {
                        const bool certain = !uncertain && !(raw & kSlotAmbiguous) &&
                                             (best_min_score == kMax || res.hi < best_min_score);
                        Model m;
                        double e = kMax;
                        if (certain) {
                            m = fetch_model(Q, (int)j);
                            tl_.mark("exact", (long)iter);
                            e = exact_score(m);  // (below best_min_score: the bounds say so)
                        } else {
                            tl_.mark("resolve", (long)iter);
                            resolve_tie(Q, j, &m, &e);
                        }
                        tl_.mark("decided", e < best_min_score ? 1 : 0);
                        if (e < best_min_score) {
                            new_best = true;
                            best_min = m;
                            best_min_score = e;
                        }
                    }
                    if (new_best) {
                        if (trace_) std::fprintf(stderr, "[engine] it=%u new best %.17g (device %.17g, solver %d, %d models)\n",
                                                 iter, best_min_score, bl, st, nm);
                        update_best(best_min_score, best_min, st, &S->best_model_score, best, &S->best_solver_type);
                    }
                    // the reference enters this block only on a new best or at
                    // lo_starting_iterations (src/hybrid_ransac.h:123-124); a `maybe` that
                    // the exact sums reject is no entry
                    const bool run_lo = (new_best || iter == lo_start) && iter >= lo_start && best_min_score < kMax;
                    if (new_best || run_lo) {
                        if (run_lo) {
                            // rewind both streams to the end of iteration `iter`
                            rewind(g, j);
                            ++S->number_lo_iterations;
                            double sc = best_min_score;
                            tl_.mark("lo", (long)iter);
                            local_opt(S->best_solver_type, &best_min, &sc, &S->best_solver_type,
                                      speculation_hook(iter + 1, Bn > 0, &sp));
                            tl_.mark("lo_end", sp.on ? 1 : 0);
                            if (trace_) std::fprintf(stderr, "[engine] it=%u LO %.17g -> %.17g\n", iter, best_min_score, sc);
                            update_best(sc, best_min, st, &S->best_model_score, best, &S->best_solver_type);
                            lo_here = true;
                            invalidated = true;
                        }
                        termination(*best, max_per);
                    }
                }
            }
            if (S->num_iterations_per_solver[st] >= max_per[st]) {
                // `break` in the reference skips the loop increment
                S->num_iterations_total = iter;
                done = true;
                if (!lo_here) rewind(g, j);
                break;
            }
            if (invalidated) {
                it = iter + 1;
                break;
            }
        }
        if (!done && !invalidated) {
            it += B;
            have_next = false;
            if (Bn > 0 && use_chain) { // drawn during the LO and the walk (chained speculation)
                tl_.mark("chained", (long)Bn);
                IterationStream crs;
                if (X_.sampler->chained(&crs)) {
                    tl_.mark("chain_joined");
                    rs_ = crs;
                    have_next = true;
                    cur ^= 1;
                } // (else rs_ stands at the end of this batch)
            } else if (Bn > 0) { // rs_ moves to the end of the drawn batch
                auto t0 = Clock::now();
                tl_.mark("join_sampler");
                have_next = X_.sampler->finish(&rs_);
                tl_.mark("joined", have_next ? 1 : 0);
                sample_s_ += secs(t0);
                if (have_next) cur ^= 1;
            }
            // (otherwise rs_ stands at the end of this batch)
        } else if (sp.on) {
            join_speculation(sp, !done);
        } else {
            if (Bn > 0) X_.sampler->cancel();
            have_next = false;
        }
        bcur = (int)grow(it);
    }
    if (!done) S->num_iterations_total = it;
    // (a speculation launched past the end may still be in flight: the next run reuses
    // the buffers)
    X_.sampler->cancel();
    drain_batches();

    if (S->num_iterations_total <= lo_start && S->best_model_score < kMax) {
        ++S->number_lo_iterations;
        local_opt(S->best_solver_type, best, &S->best_model_score, &S->best_solver_type);
        termination(*best, max_per);
    }
    if (o_.final_least_squares) {
        auto t0 = Clock::now();
        Model refined = *best;
        least_squares(lanes_[0], S->inlier_indices, &refined, false);
        double sc;
        if (score_below(lanes_[0], refined, S->best_model_score, &sc) && sc < S->best_model_score) {
            S->best_model_score = sc;
            *best = refined;
            termination(*best, max_per);
        }
        S->seconds_lo += secs(t0);
    }
    S->seconds_total = secs(t_start);
    tl_.mark("end");
    for (const auto &e : tl_.ev) std::fprintf(stderr, "[timeline %ld] %10.1f %-14s %ld\n", tl_.run, e.us, e.what, e.a);
    double tsum[3] = {0, 0, 0};
    for (const Lane &L : lanes_) {
        S->num_lo_sweeps += L.count;
        for (int k = 0; k < 3; ++k) tsum[k] += L.t[k];
    }
    if (std::getenv("MADPOSE_LO_TIMING"))
        std::fprintf(stderr, "[engine] pair: %.1f us total, %d batches (%d launched by the estimator thread, %.1f us "
                     "each), gpu wait %.1f us, sampling %.1f us, LO %.1f us\n", 1e6 * S->seconds_total,
                     (int)S->num_batches, launch_n_, launch_n_ ? 1e6 * launch_s_ / launch_n_ : 0.0,
                     1e6 * S->seconds_gpu_wait, 1e6 * sample_s_, 1e6 * S->seconds_lo);
    if (std::getenv("MADPOSE_LO_TIMING") && lo_t_[2] > 0)
        std::fprintf(stderr, "[engine] %d LO: prefix %.1f us, steps %.1f us, step sum %.1f us, step0 %.1f us, longest "
                     "step %.1f us, step0 fit %.1f us, step0 score %.1f us, other fit %.1f us, step0 lsq %.1f us, "
                     "step0 iters %.1f us, other lsq %.1f us, other iters %.1f us (avg per LO), recomputed %.2f us\n",
                     (int)lo_t_[2], 1e6 * lo_t_[0] / lo_t_[2], 1e6 * lo_t_[1] / lo_t_[2], 1e6 * lo_t_[3] / lo_t_[2],
                     1e6 * lo_t_[5] / lo_t_[2], 1e6 * lo_t_[4], 1e6 * lo_t_[6] / lo_t_[2], 1e6 * lo_t_[7] / lo_t_[2],
                     1e6 * lo_t_[8] / lo_t_[2], 1e6 * lo_t_[9] / lo_t_[2], 1e6 * lo_t_[10] / lo_t_[2],
                     1e6 * lo_t_[11] / lo_t_[2], 1e6 * lo_t_[12] / lo_t_[2], lo_t_[13] / lo_t_[2]);
    if (lo_timing_ && lm_stat_[0] > 0)
        std::fprintf(stderr, "[engine] %d big LM solves: %.1f evaluations, %.0f blocks, %.1f us each (avg)\n",
                     (int)lm_stat_[0], lm_stat_[1] / lm_stat_[0], lm_stat_[3] / lm_stat_[0], 1e6 * lm_stat_[2] / lm_stat_[0]);
    if (std::getenv("MADPOSE_LO_TIMING") && lo_t_[2] > 0)
        std::fprintf(stderr, "[engine] LO steps phase: before the parallel run %.1f us, the run %.1f us, the speculation "
                     "hook %.1f us (avg per LO)\n",
                     1e6 * lo_seg_[0] / lo_t_[2], 1e6 * lo_seg_[1] / lo_t_[2], 1e6 * lo_seg_[2] / lo_t_[2]);
    if (std::getenv("MADPOSE_SWEEP_TIMING") && S->num_lo_sweeps > 0)
        std::fprintf(stderr, "[engine] %llu host sweeps: %.2f us (avg)\n", (unsigned long long)S->num_lo_sweeps,
                     1e6 * tsum[1] / S->num_lo_sweeps);
    if (g_prof_on.load(std::memory_order_relaxed)) {
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.sample_wall_ms += 1e3 * sample_s_;
        g_prof.wait_wall_ms += 1e3 * S->seconds_gpu_wait;
        g_prof.run_wall_ms += 1e3 * S->seconds_total;
        g_prof.accepted += S->num_hypotheses;
        g_prof.tie_checks += tie_checks_;
    }
}

void validate(const PairInput &in, const RansacOptions &o) {
    if (in.variant < 0 || in.variant > 3)
        throw std::invalid_argument("variant must be 0 (calibrated), 1 (shared focal), 2 (two focal) or 3 (scale only)");
    if (in.n < 0 || in.n > (int64_t)1 << 30) throw std::invalid_argument("bad number of correspondences");
    if (in.n > 0 && (!in.x0 || !in.x1 || !in.d0 || !in.d1)) throw std::invalid_argument("null input array");
    if (!(o.squared_inlier_thresholds[0] > 0) || !(o.squared_inlier_thresholds[1] > 0))
        throw std::invalid_argument("squared_inlier_thresholds must hold two positive values");

}

} // namespace

// (MADPOSE_PROF_OFF=1: profiling stays off whatever the caller asks -- A/B of its cost)
void profile_enable(bool on) {
    static const bool off = [] {
        return env_flag("MADPOSE_PROF_OFF", false);
    }();
    g_prof_on.store(on && !off);
}
void profile_reset() {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof = KernelProfile();
}
KernelProfile profile_read() {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    return g_prof;
}

void estimate_pair(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int device, Model *out,
                   Stats *stats) {
    validate(in, opts);
    CtxLease lease(device);
    Problem P = make_problem(in, opts, cfg);
    Run r(*lease.c, P, opts, cfg);
    r.run(out, stats);
    if (in.variant == kSF) {
        out->focal0 *= P.norm_scale;
        out->focal1 = out->focal0;
    } else if (in.variant == kTF) {
        out->focal0 *= P.norm_scale;
        out->focal1 *= P.norm_scale;
    }
}

namespace {
// device allocation freed on scope exit (error paths included)
template <class T> struct DevArray {
    T *p = nullptr;
    explicit DevArray(size_t n) { MP_HIP(hipMalloc(&p, sizeof(T) * std::max<size_t>(n, 1))); }
    ~DevArray() {
        if (p) hipFree(p);
    }
    DevArray(const DevArray &) = delete;
    DevArray &operator=(const DevArray &) = delete;
};
} // namespace

void score_models(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, const Model *models,
                  int nm, double *scores, double *errors, int device, double *norm_scale) {
    validate(in, opts);
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    Problem P = make_problem(in, opts, cfg);
    if (norm_scale) *norm_scale = P.norm_scale;
    X.ensure(in.n, 64, max_models(in.variant == kScaleOnly ? kCal : in.variant));
    PairData D;
    upload_pair(X, P, &D);
    std::vector<ScoreRec> recs(std::max(nm, 1));
    for (int m = 0; m < nm; ++m) prepare_score_rec(P.C, models[m], recs[m]);
    DevArray<ScoreRec> d_recs(recs.size());
    DevArray<double> d_sc(recs.size());
    MP_HIP(hipMemcpyAsync(d_recs.p, recs.data(), sizeof(ScoreRec) * nm, hipMemcpyHostToDevice, X.stream));
    MP_HIP(launch_score_models(X.stream, D, P.C, d_recs.p, nm, d_sc.p));
    MP_HIP(hipMemcpyAsync(scores, d_sc.p, sizeof(double) * nm, hipMemcpyDeviceToHost, X.stream));
    if (errors) {
        for (int m = 0; m < nm; ++m) {
            MP_HIP(launch_sweep(X.stream, D, P.C, d_recs.p + m, X.d_err, X.d_score1));
            MP_HIP(hipMemcpyAsync(errors + (size_t)m * 3 * in.n, X.d_err, sizeof(double) * 3 * in.n,
                                  hipMemcpyDeviceToHost, X.stream));
        }
    }
    MP_HIP(hipStreamSynchronize(X.stream));
}

// score_batch's per-correspondence errors and flags of explicit models, with each
// model's per-term bounds and margin (mp_debug_score_terms; test hook of the screening
// margins, mp_score.h score_margins)
void debug_score_terms(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, const Model *models,
                       int nm, double *errors, int *flags, double *taus, double *ties, int device) {
    validate(in, opts);
    if (nm <= 0) return;
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    Problem P = make_problem(in, opts, cfg);
    X.ensure(in.n, 64, max_models(in.variant == kScaleOnly ? kCal : in.variant));
    PairData D;
    upload_pair(X, P, &D);
    std::vector<ScoreRec> recs(nm);
    for (int m = 0; m < nm; ++m) {
        prepare_score_rec(P.C, models[m], recs[m], taus ? taus + 3 * m : nullptr);
        if (ties) ties[m] = recs[m].tie;
    }
    DevArray<ScoreRec> d_recs(nm);
    DevArray<double> d_err((size_t)nm * 3 * in.n);
    DevArray<int> d_flags((size_t)nm * in.n);
    MP_HIP(hipMemcpyAsync(d_recs.p, recs.data(), sizeof(ScoreRec) * nm, hipMemcpyHostToDevice, X.stream));
    MP_HIP(launch_debug_terms(X.stream, D, P.C, d_recs.p, nm, d_err.p, d_flags.p));
    MP_HIP(hipMemcpyAsync(errors, d_err.p, sizeof(double) * nm * 3 * in.n, hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipMemcpyAsync(flags, d_flags.p, sizeof(int) * nm * in.n, hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipStreamSynchronize(X.stream));
}

// the margins score_batch would use for explicit models, formed on the host as for the
// device records (mp_debug_score_margins; test hook, no device)
void debug_score_margins(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg,
                         const Model *models, int nm, double *per_model, double *per_pair) {
    validate(in, opts);
    Problem P = make_problem(in, opts, cfg);
    for (int m = 0; m < nm; ++m) {
        ScoreRec r;
        double *o = per_model + 8 * (size_t)m;
        prepare_score_rec(P.C, models[m], r, o);
        o[3] = r.wz0;
        o[4] = r.wz1;
        o[5] = r.wl;
        o[6] = r.kg2;
        o[7] = r.tie;
    }
    if (per_pair) {
        for (int t = 0; t < 3; ++t) {
            per_pair[t] = P.C.thr[t];
            per_pair[3 + t] = P.C.w[t];
        }
        per_pair[6] = P.norm_scale;
        per_pair[7] = P.C.loss_scale;
        per_pair[8] = P.C.kstd;
    }
}

void lo_sweep_models(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, const Model *models,
                     int nm, double *scores, double *errors, double *fast_bounds) {
    validate(in, opts);
    Problem P = make_problem(in, opts, cfg);
    LoSweepData D;
    lo_sweep_prepare(P.C, P.H.x0.data(), P.H.x1.data(), P.H.d0.data(), P.H.d1.data(), &D);
    std::vector<double> err(3 * (size_t)std::max<int64_t>(in.n, 1));
    for (int m = 0; m < nm; ++m) {
        scores[m] = lo_sweep(P.C, D, models[m], err.data());
        if (errors) std::memcpy(errors + (size_t)m * 3 * in.n, err.data(), sizeof(double) * 3 * in.n);
        if (fast_bounds) lo_sweep_fast(P.C, D, models[m], err.data(), fast_bounds + 2 * m, fast_bounds + 2 * m + 1);
    }
}

// score_batch on explicit per-iteration model lists (mp_debug_score_batch, test hook):
// the estimator's launch with the pre-batch best `best`, and the exact early exit /
// record skip as flags allow; results, bounds, margins and record models back
void debug_score_batch(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int nb,
                       const int *counts, const Model *models, double best, int flags, double *res_best,
                       int *res_slot, Model *rec_models, double *res_hi_lo, double *model_ties, int device) {
    validate(in, opts);
    const int v = in.variant == kScaleOnly ? kCal : in.variant;
    const int maxm = max_models(v);
    if (nb <= 0 || nb > (1 << 20)) throw std::invalid_argument("bad iteration count");
    for (int b = 0; b < nb; ++b)
        if (counts[b] < 0 || counts[b] > maxm) throw std::invalid_argument("model count out of range");
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    Problem P = make_problem(in, opts, cfg);
    X.ensure(in.n, nb, maxm);
    PairData D;
    upload_pair(X, P, &D);
    BatchBufs &Q = X.bb[0];
    std::vector<ScoreRec> recs((size_t)nb * maxm);
    std::vector<Model> ms((size_t)nb * maxm);
    std::memset(ms.data(), 0, sizeof(Model) * ms.size());
    std::memset(recs.data(), 0, sizeof(ScoreRec) * recs.size());
    for (int b = 0; b < nb; ++b)
        for (int m = 0; m < counts[b]; ++m) {
            ms[(size_t)b * maxm + m] = models[(size_t)b * maxm + m];
            prepare_score_rec(P.C, ms[(size_t)b * maxm + m], recs[(size_t)b * maxm + m]);
        }
    if (model_ties)
        for (size_t k = 0; k < recs.size(); ++k) model_ties[k] = recs[k].tie;
    MP_HIP(hipMemcpyAsync(Q.d_recs, recs.data(), sizeof(ScoreRec) * recs.size(), hipMemcpyHostToDevice, X.stream));
    MP_HIP(hipMemcpyAsync(Q.d_models, ms.data(), sizeof(Model) * ms.size(), hipMemcpyHostToDevice, X.stream));
    MP_HIP(hipMemcpyAsync(Q.d_counts, counts, sizeof(int) * nb, hipMemcpyHostToDevice, X.stream));
    std::memset(Q.h_recmodel, 0, sizeof(Model) * nb);
    const bool exit = (flags & 1) != 0, skip = (flags & 2) != 0;
    const unsigned epoch_hi = ~(++X.epoch);
    MP_HIP(launch_score_batch(X.stream, D, P.C, Q.d_recs, Q.d_counts, nb, maxm, Q.d_scores, Q.d_res,
                              exit ? best : DBL_MAX, nullptr, skip ? X.d_recword : nullptr, epoch_hi, Q.d_models,
                              Q.d_recmodel));
    std::vector<IterResult> res(nb);
    MP_HIP(hipMemcpyAsync(res.data(), Q.d_res, sizeof(IterResult) * nb, hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipStreamSynchronize(X.stream));
    for (int b = 0; b < nb; ++b) {
        res_best[b] = res[b].best;
        res_slot[b] = res[b].slot;
        if (res_hi_lo) {
            res_hi_lo[2 * b] = res[b].hi;
            res_hi_lo[2 * b + 1] = res[b].lo;
        }
    }
    if (rec_models) std::memcpy(rec_models, Q.h_recmodel, sizeof(Model) * nb);
}

namespace {
// the problem lists of mp_lm_refine_batch: offsets[0] >= 0, non-decreasing, every
// index inside the pair (checked once, before either LM touches them)
void validate_lm_batch(const PairInput &in, int nprob, const int64_t *offsets, const int32_t *idx, const Model *models,
                       const int32_t *status) {
    if (nprob < 0) throw std::invalid_argument("negative problem count");
    if (nprob == 0) return;
    if (!offsets || !models || !status) throw std::invalid_argument("null offsets, models or status");
    if (offsets[0] < 0) throw std::invalid_argument("sample offsets must be non-negative");
    for (int64_t k = 0; k < 3 * (int64_t)nprob; ++k)
        if (offsets[k + 1] < offsets[k]) throw std::invalid_argument("sample offsets must not decrease");
    if (offsets[3 * (int64_t)nprob] > offsets[0] && !idx) throw std::invalid_argument("null index list");
    for (int64_t k = offsets[0]; k < offsets[3 * (int64_t)nprob]; ++k)
        if (idx[k] < 0 || idx[k] >= in.n) throw std::invalid_argument("sample index out of range");
}
// the host LM's settings of a job (the same Ceres settings as the device LM reads from it)
LMSettings lm_settings(const EstimatorConfig &cfg, const LmJob &J) {
    LMSettings S;
    S.use_reproj = cfg.lo_type != 1;
    S.use_sampson = cfg.lo_type != 2;
    S.use_shift = J.use_shift != 0;
    S.min_depth_constraint = J.min_depth_constraint != 0;
    S.w_sampson = J.w_sampson;
    S.ftol = J.ftol;
    S.gtol = J.gtol;
    S.ptol = J.ptol;
    S.max_iter = J.max_iter;
    S.nonmonotonic = J.nonmonotonic != 0;
    return S;
}
} // namespace

// the same problems through the host LM (host/lm.cpp) -- test hook (mp_debug_lm_refine_host);
// kinds may be NULL (every problem a LeastSquares call)
void lm_refine_batch_host(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int nprob,
                          const int32_t *kinds, const int64_t *offsets, const int32_t *idx, Model *models,
                          int32_t *status) {
    validate(in, opts);
    validate_lm_batch(in, nprob, offsets, idx, models, status);
    Problem P = make_problem(in, opts, cfg);
    const int v = P.C.variant;
    const int kmd = v == kCal ? 3 : 4, kpt = v == kCal ? 5 : (v == kSF ? 6 : 7);
    for (int j = 0; j < nprob; ++j) {
        std::vector<int> smp[3];
        int sz[3];
        for (int t = 0; t < 3; ++t) {
            smp[t].assign(idx + offsets[3 * j + t], idx + offsets[3 * j + t + 1]);
            sz[t] = (int)smp[t].size();
        }
        if ((sz[0] < kmd && sz[1] < kmd) || sz[2] < kpt) {
            status[j] = 3;
            continue;
        }
        const LmJob J = make_lm_job(P, cfg, sz, 0, kinds && kinds[j] == 1, models[j]);
        const LMSettings S = lm_settings(cfg, J);
        status[j] = lm_refine(P.H, smp, S, &models[j]) ? 1 : 0;
    }
}

void lm_refine_batch_device(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int nprob,
                            const int32_t *kinds, const int64_t *offsets, const int32_t *idx, Model *models,
                            int32_t *status, int device) {
    validate(in, opts);
    validate_lm_batch(in, nprob, offsets, idx, models, status);
    if (nprob <= 0) return;
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    Problem P = make_problem(in, opts, cfg);
    X.ensure(in.n, 64, max_models(in.variant == kScaleOnly ? kCal : in.variant));
    PairData D;
    upload_pair(X, P, &D);
    const int v = P.C.variant;
    const int kmd = v == kCal ? 3 : 4, kpt = v == kCal ? 5 : (v == kSF ? 6 : 7);
    std::vector<LmJob> jobs;
    std::vector<int> which;
    for (int j = 0; j < nprob; ++j) {
        int sz[3];
        for (int t = 0; t < 3; ++t) sz[t] = (int)(offsets[3 * j + t + 1] - offsets[3 * j + t]);
        // too few data for the solver (the size test of least_squares)
        if ((sz[0] < kmd && sz[1] < kmd) || sz[2] < kpt) {
            status[j] = 3;
            continue;
        }
        jobs.push_back(make_lm_job(P, cfg, sz, (int)offsets[3 * j], kinds && kinds[j] == 1, models[j]));
        which.push_back(j);
    }
    if (jobs.empty()) return;
    const int64_t nidx = offsets[3 * nprob];
    DevArray<LmJob> d_jobs(jobs.size());
    DevArray<int> d_idx((size_t)nidx), d_status(jobs.size());
    DevArray<Model> d_out(jobs.size());
    MP_HIP(hipMemcpyAsync(d_jobs.p, jobs.data(), sizeof(LmJob) * jobs.size(), hipMemcpyHostToDevice, X.stream));
    if (nidx > 0) MP_HIP(hipMemcpyAsync(d_idx.p, idx, sizeof(int) * nidx, hipMemcpyHostToDevice, X.stream));
    MP_HIP(launch_lm_batch(X.stream, D, P.C, d_jobs.p, (int)jobs.size(), d_idx.p, d_out.p, d_status.p));
    std::vector<Model> out(jobs.size());
    std::vector<int> st(jobs.size());
    MP_HIP(hipMemcpyAsync(out.data(), d_out.p, sizeof(Model) * out.size(), hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipMemcpyAsync(st.data(), d_status.p, sizeof(int) * st.size(), hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipStreamSynchronize(X.stream));
    for (size_t k = 0; k < which.size(); ++k) {
        models[which[k]] = out[k];
        status[which[k]] = st[k];
    }
}

// One evaluation and one step of every problem at its start model -- test hook
// (mp_debug_lm_system).  No size rule: any lists, empty ones included.  where 0: the
// device (lm_system_kernel), 1 / 2: the host's 4- / 8-wide residual evaluation over the
// block range ranges[2j], ranges[2j + 1] (null or negative: all blocks), 3: the host LM's
// evaluate().
void lm_system_batch(const PairInput &in, const RansacOptions &opts, const EstimatorConfig &cfg, int nprob,
                     const int32_t *kinds, const int64_t *offsets, const int32_t *idx, const Model *models,
                     const double *radius, int where, const int64_t *ranges, LmSystem *out, int32_t *status,
                     int device) {
    validate(in, opts);
    validate_lm_batch(in, nprob, offsets, idx, models, status);
    if (!radius || !out) throw std::invalid_argument("null radius or output");
    if (where < 0 || where > 3) throw std::invalid_argument("where must be 0..3");
    if (where == 2 && !lm_debug_have_w8()) throw std::invalid_argument("no AVX-512 on this CPU");
    if (nprob <= 0) return;
    Problem P = make_problem(in, opts, cfg);
    std::vector<LmJob> jobs;
    for (int j = 0; j < nprob; ++j) {
        int sz[3];
        for (int t = 0; t < 3; ++t) sz[t] = (int)(offsets[3 * j + t + 1] - offsets[3 * j + t]);
        jobs.push_back(make_lm_job(P, cfg, sz, (int)offsets[3 * j], kinds && kinds[j] == 1, models[j]));
    }
    if (where != 0) {
        for (int j = 0; j < nprob; ++j) {
            std::vector<int> smp[3];
            for (int t = 0; t < 3; ++t) smp[t].assign(idx + offsets[3 * j + t], idx + offsets[3 * j + t + 1]);
            lm_debug_system(P.H, smp, lm_settings(cfg, jobs[j]), models[j], radius[j], where,
                            ranges ? (long long)ranges[2 * j] : -1, ranges ? (long long)ranges[2 * j + 1] : -1, &out[j]);
            const int nb = jobs[j].n0 + jobs[j].n1 + jobs[j].n2;
            status[j] = nb == 0 ? 0 : (out[j].pd < 0 ? 2 : 1);
        }
        return;
    }
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    X.ensure(in.n, 64, max_models(in.variant == kScaleOnly ? kCal : in.variant));
    PairData D;
    upload_pair(X, P, &D);
    const int64_t nidx = offsets[3 * nprob];
    DevArray<LmJob> d_jobs(jobs.size());
    DevArray<int> d_idx((size_t)std::max<int64_t>(nidx, 1)), d_status(jobs.size());
    DevArray<double> d_radius(jobs.size());
    DevArray<LmSystem> d_sys(jobs.size());
    MP_HIP(hipMemcpyAsync(d_jobs.p, jobs.data(), sizeof(LmJob) * jobs.size(), hipMemcpyHostToDevice, X.stream));
    MP_HIP(hipMemcpyAsync(d_radius.p, radius, sizeof(double) * jobs.size(), hipMemcpyHostToDevice, X.stream));
    if (nidx > 0) MP_HIP(hipMemcpyAsync(d_idx.p, idx, sizeof(int) * nidx, hipMemcpyHostToDevice, X.stream));
    MP_HIP(launch_lm_system(X.stream, D, P.C, d_jobs.p, (int)jobs.size(), d_idx.p, d_radius.p, d_sys.p, d_status.p));
    std::vector<int> st(jobs.size());
    MP_HIP(hipMemcpyAsync(out, d_sys.p, sizeof(LmSystem) * jobs.size(), hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipMemcpyAsync(st.data(), d_status.p, sizeof(int) * st.size(), hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipStreamSynchronize(X.stream));
    for (int j = 0; j < nprob; ++j) status[j] = st[j];
}

#include "resident_pairs.h"

namespace {
// refine_run's device arrays for up to `cap` entries (null there: its own, for the call);
// ransac_lo_set sizes them once for its selection and passes them to every round's run
struct RefineBuffers {
    size_t cap;
    DevArray<RefineItem> d_items;
    DevArray<ScoreRec> d_recs;
    DevArray<RefineSweepOut> d_out;
    DevArray<LmJob> d_jobs;
    DevArray<LmPairRef> d_refs;
    DevArray<Model> d_models;
    DevArray<int> d_status;
    std::unique_ptr<DevArray<RelaxedSweepOut>> d_rout; // the relaxed first sweep only
    RefineBuffers(size_t n, bool relax)
        : cap(n), d_items(n), d_recs(n), d_out(n), d_jobs(n), d_refs(n), d_models(n), d_status(n) {
        if (relax) d_rout.reset(new DevArray<RelaxedSweepOut>(n));
    }
};

// Refinement of the models of the selected resident pairs (refine_batch's rounds; the body of
// mp_refine_batch and mp_refine_set).  models / results: entry j of the selection; the
// accepted models' lists of entry j to inlier_idx + 3 out_off[j] + t n_j (nullable).
// Per-call state only: each pair's list buffer choice starts at 0, and the lists read are
// the ones this call wrote.
// relax (mp_refine_relaxed_set; the local optimisation of ransac_lo_set): the first sweep is
// launch_refine_sweep_relaxed with the factor `multiplier` (threshold_multiplier), and round 0
// -- its size test and its LM job -- reads the relaxed counts and lists (the estimators'
// m_init, LocalOptimization's first act, src/hybrid_ransac.h:383-411); its candidate is swept
// over the relaxed lists' buffer, which are dead by then.  Everything else, the result's
// tight counts and lists included, is as without.
// swept (nullable; one per entry): the problem-unit model cur[j] the returned lists of entry j
// were swept from, whether or not a round was accepted (mp_ransac_out_set evaluates it again).
void refine_run(ResidentPairs &R, hipStream_t stream, const PairSel sel, const int64_t *out_off,
                const EstimatorConfig &cfg, int rounds, Model *models, RefineResult *results, int32_t *inlier_idx,
                bool relax = false, double multiplier = 1.0, RefineBuffers *bufs = nullptr, Model *swept = nullptr) {
    const int ns = sel.n;
    if (ns == 0) return;
    const int variant = R.variant, v = R.v;
    const int kmd = v == kCal ? 3 : 4, kpt = v == kCal ? 5 : (v == kSF ? 6 : 7);
    const int64_t T = R.T;
    int *d_lists = R.lists(2);
    const std::vector<PairConst> &Ch = R.Ch;

    // ---- per-pair state (models in problem units) ----
    std::vector<Model> cur(ns);
    std::vector<double> score(ns, 0.0);
    std::vector<int> buf(ns, 0);
    for (int j = 0; j < ns; ++j) {
        const int k = sel[j];
        cur[j] = models[j];
        if (variant == kSF || variant == kTF) {
            cur[j].focal0 /= R.norm_scale[k];
            cur[j].focal1 /= R.norm_scale[k];
        }
        RefineResult &Q = results[j];
        std::memset(&Q, 0, sizeof(Q));
        Q.norm_scale = R.norm_scale[k];
        Q.lm_status = -1;
    }
    std::unique_ptr<RefineBuffers> own;
    if (!bufs) {
        own.reset(new RefineBuffers(ns, relax));
        bufs = own.get();
    }
    if (bufs->cap < (size_t)ns || (relax && !bufs->d_rout)) throw std::logic_error("refine_run: buffers too small");
    DevArray<RefineItem> &d_items = bufs->d_items;
    DevArray<ScoreRec> &d_recs = bufs->d_recs;
    DevArray<RefineSweepOut> &d_out = bufs->d_out;
    DevArray<LmJob> &d_jobs = bufs->d_jobs;
    DevArray<LmPairRef> &d_refs = bufs->d_refs;
    DevArray<Model> &d_models = bufs->d_models;
    DevArray<int> &d_status = bufs->d_status;
    std::vector<RefineItem> items;
    std::vector<ScoreRec> recs;
    std::vector<RefineSweepOut> outs;
    // one sweep launch: model ms[i] of selection entry js[i], lists into the buffer items[i].buf
    auto sweep = [&](const std::vector<int> &js, const std::vector<Model> &ms, bool other_buf) {
        const size_t m = js.size();
        items.resize(m);
        recs.resize(m);
        outs.resize(m);
        if (m == 0) return;
        for (size_t i = 0; i < m; ++i) {
            items[i].pair = sel[js[i]];
            items[i].buf = other_buf ? buf[js[i]] ^ 1 : buf[js[i]];
            prepare_score_rec(Ch[sel[js[i]]], ms[i], recs[i]);
        }
        MP_HIP(hipMemcpyAsync(d_items.p, items.data(), sizeof(RefineItem) * m, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(d_recs.p, recs.data(), sizeof(ScoreRec) * m, hipMemcpyHostToDevice, stream));
        MP_HIP(launch_refine_sweep(stream, v, R.d_D.p, R.d_C.p, d_items.p, d_recs.p, (int)m, R.d_list_off.p, d_lists,
                                   3 * T, d_out.p));
        MP_HIP(hipMemcpyAsync(outs.data(), d_out.p, sizeof(RefineSweepOut) * m, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipStreamSynchronize(stream));
    };

    // ---- the initial sweep: score and lists of the given models ----
    std::vector<int> running(ns);
    for (int j = 0; j < ns; ++j) running[j] = j;
    std::vector<int> relaxed; // relax: entry j's relaxed counts at 3 j, their lists in its buffer 1
    if (!relax) {
        sweep(running, cur, false);
        for (int j = 0; j < ns; ++j) {
            RefineResult &Q = results[j];
            score[j] = Q.score_initial = Q.score_final = outs[j].score;
            for (int t = 0; t < 3; ++t) Q.num_inliers[t] = outs[j].count[t];
        }
    } else {
        DevArray<RelaxedSweepOut> &d_rout = *bufs->d_rout;
        std::vector<RelaxedSweepOut> routs(ns);
        items.resize(ns);
        recs.resize(ns);
        for (int j = 0; j < ns; ++j) {
            items[j].pair = sel[j];
            items[j].buf = 0;
            prepare_score_rec(Ch[sel[j]], cur[j], recs[j]);
        }
        MP_HIP(hipMemcpyAsync(d_items.p, items.data(), sizeof(RefineItem) * ns, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(d_recs.p, recs.data(), sizeof(ScoreRec) * ns, hipMemcpyHostToDevice, stream));
        MP_HIP(launch_refine_sweep_relaxed(stream, v, R.d_D.p, R.d_C.p, d_items.p, d_recs.p, ns, R.d_list_off.p,
                                           d_lists, 3 * T, multiplier, d_rout.p));
        MP_HIP(hipMemcpyAsync(routs.data(), d_rout.p, sizeof(RelaxedSweepOut) * ns, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipStreamSynchronize(stream));
        relaxed.resize(3 * (size_t)ns);
        for (int j = 0; j < ns; ++j) {
            RefineResult &Q = results[j];
            score[j] = Q.score_initial = Q.score_final = routs[j].score;
            for (int t = 0; t < 3; ++t) {
                Q.num_inliers[t] = routs[j].count[t];
                relaxed[3 * (size_t)j + t] = routs[j].relaxed[t];
            }
        }
    }
    // ---- rounds ----
    std::vector<LmJob> jobs;
    std::vector<LmPairRef> refs;
    std::vector<int> which, st, cand_j;
    std::vector<Model> lm_out, cand_m;
    for (int round = 0; round < rounds && !running.empty(); ++round) {
        jobs.clear();
        refs.clear();
        which.clear();
        for (int j : running) {
            const int k = sel[j];
            RefineResult &Q = results[j];
            ++Q.rounds_run;
            // (relax: round 0 reads the relaxed lists; every entry is still at buffer 0 then)
            const bool wide = relax && round == 0;
            const int *sz = wide ? &relaxed[3 * (size_t)j] : Q.num_inliers;
            // too few data for the solver (the size test of least_squares): the pair stops
            if ((sz[0] < kmd && sz[1] < kmd) || sz[2] < kpt) {
                Q.lm_status = 3;
                continue;
            }
            LmJob J = make_lm_job(R.Ps[k], cfg, sz, 0, false, cur[j]);
            // (the lists of a pair lie n apart, not back to back)
            J.off1 = Ch[k].n;
            J.off2 = 2 * Ch[k].n;
            jobs.push_back(J);
            LmPairRef ref;
            ref.pair = k;
            ref.pad = 0;
            ref.idx_off = refine_list(T, R.off[k], Ch[k].n, wide ? buf[j] ^ 1 : buf[j], 0);
            refs.push_back(ref);
            which.push_back(j);
        }
        running.clear();
        if (jobs.empty()) break;
        const size_t nj = jobs.size();
        lm_out.resize(nj);
        st.resize(nj);
        MP_HIP(hipMemcpyAsync(d_jobs.p, jobs.data(), sizeof(LmJob) * nj, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(d_refs.p, refs.data(), sizeof(LmPairRef) * nj, hipMemcpyHostToDevice, stream));
        MP_HIP(launch_lm_pairs(stream, v, R.d_D.p, R.d_C.p, d_jobs.p, d_refs.p, (int)nj, d_lists, d_models.p,
                               d_status.p));
        MP_HIP(hipMemcpyAsync(lm_out.data(), d_models.p, sizeof(Model) * nj, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipMemcpyAsync(st.data(), d_status.p, sizeof(int) * nj, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipStreamSynchronize(stream));
        cand_j.clear();
        cand_m.clear();
        for (size_t i = 0; i < nj; ++i) {
            results[which[i]].lm_status = st[i];
            if (st[i] != 1) continue; // (model unchanged: the pair stops)
            cand_j.push_back(which[i]);
            cand_m.push_back(lm_out[i]);
        }
        // the candidates' scores and lists, into each pair's other list buffer
        sweep(cand_j, cand_m, true);
        for (size_t i = 0; i < cand_j.size(); ++i) {
            const int j = cand_j[i];
            if (!(outs[i].score < score[j])) continue; // (not strictly lower: the pair stops)
            RefineResult &Q = results[j];
            cur[j] = cand_m[i];
            score[j] = Q.score_final = outs[i].score;
            for (int t = 0; t < 3; ++t) Q.num_inliers[t] = outs[i].count[t];
            buf[j] ^= 1;
            ++Q.rounds_accepted;
            running.push_back(j);
        }
    }
    for (int j = 0; swept && j < ns; ++j) swept[j] = cur[j];
    // ---- results: models back in user units, the accepted models' lists ----
    for (int j = 0; j < ns; ++j) {
        if (results[j].rounds_accepted == 0) continue; // (the given model, untouched)
        const double norm = R.norm_scale[sel[j]];
        Model m = cur[j];
        if (variant == kSF) {
            m.focal0 *= norm;
            m.focal1 = m.focal0;
        } else if (variant == kTF) {
            m.focal0 *= norm;
            m.focal1 *= norm;
        }
        models[j] = m;
    }
    if (inlier_idx && T > 0) {
        if (!sel.ids) { // every pair: the buffers in one copy
            const bool both = std::any_of(buf.begin(), buf.end(), [](int b) { return b != 0; });
            std::vector<int> lists((both ? 6 : 3) * (size_t)T);
            MP_HIP(hipMemcpyAsync(lists.data(), d_lists, sizeof(int) * lists.size(), hipMemcpyDeviceToHost, stream));
            MP_HIP(hipStreamSynchronize(stream));
            for (int j = 0; j < ns; ++j) {
                const int64_t n = Ch[j].n;
                for (int t = 0; t < 3; ++t)
                    std::memcpy(inlier_idx + 3 * out_off[j] + t * n, lists.data() + refine_list(T, R.off[j], n, buf[j], t),
                                sizeof(int) * (size_t)results[j].num_inliers[t]);
            }
        } else { // a selection: only its pairs' lists
            for (int j = 0; j < ns; ++j) {
                const int k = sel[j];
                const int64_t n = Ch[k].n;
                for (int t = 0; t < 3; ++t)
                    if (results[j].num_inliers[t] > 0)
                        MP_HIP(hipMemcpyAsync(inlier_idx + 3 * out_off[j] + t * n,
                                              d_lists + refine_list(T, R.off[k], n, buf[j], t),
                                              sizeof(int) * (size_t)results[j].num_inliers[t], hipMemcpyDeviceToHost,
                                              stream));
            }
        }
    }
    MP_HIP(hipStreamSynchronize(stream));
}

// lsq_fit_run's device arrays: grown to the largest run seen, so the stages of one
// ransac_lo_steps_set checkpoint (and the runs of one call) share them
struct LsqBuffers {
    size_t cap = 0, ws_cap = 0;
    std::unique_ptr<DevArray<LsqEntry>> d_entries;
    std::unique_ptr<DevArray<ScoreRec>> d_recs;
    std::unique_ptr<DevArray<LsqOut>> d_out;
    std::unique_ptr<DevArray<LmJob>> d_jobs;
    std::unique_ptr<DevArray<LmPairRef>> d_refs;
    std::unique_ptr<DevArray<Model>> d_models;
    std::unique_ptr<DevArray<int>> d_status;
    std::unique_ptr<DevArray<int>> d_ws;
    void ensure(size_t entries, size_t ws_ints) {
        if (entries > cap) {
            d_entries.reset(), d_recs.reset(), d_out.reset(), d_jobs.reset();
            d_refs.reset(), d_models.reset(), d_status.reset();
            d_entries.reset(new DevArray<LsqEntry>(entries));
            d_recs.reset(new DevArray<ScoreRec>(entries));
            d_out.reset(new DevArray<LsqOut>(entries));
            d_jobs.reset(new DevArray<LmJob>(entries));
            d_refs.reset(new DevArray<LmPairRef>(entries));
            d_models.reset(new DevArray<Model>(entries));
            d_status.reset(new DevArray<int>(entries));
            cap = entries;
        }
        if (ws_ints > ws_cap || !d_ws) {
            d_ws.reset(); // (free first)
            d_ws.reset(new DevArray<int>(ws_ints));
            ws_cap = ws_ints;
        }
    }
};

// One least-squares fit on a random subset of each entry's inliers (the body of
// mp_lsq_fit_set; the stages of ransac_lo_steps_set).  Entry e: model models[e] (user units,
// in and out) of pair pair_ids[e] (null: e) of the resident pairs -- a pair may occur in any
// number of entries, each has its own workspace slice and the pairs' list buffers are not
// touched.  Per run of entries (host/lsq_fit_plan.h): the records prepared on the host
// (prepare_score_rec: mp_score_models' bits), launch_lsq_sweep and launch_lsq_subset, the
// counts back (the first synchronisation); the rule's skip and mp_lm_refine_batch's size test
// on the subset's sizes (either: status 3, the model's bytes kept); make_lm_job on the subset's
// sizes (kind 1 for the rule kSubsetNonmin) with the lists in the entry's slice, one
// launch_lm_pairs, models and statuses back (the second).  Status 1: the LM's model in user
// units, as refine_run returns them; any other status keeps the input bytes.  subset_idx
// (nullable): entry e's subset lists to subset_idx + 3 out_off[e] + t n_e.
void lsq_fit_run(ResidentPairs &R, hipStream_t stream, const RansacOptions &opts, const EstimatorConfig &cfg,
                 int32_t ne, const int32_t *pair_ids, const int32_t *solver_types, const double *factors, int rule,
                 uint64_t seed, const int32_t *streams, const int32_t *substreams, Model *models,
                 LsqFitResult *results, int32_t *subset_idx, const int64_t *out_off, int64_t entry_chunk,
                 LsqBuffers &B) {
    if (ne <= 0) return;
    const int variant = R.variant, v = R.v;
    const int kmd = v == kCal ? 3 : 4, kpt = v == kCal ? 5 : (v == kSF ? 6 : 7);
    const std::vector<PairConst> &Ch = R.Ch;
    auto pair_of = [&](int32_t e) { return pair_ids ? pair_ids[e] : e; };
    std::vector<int64_t> ns((size_t)ne);
    for (int32_t e = 0; e < ne; ++e) ns[(size_t)e] = R.n[(size_t)pair_of(e)];
    std::vector<LsqEntry> entries;
    std::vector<ScoreRec> recs;
    std::vector<LsqOut> outs;
    std::vector<Model> cur, lm_out;
    std::vector<LmJob> jobs;
    std::vector<LmPairRef> refs;
    std::vector<int> which, st;
    for (const LsqRun &run : lsq_fit_runs(ne, ns.data(), entry_chunk)) {
        const size_t m = (size_t)(run.e1 - run.e0);
        entries.resize(m);
        recs.resize(m);
        outs.resize(m);
        cur.resize(m);
        int64_t ws_ints = 0;
        for (size_t i = 0; i < m; ++i) {
            const int32_t e = run.e0 + (int32_t)i;
            const int k = pair_of(e);
            cur[i] = models[e];
            if (variant == kSF || variant == kTF) {
                cur[i].focal0 /= R.norm_scale[(size_t)k];
                cur[i].focal1 /= R.norm_scale[(size_t)k];
            }
            LsqEntry &E = entries[i];
            E.pair = k;
            E.stype = solver_types[e];
            E.rule = rule;
            E.k = 0;
            E.stream = (uint32_t)streams[e];
            E.substream = (uint32_t)substreams[e];
            E.stride = (int)ns[(size_t)e];
            E.pad = 0;
            E.ws_off = ws_ints;
            E.factor = factors[e];
            ws_ints += 6 * ns[(size_t)e];
            prepare_score_rec(Ch[(size_t)k], cur[i], recs[i]);
        }
        B.ensure(m, (size_t)ws_ints);
        MP_HIP(hipMemcpyAsync(B.d_entries->p, entries.data(), sizeof(LsqEntry) * m, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(B.d_recs->p, recs.data(), sizeof(ScoreRec) * m, hipMemcpyHostToDevice, stream));
        MP_HIP(launch_lsq_sweep(stream, v, R.d_D.p, R.d_C.p, B.d_entries->p, B.d_recs->p, (int)m, B.d_ws->p,
                                B.d_out->p));
        MP_HIP(launch_lsq_subset(stream, B.d_entries->p, (int)m, B.d_ws->p, B.d_out->p, v,
                                 opts.min_sample_multiplicator, opts.non_min_sample_multiplier, seed, kSubsetMaskAll));
        MP_HIP(hipMemcpyAsync(outs.data(), B.d_out->p, sizeof(LsqOut) * m, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipStreamSynchronize(stream));
        jobs.clear();
        refs.clear();
        which.clear();
        for (size_t i = 0; i < m; ++i) {
            const int32_t e = run.e0 + (int32_t)i;
            const int k = pair_of(e);
            const LsqOut &O = outs[i];
            LsqFitResult &Q = results[e];
            Q.score = O.score;
            for (int t = 0; t < 3; ++t) {
                Q.num_inliers[t] = O.tight[t];
                Q.num_wide[t] = O.wide[t];
                Q.subset_sizes[t] = O.sub[t];
            }
            Q.status = 3;
            const int *sz = O.sub;
            // skipped by the rule, or too few data for the solver (the size test of least_squares)
            if (O.k < 0 || (sz[0] < kmd && sz[1] < kmd) || sz[2] < kpt) continue;
            LmJob J = make_lm_job(R.Ps[(size_t)k], cfg, sz, 0, rule == kSubsetNonmin, cur[i]);
            // (the lists of a slice lie n apart, not back to back)
            J.off1 = (int)ns[(size_t)e];
            J.off2 = 2 * (int)ns[(size_t)e];
            jobs.push_back(J);
            LmPairRef ref;
            ref.pair = k;
            ref.pad = 0;
            ref.idx_off = entries[i].ws_off + 3 * ns[(size_t)e];
            refs.push_back(ref);
            which.push_back((int)i);
        }
        const size_t nj = jobs.size();
        if (nj > 0) {
            lm_out.resize(nj);
            st.resize(nj);
            MP_HIP(hipMemcpyAsync(B.d_jobs->p, jobs.data(), sizeof(LmJob) * nj, hipMemcpyHostToDevice, stream));
            MP_HIP(hipMemcpyAsync(B.d_refs->p, refs.data(), sizeof(LmPairRef) * nj, hipMemcpyHostToDevice, stream));
            MP_HIP(launch_lm_pairs(stream, v, R.d_D.p, R.d_C.p, B.d_jobs->p, B.d_refs->p, (int)nj, B.d_ws->p,
                                   B.d_models->p, B.d_status->p));
            MP_HIP(hipMemcpyAsync(lm_out.data(), B.d_models->p, sizeof(Model) * nj, hipMemcpyDeviceToHost, stream));
            MP_HIP(hipMemcpyAsync(st.data(), B.d_status->p, sizeof(int) * nj, hipMemcpyDeviceToHost, stream));
        }
        if (subset_idx)
            for (size_t i = 0; i < m; ++i) {
                const int32_t e = run.e0 + (int32_t)i;
                const int64_t n = ns[(size_t)e];
                for (int t = 0; t < 3; ++t)
                    if (outs[i].sub[t] > 0)
                        MP_HIP(hipMemcpyAsync(subset_idx + 3 * out_off[e] + t * n,
                                              B.d_ws->p + entries[i].ws_off + (3 + t) * n,
                                              sizeof(int) * (size_t)outs[i].sub[t], hipMemcpyDeviceToHost, stream));
            }
        MP_HIP(hipStreamSynchronize(stream));
        for (size_t q = 0; q < nj; ++q) {
            const int32_t e = run.e0 + which[q];
            results[e].status = st[q];
            if (st[q] != 1) continue; // (the input bytes stay)
            const double norm = R.norm_scale[(size_t)pair_of(e)];
            Model mo = lm_out[q];
            if (variant == kSF) {
                mo.focal0 *= norm;
                mo.focal1 = mo.focal0;
            } else if (variant == kTF) {
                mo.focal0 *= norm;
                mo.focal1 *= norm;
            }
            models[e] = mo;
        }
    }
}

// the argument checks refine_batch and the pair set's creation share (all before any array
// is read beyond offsets, and before the device is touched)
void check_pair_arrays(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                       const double *d0, const double *d1) {
    if (offsets[0] < 0) throw std::invalid_argument("offsets must be non-negative");
    for (int32_t p = 0; p < num_pairs; ++p) {
        if (offsets[p + 1] < offsets[p]) throw std::invalid_argument("offsets must not decrease");
        if (offsets[p + 1] - offsets[p] > kRefinePairMax) throw std::invalid_argument("pair too large");
    }
    if (offsets[num_pairs] > 0 && (!x0 || !x1 || !d0 || !d1)) throw std::invalid_argument("null input array");
}
} // namespace

// Refinement of given models over many pairs (mp_refine_batch).  Per pair and round: the
// inliers of the model (errors of launch_sweep below the thresholds), LeastSquares over
// all of them on the device LM, and the result kept when it scores strictly lower
// (LeastSquaresFit with use_all_solver_inliers and the final least squares' score <
// best rule, src/hybrid_ransac.h:406, 484-510, 186-203).  The pairs of a run
// (host/refine_plan.h) are resident at once (host/resident_pairs.h); a round is one LM
// launch and one sweep launch over the pairs still running, and the sweep that decides
// round r is the inlier pass of round r + 1.  The host only drops stopped pairs from the
// launch lists.
void refine_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                  const double *d0, const double *d1, const double *min_depth, const double *cam0, const double *cam1,
                  const RansacOptions &opts, const EstimatorConfig &cfg, int rounds, Model *models,
                  RefineResult *results, int32_t *inlier_idx, int64_t chunk, int device) {
    if (variant < 0 || variant > 3)
        throw std::invalid_argument("variant must be 0 (calibrated), 1 (shared focal), 2 (two focal) or 3 (scale only)");
    if (num_pairs < 0) throw std::invalid_argument("negative pair count");
    if (rounds < 1 || rounds > 64) throw std::invalid_argument("rounds must be in 1..64");
    if (chunk < 0) throw std::invalid_argument("chunk must not be negative");
    {
        PairInput none; // (the option checks of every entry point)
        validate(none, opts);
    }
    if (num_pairs == 0) return;
    if (!offsets || !min_depth || !cam0 || !cam1 || !models || !results)
        throw std::invalid_argument("null offsets, min_depth, cameras, models or results");
    check_pair_arrays(variant, num_pairs, offsets, x0, x1, d0, d1);

    const int nc = (variant == kCal || variant == kScaleOnly) ? 9 : 2;
    CtxLease lease(device);
    hipStream_t stream = lease.c->stream;
    for (const RefineRun &run : refine_plan(num_pairs, offsets, chunk)) {
        const int np = run.p1 - run.p0;
        ResidentPairs R(stream, variant, np, offsets + run.p0, x0, x1, d0, d1, min_depth + 2 * (size_t)run.p0,
                        cam0 + (size_t)nc * run.p0, cam1 + (size_t)nc * run.p0, opts, cfg);
        refine_run(R, stream, PairSel{np, nullptr}, offsets + run.p0, cfg, rounds, models + run.p0,
                   results + run.p0, inlier_idx);
    }
}

namespace {
// page-locked host memory freed on scope exit
template <class T> struct PinnedArray {
    T *p = nullptr;
    explicit PinnedArray(size_t n) { MP_HIP(hipHostMalloc((void **)&p, sizeof(T) * std::max<size_t>(n, 1))); }
    ~PinnedArray() {
        if (p) hipHostFree(p);
    }
    PinnedArray(const PinnedArray &) = delete;
    PinnedArray &operator=(const PinnedArray &) = delete;
};
struct EventHolder {
    hipEvent_t e = nullptr;
    EventHolder() { MP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
    ~EventHolder() {
        if (e) hipEventDestroy(e);
    }
    EventHolder(const EventHolder &) = delete;
    EventHolder &operator=(const EventHolder &) = delete;
};
std::atomic<int> g_select_tile{0}; // 0: kSelectTile (select_tile_override)
std::mutex g_select_mu;
SelectTiming g_select_timing;
constexpr int kSelectPrepThreads = 8;         // host threads of a slab's record preparation
constexpr int64_t kSelectPrepPerThread = 2048; // candidates a thread is started for
} // namespace

int select_tile_override(int tile) {
    if (tile != 0 && tile != 1 && tile != 2 && tile != 4 && tile != 8)
        throw std::invalid_argument("tile must be 0 (the default), 1, 2, 4 or 8");
    return g_select_tile.exchange(tile);
}
SelectTiming select_timing_last() {
    std::lock_guard<std::mutex> lk(g_select_mu);
    return g_select_timing;
}

namespace {
// Ranking of the candidates of the selected resident pairs (the body of mp_select_batch and
// mp_select_set).  moff: ns + 1 offsets into models / scores / counts (entry j's candidates
// at moff[j] .. moff[j + 1] - 1); results: entry j; the winner's lists of entry j to
// inlier_idx + 3 out_off[j] + t n_j (nullable).  List buffer 0 is scratch of the call.
// prior (nullable; one score per entry): the walk of entry j continues from prior[j], the
// score of a best it already has (ransac_adaptive_set).  An entry without a candidate
// strictly below its prior is unchanged: best_index -1, best_score = prior[j], no sweep item,
// no record, and nothing written to its part of inlier_idx.
void select_run(ResidentPairs &R, hipStream_t stream, const PairSel sel, const int64_t *out_off, const int64_t *moff,
                const Model *models, double *scores, int32_t *counts, SelectResult *results, int32_t *inlier_idx,
                int64_t model_chunk, int tile, bool timed, SelectTiming &tm, const double *prior = nullptr) {
    const int ns = sel.n;
    if (ns == 0) return;
    const int variant = R.variant, v = R.v;
    const int64_t T = R.T;
    const int64_t M = moff[ns] - moff[0];
    const std::vector<PairConst> &Ch = R.Ch;
    // (timed: every stage is waited for, so the parts add up and nothing overlaps)
    auto stage_end = [&](Clock::time_point t0, double &ms) {
        if (!timed) return;
        MP_HIP(hipStreamSynchronize(stream));
        ms += 1e3 * secs(t0);
    };
    Clock::time_point t0 = Clock::now();
    int *d_lists = R.lists(1);
    std::vector<int64_t> moff_run(ns + 1);
    for (int j = 0; j <= ns; ++j) moff_run[j] = moff[j] - moff[0];
    DevArray<int64_t> d_moff(ns + 1);
    MP_HIP(hipMemcpyAsync(d_moff.p, moff_run.data(), sizeof(int64_t) * (ns + 1), hipMemcpyHostToDevice, stream));
    stage_end(t0, tm.pairs_ms);

    // the model of candidate m of the call in problem units (entry j of the selection)
    auto problem_model = [&](int j, int64_t m) {
        Model c = models[moff[0] + m];
        if (variant == kSF || variant == kTF) {
            const double norm = R.norm_scale[sel[j]];
            c.focal0 /= norm;
            c.focal1 /= norm;
        }
        return c;
    };
    // ---- the candidates' scores and counts, slab by slab ----
    DevArray<double> d_scores((size_t)M);
    DevArray<int> d_counts(3 * (size_t)M);
    const std::vector<SelectSlab> slabs = select_slabs(M, model_chunk);
    const size_t cap = slabs.empty() ? 0 : (size_t)(slabs[0].m1 - slabs[0].m0); // (the first is the largest)
    const int nbuf = slabs.size() > 1 ? 2 : 1;
    // (a work item holds at least one candidate: a slab has at most `cap` items)
    std::unique_ptr<PinnedArray<ScoreRec>> h_recs[2];
    std::unique_ptr<PinnedArray<SelectItem>> h_items[2];
    std::unique_ptr<DevArray<ScoreRec>> d_recs[2];
    std::unique_ptr<DevArray<SelectItem>> d_items[2];
    std::unique_ptr<EventHolder> uploaded[2], scored[2];
    for (int b = 0; b < nbuf && cap > 0; ++b) {
        h_recs[b].reset(new PinnedArray<ScoreRec>(cap));
        h_items[b].reset(new PinnedArray<SelectItem>(cap));
        d_recs[b].reset(new DevArray<ScoreRec>(cap));
        d_items[b].reset(new DevArray<SelectItem>(cap));
        uploaded[b].reset(new EventHolder());
        scored[b].reset(new EventHolder());
    }
    std::vector<SelectItem> items;
    for (size_t si = 0; si < slabs.size(); ++si) {
        const SelectSlab &s = slabs[si];
        const int b = (int)(si % 2) % nbuf;
        const int64_t nslab = s.m1 - s.m0;
        // (the host buffers' previous upload and the device buffers' previous launch are over)
        if (si >= 2) {
            MP_HIP(hipEventSynchronize(uploaded[b]->e));
            MP_HIP(hipEventSynchronize(scored[b]->e));
        }
        t0 = Clock::now();
        select_items(ns, moff, s, tile, items);
        // (the plan names the selection's entries; the kernels index the resident records)
        if (sel.ids)
            for (SelectItem &it : items) it.pair = sel.ids[it.pair];
        std::memcpy(h_items[b]->p, items.data(), sizeof(SelectItem) * items.size());
        ScoreRec *recs = h_recs[b]->p;
        // candidates a .. e - 1 of the slab; the entry of each by a walk from the first one's
        auto prepare = [&](int64_t a, int64_t e) {
            int j = (int)(std::upper_bound(moff_run.begin(), moff_run.end(), s.m0 + a) - moff_run.begin()) - 1;
            for (int64_t q = a; q < e; ++q) {
                const int64_t m = s.m0 + q;
                while (moff_run[j + 1] <= m) ++j;
                const Model c = problem_model(j, m);
                prepare_score_rec(Ch[sel[j]], c, recs[q]);
            }
        };
        const int nthr = (int)std::min<int64_t>(kSelectPrepThreads, nslab / kSelectPrepPerThread);
        if (nthr <= 1) {
            prepare(0, nslab);
        } else {
            std::vector<std::thread> threads;
            for (int t = 1; t < nthr; ++t) threads.emplace_back(prepare, nslab * t / nthr, nslab * (t + 1) / nthr);
            prepare(0, nslab / nthr);
            for (auto &t : threads) t.join();
        }
        if (timed) tm.prepare_ms += 1e3 * secs(t0);
        t0 = Clock::now();
        MP_HIP(hipMemcpyAsync(d_recs[b]->p, recs, sizeof(ScoreRec) * (size_t)nslab, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(d_items[b]->p, h_items[b]->p, sizeof(SelectItem) * items.size(), hipMemcpyHostToDevice,
                              stream));
        MP_HIP(hipEventRecord(uploaded[b]->e, stream));
        stage_end(t0, tm.upload_ms);
        t0 = Clock::now();
        MP_HIP(launch_select_score(stream, v, tile, R.d_D.p, R.d_C.p, d_items[b]->p, (int)items.size(), d_recs[b]->p,
                                   s.m0, d_scores.p, d_counts.p));
        MP_HIP(hipEventRecord(scored[b]->e, stream));
        stage_end(t0, tm.score_ms);
    }
    // ---- the best candidate of every pair ----
    t0 = Clock::now();
    DevArray<SelectBest> d_best(ns);
    std::vector<SelectBest> best(ns);
    if (prior) {
        DevArray<double> d_prior(ns);
        MP_HIP(hipMemcpyAsync(d_prior.p, prior, sizeof(double) * ns, hipMemcpyHostToDevice, stream));
        MP_HIP(launch_select_argmin_seeded(stream, d_moff.p, ns, d_scores.p, d_prior.p, d_best.p));
        MP_HIP(hipStreamSynchronize(stream)); // (d_prior dies here)
    } else {
        MP_HIP(launch_select_argmin(stream, d_moff.p, ns, d_scores.p, d_best.p));
    }
    MP_HIP(hipMemcpyAsync(best.data(), d_best.p, sizeof(SelectBest) * ns, hipMemcpyDeviceToHost, stream));
    if (scores && M > 0)
        MP_HIP(hipMemcpyAsync(scores + moff[0], d_scores.p, sizeof(double) * (size_t)M, hipMemcpyDeviceToHost, stream));
    if (counts && M > 0)
        MP_HIP(hipMemcpyAsync(counts + 3 * moff[0], d_counts.p, sizeof(int) * 3 * (size_t)M, hipMemcpyDeviceToHost,
                              stream));
    MP_HIP(hipStreamSynchronize(stream));
    if (timed) tm.argmin_ms += 1e3 * secs(t0);
    // ---- the winners' lists: refine_batch's sweep, one item per pair with a winner ----
    t0 = Clock::now();
    std::vector<RefineItem> ritems;
    std::vector<ScoreRec> rrecs;
    std::vector<int> which;
    for (int j = 0; j < ns; ++j) {
        SelectResult &Q = results[j];
        std::memset(&Q, 0, sizeof(Q));
        Q.best_score = prior ? prior[j] : DBL_MAX;
        Q.norm_scale = R.norm_scale[sel[j]];
        Q.best_index = -1;
        if (best[j].index < 0) continue;
        if (best[j].index >= moff[j + 1] - moff[j]) throw std::runtime_error("select_argmin: index out of range");
        RefineItem it;
        it.pair = sel[j];
        it.buf = 0;
        ritems.push_back(it);
        rrecs.emplace_back();
        prepare_score_rec(Ch[sel[j]], problem_model(j, moff_run[j] + best[j].index), rrecs.back());
        which.push_back(j);
    }
    const size_t nw = which.size();
    if (nw > 0) {
        DevArray<RefineItem> d_ritems(nw);
        DevArray<ScoreRec> d_rrecs(nw);
        DevArray<RefineSweepOut> d_out(nw);
        std::vector<RefineSweepOut> outs(nw);
        MP_HIP(hipMemcpyAsync(d_ritems.p, ritems.data(), sizeof(RefineItem) * nw, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(d_rrecs.p, rrecs.data(), sizeof(ScoreRec) * nw, hipMemcpyHostToDevice, stream));
        MP_HIP(launch_refine_sweep(stream, v, R.d_D.p, R.d_C.p, d_ritems.p, d_rrecs.p, (int)nw, R.d_list_off.p, d_lists,
                                   3 * T, d_out.p));
        MP_HIP(hipMemcpyAsync(outs.data(), d_out.p, sizeof(RefineSweepOut) * nw, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipStreamSynchronize(stream));
        for (size_t i = 0; i < nw; ++i) {
            const int j = which[i];
            SelectResult &Q = results[j];
            // (the same record through the same arithmetic: anything else is a defect; the
            // measurement hook's other work-item sizes are not pinned to these bits)
            if (tile == kSelectTile && std::memcmp(&outs[i].score, &best[j].score, sizeof(double)) != 0)
                throw std::runtime_error("select_batch: the winner's sweep score differs from its selected score");
            Q.best_score = best[j].score;
            Q.best_index = best[j].index;
            for (int t = 0; t < 3; ++t) Q.num_inliers[t] = outs[i].count[t];
        }
        if (inlier_idx && T > 0) {
            if (!sel.ids) { // every pair: the buffer in one copy
                std::vector<int> lists(3 * (size_t)T);
                MP_HIP(hipMemcpyAsync(lists.data(), d_lists, sizeof(int) * lists.size(), hipMemcpyDeviceToHost, stream));
                MP_HIP(hipStreamSynchronize(stream));
                for (int j : which) {
                    const int64_t n = Ch[j].n;
                    for (int t = 0; t < 3; ++t)
                        std::memcpy(inlier_idx + 3 * out_off[j] + t * n, lists.data() + refine_list(T, R.off[j], n, 0, t),
                                    sizeof(int) * (size_t)results[j].num_inliers[t]);
                }
            } else { // a selection: only its winners' lists
                for (int j : which) {
                    const int k = sel[j];
                    const int64_t n = Ch[k].n;
                    for (int t = 0; t < 3; ++t)
                        if (results[j].num_inliers[t] > 0)
                            MP_HIP(hipMemcpyAsync(inlier_idx + 3 * out_off[j] + t * n,
                                                  d_lists + refine_list(T, R.off[k], n, 0, t),
                                                  sizeof(int) * (size_t)results[j].num_inliers[t],
                                                  hipMemcpyDeviceToHost, stream));
                }
            }
        }
    }
    MP_HIP(hipStreamSynchronize(stream));
    if (timed) tm.winners_ms += 1e3 * secs(t0);
}
} // namespace

// Ranking of given candidate models over many pairs (mp_select_batch).  The pairs of a run
// (host/refine_plan.h) are resident at once.  Per run: the candidates' score records,
// prepared on the host (prepare_score_rec: mp_score_models' bits), go to the device in
// slabs (host/select_plan.h), one select_score launch each; one select_argmin launch over
// the run's scores; the winners' inlier lists by refine_batch's sweep.  Two record
// buffers: slab k + 1 is prepared and uploaded while slab k is scored.
void select_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                  const double *d0, const double *d1, const double *cam0, const double *cam1,
                  const RansacOptions &opts, const EstimatorConfig &cfg, const int64_t *model_offsets,
                  const Model *models, double *scores, int32_t *counts, SelectResult *results, int32_t *inlier_idx,
                  int64_t chunk, int64_t model_chunk, int device) {
    if (variant < 0 || variant > 3)
        throw std::invalid_argument("variant must be 0 (calibrated), 1 (shared focal), 2 (two focal) or 3 (scale only)");
    if (num_pairs < 0) throw std::invalid_argument("negative pair count");
    if (chunk < 0) throw std::invalid_argument("chunk must not be negative");
    if (model_chunk < 0) throw std::invalid_argument("model_chunk must not be negative");
    {
        PairInput none; // (the option checks of every entry point)
        validate(none, opts);
    }
    if (num_pairs == 0) return;
    if (!offsets || !model_offsets || !cam0 || !cam1 || !results)
        throw std::invalid_argument("null offsets, model_offsets, cameras or results");
    if (offsets[0] < 0 || model_offsets[0] < 0) throw std::invalid_argument("offsets must be non-negative");
    for (int32_t p = 0; p < num_pairs; ++p) {
        if (offsets[p + 1] < offsets[p] || model_offsets[p + 1] < model_offsets[p])
            throw std::invalid_argument("offsets must not decrease");
        if (offsets[p + 1] - offsets[p] > kRefinePairMax) throw std::invalid_argument("pair too large");
    }
    if (model_offsets[num_pairs] - model_offsets[0] > kSelectModelsMax)
        throw std::invalid_argument("more than 2^28 candidates");
    if (offsets[num_pairs] > 0 && (!x0 || !x1 || !d0 || !d1)) throw std::invalid_argument("null input array");
    if (model_offsets[num_pairs] > model_offsets[0] && !models) throw std::invalid_argument("null models");

    const int nc = (variant == kCal || variant == kScaleOnly) ? 9 : 2;
    const int tile_set = g_select_tile.load();
    const int tile = tile_set ? tile_set : kSelectTile;
    const bool timed = g_prof_on.load();
    SelectTiming tm;
    CtxLease lease(device);
    hipStream_t stream = lease.c->stream;

    for (const RefineRun &run : refine_plan(num_pairs, offsets, chunk)) {
        const int np = run.p1 - run.p0;
        // ---- problems, packed upload, pair records (host/resident_pairs.h) ----
        Clock::time_point t0 = Clock::now();
        ResidentPairs R(stream, variant, np, offsets + run.p0, x0, x1, d0, d1, nullptr, cam0 + (size_t)nc * run.p0,
                        cam1 + (size_t)nc * run.p0, opts, cfg);
        if (timed) tm.pairs_ms += 1e3 * secs(t0);
        select_run(R, stream, PairSel{np, nullptr}, offsets + run.p0, model_offsets + run.p0, models, scores, counts,
                   results + run.p0, inlier_idx, model_chunk, tile, timed, tm);
    }
    if (timed) {
        std::lock_guard<std::mutex> lk(g_select_mu);
        g_select_timing = tm;
    }
}

namespace {
std::mutex g_hyp_mu;
HypTiming g_hyp_timing;
} // namespace

HypTiming hypothesize_timing_last() {
    std::lock_guard<std::mutex> lk(g_hyp_mu);
    return g_hyp_timing;
}

namespace {
// what mp_hypothesize_batch and mp_hypothesize_set run on: variants 0 .. 2, use_shift on,
// the default MD solvers
void check_hyp_supported(int variant, const RansacOptions &opts, const EstimatorConfig &cfg) {
    if (variant == kScaleOnly)
        throw std::invalid_argument("hypothesize_batch does not support MP_SCALE_ONLY (variant 3)");
    if (variant < 0 || variant > 2)
        throw std::invalid_argument("variant must be 0 (calibrated), 1 (shared focal) or 2 (two focal)");
    if (!cfg.use_shift) throw std::invalid_argument("hypothesize_batch does not support use_shift = 0");
    if (opts.use_ours || opts.use_4p4d)
        throw std::invalid_argument("hypothesize_batch does not support the alternate MD solvers (use_ours / use_4p4d)");
}
// the samples of ne entries (pairs of a call, or of a selection): entry e has n(e)
// correspondences and the samples sample_offsets[e] .. sample_offsets[e + 1] - 1.  Types,
// ranges and repeats; a kernel only ever reads indices that passed here.
template <class N>
void check_hyp_samples(int v, int32_t ne, N n_of, const int64_t *sample_offsets, const int32_t *sample_types,
                       const int32_t *sample_idx) {
    const int ksz[2] = {v == kCal ? 3 : 4, v == kCal ? 5 : (v == kSF ? 6 : 7)};
    static_assert(kSampleStride == 8, "a sample has 8 index slots (mp_hypothesize_batch)");
    for (int32_t p = 0; p < ne; ++p) {
        const int64_t n = n_of(p);
        for (int64_t s = sample_offsets[p]; s < sample_offsets[p + 1]; ++s) {
            const int32_t t = sample_types[s];
            if (t != 0 && t != 1)
                throw std::invalid_argument("sample " + std::to_string(s) + ": type must be 0 (MD solver) or 1 (point solver)");
            const int k = ksz[t];
            if (n < k)
                throw std::invalid_argument("sample " + std::to_string(s) + ": pair " + std::to_string(p) +
                                            " has too few correspondences for the solver");
            const int32_t *q = sample_idx + kSampleStride * s;
            for (int a = 0; a < k; ++a) {
                if (q[a] < 0 || q[a] >= n)
                    throw std::invalid_argument("sample " + std::to_string(s) + ": index outside the pair");
                for (int b = 0; b < a; ++b)
                    if (q[a] == q[b])
                        throw std::invalid_argument("sample " + std::to_string(s) + ": repeated index");
            }
        }
    }
}

// one slab's device and host buffers, sized for the largest slab of a call of S_all samples
struct HypBuffers {
    int64_t slab_cap;
    DevArray<int> d_samples, d_list, d_counts;
    DevArray<HypItem> d_items;
    DevArray<Model> d_models;
    DevArray<double> d_cand, d_pen;
    DevArray<int> d_ncand, d_valid;
    DevArray<Model> d_slots;
    PtWorkspace W;
    std::vector<int> h_samples, h_list;
    std::vector<HypItem> h_items;
    HypPlan plan;
    // the compact output mode (HypCompact): the scan's bases, the gathered models, their tags
    std::unique_ptr<DevArray<int>> d_base, d_tags;
    std::unique_ptr<DevArray<Model>> d_cmodels;
    std::vector<int> h_tags;
    // device-drawn samples (HypDraw): the sampler's items and the types it writes
    std::unique_ptr<DevArray<DrawItem>> d_ditems;
    std::unique_ptr<DevArray<int>> d_types;
    std::vector<DrawItem> h_ditems;
    HypBuffers(int v, int64_t S_all, int64_t sample_chunk, bool compact = false, bool draw = false)
        : slab_cap(std::min<int64_t>(S_all, hyp_slabs(S_all, sample_chunk)[0].s1)),
          d_samples((size_t)slab_cap * kSampleStride), d_list((size_t)slab_cap), d_counts((size_t)slab_cap),
          d_items((size_t)slab_cap), d_models((size_t)slab_cap * max_models(v)),
          d_cand((size_t)slab_cap * kPtCandStride), d_pen(v == kSF ? (size_t)slab_cap * kPtPenStride : 1),
          d_ncand((size_t)slab_cap), d_valid((size_t)slab_cap * kPtSlotStride),
          d_slots((size_t)slab_cap * kPtSlotStride), W{d_cand.p, d_ncand.p, d_slots.p, d_valid.p, d_pen.p},
          h_samples((size_t)slab_cap * kSampleStride), h_list((size_t)slab_cap), h_items((size_t)slab_cap) {
        if (compact) {
            d_base.reset(new DevArray<int>((size_t)slab_cap + 1));
            d_cmodels.reset(new DevArray<Model>((size_t)slab_cap * max_models(v)));
            d_tags.reset(new DevArray<int>(2 * (size_t)slab_cap * max_models(v)));
        }
        if (draw) {
            // (an item holds at least one sample: a slab has at most slab_cap items)
            d_ditems.reset(new DevArray<DrawItem>((size_t)slab_cap));
            d_types.reset(new DevArray<int>((size_t)slab_cap));
        }
    }
};

// The samples of a hypothesize_run drawn on the device instead of given (mp_ransac_set with a
// budget): the slab's samples are written by launch_draw_samples where the upload would put
// them, in the same form (the slots a solver does not read are 0), and never reach the
// host.  sample_types of the run are then the host's draw_type values (word 0 only), which
// the planning needs, and sample_idx is null.  pair_n: the per-pair sizes on the device.
struct HypDraw {
    uint64_t seed;
    int point_share;
    const int *d_pair_n;
    // per entry of the selection, nullable: the entry's samples are first[j], first[j] + 1, ...
    // of its pair (a later round of ransac_adaptive_set); sample_types are those samples'
    const int32_t *first = nullptr;
    // the confidence weights of the call (DrawWeights; null: the uniform draw): the tables, the
    // table offset of every pair of the set, and whether the pair draws by its table
    const uint32_t *d_cum = nullptr;
    const int64_t *d_cum_off = nullptr;
    const unsigned char *d_weighted = nullptr;
};
// The compact output mode of hypothesize_run (mp_candidates_set, mp_ransac_set): instead of
// the slot array, only the models that exist come back -- models in (sample, slot) order, in
// user units, with plan.moff / plan.sample / plan.slot (host/candidates_plan.h).  Per slab
// the counts (4 bytes per sample), the gathered models and their tags are copied back.
struct HypCompact {
    CandPlan plan;
    std::vector<Model> models;
    int64_t bytes_back = 0;  // what the slabs copied back
    int64_t bytes_slots = 0; // what the slot array and the counts would have been
};

constexpr bool kDrawStageDefault = true; // (the staged form against the global one)

// One slab of device-drawn samples: items of the selection's entries over slab `s`, mapped to
// the set's pairs, drawn into d_samples / d_types (slab positions).
void draw_slab(hipStream_t stream, int v, const PairSel sel, const int64_t *soff, const HypSlab &s, const HypDraw &dr,
               std::vector<DrawItem> &h_items, DrawItem *d_items, int *d_samples, int *d_types) {
    draw_items(sel.n, soff, dr.first, s, h_items);
    if ((int64_t)h_items.size() > s.s1 - s.s0) throw std::logic_error("draw: more items than samples");
    for (DrawItem &it : h_items) it.pair = sel[it.pair];
    if (h_items.empty()) return;
    MP_HIP(hipMemcpyAsync(d_items, h_items.data(), sizeof(DrawItem) * h_items.size(), hipMemcpyHostToDevice, stream));
    if (dr.d_cum) {
        // (MADPOSE_DRAW_STAGE=0: every table from global memory, the A/B of tools/draw_weighted_bench.py)
        const bool stage = env_flag("MADPOSE_DRAW_STAGE", kDrawStageDefault);
        MP_HIP(launch_draw_samples_weighted(stream, v, d_items, (int)h_items.size(), dr.d_pair_n, dr.d_cum,
                                            dr.d_cum_off, dr.d_weighted, stage, dr.seed, dr.point_share, d_samples,
                                            d_types));
        return;
    }
    MP_HIP(launch_draw_samples(stream, v, d_items, (int)h_items.size(), dr.d_pair_n, dr.seed, dr.point_share,
                               d_samples, d_types));
}

// The sample models of the selected resident pairs (the body of mp_hypothesize_batch and
// mp_hypothesize_set), S = soff[ns] - soff[0] > 0 samples, checked by check_hyp_samples.
// soff: ns + 1 offsets into sample_types / sample_idx / counts (models: max_models slots per
// sample); the run's samples go through the device in slabs (host/hypothesis_plan.h), one
// launch_hyp_solve each.  draw (nullable): the samples are drawn on the device (HypDraw).
// compact (nullable): the compact output mode (HypCompact; B built for it): `models` is not
// written, counts still is.  Neither changes a model's bytes.
void hypothesize_run(ResidentPairs &R, hipStream_t stream, const PairSel sel, const int64_t *soff,
                     const int32_t *sample_types, const int32_t *sample_idx, Model *models, int32_t *counts,
                     int64_t sample_chunk, HypBuffers &B, bool timed, HypTiming &tm, const HypDraw *draw = nullptr,
                     HypCompact *compact = nullptr) {
    const int ns_sel = sel.n;
    const int v = R.v;
    const int ksz[2] = {v == kCal ? 3 : 4, v == kCal ? 5 : (v == kSF ? 6 : 7)};
    const int maxm = max_models(v);
    const int cap[2] = {hyp_md_cap(v), hyp_pt_cap(v)};
    const int64_t S = soff[ns_sel] - soff[0];
    auto stage_end = [&](Clock::time_point t0, double &ms) {
        if (!timed) return;
        MP_HIP(hipStreamSynchronize(stream));
        ms += 1e3 * secs(t0);
    };
    HypPlan &plan = B.plan;
    if (compact) compact->plan.begin(ns_sel, soff, maxm);
    for (const HypSlab &s : hyp_slabs(S, sample_chunk)) {
        const int64_t ns = s.s1 - s.s0;
        const int64_t g0 = soff[0] + s.s0; // the slab's first sample in the caller's arrays
        Clock::time_point t0 = Clock::now();
        hyp_items(ns_sel, soff, sample_types + soff[0], s, cap, plan);
        const size_t nl[2] = {plan.list[0].size(), plan.list[1].size()};
        const size_t ni[2] = {plan.items[0].size(), plan.items[1].size()};
        if ((int64_t)(nl[0] + nl[1]) != ns || (int64_t)(ni[0] + ni[1]) > ns)
            throw std::logic_error("hypothesize_batch: the slab's lists do not cover its samples");
        // (only the slots a solver reads, range-checked before, reach the device)
        for (int64_t b = 0; b < ns && !draw; ++b) {
            const int k = ksz[sample_types[g0 + b] != 0 ? 1 : 0];
            const int32_t *q = sample_idx + kSampleStride * (g0 + b);
            int *o = B.h_samples.data() + kSampleStride * b;
            for (int a = 0; a < kSampleStride; ++a) o[a] = a < k ? q[a] : 0;
        }
        std::copy(plan.list[0].begin(), plan.list[0].end(), B.h_list.begin());
        std::copy(plan.list[1].begin(), plan.list[1].end(), B.h_list.begin() + nl[0]);
        std::copy(plan.items[0].begin(), plan.items[0].end(), B.h_items.begin());
        std::copy(plan.items[1].begin(), plan.items[1].end(), B.h_items.begin() + ni[0]);
        // (the plan names the selection's entries; the kernels index the resident records)
        if (sel.ids)
            for (size_t i = 0; i < ni[0] + ni[1]; ++i) B.h_items[i].pair = sel.ids[B.h_items[i].pair];
        if (timed) tm.plan_ms += 1e3 * secs(t0);
        t0 = Clock::now();
        if (draw) {
            draw_slab(stream, v, sel, soff, s, *draw, B.h_ditems, B.d_ditems->p, B.d_samples.p, B.d_types->p);
            stage_end(t0, tm.draw_ms);
            t0 = Clock::now();
        } else {
            MP_HIP(hipMemcpyAsync(B.d_samples.p, B.h_samples.data(), sizeof(int) * kSampleStride * (size_t)ns,
                                  hipMemcpyHostToDevice, stream));
        }
        MP_HIP(hipMemcpyAsync(B.d_list.p, B.h_list.data(), sizeof(int) * (size_t)ns, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(B.d_items.p, B.h_items.data(), sizeof(HypItem) * (ni[0] + ni[1]), hipMemcpyHostToDevice,
                              stream));
        MP_HIP(hipMemsetAsync(B.d_models.p, 0, sizeof(Model) * (size_t)ns * maxm, stream));
        MP_HIP(hipMemsetAsync(B.d_counts.p, 0, sizeof(int) * (size_t)ns, stream));
        stage_end(t0, tm.upload_ms);
        t0 = Clock::now();
        MP_HIP(launch_hyp_solve(stream, v, R.d_D.p, R.d_C.p, B.d_items.p, (int)ni[0], B.d_list.p, B.d_items.p + ni[0],
                                (int)ni[1], B.d_list.p + nl[0], (int)nl[1], B.d_samples.p, B.W, B.d_models.p,
                                B.d_counts.p));
        stage_end(t0, tm.solve_ms);
        t0 = Clock::now();
        if (compact) {
            MP_HIP(launch_hyp_compact(stream, v, B.d_models.p, B.d_counts.p, (int)ns, B.d_base->p, B.d_cmodels->p,
                                      B.d_tags->p));
            stage_end(t0, tm.compact_ms);
            t0 = Clock::now();
            int total = -1;
            MP_HIP(hipMemcpyAsync(counts + g0, B.d_counts.p, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, stream));
            MP_HIP(hipMemcpyAsync(&total, B.d_base->p + ns, sizeof(int), hipMemcpyDeviceToHost, stream));
            MP_HIP(hipStreamSynchronize(stream));
            CandPlan &cp = compact->plan;
            const size_t old_size = compact->models.size();
            const int64_t nm = cp.add_slab(s, counts + g0); // (refuses a count outside 0 .. maxm)
            if (nm != total) throw std::runtime_error("hypothesize: the device scan does not match the counts");
            compact->models.resize(old_size + (size_t)nm);
            B.h_tags.resize(2 * (size_t)nm);
            if (nm > 0) {
                MP_HIP(hipMemcpyAsync(compact->models.data() + old_size, B.d_cmodels->p, sizeof(Model) * (size_t)nm,
                                      hipMemcpyDeviceToHost, stream));
                MP_HIP(hipMemcpyAsync(B.h_tags.data(), B.d_tags->p, sizeof(int) * 2 * (size_t)nm, hipMemcpyDeviceToHost,
                                      stream));
                MP_HIP(hipStreamSynchronize(stream));
            }
            // the device's tags against the plan's; user units as below (one product each)
            int j = (int)(std::upper_bound(soff, soff + ns_sel + 1, g0) - soff) - 1;
            for (int64_t m = 0; m < nm; ++m) {
                const int b = cp.slab_pos[(size_t)m];
                if (B.h_tags[2 * (size_t)m] != b || B.h_tags[2 * (size_t)m + 1] != cp.slot[old_size + (size_t)m])
                    throw std::runtime_error("hypothesize: the gathered models are out of order");
                if (v != kCal) {
                    while (soff[j + 1] <= g0 + b) ++j;
                    const double norm = R.norm_scale[sel[j]];
                    Model &mm = compact->models[old_size + (size_t)m];
                    mm.focal0 *= norm;
                    mm.focal1 *= norm;
                }
            }
            compact->bytes_back += (int64_t)sizeof(int) * (ns + 1) + nm * (int64_t)(sizeof(Model) + 2 * sizeof(int));
            compact->bytes_slots += ns * (int64_t)(sizeof(Model) * maxm + sizeof(int));
            if (timed) tm.download_ms += 1e3 * secs(t0);
            continue;
        }
        Model *out = models + (size_t)g0 * maxm;
        MP_HIP(hipMemcpyAsync(out, B.d_models.p, sizeof(Model) * (size_t)ns * maxm, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipMemcpyAsync(counts + g0, B.d_counts.p, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, stream));
        // (the host buffers are rewritten for the next slab, the device ones by its launches)
        MP_HIP(hipStreamSynchronize(stream));
        // user units: the focals times the pair's normalisation scale (one product each)
        if (v != kCal) {
            int j = (int)(std::upper_bound(soff, soff + ns_sel + 1, g0) - soff) - 1;
            for (int64_t b = 0; b < ns; ++b) {
                while (soff[j + 1] <= g0 + b) ++j;
                const double norm = R.norm_scale[sel[j]];
                const int cnt = counts[g0 + b];
                if (cnt < 0 || cnt > maxm) throw std::runtime_error("hypothesize_batch: model count out of range");
                for (int i = 0; i < cnt; ++i) {
                    Model &m = out[(size_t)b * maxm + i];
                    m.focal0 *= norm;
                    m.focal1 *= norm;
                }
            }
        }
        if (timed) tm.download_ms += 1e3 * secs(t0);
    }
    if (compact) compact->plan.finish();
}
} // namespace

// The estimators' sample models over many pairs (mp_hypothesize_batch).  Every argument is
// checked on the host before the device is touched: a kernel only ever reads indices that
// were range-checked here, from a copy in which the unused slots of a sample are zero.  The
// pairs of a run (host/refine_plan.h) are resident at once (host/resident_pairs.h, as
// refine_batch's and select_batch's); the run's samples go through hypothesize_run.
void hypothesize_batch(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                       const double *d0, const double *d1, const double *min_depth, const double *cam0,
                       const double *cam1, const RansacOptions &opts, const EstimatorConfig &cfg,
                       const int64_t *sample_offsets, const int32_t *sample_types, const int32_t *sample_idx,
                       Model *models, int32_t *counts, double *norm_scale, int64_t chunk, int64_t sample_chunk,
                       int device) {
    if (variant == kScaleOnly)
        throw std::invalid_argument("hypothesize_batch does not support MP_SCALE_ONLY (variant 3)");
    if (variant < 0 || variant > 2)
        throw std::invalid_argument("variant must be 0 (calibrated), 1 (shared focal) or 2 (two focal)");
    if (num_pairs < 0) throw std::invalid_argument("negative pair count");
    if (chunk < 0) throw std::invalid_argument("chunk must not be negative");
    if (sample_chunk < 0) throw std::invalid_argument("sample_chunk must not be negative");
    check_hyp_supported(variant, opts, cfg);
    {
        PairInput none; // (the option checks of every entry point)
        validate(none, opts);
    }
    if (num_pairs == 0) return;
    if (!offsets || !sample_offsets || !min_depth || !cam0 || !cam1)
        throw std::invalid_argument("null offsets, sample_offsets, min_depth or cameras");
    if (offsets[0] < 0 || sample_offsets[0] < 0) throw std::invalid_argument("offsets must be non-negative");
    for (int32_t p = 0; p < num_pairs; ++p) {
        if (offsets[p + 1] < offsets[p] || sample_offsets[p + 1] < sample_offsets[p])
            throw std::invalid_argument("offsets must not decrease");
        if (offsets[p + 1] - offsets[p] > kRefinePairMax) throw std::invalid_argument("pair too large");
    }
    const int64_t S_all = sample_offsets[num_pairs] - sample_offsets[0];
    if (S_all > kHypSamplesMax) throw std::invalid_argument("more than 2^22 samples");
    if (offsets[num_pairs] > 0 && (!x0 || !x1 || !d0 || !d1)) throw std::invalid_argument("null input array");
    if (S_all > 0 && (!sample_types || !sample_idx || !models || !counts))
        throw std::invalid_argument("null sample_types, sample_idx, models or counts");
    const int v = variant;
    check_hyp_samples(v, num_pairs, [&](int32_t p) { return offsets[p + 1] - offsets[p]; }, sample_offsets,
                      sample_types, sample_idx);

    const int nc = v == kCal ? 9 : 2;
    auto pair_input = [&](int32_t p) {
        const int64_t o = offsets[p];
        PairInput in;
        in.variant = variant;
        in.n = offsets[p + 1] - o;
        in.x0 = x0 + 2 * o;
        in.x1 = x1 + 2 * o;
        in.d0 = d0 + o;
        in.d1 = d1 + o;
        in.min_depth[0] = min_depth[2 * p];
        in.min_depth[1] = min_depth[2 * p + 1];
        std::memcpy(in.cam0, cam0 + (size_t)nc * p, sizeof(double) * nc);
        std::memcpy(in.cam1, cam1 + (size_t)nc * p, sizeof(double) * nc);
        return in;
    };
    if (S_all == 0) { // (no device work: the normalisation scales are host values)
        if (norm_scale)
            for (int32_t p = 0; p < num_pairs; ++p) norm_scale[p] = make_problem(pair_input(p), opts, cfg).norm_scale;
        return;
    }

    const bool timed = g_prof_on.load();
    HypTiming tm;
    CtxLease lease(device);
    hipStream_t stream = lease.c->stream;
    HypBuffers B(v, S_all, sample_chunk);

    for (const RefineRun &run : refine_plan(num_pairs, offsets, chunk)) {
        const int np = run.p1 - run.p0;
        const int64_t *soff = sample_offsets + run.p0; // np + 1 values; sample 0 of the run at soff[0]
        if (soff[np] - soff[0] == 0) {
            if (norm_scale)
                for (int k = 0; k < np; ++k)
                    norm_scale[run.p0 + k] = make_problem(pair_input(run.p0 + k), opts, cfg).norm_scale;
            continue;
        }
        // ---- problems, packed upload, pair records (host/resident_pairs.h) ----
        Clock::time_point t0 = Clock::now();
        ResidentPairs R(stream, variant, np, offsets + run.p0, x0, x1, d0, d1, min_depth + 2 * (size_t)run.p0,
                        cam0 + (size_t)nc * run.p0, cam1 + (size_t)nc * run.p0, opts, cfg);
        if (norm_scale) std::copy(R.norm_scale.begin(), R.norm_scale.end(), norm_scale + run.p0);
        if (timed) tm.pairs_ms += 1e3 * secs(t0);
        hypothesize_run(R, stream, PairSel{np, nullptr}, soff, sample_types, sample_idx, models, counts, sample_chunk,
                        B, timed, tm);
    }
    if (timed) {
        std::lock_guard<std::mutex> lk(g_hyp_mu);
        g_hyp_timing = tm;
    }
}

// ---- the pair set (mp_pair_set_*): pairs set up once, resident until destroyed ----
struct PairSet {
    std::mutex mu; // calls on one set are serialised
    int device = 0;
    int variant = 0;
    RansacOptions opts;
    EstimatorConfig cfg;
    std::unique_ptr<ResidentPairs> R; // null: an empty set (no pairs)
    int32_t num_pairs = 0;
    std::vector<char> seen;        // check_selection's scratch
    std::vector<int64_t> out_off;  // the selection's positions in inlier_idx
    std::unique_ptr<DevArray<int>> d_pair_n; // the pairs' sizes for the sampler, made at the first draw
    // the candidates of the last candidates_set, until they are fetched (candidates_fetch),
    // replaced or the set is destroyed; no other call reads them
    std::unique_ptr<HypCompact> cand;
    const int *pair_sizes(hipStream_t stream) {
        if (!d_pair_n) {
            std::vector<int> hn((size_t)num_pairs);
            for (int32_t k = 0; k < num_pairs; ++k) hn[(size_t)k] = (int)R->n[(size_t)k];
            d_pair_n.reset(new DevArray<int>((size_t)num_pairs));
            MP_HIP(hipMemcpyAsync(d_pair_n->p, hn.data(), sizeof(int) * hn.size(), hipMemcpyHostToDevice, stream));
            MP_HIP(hipStreamSynchronize(stream)); // (hn dies here)
        }
        return d_pair_n->p;
    }
    // the selection of a call, checked; out_off[j]: the correspondences of the entries before j
    PairSel select(int32_t num_sel, const int32_t *pair_ids) {
        check_selection(num_pairs, num_sel, pair_ids, seen);
        out_off.assign((size_t)num_sel + 1, 0);
        for (int32_t j = 0; j < num_sel; ++j) out_off[j + 1] = out_off[j] + R->n[pair_ids ? pair_ids[j] : j];
        return PairSel{num_sel, pair_ids};
    }
};

// The confidence weights of one set (mp_draw_weights_*; include/mp_draw.h, kernels/
// draw_weighted.h): the pairs' tables on the device and what mp_draw_weights_info returns.
// Immutable once created; the calls that take it only read it, so the set holds nothing of it.
// When its set is destroyed the device arrays go and `set` becomes null: the handle stays a
// valid object that every call refuses until mp_draw_weights_destroy deletes it.
struct DrawWeights {
    const PairSet *set = nullptr;
    std::unique_ptr<DevArray<uint32_t>> d_cum;          // T + num_pairs entries: pair p's at off[p] + p
    std::unique_ptr<DevArray<int64_t>> d_cum_off;       // num_pairs
    std::unique_ptr<DevArray<unsigned char>> d_weighted; // num_pairs
    std::vector<int32_t> weighted, positive;
    std::vector<uint32_t> total;
};

namespace {
// the handles of `set` (null: of every set) lose their device arrays and their set
void invalidate_weights(const PairSet *set) {
    std::lock_guard<std::mutex> lk(g_weights_mu);
    for (DrawWeights *w : g_weights) {
        if (set && w->set != set) continue;
        w->d_cum.reset();
        w->d_cum_off.reset();
        w->d_weighted.reset();
        w->set = nullptr;
    }
}
// a call's weights, checked under the set's lock: a live handle of this set
void check_draw_weights(const PairSet *set, const DrawWeights *w) {
    if (!w) throw std::invalid_argument("null draw weights");
    std::lock_guard<std::mutex> lk(g_weights_mu);
    if (std::find(g_weights.begin(), g_weights.end(), w) == g_weights.end())
        throw std::invalid_argument("not a live draw-weights handle");
    if (!w->set) throw std::invalid_argument("the draw weights' pair set was destroyed");
    if (w->set != set) throw std::invalid_argument("the draw weights belong to another pair set");
}
void bind_weights(HypDraw &dr, const DrawWeights *w) {
    if (!w || !w->d_cum) return; // (no pair was given weights: the uniform launch)
    dr.d_cum = w->d_cum->p;
    dr.d_cum_off = w->d_cum_off->p;
    dr.d_weighted = w->d_weighted->p;
}

void release_live_sets() {
    invalidate_weights(nullptr);
    std::vector<PairSet *> sets;
    {
        std::lock_guard<std::mutex> lk(g_sets_mu);
        sets.swap(g_sets);
    }
    for (PairSet *s : sets) delete s;
}
} // namespace

int pair_set_prep_mode(int mode) {
    if (mode != 0 && mode != 1)
        throw std::invalid_argument("mode must be 0 (one preparation launch) or 1 (one launch per pair)");
    return g_pair_set_prep.exchange(mode);
}

PairSet *pair_set_create(int variant, int32_t num_pairs, const int64_t *offsets, const double *x0, const double *x1,
                         const double *d0, const double *d1, const double *min_depth, const double *cam0,
                         const double *cam1, const RansacOptions &opts, const EstimatorConfig &cfg, int device) {
    if (variant < 0 || variant > 3)
        throw std::invalid_argument("variant must be 0 (calibrated), 1 (shared focal), 2 (two focal) or 3 (scale only)");
    if (num_pairs < 0) throw std::invalid_argument("negative pair count");
    {
        PairInput none; // (the option checks of every entry point)
        validate(none, opts);
    }
    if (num_pairs > 0) {
        if (!offsets || !min_depth || !cam0 || !cam1)
            throw std::invalid_argument("null offsets, min_depth or cameras");
        check_pair_arrays(variant, num_pairs, offsets, x0, x1, d0, d1);
        if (offsets[num_pairs] - offsets[0] > kPairSetMaxCorr)
            throw std::invalid_argument("more than 2^26 correspondences in one set");
    }
    std::unique_ptr<PairSet> S(new PairSet());
    S->device = device;
    S->variant = variant;
    S->opts = opts;
    S->cfg = cfg;
    S->num_pairs = num_pairs;
    if (num_pairs > 0) {
        CtxLease lease(device);
        S->R.reset(new ResidentPairs(lease.c->stream, variant, num_pairs, offsets, x0, x1, d0, d1, min_depth, cam0,
                                     cam1, opts, cfg));
    }
    std::lock_guard<std::mutex> lk(g_sets_mu);
    g_sets.push_back(S.get());
    return S.release();
}

PairSet *pair_set_create_device(int variant, int32_t num_pairs, const int64_t *offsets, const DevicePairArrays &in,
                                const double *min_depth, const double *cam0, const double *cam1,
                                const RansacOptions &opts, const EstimatorConfig &cfg, int device) {
    if (variant < 0 || variant > 3)
        throw std::invalid_argument("variant must be 0 (calibrated), 1 (shared focal), 2 (two focal) or 3 (scale only)");
    if (num_pairs < 0) throw std::invalid_argument("negative pair count");
    {
        PairInput none; // (the option checks of every entry point)
        validate(none, opts);
    }
    if (num_pairs > 0) {
        if (!offsets || !min_depth || !cam0 || !cam1)
            throw std::invalid_argument("null offsets, min_depth or cameras");
        auto type_ok = [](int t) { return t == 0 || t == 1; };
        if (!type_ok(in.xy_type)) throw std::invalid_argument("xy_type must be 0 (float32) or 1 (float64)");
        if (offsets[0] < 0) throw std::invalid_argument("offsets must be non-negative");
        for (int32_t p = 0; p < num_pairs; ++p) {
            if (offsets[p + 1] < offsets[p]) throw std::invalid_argument("offsets must not decrease");
            if (offsets[p + 1] - offsets[p] > kRefinePairMax) throw std::invalid_argument("pair too large");
        }
        if (offsets[num_pairs] - offsets[0] > kPairSetMaxCorr)
            throw std::invalid_argument("more than 2^26 correspondences in one set");
        const bool arrays = in.d0 || in.d1;
        const bool maps = in.maps || in.num_maps != 0 || in.map_dims || in.map_ids;
        if (arrays && maps)
            throw std::invalid_argument("both depth sources given: pass d0 / d1 or the depth maps, not both");
        if (!arrays && !maps)
            throw std::invalid_argument("no depth source given: pass d0 / d1 or the depth maps");
        if (arrays) {
            if (!type_ok(in.depth_type)) throw std::invalid_argument("depth_type must be 0 (float32) or 1 (float64)");
            if (offsets[num_pairs] > 0 && (!in.d0 || !in.d1)) throw std::invalid_argument("null input array d0 or d1");
        } else {
            if (!type_ok(in.map_type)) throw std::invalid_argument("map_type must be 0 (float32) or 1 (float64)");
            if (in.num_maps <= 0 || !in.maps || !in.map_dims || !in.map_ids)
                throw std::invalid_argument("the map source needs maps, map_dims, map_ids and num_maps > 0");
            for (int32_t m = 0; m < in.num_maps; ++m) {
                const int64_t *d = in.map_dims + 4 * (size_t)m;
                if (d[0] <= 0 || d[1] <= 0 || d[2] <= 0 || d[3] <= 0)
                    throw std::invalid_argument("map_dims[" + std::to_string(m) + "]: bad depth-map or image size");
                if (!in.maps[m]) throw std::invalid_argument("depth_maps[" + std::to_string(m) + "] is null");
            }
            for (int64_t j = 0; j < 2 * (int64_t)num_pairs; ++j)
                if (in.map_ids[j] < 0 || in.map_ids[j] >= in.num_maps)
                    throw std::invalid_argument("map_ids[" + std::to_string(j) + "] = " + std::to_string(in.map_ids[j]) +
                                                " is outside the " + std::to_string(in.num_maps) + " maps");
        }
        if (offsets[num_pairs] > 0 && (!in.x0 || !in.x1)) throw std::invalid_argument("null input array x0 or x1");
    }
    std::unique_ptr<PairSet> S(new PairSet());
    S->device = device;
    S->variant = variant;
    S->opts = opts;
    S->cfg = cfg;
    S->num_pairs = num_pairs;
    if (num_pairs > 0) {
        CtxLease lease(device);
        S->R.reset(new ResidentPairs(lease.c->stream, device, variant, num_pairs, offsets, in, min_depth, cam0, cam1, opts,
                                     cfg));
    }
    std::lock_guard<std::mutex> lk(g_sets_mu);
    g_sets.push_back(S.get());
    return S.release();
}

void pair_set_record(const PairSet *set, int32_t pair, double *out) {
    if (!set) throw std::invalid_argument("null pair set");
    if (pair < 0 || pair >= set->num_pairs) throw std::invalid_argument("pair outside the set");
    if (!out) throw std::invalid_argument("null output");
    std::lock_guard<std::mutex> lk(const_cast<PairSet *>(set)->mu);
    const ResidentPairs &R = *set->R;
    CtxLease lease(set->device);
    hipStream_t stream = lease.c->stream;
    PairConst C;
    MP_HIP(hipMemcpyAsync(&C, R.d_C.p + pair, sizeof(PairConst), hipMemcpyDeviceToHost, stream));
    MP_HIP(hipStreamSynchronize(stream));
    pair_record_values(C, R.norm_scale[(size_t)pair], out);
}

void ingest_info(int32_t *out) {
    if (!out) throw std::invalid_argument("null output");
    out[0] = kIngestBlock;
    out[1] = kIngestChunk;
    out[2] = kIngestSpan;
}

void device_extent(const void *ptr, int device, int64_t *out) {
    if (!ptr || !out) throw std::invalid_argument("null pointer or output");
    CtxLease lease(device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(ptr)) != hipSuccess) {
        (void)hipGetLastError();
        throw std::invalid_argument("the pointer has no allocation range");
    }
    out[0] = (int64_t)(uintptr_t)base;
    out[1] = (int64_t)size;
}

void pair_set_destroy(PairSet *set) {
    if (!set) return;
    {
        std::lock_guard<std::mutex> lk(g_sets_mu);
        auto it = std::find(g_sets.begin(), g_sets.end(), set);
        if (it == g_sets.end()) throw std::invalid_argument("not a live pair set");
        g_sets.erase(it);
    }
    { std::lock_guard<std::mutex> lk(set->mu); } // (a call still running on it ends first)
    invalidate_weights(set);
    delete set;
}

DrawWeights *draw_weights_create(PairSet *set, const void *weights, int dtype, bool on_device,
                                 const unsigned char *given, void *producer_stream) {
    if (!set) throw std::invalid_argument("null pair set");
    if (dtype != 0 && dtype != 1) throw std::invalid_argument("dtype must be 0 (float32) or 1 (float64)");
    std::lock_guard<std::mutex> lk(set->mu);
    check_hyp_supported(set->variant, set->opts, set->cfg);
    const int32_t np = set->num_pairs;
    std::unique_ptr<DrawWeights> H(new DrawWeights());
    H->set = set;
    H->weighted.assign((size_t)np, 0);
    H->positive.assign((size_t)np, 0);
    H->total.assign((size_t)np, 0);
    bool any = false;
    for (int32_t p = 0; p < np; ++p) {
        if (given && !given[p]) continue;
        if (set->R->n[(size_t)p] > kDrawWeightMaxN)
            throw std::invalid_argument("pair " + std::to_string(p) + " has more than 65535 correspondences: pass no weights for it");
        any = any || set->R->n[(size_t)p] > 0;
    }
    if (any) {
        if (!weights) throw std::invalid_argument("null weights");
        const ResidentPairs &R = *set->R;
        const int v = R.v, kmd = draw_k_md(v), kpt = draw_k_pt(v);
        const int64_t T = R.T, e = dtype ? 8 : 4;
        CtxLease lease(set->device);
        hipStream_t stream = lease.c->stream;
        const void *d_w = weights;
        std::unique_ptr<DevArray<unsigned char>> up;
        struct Event {
            hipEvent_t ev = nullptr;
            ~Event() {
                if (ev) (void)hipEventDestroy(ev);
            }
        } produced;
        if (on_device) {
            // the pointer before any launch or copy, then the producer's work: an event on its
            // stream, no host wait (as the device ingest)
            check_device_array("weights", weights, ingest_bytes(T, 1, e), e, set->device);
            MP_HIP(hipEventCreateWithFlags(&produced.ev, hipEventDisableTiming));
            MP_HIP(hipEventRecord(produced.ev, static_cast<hipStream_t>(producer_stream)));
            MP_HIP(hipStreamWaitEvent(stream, produced.ev, 0));
        } else {
            up.reset(new DevArray<unsigned char>((size_t)(T * e)));
            MP_HIP(hipMemcpyAsync(up->p, weights, (size_t)(T * e), hipMemcpyHostToDevice, stream));
            d_w = up->p;
        }
        H->d_cum.reset(new DevArray<uint32_t>((size_t)T + (size_t)np));
        H->d_cum_off.reset(new DevArray<int64_t>((size_t)np));
        H->d_weighted.reset(new DevArray<unsigned char>((size_t)np));
        DevArray<int64_t> d_off((size_t)np);
        DevArray<unsigned char> d_given((size_t)np);
        DevArray<int> d_pos((size_t)np), d_bad(1);
        DevArray<uint32_t> d_total((size_t)np);
        std::vector<int64_t> cum_off((size_t)np);
        for (int32_t p = 0; p < np; ++p) cum_off[(size_t)p] = R.off[(size_t)p] + p;
        int bad = INT_MAX;
        const int *d_n = set->pair_sizes(stream);
        MP_HIP(hipMemcpyAsync(d_off.p, R.off.data(), sizeof(int64_t) * (size_t)np, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(H->d_cum_off->p, cum_off.data(), sizeof(int64_t) * (size_t)np, hipMemcpyHostToDevice,
                              stream));
        if (given) MP_HIP(hipMemcpyAsync(d_given.p, given, (size_t)np, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(d_bad.p, &bad, sizeof(int), hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemsetAsync(d_pos.p, 0, sizeof(int) * (size_t)np, stream));
        MP_HIP(hipMemsetAsync(d_total.p, 0, sizeof(uint32_t) * (size_t)np, stream));
        MP_HIP(launch_draw_weights_table(stream, d_w, dtype, d_off.p, d_n, given ? d_given.p : nullptr, np,
                                         H->d_cum->p, d_pos.p, d_total.p, d_bad.p));
        int bad_back = INT_MAX;
        MP_HIP(hipMemcpyAsync(H->positive.data(), d_pos.p, sizeof(int) * (size_t)np, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipMemcpyAsync(H->total.data(), d_total.p, sizeof(uint32_t) * (size_t)np, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipMemcpyAsync(&bad_back, d_bad.p, sizeof(int), hipMemcpyDeviceToHost, stream));
        MP_HIP(hipStreamSynchronize(stream)); // (the caller's array is not read after this)
        if (bad_back != INT_MAX) {
            const int p = (int)(std::upper_bound(R.off.begin(), R.off.end(), (int64_t)bad_back) - R.off.begin()) - 1;
            throw std::invalid_argument("weights[" + std::to_string(bad_back) + "] (pair " + std::to_string(p) +
                                        ", correspondence " + std::to_string(bad_back - R.off[(size_t)p]) +
                                        ") is not a finite value in 0..1");
        }
        std::vector<unsigned char> flags((size_t)np, 0);
        for (int32_t p = 0; p < np; ++p) {
            const bool g = !given || given[p];
            flags[(size_t)p] = g && H->positive[(size_t)p] >= draw_weighted_need(R.n[(size_t)p], kmd, kpt) ? 1 : 0;
            H->weighted[(size_t)p] = flags[(size_t)p];
        }
        MP_HIP(hipMemcpyAsync(H->d_weighted->p, flags.data(), (size_t)np, hipMemcpyHostToDevice, stream));
        MP_HIP(hipStreamSynchronize(stream));
    }
    std::lock_guard<std::mutex> lk2(g_weights_mu);
    g_weights.push_back(H.get());
    return H.release();
}

void draw_weights_info(const DrawWeights *w, int32_t *weighted, int32_t *positive, uint32_t *total) {
    if (!w) throw std::invalid_argument("null draw weights");
    std::lock_guard<std::mutex> lk(g_weights_mu);
    if (std::find(g_weights.begin(), g_weights.end(), w) == g_weights.end())
        throw std::invalid_argument("not a live draw-weights handle");
    if (!w->set) throw std::invalid_argument("the draw weights' pair set was destroyed");
    if (weighted) std::copy(w->weighted.begin(), w->weighted.end(), weighted);
    if (positive) std::copy(w->positive.begin(), w->positive.end(), positive);
    if (total) std::copy(w->total.begin(), w->total.end(), total);
}

void draw_weights_destroy(DrawWeights *w) {
    if (!w) return;
    const PairSet *set = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_weights_mu);
        auto it = std::find(g_weights.begin(), g_weights.end(), w);
        if (it == g_weights.end()) throw std::invalid_argument("not a live draw-weights handle");
        g_weights.erase(it);
        set = w->set;
    }
    // (a call still reading it ends first)
    if (set) { std::lock_guard<std::mutex> lk(const_cast<PairSet *>(set)->mu); }
    delete w;
}

void draw_weights_host(int64_t n, const void *weights, int dtype, uint32_t *cum, int32_t *positive) {
    if (n < 0 || n > kDrawWeightMaxN) throw std::invalid_argument("n must be in 0..65535");
    if (dtype != 0 && dtype != 1) throw std::invalid_argument("dtype must be 0 (float32) or 1 (float64)");
    if (!cum || !positive || (n > 0 && !weights)) throw std::invalid_argument("null weights or output");
    cum[0] = 0;
    int32_t pos = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double w = dtype ? static_cast<const double *>(weights)[i] : (double)static_cast<const float *>(weights)[i];
        uint32_t q;
        if (!draw_quantise(w, &q))
            throw std::invalid_argument("weights[" + std::to_string(i) + "] is not a finite value in 0..1");
        cum[i + 1] = cum[i] + q;
        pos += q > 0 ? 1 : 0;
    }
    *positive = pos;
}

void draw_weighted_host(int variant, int64_t n, const uint32_t *cum, uint64_t seed, int32_t point_share, int32_t pair,
                        int32_t s, int32_t *out) {
    if (variant < 0 || variant > 2) throw std::invalid_argument("variant must be 0, 1 or 2");
    if (n < 0 || n > kDrawWeightMaxN) throw std::invalid_argument("n must be in 0..65535");
    if (point_share < 0 || point_share > kDrawShareMax) throw std::invalid_argument("point_share must be in 0..256");
    if (pair < 0 || s < 0 || !out || !cum) throw std::invalid_argument("negative pair or sample, or null table or output");
    if (cum[0] != 0) throw std::invalid_argument("cum[0] must be 0");
    int64_t pos = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (cum[i + 1] < cum[i] || cum[i + 1] - cum[i] > kDrawWeightQMax)
            throw std::invalid_argument("cum must rise by at most 65535 per entry");
        pos += cum[i + 1] != cum[i] ? 1 : 0;
    }
    const int kmd = draw_k_md(variant), kpt = draw_k_pt(variant);
    if (pos < draw_weighted_need(n, kmd, kpt))
        throw std::invalid_argument("not a weighted pair: fewer positive weights than the largest sample");
    int idx[8];
    bool fill = false;
    out[0] = draw_sample_weighted((int)n, kmd, kpt, seed, point_share, (uint32_t)pair, (uint32_t)s, cum, idx, &fill);
    for (int a = 0; a < 8; ++a) out[1 + a] = idx[a];
    out[9] = fill ? 1 : 0;
}

void pair_set_info(const PairSet *set, int32_t *variant, int32_t *num_pairs, int64_t *correspondences,
                   int64_t *resident_bytes, int32_t *device) {
    if (!set) throw std::invalid_argument("null pair set");
    std::lock_guard<std::mutex> lk(const_cast<PairSet *>(set)->mu);
    if (variant) *variant = set->variant;
    if (num_pairs) *num_pairs = set->num_pairs;
    if (correspondences) *correspondences = set->R ? set->R->T : 0;
    if (resident_bytes) *resident_bytes = set->R ? set->R->resident_bytes() : 0;
    if (device) *device = set->device;
}

void pair_set_norm_scales(const PairSet *set, double *out) {
    if (!set) throw std::invalid_argument("null pair set");
    if (set->num_pairs == 0) return;
    if (!out) throw std::invalid_argument("null output");
    std::copy(set->R->norm_scale.begin(), set->R->norm_scale.end(), out);
}

void pair_set_rows(const PairSet *set, int32_t pair, double *out) {
    if (!set) throw std::invalid_argument("null pair set");
    if (pair < 0 || pair >= set->num_pairs) throw std::invalid_argument("pair outside the set");
    std::lock_guard<std::mutex> lk(const_cast<PairSet *>(set)->mu);
    const ResidentPairs &R = *set->R;
    const int64_t n = R.n[pair];
    if (n == 0) return;
    if (!out) throw std::invalid_argument("null output");
    CtxLease lease(set->device);
    hipStream_t stream = lease.c->stream;
    // rows 0 .. 5 and 6 .. 11 of a pair are each contiguous (host/refine_plan.h refine_row)
    MP_HIP(hipMemcpyAsync(out, R.d_data.p + refine_row(R.T, R.off[pair], n, 0), sizeof(double) * 6 * (size_t)n,
                          hipMemcpyDeviceToHost, stream));
    MP_HIP(hipMemcpyAsync(out + 6 * n, R.d_data.p + refine_row(R.T, R.off[pair], n, 6), sizeof(double) * 6 * (size_t)n,
                          hipMemcpyDeviceToHost, stream));
    MP_HIP(hipStreamSynchronize(stream));
}

void refine_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int rounds, Model *models,
                RefineResult *results, int32_t *inlier_idx, bool relax) {
    if (!set) throw std::invalid_argument("null pair set");
    if (rounds < 1 || rounds > 64) throw std::invalid_argument("rounds must be in 1..64");
    std::lock_guard<std::mutex> lk(set->mu);
    if (set->num_pairs == 0) {
        std::vector<char> seen;
        check_selection(0, num_sel, pair_ids, seen);
        return;
    }
    const PairSel sel = set->select(num_sel, pair_ids);
    if (num_sel == 0) return;
    if (!models || !results) throw std::invalid_argument("null models or results");
    CtxLease lease(set->device);
    refine_run(*set->R, lease.c->stream, sel, set->out_off.data(), set->cfg, rounds, models, results, inlier_idx,
               relax, set->opts.threshold_multiplier);
}

void lsq_fit_set(PairSet *set, int32_t num_entries, const int32_t *pair_ids, const int32_t *solver_types,
                 const double *factors, int rule, uint64_t seed, const int32_t *streams, const int32_t *substreams,
                 Model *models, LsqFitResult *results, int32_t *subset_idx, int64_t entry_chunk) {
    if (!set) throw std::invalid_argument("null pair set");
    std::lock_guard<std::mutex> lk(set->mu);
    check_lsq_entries(set->num_pairs, num_entries, pair_ids, solver_types, factors, rule, streams, substreams,
                      entry_chunk);
    if (num_entries == 0) return;
    if (!models || !results) throw std::invalid_argument("null models or results");
    ResidentPairs &R = *set->R;
    std::vector<int64_t> out_off((size_t)num_entries + 1, 0);
    for (int32_t e = 0; e < num_entries; ++e)
        out_off[(size_t)e + 1] = out_off[(size_t)e] + R.n[(size_t)(pair_ids ? pair_ids[e] : e)];
    CtxLease lease(set->device);
    LsqBuffers B;
    lsq_fit_run(R, lease.c->stream, set->opts, set->cfg, num_entries, pair_ids, solver_types, factors, rule, seed,
                streams, substreams, models, results, subset_idx, out_off.data(), entry_chunk, B);
}

namespace {
void check_subset_lists(const int64_t *offsets, const int32_t *idx, int64_t k, int32_t pair, int32_t stream,
                        int32_t substream, const int32_t *out_sizes) {
    if (!offsets || !out_sizes) throw std::invalid_argument("null offsets or sizes");
    if (offsets[0] != 0) throw std::invalid_argument("offsets must start at 0");
    for (int t = 0; t < 3; ++t) {
        if (offsets[t + 1] < offsets[t]) throw std::invalid_argument("offsets must not decrease");
        if (offsets[t + 1] - offsets[t] > (int64_t)kSubsetIndexMax) throw std::invalid_argument("list too long");
    }
    if (offsets[3] > 0 && !idx) throw std::invalid_argument("null idx");
    for (int t = 0; t < 3; ++t)
        for (int64_t j = offsets[t]; j < offsets[t + 1]; ++j) {
            if (idx[j] < 0 || (uint32_t)idx[j] >= kSubsetIndexMax)
                throw std::invalid_argument("index outside 0 .. 2^28 - 1");
            if (j > offsets[t] && idx[j] <= idx[j - 1]) throw std::invalid_argument("lists must ascend strictly");
        }
    if (k < 0 || k > INT32_MAX) throw std::invalid_argument("k must be in 0 .. 2^31 - 1");
    if (pair < 0 || stream < 0 || substream < 0 || (uint32_t)substream >= kSubsetSubstreamMax)
        throw std::invalid_argument("pair, stream or substream out of range");
}
} // namespace

void subset_select_host_hook(const int64_t *offsets, const int32_t *idx, int64_t k, uint64_t seed, int32_t pair,
                             int32_t stream, int32_t substream, uint64_t key_mask, int32_t *out_idx,
                             int32_t *out_sizes) {
    check_subset_lists(offsets, idx, k, pair, stream, substream, out_sizes);
    const int *lists[3] = {idx + offsets[0], idx + offsets[1], idx + offsets[2]};
    const int M[3] = {(int)(offsets[1] - offsets[0]), (int)(offsets[2] - offsets[1]), (int)(offsets[3] - offsets[2])};
    std::vector<int> out[3];
    subset_select_host(lists, M, k, seed, (uint32_t)pair, (uint32_t)stream, (uint32_t)substream, key_mask, out);
    for (int t = 0; t < 3; ++t) {
        out_sizes[t] = (int32_t)out[t].size();
        if (!out[t].empty()) {
            if (!out_idx) throw std::invalid_argument("null output");
            std::copy(out[t].begin(), out[t].end(), out_idx + offsets[t]);
        }
    }
}

void subset_select_device(const int64_t *offsets, const int32_t *idx, int64_t k, uint64_t seed, int32_t pair,
                          int32_t stream, int32_t substream, uint64_t key_mask, int32_t *out_idx, int32_t *out_sizes,
                          int device) {
    check_subset_lists(offsets, idx, k, pair, stream, substream, out_sizes);
    if (offsets[3] > 0 && !out_idx) throw std::invalid_argument("null output");
    // one entry whose three lists lie `stride` apart, as lsq_sweep_kernel leaves them
    int64_t stride = 1;
    for (int t = 0; t < 3; ++t) stride = std::max(stride, offsets[t + 1] - offsets[t]);
    CtxLease lease(device);
    hipStream_t s = lease.c->stream;
    DevArray<int> d_ws((size_t)(6 * stride));
    DevArray<LsqEntry> d_entry(1);
    DevArray<LsqOut> d_out(1);
    LsqEntry E;
    std::memset(&E, 0, sizeof(E));
    E.pair = pair;
    E.rule = -1;
    E.k = (int)k;
    E.stream = (uint32_t)stream;
    E.substream = (uint32_t)substream;
    E.stride = (int)stride;
    E.factor = 1.0;
    LsqOut O;
    std::memset(&O, 0, sizeof(O));
    for (int t = 0; t < 3; ++t) {
        O.wide[t] = (int)(offsets[t + 1] - offsets[t]);
        if (O.wide[t] > 0)
            MP_HIP(hipMemcpyAsync(d_ws.p + t * stride, idx + offsets[t], sizeof(int) * (size_t)O.wide[t],
                                  hipMemcpyHostToDevice, s));
    }
    MP_HIP(hipMemcpyAsync(d_entry.p, &E, sizeof(E), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(d_out.p, &O, sizeof(O), hipMemcpyHostToDevice, s));
    MP_HIP(launch_lsq_subset(s, d_entry.p, 1, d_ws.p, d_out.p, 0, 1, 1, seed, key_mask));
    MP_HIP(hipMemcpyAsync(&O, d_out.p, sizeof(O), hipMemcpyDeviceToHost, s));
    MP_HIP(hipStreamSynchronize(s));
    for (int t = 0; t < 3; ++t) {
        out_sizes[t] = O.sub[t];
        if (O.sub[t] < 0 || O.sub[t] > O.wide[t]) throw std::logic_error("subset_select: a size outside its list");
        if (O.sub[t] > 0)
            MP_HIP(hipMemcpyAsync(out_idx + offsets[t], d_ws.p + (3 + t) * stride, sizeof(int) * (size_t)O.sub[t],
                                  hipMemcpyDeviceToHost, s));
    }
    MP_HIP(hipStreamSynchronize(s));
}

int lsq_subset_size(int rule, int solver_type, int variant, int mu, int nu, const int32_t *sizes, int64_t *k) {
    if (rule != kSubsetLsq && rule != kSubsetNonmin) throw std::invalid_argument("rule must be 0 (lsq) or 1 (nonmin)");
    if (solver_type != 0 && solver_type != 1) throw std::invalid_argument("solver_type must be 0 or 1");
    if (variant < 0 || variant > 3) throw std::invalid_argument("variant must be in 0..3");
    if (!sizes || !k) throw std::invalid_argument("null sizes or k");
    for (int t = 0; t < 3; ++t)
        if (sizes[t] < 0 || (uint32_t)sizes[t] > kSubsetIndexMax)
            throw std::invalid_argument("sizes must be in 0 .. 2^28");
    if (mu < 0 || nu < 0) throw std::invalid_argument("negative multiplier");
    const int M[3] = {sizes[0], sizes[1], sizes[2]};
    return subset_size(rule, solver_type, variant == kScaleOnly ? kCal : variant, mu, nu, M, k) ? 1 : 0;
}

void select_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *model_offsets,
                const Model *models, double *scores, int32_t *counts, SelectResult *results, int32_t *inlier_idx,
                int64_t model_chunk) {
    if (!set) throw std::invalid_argument("null pair set");
    if (model_chunk < 0) throw std::invalid_argument("model_chunk must not be negative");
    std::lock_guard<std::mutex> lk(set->mu);
    if (set->num_pairs == 0) {
        std::vector<char> seen;
        check_selection(0, num_sel, pair_ids, seen);
        return;
    }
    const PairSel sel = set->select(num_sel, pair_ids);
    if (num_sel == 0) return;
    if (!model_offsets || !results) throw std::invalid_argument("null model_offsets or results");
    if (model_offsets[0] < 0) throw std::invalid_argument("offsets must be non-negative");
    for (int32_t j = 0; j < num_sel; ++j)
        if (model_offsets[j + 1] < model_offsets[j]) throw std::invalid_argument("offsets must not decrease");
    if (model_offsets[num_sel] - model_offsets[0] > kSelectModelsMax)
        throw std::invalid_argument("more than 2^28 candidates");
    if (model_offsets[num_sel] > model_offsets[0] && !models) throw std::invalid_argument("null models");
    const int tile_set = g_select_tile.load();
    const int tile = tile_set ? tile_set : kSelectTile;
    const bool timed = g_prof_on.load();
    SelectTiming tm;
    CtxLease lease(set->device);
    select_run(*set->R, lease.c->stream, sel, set->out_off.data(), model_offsets, models, scores, counts, results,
               inlier_idx, model_chunk, tile, timed, tm);
    if (timed) {
        std::lock_guard<std::mutex> lk2(g_select_mu);
        g_select_timing = tm;
    }
}

void hypothesize_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *sample_offsets,
                     const int32_t *sample_types, const int32_t *sample_idx, Model *models, int32_t *counts,
                     int64_t sample_chunk) {
    if (!set) throw std::invalid_argument("null pair set");
    if (sample_chunk < 0) throw std::invalid_argument("sample_chunk must not be negative");
    std::lock_guard<std::mutex> lk(set->mu);
    check_hyp_supported(set->variant, set->opts, set->cfg);
    if (set->num_pairs == 0) {
        std::vector<char> seen;
        check_selection(0, num_sel, pair_ids, seen);
        return;
    }
    const PairSel sel = set->select(num_sel, pair_ids);
    if (num_sel == 0) return;
    if (!sample_offsets) throw std::invalid_argument("null sample_offsets");
    if (sample_offsets[0] < 0) throw std::invalid_argument("offsets must be non-negative");
    for (int32_t j = 0; j < num_sel; ++j)
        if (sample_offsets[j + 1] < sample_offsets[j]) throw std::invalid_argument("offsets must not decrease");
    const int64_t S = sample_offsets[num_sel] - sample_offsets[0];
    if (S > kHypSamplesMax) throw std::invalid_argument("more than 2^22 samples");
    if (S == 0) return;
    if (!sample_types || !sample_idx || !models || !counts)
        throw std::invalid_argument("null sample_types, sample_idx, models or counts");
    const ResidentPairs &R = *set->R;
    check_hyp_samples(R.v, num_sel, [&](int32_t j) { return R.n[sel[j]]; }, sample_offsets, sample_types, sample_idx);
    const bool timed = g_prof_on.load();
    HypTiming tm;
    CtxLease lease(set->device);
    HypBuffers B(R.v, S, sample_chunk);
    hypothesize_run(*set->R, lease.c->stream, sel, sample_offsets, sample_types, sample_idx, models, counts,
                    sample_chunk, B, timed, tm);
    if (timed) {
        std::lock_guard<std::mutex> lk2(g_hyp_mu);
        g_hyp_timing = tm;
    }
}

namespace {
std::mutex g_ransac_mu;
RansacTiming g_ransac_timing;

// the checks mp_hypothesize_set makes on given samples (all before any device call); returns S
int64_t check_set_samples(const ResidentPairs &R, const PairSel sel, const int64_t *sample_offsets,
                          const int32_t *sample_types, const int32_t *sample_idx) {
    if (!sample_offsets) throw std::invalid_argument("null sample_offsets");
    if (sample_offsets[0] < 0) throw std::invalid_argument("offsets must be non-negative");
    for (int32_t j = 0; j < sel.n; ++j)
        if (sample_offsets[j + 1] < sample_offsets[j]) throw std::invalid_argument("offsets must not decrease");
    const int64_t S = sample_offsets[sel.n] - sample_offsets[0];
    if (S > kHypSamplesMax) throw std::invalid_argument("more than 2^22 samples");
    if (S > 0 && (!sample_types || !sample_idx)) throw std::invalid_argument("null sample_types or sample_idx");
    check_hyp_samples(R.v, sel.n, [&](int32_t j) { return R.n[sel[j]]; }, sample_offsets, sample_types, sample_idx);
    return S;
}

void check_draw_args(int32_t num_sel, int32_t budget, int32_t point_share) {
    if (budget < 0) throw std::invalid_argument("budget must not be negative");
    if (point_share < -1 || point_share > kDrawShareMax) throw std::invalid_argument("point_share must be in -1..256");
    if ((int64_t)(num_sel > 0 ? num_sel : 0) * budget > kHypSamplesMax)
        throw std::invalid_argument("more than 2^22 samples (num_sel x budget)");
}

// The drawn samples of a selection: budget per entry, none for a pair too small for the MD
// solver; soff (ns + 1, from 0) and the types from word 0 of each sample's stream (host).
void draw_plan(const ResidentPairs &R, const PairSel sel, int32_t budget, uint64_t seed, int share,
               std::vector<int64_t> &soff, std::vector<int32_t> &types) {
    const int kmd = draw_k_md(R.v), kpt = draw_k_pt(R.v);
    soff.assign((size_t)sel.n + 1, 0);
    for (int j = 0; j < sel.n; ++j) soff[(size_t)j + 1] = soff[(size_t)j] + (R.n[sel[j]] >= kmd ? budget : 0);
    types.resize((size_t)soff[(size_t)sel.n]);
    for (int j = 0; j < sel.n; ++j) {
        const int64_t n = R.n[sel[j]];
        int32_t *t = types.data() + soff[(size_t)j];
        for (int64_t s = 0; s < soff[(size_t)j + 1] - soff[(size_t)j]; ++s)
            t[s] = draw_type(n, kpt, seed, share, (uint32_t)sel[j], (uint32_t)s);
    }
}
// One round of ransac_adaptive_set: entry j takes its pair's samples first[j] ..
// first[j] + count[j] - 1 (every entry's pair is large enough for the MD solver).
void draw_plan(const ResidentPairs &R, const PairSel sel, const int32_t *first, const int32_t *count, uint64_t seed,
               int share, std::vector<int64_t> &soff, std::vector<int32_t> &types) {
    const int kpt = draw_k_pt(R.v);
    soff.assign((size_t)sel.n + 1, 0);
    for (int j = 0; j < sel.n; ++j) soff[(size_t)j + 1] = soff[(size_t)j] + count[j];
    types.resize((size_t)soff[(size_t)sel.n]);
    for (int j = 0; j < sel.n; ++j) {
        const int64_t n = R.n[sel[j]];
        int32_t *t = types.data() + soff[(size_t)j];
        for (int32_t s = 0; s < count[j]; ++s)
            t[s] = draw_type(n, kpt, seed, share, (uint32_t)sel[j], (uint32_t)(first[j] + s));
    }
}

// The last stage of ransac_set and ransac_adaptive_set: the entries with a winner
// (best_candidate >= 0, models[j] the winner) go through one refine_run, their lists to their
// places in the selection; rounds = 0: nothing.
// swept (nullable; one per entry of the selection): for the entries with a winner, the
// problem-unit model their returned lists were swept from -- refine_run's, or with rounds = 0 the
// selected candidate with its focals divided by norm_scale, as select_run divides them.
void refine_winners(PairSet *set, hipStream_t stream, const PairSel sel, int32_t rounds, Model *models,
                    RansacResult *results, int32_t *inlier_idx, Model *swept = nullptr) {
    if (rounds < 1) {
        const ResidentPairs &R = *set->R;
        for (int j = 0; swept && j < sel.n; ++j) {
            if (results[j].best_candidate < 0) continue;
            swept[j] = models[j];
            if (R.variant == kSF || R.variant == kTF) {
                swept[j].focal0 /= R.norm_scale[sel[j]];
                swept[j].focal1 /= R.norm_scale[sel[j]];
            }
        }
        return;
    }
    std::vector<int32_t> win_ids;
    std::vector<int> win_j;
    std::vector<int64_t> win_off;
    std::vector<Model> win_models;
    for (int j = 0; j < sel.n; ++j) {
        if (results[j].best_candidate < 0) continue;
        win_j.push_back(j);
        win_ids.push_back(sel[j]);
        win_off.push_back(set->out_off[(size_t)j]);
        win_models.push_back(models[j]);
    }
    if (win_j.empty()) return;
    const int nw = (int)win_j.size();
    std::vector<RefineResult> rres((size_t)nw);
    std::vector<Model> win_swept(swept ? (size_t)nw : 0);
    refine_run(*set->R, stream, PairSel{nw, win_ids.data()}, win_off.data(), set->cfg, rounds, win_models.data(),
               rres.data(), inlier_idx, false, 1.0, nullptr, swept ? win_swept.data() : nullptr);
    for (int i = 0; i < nw; ++i) {
        RansacResult &Q = results[win_j[(size_t)i]];
        const RefineResult &F = rres[(size_t)i];
        if (swept) swept[win_j[(size_t)i]] = win_swept[(size_t)i];
        models[win_j[(size_t)i]] = win_models[(size_t)i];
        Q.score_initial = F.score_initial;
        Q.score_final = F.score_final;
        Q.rounds_run = F.rounds_run;
        Q.rounds_accepted = F.rounds_accepted;
        Q.lm_status = F.lm_status;
        for (int t = 0; t < 3; ++t) Q.num_inliers[t] = F.num_inliers[t];
    }
}

// mass_run's device arrays, grown to the largest run seen: the adaptive bodies size them once
// for their selection, so nothing grows with the rounds
struct MassBuffers {
    size_t cap = 0;
    std::unique_ptr<DevArray<unsigned char>> d_in; // cap ScoreRec, then cap MassItem: one upload
    std::unique_ptr<DevArray<MassOut>> d_out;
    std::vector<unsigned char> h_in;
    void ensure(size_t n) {
        if (n <= cap) return;
        d_in.reset();
        d_out.reset();
        d_in.reset(new DevArray<unsigned char>(n * (sizeof(ScoreRec) + sizeof(MassItem))));
        d_out.reset(new DevArray<MassOut>(n));
        cap = n;
    }
};

std::mutex g_mass_mu;
int64_t g_mass_launches = 0;
double g_mass_ms = 0.0;

// The weight mass of the inlier lists of given models (kernels/inlier_mass.h; the body of
// mp_inlier_mass_set and the weighted rule's stage).  Entry e is the model models[e] (user units)
// of pair pairs[e]; it goes to problem units and to a ScoreRec by the path of refine_run and of
// select_run's winner sweep, so the lists are the ones select returns for that single model.
// weighted[e] != 0: the rows weigh the q_i of the pair's table in w; 0: 1 each, total = n.  One
// upload, one launch, one copy back and one synchronise per run; it reads the set and the
// tables and writes only out (no list buffer of the set is touched, so a pair may repeat).
void mass_run(ResidentPairs &R, hipStream_t stream, const DrawWeights *w, size_t m, const int32_t *pairs,
              const unsigned char *weighted, const Model *models, MassOut *out, MassBuffers &B) {
    if (m == 0) return;
    static_assert(sizeof(ScoreRec) % alignof(MassItem) == 0 && sizeof(MassOut) == 32, "mass_run's packing");
    const auto t0 = Clock::now();
    const int variant = R.variant;
    B.ensure(m);
    B.h_in.resize(m * (sizeof(ScoreRec) + sizeof(MassItem)));
    ScoreRec *recs = reinterpret_cast<ScoreRec *>(B.h_in.data());
    MassItem *items = reinterpret_cast<MassItem *>(B.h_in.data() + m * sizeof(ScoreRec));
    bool any = false;
    for (size_t e = 0; e < m; ++e) {
        const int k = pairs[e];
        Model c = models[e];
        if (variant == kSF || variant == kTF) {
            c.focal0 /= R.norm_scale[(size_t)k];
            c.focal1 /= R.norm_scale[(size_t)k];
        }
        prepare_score_rec(R.Ch[(size_t)k], c, recs[e]);
        items[e].pair = k;
        items[e].weighted = weighted[e] ? 1 : 0;
        any = any || weighted[e];
    }
    if (any && (!w || !w->d_cum)) throw std::logic_error("mass_run: a weighted entry without a table");
    const unsigned char *d_in = B.d_in->p;
    MP_HIP(hipMemcpyAsync(B.d_in->p, B.h_in.data(), B.h_in.size(), hipMemcpyHostToDevice, stream));
    MP_HIP(launch_inlier_mass(stream, R.v, R.d_D.p, R.d_C.p, reinterpret_cast<const MassItem *>(d_in + m * sizeof(ScoreRec)),
                              reinterpret_cast<const ScoreRec *>(d_in), (int)m, any ? w->d_cum->p : nullptr,
                              any ? w->d_cum_off->p : nullptr, B.d_out->p));
    MP_HIP(hipMemcpyAsync(out, B.d_out->p, sizeof(MassOut) * m, hipMemcpyDeviceToHost, stream));
    MP_HIP(hipStreamSynchronize(stream));
    std::lock_guard<std::mutex> lk(g_mass_mu);
    ++g_mass_launches;
    g_mass_ms += 1e3 * secs(t0);
}

// The weighted rule's per-entry state of the adaptive bodies (weighted_stop): what the rule
// last read.  For an entry of a weighted pair the masses of its rule model's lists, replaced
// exactly when the rule model is; for any other entry its counts over n.
struct RuleMass {
    std::vector<InlierMass> rm;      // per entry
    std::vector<unsigned char> dirty; // the rule model changed during this checkpoint
    MassBuffers bufs;
    std::vector<int32_t> pairs;
    std::vector<unsigned char> flags;
    std::vector<Model> ms;
    std::vector<MassOut> outs;
    std::vector<int> which;
    void init(const ResidentPairs &R, const PairSel sel, const DrawWeights *w) {
        rm.assign((size_t)sel.n, InlierMass{});
        dirty.assign((size_t)sel.n, 0);
        for (int j = 0; j < sel.n; ++j) {
            const int k = sel[j];
            rm[(size_t)j].weighted = w->weighted[(size_t)k];
            rm[(size_t)j].total = w->weighted[(size_t)k] ? w->total[(size_t)k] : (uint32_t)R.n[(size_t)k];
        }
        bufs.ensure((size_t)sel.n);
    }
    // One mass_run over the active entries of weighted pairs whose rule model changed; counts_of(j):
    // the track's counts of entry j's rule model, which the kernel's must equal.
    template <class F>
    void update(ResidentPairs &R, hipStream_t stream, const DrawWeights *w, const PairSel sel,
                const std::vector<int> &active, const Model *models, F counts_of) {
        which.clear(), pairs.clear(), flags.clear(), ms.clear();
        for (int j : active) {
            if (!dirty[(size_t)j]) continue;
            dirty[(size_t)j] = 0;
            InlierMass &M = rm[(size_t)j];
            const int32_t *c = counts_of(j);
            if (!M.weighted) { // (not weighted: the counts, as the count rule reads them)
                for (int t = 0; t < 3; ++t) M.mass[t] = (uint32_t)c[t], M.count[t] = c[t];
                continue;
            }
            which.push_back(j);
            pairs.push_back(sel[j]);
            flags.push_back(1);
            ms.push_back(models[j]);
        }
        if (which.empty()) return;
        outs.resize(which.size());
        mass_run(R, stream, w, which.size(), pairs.data(), flags.data(), ms.data(), outs.data(), bufs);
        for (size_t i = 0; i < which.size(); ++i) {
            const int j = which[i];
            InlierMass &M = rm[(size_t)j];
            const MassOut &O = outs[i];
            const int32_t *c = counts_of(j);
            if (O.count[0] != c[0] || O.count[1] != c[1] || O.count[2] != c[2] || O.total != M.total)
                throw std::logic_error("weighted stop: the mass stage's counts of pair " + std::to_string(sel[j]) +
                                       " differ from its track's");
            for (int t = 0; t < 3; ++t) {
                if (O.mass[t] > O.total)
                    throw std::logic_error("weighted stop: a mass above the total, pair " + std::to_string(sel[j]));
                M.mass[t] = O.mass[t], M.count[t] = O.count[t];
            }
        }
    }
    // req[0 .. 1] of entry j: the weighted rule on its masses, or the count rule on its counts
    void required(int j, int kmd, int kpt, int64_t n, bool winner, const int32_t *counts, const StopOptions &so,
                  uint32_t req[2]) const {
        const InlierMass &M = rm[(size_t)j];
        for (int s = 0; s < 2; ++s)
            req[s] = M.weighted ? required_samples_mass(s, kmd, kpt, M.total, winner ? M.mass : nullptr, so)
                                : required_samples(s, kmd, kpt, n, winner ? counts : nullptr, so);
    }
};
} // namespace

void inlier_mass_stats(int64_t *launches, double *ms, bool reset) {
    std::lock_guard<std::mutex> lk(g_mass_mu);
    if (launches) *launches = g_mass_launches;
    if (ms) *ms = g_mass_ms;
    if (reset) g_mass_launches = 0, g_mass_ms = 0.0;
}

void inlier_mass_set(PairSet *set, const DrawWeights *weights, int32_t num_entries, const int32_t *pair_ids,
                     const Model *models, InlierMass *out) {
    if (!set) throw std::invalid_argument("null pair set");
    if (num_entries < 0 || num_entries > kMassEntriesMax) throw std::invalid_argument("num_entries must be in 0..2^24");
    std::lock_guard<std::mutex> lk(set->mu);
    check_draw_weights(set, weights);
    if (!pair_ids && num_entries > set->num_pairs) throw std::invalid_argument("more entries than pairs without pair_ids");
    for (int32_t e = 0; pair_ids && e < num_entries; ++e)
        if (pair_ids[e] < 0 || pair_ids[e] >= set->num_pairs)
            throw std::invalid_argument("pair_ids[" + std::to_string(e) + "] is outside the set");
    if (num_entries == 0) return;
    if (!models || !out) throw std::invalid_argument("null models or output");
    ResidentPairs &R = *set->R;
    std::vector<int32_t> pairs((size_t)num_entries);
    std::vector<unsigned char> flags((size_t)num_entries);
    for (int32_t e = 0; e < num_entries; ++e) {
        pairs[(size_t)e] = pair_ids ? pair_ids[e] : e;
        flags[(size_t)e] = weights->weighted[(size_t)pairs[(size_t)e]] ? 1 : 0;
    }
    std::vector<MassOut> outs((size_t)num_entries);
    CtxLease lease(set->device);
    MassBuffers B;
    mass_run(R, lease.c->stream, weights, (size_t)num_entries, pairs.data(), flags.data(), models, outs.data(), B);
    for (int32_t e = 0; e < num_entries; ++e) {
        const MassOut &O = outs[(size_t)e];
        const int k = pairs[(size_t)e];
        const uint32_t total = flags[(size_t)e] ? weights->total[(size_t)k] : (uint32_t)R.n[(size_t)k];
        if (O.total != total) throw std::logic_error("inlier_mass: the table's total of pair " + std::to_string(k) + " differs from the handle's");
        InlierMass &M = out[e];
        for (int t = 0; t < 3; ++t) M.mass[t] = O.mass[t], M.count[t] = O.count[t];
        M.total = O.total;
        M.weighted = flags[(size_t)e];
    }
}

void ransac_required_mass(int variant, uint32_t total, const uint32_t *mass, const RansacOptions &opts, uint32_t *req) {
    if (variant < 0 || variant > 2) throw std::invalid_argument("variant must be 0, 1 or 2");
    if (!req) throw std::invalid_argument("null output");
    for (int t = 0; mass && t < 3; ++t)
        if (mass[t] > total) throw std::invalid_argument("mass must be in 0..total");
    const StopOptions so{opts.success_probability, opts.min_num_iterations, opts.max_num_iterations_per_solver};
    for (int s = 0; s < 2; ++s) req[s] = required_samples_mass(s, draw_k_md(variant), draw_k_pt(variant), total, mass, so);
}

void inlier_mass_host_hook(int64_t n, const uint32_t *cum, const int64_t *offsets, const int32_t *idx, uint32_t *mass) {
    if (n < 0 || n > kDrawWeightMaxN) throw std::invalid_argument("n must be in 0..65535");
    if (!cum || !offsets || !mass) throw std::invalid_argument("null table, offsets or output");
    if (cum[0] != 0) throw std::invalid_argument("cum[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
        if (cum[i + 1] < cum[i] || cum[i + 1] - cum[i] > kDrawWeightQMax)
            throw std::invalid_argument("cum must rise by at most 65535 per entry");
    if (offsets[0] != 0) throw std::invalid_argument("offsets must start at 0");
    for (int t = 0; t < 3; ++t)
        if (offsets[t + 1] < offsets[t] || offsets[t + 1] - offsets[t] > n)
            throw std::invalid_argument("a list must hold 0..n indices");
    if (offsets[3] > 0 && !idx) throw std::invalid_argument("null idx");
    for (int t = 0; t < 3; ++t)
        for (int64_t j = offsets[t]; j < offsets[t + 1]; ++j) {
            if (idx[j] < 0 || idx[j] >= n) throw std::invalid_argument("index outside 0 .. n - 1");
            if (j > offsets[t] && idx[j] <= idx[j - 1]) throw std::invalid_argument("lists must ascend strictly");
        }
    inlier_mass_host(cum, offsets, idx, mass);
}

// ---- the errors and inlier mask of every correspondence (mp_residuals_set) ----
namespace {
std::mutex g_resid_mu;
int64_t g_resid_launches = 0;
double g_resid_ms = 0.0;

// residuals_set's checks, all before the device is touched
void residuals_check(const PairSet *set, int32_t ne, const int32_t *pair_ids, const Model *models,
                     const double *factors) {
    if (!pair_ids && ne != set->num_pairs)
        throw std::invalid_argument("num_entries must be the pair count without pair_ids");
    for (int32_t e = 0; factors && e < ne; ++e)
        if (!(std::isfinite(factors[e]) && factors[e] > 0.0))
            throw std::invalid_argument("factors[" + std::to_string(e) + "] must be finite and > 0");
    for (int32_t e = 0; pair_ids && e < ne; ++e)
        if (pair_ids[e] < 0 || pair_ids[e] >= set->num_pairs)
            throw std::invalid_argument("pair_ids[" + std::to_string(e) + "] is outside the set");
    if (ne > 0 && !models) throw std::invalid_argument("null models");
}
} // namespace

void residuals_stats(int64_t *launches, double *ms, bool reset) {
    std::lock_guard<std::mutex> lk(g_resid_mu);
    if (launches) *launches = g_resid_launches;
    if (ms) *ms = g_resid_ms;
    if (reset) g_resid_launches = 0, g_resid_ms = 0.0;
}

void residuals_set(PairSet *set, int32_t num_entries, const int32_t *pair_ids, const Model *models,
                   const double *factors, const ResidualsOut &out, int64_t *row_offsets, int32_t *counts) {
    if (!set) throw std::invalid_argument("null pair set");
    if (!out.mask) throw std::invalid_argument("null mask");
    if (!row_offsets || !counts) throw std::invalid_argument("null row_offsets or counts");
    if (num_entries < 0 || num_entries > kResidEntriesMax)
        throw std::invalid_argument("num_entries must be in 0..2^24");
    std::lock_guard<std::mutex> lk(set->mu);
    residuals_check(set, num_entries, pair_ids, models, factors);
    row_offsets[0] = 0;
    if (num_entries == 0) return;
    const int32_t ne = num_entries;
    ResidentPairs &R = *set->R;
    const int variant = R.variant;
    std::vector<int32_t> pairs((size_t)ne);
    std::vector<int64_t> sizes((size_t)ne);
    for (int32_t e = 0; e < ne; ++e) {
        pairs[(size_t)e] = pair_ids ? pair_ids[e] : e;
        sizes[(size_t)e] = R.n[(size_t)pairs[(size_t)e]];
    }
    resid_offsets(ne, sizes.data(), row_offsets);
    std::fill(counts, counts + 3 * (size_t)ne, 0);
    const int64_t rows = row_offsets[ne];
    if (rows == 0) return; // (no row: nothing is launched or written)
    const bool dev = out.on_device != 0, want_err = out.errors != nullptr;

    CtxLease lease(set->device);
    hipStream_t stream = lease.c->stream;
    struct Event { // (destroyed after the last synchronise, or on the way out)
        hipEvent_t ev = nullptr;
        ~Event() {
            if (ev) (void)hipEventDestroy(ev);
        }
    } produced, t0, t1;
    if (dev) {
        // ---- both device pointers, before any launch or copy ----
        const int64_t mb = resid_mask_bytes(rows), eb = resid_error_bytes(rows);
        check_device_array("mask", out.mask, mb, 1, set->device);
        if (want_err) {
            check_device_array("errors", out.errors, eb, 8, set->device);
            if (resid_overlap((uint64_t)(uintptr_t)out.mask, mb, (uint64_t)(uintptr_t)out.errors, eb))
                throw std::invalid_argument("device arrays mask and errors overlap");
        }
        // ---- the producer's work first: an event on its stream, no host wait ----
        MP_HIP(hipEventCreateWithFlags(&produced.ev, hipEventDisableTiming));
        MP_HIP(hipEventRecord(produced.ev, static_cast<hipStream_t>(out.producer_stream)));
        MP_HIP(hipStreamWaitEvent(stream, produced.ev, 0));
    }
    const bool timed = g_prof_on.load();
    if (timed) {
        MP_HIP(hipEventCreate(&t0.ev));
        MP_HIP(hipEventCreate(&t1.ev));
    }

    // (MADPOSE_RESIDUALS_RUN_ROWS / _RUN_ENTRIES: smaller runs, for the tests of the cut)
    const int64_t row_bound = dev ? kResidRunRowsDevice : kResidRunRows;
    const int64_t run_rows = env_int("MADPOSE_RESIDUALS_RUN_ROWS", row_bound, 1, row_bound);
    const int32_t run_entries = (int32_t)env_int("MADPOSE_RESIDUALS_RUN_ENTRIES", kResidRunEntries, 1, kResidRunEntries);
    std::vector<ResidRun> runs;
    resid_runs(ne, row_offsets, run_rows, run_entries, runs);
    size_t max_e = 0, max_items = 0;
    int64_t max_rows = 0;
    for (const ResidRun &r : runs) {
        max_e = std::max(max_e, (size_t)(r.e1 - r.e0));
        // (an entry of n rows has ceil(n / kResidItemRows) <= n / kResidItemRows + 1 items)
        max_items = std::max(max_items, (size_t)(r.e1 - r.e0) + (size_t)(r.rows / kResidItemRows));
        max_rows = std::max(max_rows, r.rows);
    }
    DevArray<ScoreRec> d_recs(max_e);
    DevArray<ResidItem> d_items(max_items);
    DevArray<ResidCount> d_cnt(max_items);
    // host outputs: the scratch of one run (device outputs are written in place)
    std::unique_ptr<DevArray<unsigned char>> d_mask;
    std::unique_ptr<DevArray<double>> d_err;
    if (!dev) {
        d_mask.reset(new DevArray<unsigned char>((size_t)max_rows));
        if (want_err) d_err.reset(new DevArray<double>(3 * (size_t)max_rows));
    }
    std::vector<ScoreRec> recs;
    std::vector<ResidItem> items;
    std::vector<int64_t> first_item;
    std::vector<ResidCount> cnt;
    int64_t launches = 0;
    double ms = 0.0;
    for (const ResidRun &r : runs) {
        if (r.rows == 0) continue; // (entries without correspondences: their counts are 0)
        recs.resize((size_t)(r.e1 - r.e0));
        for (int32_t e = r.e0; e < r.e1; ++e) {
            const int k = pairs[(size_t)e];
            Model c = models[e];
            if (variant == kSF || variant == kTF) {
                c.focal0 /= R.norm_scale[(size_t)k];
                c.focal1 /= R.norm_scale[(size_t)k];
            }
            prepare_score_rec(R.Ch[(size_t)k], c, recs[(size_t)(e - r.e0)]);
        }
        resid_items(r, pairs.data(), factors, row_offsets, dev ? 0 : r.row0, items, first_item);
        if (items.size() > max_items) throw std::logic_error("residuals: more items than planned");
        cnt.resize(items.size());
        unsigned char *mask = dev ? static_cast<unsigned char *>(out.mask) : d_mask->p;
        double *err = !want_err ? nullptr : dev ? static_cast<double *>(out.errors) : d_err->p;
        const int64_t stride = dev ? rows : r.rows;
        MP_HIP(hipMemcpyAsync(d_recs.p, recs.data(), sizeof(ScoreRec) * recs.size(), hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(d_items.p, items.data(), sizeof(ResidItem) * items.size(), hipMemcpyHostToDevice,
                              stream));
        if (timed) MP_HIP(hipEventRecord(t0.ev, stream));
        MP_HIP(launch_residuals(stream, R.v, R.d_D.p, R.d_C.p, d_items.p, (int)items.size(), d_recs.p, mask, err,
                                stride, d_cnt.p));
        if (timed) MP_HIP(hipEventRecord(t1.ev, stream));
        MP_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(ResidCount) * items.size(), hipMemcpyDeviceToHost, stream));
        if (!dev) {
            MP_HIP(hipMemcpyAsync(static_cast<unsigned char *>(out.mask) + r.row0, d_mask->p, (size_t)r.rows,
                                  hipMemcpyDeviceToHost, stream));
            for (int t = 0; want_err && t < 3; ++t)
                MP_HIP(hipMemcpyAsync(static_cast<double *>(out.errors) + (int64_t)t * rows + r.row0,
                                      d_err->p + (int64_t)t * r.rows, sizeof(double) * (size_t)r.rows,
                                      hipMemcpyDeviceToHost, stream));
        }
        MP_HIP(hipStreamSynchronize(stream)); // (recs, items and the scratch are reused by the next run)
        if (timed) {
            float f = 0.f;
            MP_HIP(hipEventElapsedTime(&f, t0.ev, t1.ev));
            ms += f;
        }
        ++launches;
        for (int32_t e = r.e0; e < r.e1; ++e)
            for (int64_t j = first_item[(size_t)(e - r.e0)]; j < first_item[(size_t)(e - r.e0) + 1]; ++j)
                for (int t = 0; t < 3; ++t) counts[3 * (size_t)e + t] += cnt[(size_t)j].count[t];
    }
    std::lock_guard<std::mutex> sl(g_resid_mu);
    g_resid_launches += launches;
    g_resid_ms += ms;
}

// ---- the Gauss-Newton system over a model's inliers and its inverse (mp_information_set) ----
namespace {
std::mutex g_info_mu;
int64_t g_info_launches = 0;
double g_info_rows_ms = 0.0, g_info_finish_ms = 0.0;
} // namespace

void information_stats(int64_t *launches, double *rows_ms, double *finish_ms, bool reset) {
    std::lock_guard<std::mutex> lk(g_info_mu);
    if (launches) *launches = g_info_launches;
    if (rows_ms) *rows_ms = g_info_rows_ms;
    if (finish_ms) *finish_ms = g_info_finish_ms;
    if (reset) g_info_launches = 0, g_info_rows_ms = g_info_finish_ms = 0.0;
}

void information_set(PairSet *set, int32_t num_entries, const int32_t *pair_ids, const Model *models,
                     const double *factors, const InformationOut &out, InfoRecord *entries) {
    static_assert(sizeof(Model) == 17 * sizeof(double), "InfoJob::m");
    if (!set) throw std::invalid_argument("null pair set");
    if (num_entries < 0 || num_entries > kInfoEntriesMax) throw std::invalid_argument("num_entries must be in 0..2^24");
    if (num_entries > 0 && !entries) throw std::invalid_argument("null entries");
    std::lock_guard<std::mutex> lk(set->mu);
    residuals_check(set, num_entries, pair_ids, models, factors);
    if (num_entries == 0) return;
    const int32_t ne = num_entries;
    ResidentPairs &R = *set->R;
    const int variant = R.variant;
    std::vector<int32_t> pairs((size_t)ne);
    std::vector<int64_t> sizes((size_t)ne), row_off((size_t)ne + 1);
    for (int32_t e = 0; e < ne; ++e) {
        pairs[(size_t)e] = pair_ids ? pair_ids[e] : e;
        sizes[(size_t)e] = R.n[(size_t)pairs[(size_t)e]];
    }
    resid_offsets(ne, sizes.data(), row_off.data());
    const int64_t rows = row_off[(size_t)ne];
    const bool dev = out.on_device != 0;
    static const char *const names[kInfoArrays] = {"H", "g", "cost", "cov"};
    const int64_t per[kInfoArrays] = {kInfoPack, kInfoN, 1, kInfoN * kInfoN};
    void *const ptr[kInfoArrays] = {out.H, out.g, out.cost, out.cov};
    const int64_t bytes[kInfoArrays] = {info_H_bytes(ne), info_g_bytes(ne), info_cost_bytes(ne), info_cov_bytes(ne)};
    {
        // the outputs' extents, host or device: differences only, before anything is written
        uint64_t addr[kInfoArrays];
        for (int i = 0; i < kInfoArrays; ++i) {
            addr[i] = (uint64_t)(uintptr_t)ptr[i];
            if (addr[i] && bytes[i] < 0) throw std::invalid_argument(std::string("array ") + names[i] + " leaves int64");
        }
        int a = 0, b = 0;
        if (info_out_overlap(addr, bytes, &a, &b))
            throw std::invalid_argument(std::string(dev ? "device arrays " : "arrays ") + names[a] + " and " +
                                        names[b] + " overlap");
    }
    InfoRecord none;
    std::memset(&none, 0, sizeof(none));
    none.pd = -1;
    std::fill(entries, entries + ne, none);
    if (rows == 0 && !dev) { // (no row: nothing is launched; every entry is status 0)
        for (int i = 0; i < kInfoArrays; ++i)
            if (ptr[i]) std::memset(ptr[i], 0, (size_t)bytes[i]);
        return;
    }

    CtxLease lease(set->device);
    hipStream_t stream = lease.c->stream;
    struct Event { // (destroyed after the last synchronise, or on the way out)
        hipEvent_t ev = nullptr;
        ~Event() {
            if (ev) (void)hipEventDestroy(ev);
        }
    } produced, t0, t1, t2;
    if (dev) {
        // ---- every device pointer, before any launch or copy ----
        for (int i = 0; i < kInfoArrays; ++i)
            if (ptr[i]) check_device_array(names[i], ptr[i], bytes[i], 8, set->device);
        // ---- the producer's work first: an event on its stream, no host wait ----
        MP_HIP(hipEventCreateWithFlags(&produced.ev, hipEventDisableTiming));
        MP_HIP(hipEventRecord(produced.ev, static_cast<hipStream_t>(out.producer_stream)));
        MP_HIP(hipStreamWaitEvent(stream, produced.ev, 0));
        if (rows == 0) { // (no row: no kernel; the entries' rows of the outputs are zero)
            for (int i = 0; i < kInfoArrays; ++i)
                if (ptr[i]) MP_HIP(hipMemsetAsync(ptr[i], 0, (size_t)bytes[i], stream));
            MP_HIP(hipStreamSynchronize(stream));
            return;
        }
    }
    const bool timed = g_prof_on.load();
    if (timed) {
        MP_HIP(hipEventCreate(&t0.ev));
        MP_HIP(hipEventCreate(&t1.ev));
        MP_HIP(hipEventCreate(&t2.ev));
    }

    // (MADPOSE_INFORMATION_RUN_ROWS / _RUN_ENTRIES: smaller runs, for the tests of the cut)
    const int64_t run_rows = env_int("MADPOSE_INFORMATION_RUN_ROWS", kInfoRunRows, 1, kInfoRunRows);
    const int32_t run_entries = (int32_t)env_int("MADPOSE_INFORMATION_RUN_ENTRIES", kInfoRunEntries, 1, kInfoRunEntries);
    std::vector<ResidRun> runs;
    resid_runs(ne, row_off.data(), run_rows, run_entries, runs);
    size_t max_e = 0;
    int64_t max_items = 0;
    for (const ResidRun &r : runs) {
        max_e = std::max(max_e, (size_t)(r.e1 - r.e0));
        max_items = std::max(max_items, info_max_items(r));
    }
    if (info_workspace_bytes(max_items) < 0) throw std::invalid_argument("information: the workspace leaves int64");
    DevArray<ScoreRec> d_recs(max_e);
    DevArray<InfoJob> d_jobs(max_e);
    DevArray<InfoRecord> d_out(max_e);
    DevArray<ResidItem> d_items((size_t)std::max<int64_t>(max_items, 1));
    DevArray<InfoPartial> d_part((size_t)std::max<int64_t>(max_items, 1));
    // host outputs: the scratch of one run (device outputs are written in place)
    std::unique_ptr<DevArray<double>> d_scr[kInfoArrays];
    for (int i = 0; i < kInfoArrays && !dev; ++i)
        if (ptr[i]) d_scr[i].reset(new DevArray<double>((size_t)per[i] * max_e));
    std::vector<ScoreRec> recs;
    std::vector<InfoJob> jobs;
    std::vector<ResidItem> items;
    std::vector<int64_t> first_item;
    const int one[3] = {1, 1, 1};
    int64_t launches = 0;
    double rows_ms = 0.0, finish_ms = 0.0;
    for (const ResidRun &r : runs) {
        const size_t nr = (size_t)(r.e1 - r.e0);
        recs.resize(nr);
        jobs.resize(nr);
        resid_items(r, pairs.data(), factors, row_off.data(), r.row0, items, first_item);
        if ((int64_t)items.size() > max_items) throw std::logic_error("information: more items than planned");
        for (int32_t e = r.e0; e < r.e1; ++e) {
            const int k = pairs[(size_t)e];
            Model c = models[e];
            if (variant == kSF || variant == kTF) {
                c.focal0 /= R.norm_scale[(size_t)k];
                c.focal1 /= R.norm_scale[(size_t)k];
            }
            prepare_score_rec(R.Ch[(size_t)k], c, recs[(size_t)(e - r.e0)]);
            // the flags of the job refine would run on these lists (sizes 1: what the LO type leaves)
            const LmJob L = make_lm_job(R.Ps[(size_t)k], set->cfg, one, 0, false, c);
            InfoJob &J = jobs[(size_t)(e - r.e0)];
            std::memcpy(J.m, &c, sizeof(J.m));
            J.w_sampson = L.w_sampson;
            J.use_reproj = L.n0 > 0 ? 1 : 0;
            J.use_sampson = L.n2 > 0 ? 1 : 0;
            J.use_shift = L.use_shift;
            J.first_item = first_item[(size_t)(e - r.e0)];
            J.nitems = (int)(first_item[(size_t)(e - r.e0) + 1] - J.first_item);
            J.out_row = dev ? (int64_t)e : (int64_t)(e - r.e0);
        }
        double *o[kInfoArrays];
        for (int i = 0; i < kInfoArrays; ++i)
            o[i] = !ptr[i] ? nullptr : dev ? static_cast<double *>(ptr[i]) : d_scr[i]->p;
        MP_HIP(hipMemcpyAsync(d_recs.p, recs.data(), sizeof(ScoreRec) * nr, hipMemcpyHostToDevice, stream));
        MP_HIP(hipMemcpyAsync(d_jobs.p, jobs.data(), sizeof(InfoJob) * nr, hipMemcpyHostToDevice, stream));
        if (!items.empty())
            MP_HIP(hipMemcpyAsync(d_items.p, items.data(), sizeof(ResidItem) * items.size(), hipMemcpyHostToDevice,
                                  stream));
        if (timed) MP_HIP(hipEventRecord(t0.ev, stream));
        MP_HIP(launch_information(stream, R.v, R.d_D.p, R.d_C.p, d_items.p, (int)items.size(), d_recs.p, d_jobs.p,
                                  d_part.p));
        if (timed) MP_HIP(hipEventRecord(t1.ev, stream));
        MP_HIP(launch_information_finish(stream, R.v, d_jobs.p, (int)nr, d_part.p, o[0], o[1], o[2], o[3], d_out.p));
        if (timed) MP_HIP(hipEventRecord(t2.ev, stream));
        MP_HIP(hipMemcpyAsync(entries + r.e0, d_out.p, sizeof(InfoRecord) * nr, hipMemcpyDeviceToHost, stream));
        for (int i = 0; i < kInfoArrays && !dev; ++i)
            if (ptr[i])
                MP_HIP(hipMemcpyAsync(static_cast<double *>(ptr[i]) + per[i] * (int64_t)r.e0, d_scr[i]->p,
                                      sizeof(double) * (size_t)per[i] * nr, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipStreamSynchronize(stream)); // (records, items and the scratch are reused by the next run)
        if (timed) {
            float f = 0.f;
            MP_HIP(hipEventElapsedTime(&f, t0.ev, t1.ev));
            rows_ms += f;
            MP_HIP(hipEventElapsedTime(&f, t1.ev, t2.ev));
            finish_ms += f;
        }
        ++launches;
    }
    std::lock_guard<std::mutex> sl(g_info_mu);
    g_info_launches += launches;
    g_info_rows_ms += rows_ms;
    g_info_finish_ms += finish_ms;
}

// ---- ransac's results into the caller's device arrays (mp_ransac_out_set) ----
namespace {
std::mutex g_rout_mu;
int64_t g_rout_launches = 0;
double g_rout_ms = 0.0;

// The output stage of the ransac bodies, under the set's mutex: check_args before anything,
// begin once the selection is known and the context leased (every pointer check, then the
// producer's event; nothing has been launched), swept() to refine_winners, finish after it.
// Without outputs every step does nothing.
struct RansacOutStage {
    const RansacOut *out;
    bool on = false;
    int64_t rows = 0;
    std::vector<Model> pm; // per entry: the problem-unit model its returned lists were swept from
    hipEvent_t produced = nullptr;

    explicit RansacOutStage(const RansacOut *o) : out(o && o->any() ? o : nullptr) {}
    RansacOutStage(const RansacOutStage &) = delete;
    RansacOutStage &operator=(const RansacOutStage &) = delete;
    ~RansacOutStage() {
        if (produced) (void)hipEventDestroy(produced);
    }

    void check_args(int32_t rounds, int32_t lo_rounds) const {
        if (!out) return;
        if (out->errors && !out->mask) throw std::invalid_argument("device array errors needs mask");
        if (lo_rounds >= 1 && rounds == 0)
            throw std::invalid_argument("device outputs with lo_rounds need rounds >= 1: without final rounds the "
                                        "overall best's lists may be a local optimisation's, whose model in problem "
                                        "units is not kept");
    }

    void begin(PairSet *set, int32_t num_sel, hipStream_t stream) {
        if (!out) return;
        rows = set->out_off[(size_t)num_sel];
        static const char *const names[kRansacOutArrays] = {"mask", "errors", "models", "index", "counts"};
        const int64_t elem[kRansacOutArrays] = {1, 8, 8, 4, 4};
        const void *ptr[kRansacOutArrays] = {out->mask, out->errors, out->models, out->index, out->counts};
        const int64_t bytes[kRansacOutArrays] = {resid_mask_bytes(rows), resid_error_bytes(rows),
                                                 ransac_out_models_bytes(num_sel), ransac_out_index_bytes(num_sel),
                                                 ransac_out_counts_bytes(num_sel)};
        uint64_t addr[kRansacOutArrays];
        for (int i = 0; i < kRansacOutArrays; ++i) {
            addr[i] = bytes[i] == 0 ? 0 : (uint64_t)(uintptr_t)ptr[i]; // (no element: nothing is written)
            if (addr[i]) check_device_array(names[i], ptr[i], bytes[i], elem[i], set->device);
        }
        int a = 0, b = 0;
        if (ransac_out_overlap(addr, bytes, &a, &b))
            throw std::invalid_argument(std::string("device arrays ") + names[a] + " and " + names[b] + " overlap");
        // ---- the producer's work first: an event on its stream, no host wait ----
        MP_HIP(hipEventCreateWithFlags(&produced, hipEventDisableTiming));
        MP_HIP(hipEventRecord(produced, static_cast<hipStream_t>(out->producer_stream)));
        MP_HIP(hipStreamWaitEvent(stream, produced, 0));
        pm.assign((size_t)num_sel, Model{});
        on = true;
    }

    Model *swept() { return on ? pm.data() : nullptr; }

    void finish(PairSet *set, const PairSel sel, hipStream_t stream, const Model *models, const RansacResult *results) {
        if (!on) return;
        static_assert(sizeof(Model) == 17 * sizeof(double) && sizeof(RansacOutPair) == 152, "per-pair row layout");
        const int32_t ns = sel.n;
        ResidentPairs &R = *set->R;
        const int64_t *row_off = set->out_off.data();
        std::vector<int32_t> pairs((size_t)ns);
        std::vector<unsigned char> winner((size_t)ns);
        for (int32_t j = 0; j < ns; ++j) {
            pairs[(size_t)j] = sel[j];
            winner[(size_t)j] = results[j].best_candidate >= 0 ? 1 : 0;
        }
        // ---- the per-pair rows: one small launch from an uploaded record per entry ----
        std::unique_ptr<DevArray<RansacOutPair>> d_rows;
        std::vector<RansacOutPair> h_rows;
        if (out->models || out->index || out->counts) {
            h_rows.resize((size_t)ns);
            for (int32_t j = 0; j < ns; ++j)
                h_rows[(size_t)j] = ransac_out_pair(winner[(size_t)j] != 0, reinterpret_cast<const double *>(&models[j]),
                                                    results[j].best_candidate, results[j].num_inliers);
            d_rows.reset(new DevArray<RansacOutPair>((size_t)ns));
            MP_HIP(hipMemcpyAsync(d_rows->p, h_rows.data(), sizeof(RansacOutPair) * (size_t)ns, hipMemcpyHostToDevice,
                                  stream));
            MP_HIP(launch_ransac_out_pairs(stream, d_rows->p, ns, static_cast<double *>(out->models),
                                           static_cast<int *>(out->index), static_cast<int *>(out->counts)));
        }
        // ---- the rows: the runs and items of host/residuals_plan.h, written in place ----
        int64_t launches = 0;
        double ms = 0.0;
        if (out->mask && rows > 0) {
            struct Event {
                hipEvent_t ev = nullptr;
                ~Event() {
                    if (ev) (void)hipEventDestroy(ev);
                }
            } t0, t1;
            const bool timed = g_prof_on.load();
            if (timed) {
                MP_HIP(hipEventCreate(&t0.ev));
                MP_HIP(hipEventCreate(&t1.ev));
            }
            const int64_t run_rows =
                env_int("MADPOSE_RESIDUALS_RUN_ROWS", kResidRunRowsDevice, 1, kResidRunRowsDevice);
            const int32_t run_entries =
                (int32_t)env_int("MADPOSE_RESIDUALS_RUN_ENTRIES", kResidRunEntries, 1, kResidRunEntries);
            std::vector<ResidRun> runs;
            resid_runs(ns, row_off, run_rows, run_entries, runs);
            size_t max_e = 0, max_items = 0;
            for (const ResidRun &r : runs) {
                max_e = std::max(max_e, (size_t)(r.e1 - r.e0));
                max_items = std::max(max_items, (size_t)(r.e1 - r.e0) + (size_t)(r.rows / kResidItemRows));
            }
            DevArray<ScoreRec> d_recs(max_e);
            DevArray<ResidItem> d_items(max_items);
            DevArray<ResidCount> d_cnt(max_items);
            std::vector<ScoreRec> recs;
            std::vector<ResidItem> items;
            std::vector<int64_t> first_item;
            std::vector<ResidCount> cnt;
            for (const ResidRun &r : runs) {
                if (r.rows == 0) continue; // (pairs without correspondences: no row to write)
                recs.assign((size_t)(r.e1 - r.e0), ScoreRec{});
                for (int32_t e = r.e0; e < r.e1; ++e)
                    if (winner[(size_t)e])
                        prepare_score_rec(R.Ch[(size_t)pairs[(size_t)e]], pm[(size_t)e], recs[(size_t)(e - r.e0)]);
                ransac_out_items(r, pairs.data(), winner.data(), row_off, items, first_item);
                if (items.size() > max_items) throw std::logic_error("ransac_out: more items than planned");
                cnt.resize(items.size());
                MP_HIP(hipMemcpyAsync(d_recs.p, recs.data(), sizeof(ScoreRec) * recs.size(), hipMemcpyHostToDevice,
                                      stream));
                MP_HIP(hipMemcpyAsync(d_items.p, items.data(), sizeof(ResidItem) * items.size(), hipMemcpyHostToDevice,
                                      stream));
                if (timed) MP_HIP(hipEventRecord(t0.ev, stream));
                MP_HIP(launch_ransac_out(stream, R.v, R.d_D.p, R.d_C.p, d_items.p, (int)items.size(), d_recs.p,
                                         static_cast<unsigned char *>(out->mask), static_cast<double *>(out->errors),
                                         rows, d_cnt.p));
                if (timed) MP_HIP(hipEventRecord(t1.ev, stream));
                MP_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(ResidCount) * items.size(), hipMemcpyDeviceToHost,
                                      stream));
                MP_HIP(hipStreamSynchronize(stream)); // (recs and items are reused by the next run)
                if (timed) {
                    float f = 0.f;
                    MP_HIP(hipEventElapsedTime(&f, t0.ev, t1.ev));
                    ms += f;
                }
                ++launches;
                // the mask's counts are the returned lists' lengths, or the evaluation is not the sweep's
                for (int32_t e = r.e0; e < r.e1; ++e) {
                    int64_t sum[3] = {0, 0, 0};
                    for (int64_t j = first_item[(size_t)(e - r.e0)]; j < first_item[(size_t)(e - r.e0) + 1]; ++j)
                        for (int t = 0; t < 3; ++t) sum[t] += cnt[(size_t)j].count[t];
                    for (int t = 0; t < 3; ++t)
                        if (sum[t] != (winner[(size_t)e] ? results[e].num_inliers[t] : 0))
                            throw std::logic_error("ransac_out: the mask of pair " + std::to_string(pairs[(size_t)e]) +
                                                   " counts other rows than its lists hold");
                }
            }
        }
        MP_HIP(hipStreamSynchronize(stream));
        std::lock_guard<std::mutex> sl(g_rout_mu);
        g_rout_launches += launches;
        g_rout_ms += ms;
    }
};
} // namespace

void ransac_out_stats(int64_t *launches, double *ms, bool reset) {
    std::lock_guard<std::mutex> lk(g_rout_mu);
    if (launches) *launches = g_rout_launches;
    if (ms) *ms = g_rout_ms;
    if (reset) g_rout_launches = 0, g_rout_ms = 0.0;
}

RansacTiming ransac_timing_last() {
    std::lock_guard<std::mutex> lk(g_ransac_mu);
    return g_ransac_timing;
}

void draw_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, uint64_t seed,
              int32_t point_share, int32_t *sample_types, int32_t *sample_idx, int32_t *sample_counts,
              const DrawWeights *weights) {
    if (!set) throw std::invalid_argument("null pair set");
    check_draw_args(num_sel, budget, point_share);
    std::lock_guard<std::mutex> lk(set->mu);
    if (weights) check_draw_weights(set, weights);
    check_hyp_supported(set->variant, set->opts, set->cfg);
    if (set->num_pairs == 0) {
        std::vector<char> seen;
        check_selection(0, num_sel, pair_ids, seen);
        return;
    }
    const PairSel sel = set->select(num_sel, pair_ids);
    if (num_sel == 0) return;
    if (!sample_counts) throw std::invalid_argument("null sample_counts");
    if (budget > 0 && (!sample_types || !sample_idx)) throw std::invalid_argument("null sample_types or sample_idx");
    const ResidentPairs &R = *set->R;
    const int share = point_share < 0 ? draw_default_share(set->cfg.solver_type) : point_share;
    std::vector<int64_t> soff;
    std::vector<int32_t> types;
    draw_plan(R, sel, budget, seed, share, soff, types);
    for (int j = 0; j < num_sel; ++j) sample_counts[j] = (int32_t)(soff[(size_t)j + 1] - soff[(size_t)j]);
    const int64_t S = soff[(size_t)num_sel];
    if (S == 0) return;
    CtxLease lease(set->device);
    hipStream_t stream = lease.c->stream;
    HypDraw dr{seed, share, set->pair_sizes(stream)};
    bind_weights(dr, weights);
    const std::vector<HypSlab> slabs = hyp_slabs(S, 0);
    const size_t cap = (size_t)(slabs[0].s1 - slabs[0].s0);
    DevArray<DrawItem> d_items(cap);
    DevArray<int> d_samples(cap * kSampleStride), d_types(cap);
    std::vector<DrawItem> h_items;
    for (const HypSlab &s : slabs) {
        const size_t ns = (size_t)(s.s1 - s.s0);
        draw_slab(stream, R.v, sel, soff.data(), s, dr, h_items, d_items.p, d_samples.p, d_types.p);
        MP_HIP(hipMemcpyAsync(sample_idx + kSampleStride * s.s0, d_samples.p, sizeof(int) * kSampleStride * ns,
                              hipMemcpyDeviceToHost, stream));
        MP_HIP(hipMemcpyAsync(sample_types + s.s0, d_types.p, sizeof(int) * ns, hipMemcpyDeviceToHost, stream));
        MP_HIP(hipStreamSynchronize(stream));
    }
    // (the planning of mp_ransac_set rests on the host's types being the device's)
    if (std::memcmp(sample_types, types.data(), sizeof(int32_t) * (size_t)S) != 0)
        throw std::runtime_error("draw: the device's sample types are not the host's");
}

void draw_host(int variant, int64_t n, uint64_t seed, int32_t point_share, int32_t pair, int32_t s, int32_t *out) {
    if (variant < 0 || variant > 2) throw std::invalid_argument("variant must be 0, 1 or 2");
    if (n < 0 || n > kRefinePairMax) throw std::invalid_argument("n out of range");
    if (point_share < 0 || point_share > kDrawShareMax) throw std::invalid_argument("point_share must be in 0..256");
    if (pair < 0 || s < 0 || !out) throw std::invalid_argument("negative pair or sample, or null output");
    int idx[8];
    bool fill = false;
    out[0] = draw_sample(n, draw_k_md(variant), draw_k_pt(variant), seed, point_share, (uint32_t)pair, (uint32_t)s, idx,
                         &fill);
    for (int a = 0; a < 8; ++a) out[1 + a] = idx[a];
    out[9] = fill ? 1 : 0;
}

int64_t candidates_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, const int64_t *sample_offsets,
                       const int32_t *sample_types, const int32_t *sample_idx, int64_t sample_chunk) {
    if (!set) throw std::invalid_argument("null pair set");
    if (sample_chunk < 0) throw std::invalid_argument("sample_chunk must not be negative");
    std::lock_guard<std::mutex> lk(set->mu);
    check_hyp_supported(set->variant, set->opts, set->cfg);
    set->cand.reset();
    if (set->num_pairs == 0) {
        std::vector<char> seen;
        check_selection(0, num_sel, pair_ids, seen);
        set->cand.reset(new HypCompact());
        set->cand->plan.moff.assign(1, 0);
        return 0;
    }
    const PairSel sel = set->select(num_sel, pair_ids);
    std::unique_ptr<HypCompact> co(new HypCompact());
    static const int64_t kNone[1] = {0};
    if (num_sel == 0) {
        co->plan.begin(0, kNone, max_models(set->R->v));
        co->plan.finish();
    } else {
        const ResidentPairs &R = *set->R;
        const int64_t S = check_set_samples(R, sel, sample_offsets, sample_types, sample_idx);
        if (S == 0) {
            co->plan.begin(num_sel, sample_offsets, max_models(R.v));
            co->plan.finish();
        } else {
            const bool timed = g_prof_on.load();
            HypTiming tm;
            std::vector<int32_t> counts((size_t)sample_offsets[num_sel]);
            CtxLease lease(set->device);
            HypBuffers B(R.v, S, sample_chunk, true, false);
            hypothesize_run(*set->R, lease.c->stream, sel, sample_offsets, sample_types, sample_idx, nullptr,
                            counts.data(), sample_chunk, B, timed, tm, nullptr, co.get());
            if (timed) {
                std::lock_guard<std::mutex> lk2(g_hyp_mu);
                g_hyp_timing = tm;
            }
        }
        co->plan.soff = nullptr; // (the caller's array: not read again)
    }
    set->cand = std::move(co);
    return (int64_t)set->cand->models.size();
}

void candidates_fetch(PairSet *set, Model *models, int64_t *model_offsets, int32_t *cand_sample, int32_t *cand_slot) {
    if (!set) throw std::invalid_argument("null pair set");
    std::lock_guard<std::mutex> lk(set->mu);
    if (!set->cand) throw std::invalid_argument("no candidates to fetch: call mp_candidates_set first");
    const HypCompact &co = *set->cand;
    const size_t M = co.models.size();
    if (!model_offsets) throw std::invalid_argument("null model_offsets");
    if (M > 0 && (!models || !cand_sample || !cand_slot))
        throw std::invalid_argument("null models, cand_sample or cand_slot");
    std::copy(co.plan.moff.begin(), co.plan.moff.end(), model_offsets);
    if (M > 0) {
        std::memcpy(models, co.models.data(), sizeof(Model) * M);
        std::copy(co.plan.sample.begin(), co.plan.sample.end(), cand_sample);
        std::copy(co.plan.slot.begin(), co.plan.slot.end(), cand_slot);
    }
    set->cand.reset();
}

void ransac_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, uint64_t seed,
                int32_t point_share, const int64_t *sample_offsets, const int32_t *sample_types,
                const int32_t *sample_idx, int32_t rounds, Model *models, RansacResult *results, int32_t *inlier_idx,
                int64_t sample_chunk, int64_t model_chunk, const DrawWeights *weights, const RansacOut *out) {
    if (!set) throw std::invalid_argument("null pair set");
    RansacOutStage stage(out);
    stage.check_args(rounds, 0);
    if (rounds < 0 || rounds > 64) throw std::invalid_argument("rounds must be in 0..64");
    if (sample_chunk < 0) throw std::invalid_argument("sample_chunk must not be negative");
    if (model_chunk < 0) throw std::invalid_argument("model_chunk must not be negative");
    const bool given = sample_offsets != nullptr;
    if (given && budget != -1) throw std::invalid_argument("either samples or a budget: with samples, budget must be -1");
    if (!given && (sample_types || sample_idx))
        throw std::invalid_argument("sample_types / sample_idx without sample_offsets");
    if (!given) check_draw_args(num_sel, budget, point_share);
    if (given && weights) throw std::invalid_argument("draw weights with given samples: nothing is drawn");
    std::lock_guard<std::mutex> lk(set->mu);
    if (weights) check_draw_weights(set, weights);
    check_hyp_supported(set->variant, set->opts, set->cfg);
    if (set->num_pairs == 0) {
        std::vector<char> seen;
        check_selection(0, num_sel, pair_ids, seen);
        return;
    }
    const PairSel sel = set->select(num_sel, pair_ids);
    if (num_sel == 0) return;
    if (!models || !results) throw std::invalid_argument("null models or results");
    ResidentPairs &R = *set->R;
    const int v = R.v;
    std::vector<int64_t> soff_drawn;
    std::vector<int32_t> types_drawn;
    const int64_t *soff = sample_offsets;
    const int32_t *types = sample_types;
    int share = 0;
    const bool timed = g_prof_on.load();
    RansacTiming rt;
    Clock::time_point t_all = Clock::now();
    if (given) {
        check_set_samples(R, sel, sample_offsets, sample_types, sample_idx);
    } else {
        share = point_share < 0 ? draw_default_share(set->cfg.solver_type) : point_share;
        draw_plan(R, sel, budget, seed, share, soff_drawn, types_drawn);
        soff = soff_drawn.data();
        types = types_drawn.data();
    }
    rt.samples_ms = 1e3 * secs(t_all);
    const int64_t S = soff[num_sel] - soff[0];
    CtxLease lease(set->device);
    hipStream_t stream = lease.c->stream;
    stage.begin(set, num_sel, stream);

    // ---- draw -> hypothesize -> compact ----
    HypCompact co;
    std::vector<int32_t> counts((size_t)soff[num_sel]);
    Clock::time_point t0 = Clock::now();
    if (S > 0) {
        HypDraw dr{seed, share, nullptr};
        if (!given) dr.d_pair_n = set->pair_sizes(stream);
        if (!given) bind_weights(dr, weights);
        HypBuffers B(v, S, sample_chunk, true, !given);
        hypothesize_run(R, stream, sel, soff, types, given ? sample_idx : nullptr, nullptr, counts.data(), sample_chunk,
                        B, timed, rt.hyp, given ? nullptr : &dr, &co);
    } else {
        co.plan.begin(num_sel, soff, max_models(v));
        co.plan.finish();
    }
    rt.hypothesize_ms = 1e3 * secs(t0);
    rt.bytes_back = co.bytes_back;
    rt.bytes_slots = co.bytes_slots;
    const CandPlan &cp = co.plan;

    // ---- select ----
    t0 = Clock::now();
    std::vector<SelectResult> sres((size_t)num_sel);
    const int tile_set = g_select_tile.load();
    // (mp_ransac_out_set, out not null: with a refinement to come the winners' lists are refine_run's)
    select_run(R, stream, sel, set->out_off.data(), cp.moff.data(), co.models.data(), nullptr, nullptr, sres.data(),
               out && rounds >= 1 ? nullptr : inlier_idx, model_chunk, tile_set ? tile_set : kSelectTile, timed,
               rt.select);
    rt.select_ms = 1e3 * secs(t0);
    for (int j = 0; j < num_sel; ++j) {
        RansacResult &Q = results[j];
        std::memset(&Q, 0, sizeof(Q));
        std::memset(&models[j], 0, sizeof(Model));
        const SelectResult &B = sres[(size_t)j];
        Q.num_samples = (int32_t)(soff[j + 1] - soff[j]);
        Q.num_candidates = (int32_t)(cp.moff[(size_t)j + 1] - cp.moff[(size_t)j]);
        Q.best_candidate = B.best_index;
        Q.best_sample = Q.best_slot = Q.best_type = -1;
        Q.score_selected = Q.score_initial = Q.score_final = B.best_score;
        Q.norm_scale = B.norm_scale;
        Q.lm_status = -1;
        for (int t = 0; t < 3; ++t) Q.num_inliers[t] = B.num_inliers[t];
        if (B.best_index < 0) continue;
        cand_origin(cp, j, B.best_index, &Q.best_sample, &Q.best_slot);
        Q.best_type = types[soff[j] + Q.best_sample];
        models[j] = co.models[(size_t)(cp.moff[(size_t)j] + B.best_index)];
    }

    // ---- refine: the pairs with a winner, their lists to their places in the selection ----
    t0 = Clock::now();
    refine_winners(set, stream, sel, rounds, models, results, inlier_idx, stage.swept());
    rt.refine_ms = 1e3 * secs(t0);
    stage.finish(set, sel, stream, models, results);
    rt.total_ms = 1e3 * secs(t_all);
    if (timed) {
        std::lock_guard<std::mutex> lk2(g_ransac_mu);
        g_ransac_timing = rt;
    }
}

void ransac_required(int variant, int64_t n, const int32_t *counts, const RansacOptions &opts, uint32_t *req) {
    if (variant < 0 || variant > 2) throw std::invalid_argument("variant must be 0, 1 or 2");
    if (n < 0 || n > kRefinePairMax) throw std::invalid_argument("n out of range");
    if (!counts || !req) throw std::invalid_argument("null counts or output");
    for (int t = 0; t < 3; ++t)
        if (counts[t] < 0 || counts[t] > n) throw std::invalid_argument("counts must be in 0..n");
    const StopOptions so{opts.success_probability, opts.min_num_iterations, opts.max_num_iterations_per_solver};
    for (int s = 0; s < 2; ++s) req[s] = required_samples(s, draw_k_md(variant), draw_k_pt(variant), n, counts, so);
}

void select_argmin_direct(int32_t num_pairs, const int64_t *model_offsets, const double *scores, const double *prior,
                          int32_t *index, double *score, int device) {
    if (num_pairs < 0) throw std::invalid_argument("negative pair count");
    if (num_pairs == 0) return;
    if (!model_offsets || !index || !score) throw std::invalid_argument("null model_offsets, index or score");
    if (model_offsets[0] != 0) throw std::invalid_argument("model_offsets must start at 0");
    for (int32_t p = 0; p < num_pairs; ++p)
        if (model_offsets[p + 1] < model_offsets[p]) throw std::invalid_argument("offsets must not decrease");
    const int64_t M = model_offsets[num_pairs];
    if (M > kSelectModelsMax) throw std::invalid_argument("more than 2^28 candidates");
    if (M > 0 && !scores) throw std::invalid_argument("null scores");
    CtxLease lease(device);
    hipStream_t stream = lease.c->stream;
    DevArray<int64_t> d_moff((size_t)num_pairs + 1);
    DevArray<double> d_scores((size_t)std::max<int64_t>(M, 1)), d_prior((size_t)num_pairs);
    DevArray<SelectBest> d_best((size_t)num_pairs);
    std::vector<SelectBest> best((size_t)num_pairs);
    MP_HIP(hipMemcpyAsync(d_moff.p, model_offsets, sizeof(int64_t) * ((size_t)num_pairs + 1), hipMemcpyHostToDevice,
                          stream));
    if (M > 0) MP_HIP(hipMemcpyAsync(d_scores.p, scores, sizeof(double) * (size_t)M, hipMemcpyHostToDevice, stream));
    if (prior) {
        MP_HIP(hipMemcpyAsync(d_prior.p, prior, sizeof(double) * (size_t)num_pairs, hipMemcpyHostToDevice, stream));
        MP_HIP(launch_select_argmin_seeded(stream, d_moff.p, num_pairs, d_scores.p, d_prior.p, d_best.p));
    } else {
        MP_HIP(launch_select_argmin(stream, d_moff.p, num_pairs, d_scores.p, d_best.p));
    }
    MP_HIP(hipMemcpyAsync(best.data(), d_best.p, sizeof(SelectBest) * (size_t)num_pairs, hipMemcpyDeviceToHost, stream));
    MP_HIP(hipStreamSynchronize(stream));
    for (int32_t p = 0; p < num_pairs; ++p) {
        if (best[(size_t)p].index >= model_offsets[p + 1] - model_offsets[p])
            throw std::runtime_error("select_argmin: index out of range");
        index[p] = best[(size_t)p].index;
        score[p] = best[(size_t)p].score;
    }
}

void ransac_adaptive_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                         uint64_t seed, int32_t point_share, int32_t rounds, Model *models, RansacResult *results,
                         int32_t *inlier_idx, int32_t *stopped, int64_t sample_chunk, int64_t model_chunk,
                         const DrawWeights *weights, bool weighted_stop, InlierMass *rule_mass,
                         const RansacOut *out) {
    if (!set) throw std::invalid_argument("null pair set");
    RansacOutStage stage(out);
    stage.check_args(rounds, 0);
    if (weighted_stop && !weights) throw std::invalid_argument("weighted_stop needs draw weights");
    if (rounds < 0 || rounds > 64) throw std::invalid_argument("rounds must be in 0..64");
    if (sample_chunk < 0) throw std::invalid_argument("sample_chunk must not be negative");
    if (model_chunk < 0) throw std::invalid_argument("model_chunk must not be negative");
    if (step < 1) throw std::invalid_argument("step must be at least 1");
    if (budget < 0 || budget > kAdaptiveBudgetMax) throw std::invalid_argument("budget must be in 0..2^20");
    // (a round obeys the bound a fixed-budget call obeys)
    check_draw_args(num_sel, std::min(step, budget), point_share);
    std::lock_guard<std::mutex> lk(set->mu);
    if (weights) check_draw_weights(set, weights);
    check_hyp_supported(set->variant, set->opts, set->cfg);
    if (set->num_pairs == 0) {
        std::vector<char> seen;
        check_selection(0, num_sel, pair_ids, seen);
        return;
    }
    const PairSel sel = set->select(num_sel, pair_ids);
    if (num_sel == 0) return;
    if (!models || !results) throw std::invalid_argument("null models or results");
    ResidentPairs &R = *set->R;
    const int v = R.v, kmd = draw_k_md(v), kpt = draw_k_pt(v);
    const int share = point_share < 0 ? draw_default_share(set->cfg.solver_type) : point_share;
    const StopOptions so{set->opts.success_probability, set->opts.min_num_iterations,
                         set->opts.max_num_iterations_per_solver};
    const int tile_set = g_select_tile.load();
    const int tile = tile_set ? tile_set : kSelectTile;

    // per entry: the running best in results / models; the samples had so far are
    // results[j].num_samples, the candidates num_candidates, the samples per type drawn[2 j + s]
    std::vector<int64_t> drawn(2 * (size_t)num_sel, 0);
    std::vector<int> active; // the entries still sampling, in selection order
    for (int j = 0; j < num_sel; ++j) {
        RansacResult &Q = results[j];
        std::memset(&Q, 0, sizeof(Q));
        std::memset(&models[j], 0, sizeof(Model));
        Q.best_candidate = Q.best_sample = Q.best_slot = Q.best_type = -1;
        Q.score_selected = Q.score_initial = Q.score_final = DBL_MAX;
        Q.norm_scale = R.norm_scale[sel[j]];
        Q.lm_status = -1;
        if (stopped) stopped[j] = 0;
        if (R.n[sel[j]] >= kmd && budget > 0) active.push_back(j);
    }
    CtxLease lease(set->device);
    hipStream_t stream = lease.c->stream;
    stage.begin(set, num_sel, stream);
    RuleMass rule; // (weighted_stop: what the rule reads, host/ransac_stop.h required_samples_mass)
    if (weighted_stop) rule.init(R, sel, weights);
    if (!active.empty()) {
        // (the first round is the largest: its buffers serve every round)
        HypBuffers B(v, (int64_t)active.size() * std::min(step, budget), sample_chunk, true, true);
        HypDraw dr{seed, share, set->pair_sizes(stream), nullptr};
        bind_weights(dr, weights);
        HypTiming htm;
        SelectTiming stm;
        std::vector<int32_t> ids, first, count, types, counts;
        std::vector<int64_t> out_off, soff;
        std::vector<double> prior;
        std::vector<SelectResult> sres;
        std::vector<int> next;
        while (!active.empty()) {
            const int na = (int)active.size();
            ids.resize((size_t)na);
            first.resize((size_t)na);
            count.resize((size_t)na);
            out_off.resize((size_t)na);
            prior.resize((size_t)na);
            sres.resize((size_t)na);
            for (int a = 0; a < na; ++a) {
                const int j = active[(size_t)a];
                ids[(size_t)a] = sel[j];
                first[(size_t)a] = results[j].num_samples;
                count[(size_t)a] = round_count(results[j].num_samples, step, budget);
                out_off[(size_t)a] = set->out_off[(size_t)j];
                prior[(size_t)a] = results[j].score_selected;
            }
            const PairSel asel{na, ids.data()};
            draw_plan(R, asel, first.data(), count.data(), seed, share, soff, types);
            const int64_t S = soff[(size_t)na];
            if (S <= 0 || S > kHypSamplesMax) throw std::logic_error("ransac_adaptive: a round without samples");
            counts.assign((size_t)S, 0);
            // ---- draw -> hypothesize -> compact -> select, the walk continued from the prior ----
            HypCompact co;
            dr.first = first.data();
            hypothesize_run(R, stream, asel, soff.data(), types.data(), nullptr, nullptr, counts.data(), sample_chunk, B,
                            false, htm, &dr, &co);
            const CandPlan &cp = co.plan;
            // (with a refinement to come the winners' lists are refine_run's: the rounds copy none)
            select_run(R, stream, asel, out_off.data(), cp.moff.data(), co.models.data(), nullptr, nullptr, sres.data(),
                       rounds >= 1 ? nullptr : inlier_idx, model_chunk, tile, false, stm, prior.data());
            next.clear();
            for (int a = 0; a < na; ++a) {
                const int j = active[(size_t)a];
                RansacResult &Q = results[j];
                const SelectResult &W = sres[(size_t)a];
                const int32_t *t = types.data() + soff[(size_t)a];
                for (int32_t s = 0; s < count[(size_t)a]; ++s) ++drawn[2 * (size_t)j + (t[s] != 0 ? 1 : 0)];
                if (W.best_index >= 0) { // strictly below the running best: it replaces it
                    int32_t sample = -1, slot = -1;
                    cand_origin(cp, a, W.best_index, &sample, &slot);
                    Q.best_candidate = Q.num_candidates + W.best_index;
                    Q.best_sample = first[(size_t)a] + sample;
                    Q.best_slot = slot;
                    Q.best_type = t[sample];
                    Q.score_selected = Q.score_initial = Q.score_final = W.best_score;
                    for (int k = 0; k < 3; ++k) Q.num_inliers[k] = W.num_inliers[k];
                    models[j] = co.models[(size_t)(cp.moff[(size_t)a] + W.best_index)];
                    if (weighted_stop) rule.dirty[(size_t)j] = 1;
                }
                Q.num_samples += count[(size_t)a];
                Q.num_candidates += (int32_t)(cp.moff[(size_t)a + 1] - cp.moff[(size_t)a]);
            }
            // ---- weighted_stop: one mass_run over the entries whose running best was replaced ----
            if (weighted_stop)
                rule.update(R, stream, weights, sel, active, models, [&](int j) { return results[j].num_inliers; });
            // ---- the rule, on the running best's counts (weighted_stop: its masses) ----
            for (int a = 0; a < na; ++a) {
                const int j = active[(size_t)a];
                RansacResult &Q = results[j];
                uint32_t req[2];
                if (weighted_stop)
                    rule.required(j, kmd, kpt, R.n[sel[j]], Q.best_candidate >= 0, Q.num_inliers, so, req);
                else
                    for (int s = 0; s < 2; ++s)
                        req[s] = required_samples(s, kmd, kpt, R.n[sel[j]],
                                                  Q.best_candidate >= 0 ? Q.num_inliers : nullptr, so);
                if (stop_reached(req, &drawn[2 * (size_t)j])) {
                    if (stopped) stopped[j] = 1;
                } else if (Q.num_samples < budget) {
                    next.push_back(j);
                }
            }
            active.swap(next);
        }
    }
    if (weighted_stop && rule_mass) std::copy(rule.rm.begin(), rule.rm.end(), rule_mass);
    // ---- refine: once, the pairs with a winner ----
    refine_winners(set, stream, sel, rounds, models, results, inlier_idx, stage.swept());
    stage.finish(set, sel, stream, models, results);
}

namespace {
// ransac_lo_set (lo_steps = 0: its launches and its bytes) and ransac_lo_steps_set
void ransac_lo_run(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step, uint64_t seed,
                   int32_t point_share, int32_t rounds, int32_t lo_rounds, Model *models, RansacResult *results,
                   int32_t *inlier_idx, int32_t *stopped, RansacLoInfo *lo_info, int64_t sample_chunk,
                   int64_t model_chunk, int32_t lo_steps, RansacLoStepsInfo *steps_info, const DrawWeights *weights,
                   bool weighted_stop, InlierMass *rule_mass, const RansacOut *out) {
    if (!set) throw std::invalid_argument("null pair set");
    RansacOutStage stage(out);
    stage.check_args(rounds, 1);
    if (weighted_stop && !weights) throw std::invalid_argument("weighted_stop needs draw weights");
    if (rounds < 0 || rounds > 64) throw std::invalid_argument("rounds must be in 0..64");
    if (lo_rounds < 1 || lo_rounds > 64) throw std::invalid_argument("lo_rounds must be in 1..64");
    if (num_sel > 0 && !lo_info) throw std::invalid_argument("null lo_info");
    if (sample_chunk < 0) throw std::invalid_argument("sample_chunk must not be negative");
    if (model_chunk < 0) throw std::invalid_argument("model_chunk must not be negative");
    if (step < 1) throw std::invalid_argument("step must be at least 1");
    if (budget < 0 || budget > kAdaptiveBudgetMax) throw std::invalid_argument("budget must be in 0..2^20");
    // (a round obeys the bound a fixed-budget call obeys)
    check_draw_args(num_sel, std::min(step, budget), point_share);
    std::lock_guard<std::mutex> lk(set->mu);
    if (weights) check_draw_weights(set, weights);
    check_hyp_supported(set->variant, set->opts, set->cfg);
    if (set->num_pairs == 0) {
        std::vector<char> seen;
        check_selection(0, num_sel, pair_ids, seen);
        return;
    }
    const PairSel sel = set->select(num_sel, pair_ids);
    if (num_sel == 0) return;
    if (!models || !results) throw std::invalid_argument("null models or results");
    ResidentPairs &R = *set->R;
    const int v = R.v, kmd = draw_k_md(v), kpt = draw_k_pt(v);
    const int share = point_share < 0 ? draw_default_share(set->cfg.solver_type) : point_share;
    const StopOptions so{set->opts.success_probability, set->opts.min_num_iterations,
                         set->opts.max_num_iterations_per_solver};
    const int tile_set = g_select_tile.load();
    const int tile = tile_set ? tile_set : kSelectTile;

    // per entry, the minimal track: results[j] and minimal[j], as ransac_adaptive_set keeps
    // them; the overall best: track[j] (host/ransac_lo_track.h) and models[j] (user units)
    std::vector<Model> minimal((size_t)num_sel);
    std::vector<LoTrack> track((size_t)num_sel);
    std::vector<LoStepTrack> strack((size_t)num_sel); // (lo_steps > 0: what the steps gave)
    std::vector<int64_t> drawn(2 * (size_t)num_sel, 0);
    std::vector<int> active; // the entries still sampling, in selection order
    for (int j = 0; j < num_sel; ++j) {
        RansacResult &Q = results[j];
        std::memset(&Q, 0, sizeof(Q));
        std::memset(&models[j], 0, sizeof(Model));
        std::memset(&minimal[(size_t)j], 0, sizeof(Model));
        Q.best_candidate = Q.best_sample = Q.best_slot = Q.best_type = -1;
        Q.score_selected = Q.score_initial = Q.score_final = DBL_MAX;
        Q.norm_scale = R.norm_scale[sel[j]];
        Q.lm_status = -1;
        if (stopped) stopped[j] = 0;
        if (R.n[sel[j]] >= kmd && budget > 0) active.push_back(j);
    }
    CtxLease lease(set->device);
    hipStream_t stream = lease.c->stream;
    stage.begin(set, num_sel, stream);
    RuleMass rule; // (weighted_stop: what the rule reads, host/ransac_stop.h required_samples_mass)
    if (weighted_stop) rule.init(R, sel, weights);
    if (!active.empty()) {
        // (the first round is the largest: its buffers serve every round)
        HypBuffers B(v, (int64_t)active.size() * std::min(step, budget), sample_chunk, true, true);
        HypDraw dr{seed, share, set->pair_sizes(stream), nullptr};
        bind_weights(dr, weights);
        RefineBuffers lo_bufs(active.size(), true);
        R.lists(2); // (select takes one buffer, the LO both: no regrowth between the rounds)
        // With rounds = 0 the overall best's lists are the result's.  Both stages write their
        // lists to `lists` (the selection's layout); an entry's are copied to inlier_idx only
        // when its model becomes the overall best, so neither track writes over the other's.
        const bool keep_lists = rounds == 0 && inlier_idx && set->out_off[(size_t)num_sel] > 0;
        std::vector<int32_t> lists(keep_lists ? 3 * (size_t)set->out_off[(size_t)num_sel] : 0);
        auto take_lists = [&](int j, const int32_t *counts) {
            if (!keep_lists) return;
            const int64_t n = R.n[sel[j]], at = 3 * set->out_off[(size_t)j];
            for (int t = 0; t < 3; ++t)
                std::memcpy(inlier_idx + at + t * n, lists.data() + at + t * n, sizeof(int32_t) * (size_t)counts[t]);
        };
        HypTiming htm;
        SelectTiming stm;
        std::vector<int32_t> ids, first, count, types, counts, lo_ids;
        std::vector<int64_t> out_off, soff, lo_off;
        std::vector<double> prior;
        std::vector<SelectResult> sres;
        std::vector<int> next, lo_j;
        std::vector<Model> lo_models;
        std::vector<RefineResult> lo_res;
        // the steps: the live steps' entry (index into lo_j), step and current model, a stage's
        // arguments and results, and the finals' select
        LsqBuffers lsq_bufs;
        std::vector<int> st_i, st_r, fin_first;
        std::vector<Model> st_m, st_in;
        std::vector<int32_t> st_ids, st_types, st_streams, st_sub, fin_ids;
        std::vector<double> st_fac;
        std::vector<LsqFitResult> st_res;
        std::vector<int64_t> fin_off, fin_moff;
        std::vector<SelectResult> fin_res;
        while (!active.empty()) {
            const int na = (int)active.size();
            ids.resize((size_t)na);
            first.resize((size_t)na);
            count.resize((size_t)na);
            out_off.resize((size_t)na);
            prior.resize((size_t)na);
            sres.resize((size_t)na);
            for (int a = 0; a < na; ++a) {
                const int j = active[(size_t)a];
                ids[(size_t)a] = sel[j];
                first[(size_t)a] = results[j].num_samples;
                count[(size_t)a] = round_count(results[j].num_samples, step, budget);
                out_off[(size_t)a] = set->out_off[(size_t)j];
                prior[(size_t)a] = results[j].score_selected; // (the minimal best's: the walk is the adaptive entry's)
            }
            const PairSel asel{na, ids.data()};
            draw_plan(R, asel, first.data(), count.data(), seed, share, soff, types);
            const int64_t S = soff[(size_t)na];
            if (S <= 0 || S > kHypSamplesMax) throw std::logic_error("ransac_lo: a round without samples");
            counts.assign((size_t)S, 0);
            // ---- draw -> hypothesize -> compact -> select, the walk continued from the prior ----
            HypCompact co;
            dr.first = first.data();
            hypothesize_run(R, stream, asel, soff.data(), types.data(), nullptr, nullptr, counts.data(), sample_chunk, B,
                            false, htm, &dr, &co);
            const CandPlan &cp = co.plan;
            select_run(R, stream, asel, out_off.data(), cp.moff.data(), co.models.data(), nullptr, nullptr, sres.data(),
                       keep_lists ? lists.data() : nullptr, model_chunk, tile, false, stm, prior.data());
            // ---- the minimal track, and step 1 for the entries whose minimal best was replaced ----
            lo_j.clear();
            lo_ids.clear();
            lo_off.clear();
            lo_models.clear();
            for (int a = 0; a < na; ++a) {
                const int j = active[(size_t)a];
                RansacResult &Q = results[j];
                const SelectResult &W = sres[(size_t)a];
                const int32_t *t = types.data() + soff[(size_t)a];
                for (int32_t s = 0; s < count[(size_t)a]; ++s) ++drawn[2 * (size_t)j + (t[s] != 0 ? 1 : 0)];
                if (W.best_index >= 0) { // strictly below the minimal best: it replaces it
                    int32_t sample = -1, slot = -1;
                    cand_origin(cp, a, W.best_index, &sample, &slot);
                    Q.best_candidate = Q.num_candidates + W.best_index;
                    Q.best_sample = first[(size_t)a] + sample;
                    Q.best_slot = slot;
                    Q.best_type = t[sample];
                    Q.score_selected = W.best_score;
                    minimal[(size_t)j] = co.models[(size_t)(cp.moff[(size_t)a] + W.best_index)];
                    if (lo_take_minimal(track[(size_t)j], W.best_score, W.num_inliers)) {
                        lo_step_clear(strack[(size_t)j]);
                        models[j] = minimal[(size_t)j];
                        take_lists(j, W.num_inliers);
                        if (weighted_stop) rule.dirty[(size_t)j] = 1;
                    }
                    lo_j.push_back(j);
                    lo_ids.push_back(sel[j]);
                    lo_off.push_back(set->out_off[(size_t)j]);
                    lo_models.push_back(minimal[(size_t)j]);
                }
                Q.num_samples += count[(size_t)a];
                Q.num_candidates += (int32_t)(cp.moff[(size_t)a + 1] - cp.moff[(size_t)a]);
            }
            // ---- step 2: one relaxed refinement over the new minimal bests ----
            if (!lo_j.empty()) {
                const int nl = (int)lo_j.size();
                lo_res.resize((size_t)nl);
                refine_run(R, stream, PairSel{nl, lo_ids.data()}, lo_off.data(), set->cfg, lo_rounds, lo_models.data(),
                           lo_res.data(), keep_lists ? lists.data() : nullptr, true, set->opts.threshold_multiplier,
                           &lo_bufs);
                for (int i = 0; i < nl; ++i) {
                    const int j = lo_j[(size_t)i];
                    const RefineResult &F = lo_res[(size_t)i];
                    if (lo_take_refined(track[(size_t)j], results[j].best_candidate, F.rounds_accepted, F.score_final,
                                        F.num_inliers)) {
                        lo_step_clear(strack[(size_t)j]);
                        models[j] = lo_models[(size_t)i];
                        take_lists(j, F.num_inliers);
                        if (weighted_stop) rule.dirty[(size_t)j] = 1;
                    }
                }
                // ---- the LO steps (host/ransac_lo_steps.h): every step of every such entry goes
                // through each stage in one lsq_fit_run, then one select over the finals ----
                if (lo_steps > 0) {
                    const int Q = set->opts.num_lsq_iterations;
                    const double lambda = set->opts.threshold_multiplier;
                    // the live steps, entry-major in step order: (i, r) and the step's current model
                    st_i.clear(), st_r.clear(), st_m.clear();
                    for (int i = 0; i < nl; ++i)
                        for (int r = 0; r < lo_steps; ++r) {
                            st_i.push_back(i);
                            st_r.push_back(r);
                            st_m.push_back(lo_models[(size_t)i]); // (a: what the relaxed refinement returned)
                        }
                    for (int q = 0; q <= 1 + Q && !st_i.empty(); ++q) {
                        const size_t m = st_i.size();
                        st_ids.resize(m), st_types.resize(m), st_streams.resize(m), st_sub.resize(m);
                        st_res.resize(m);
                        st_fac.assign(m, q < 2 ? 1.0 : lo_step_factor(q - 2, Q, lambda));
                        st_in = st_m;
                        for (size_t e = 0; e < m; ++e) {
                            const int j = lo_j[(size_t)st_i[e]];
                            st_ids[e] = sel[j];
                            st_types[e] = results[j].best_type;
                            st_streams[e] = results[j].best_candidate;
                            st_sub[e] = lo_step_substream(st_r[e], q);
                        }
                        lsq_fit_run(R, stream, set->opts, set->cfg, (int32_t)m, st_ids.data(), st_types.data(),
                                    st_fac.data(), q == 0 ? kSubsetNonmin : kSubsetLsq, seed, st_streams.data(),
                                    st_sub.data(), st_m.data(), st_res.data(), nullptr, nullptr, 0, lsq_bufs);
                        if (q == 0) { // a step whose non-minimal fit gave no model ends and offers nothing
                            size_t w = 0;
                            for (size_t e = 0; e < m; ++e) {
                                if (st_res[e].status != 1) continue;
                                st_i[w] = st_i[e], st_r[w] = st_r[e], st_m[w] = st_m[e];
                                ++w;
                            }
                            st_i.resize(w), st_r.resize(w), st_m.resize(w);
                            continue;
                        }
                        // the stage scored its input, the model stage q - 1 produced: offered in step order
                        for (size_t e = 0; e < m; ++e) {
                            const int j = lo_j[(size_t)st_i[e]];
                            if (lo_step_offer(track[(size_t)j], strack[(size_t)j], results[j].best_candidate, st_r[e],
                                              q - 1, st_res[e].score, st_res[e].num_inliers)) {
                                models[j] = st_in[e];
                                if (weighted_stop) rule.dirty[(size_t)j] = 1;
                            }
                        }
                    }
                    // the finals: one select over each entry's live steps' last models, in step order
                    if (!st_i.empty()) {
                        fin_ids.clear(), fin_off.clear(), fin_first.clear();
                        fin_moff.assign(1, 0);
                        for (size_t e = 0; e < st_i.size(); ++e) {
                            if (e == 0 || st_i[e] != st_i[e - 1]) {
                                const int j = lo_j[(size_t)st_i[e]];
                                fin_ids.push_back(sel[j]);
                                fin_off.push_back(set->out_off[(size_t)j]);
                                fin_first.push_back((int)e);
                                fin_moff.push_back(fin_moff.back());
                            }
                            ++fin_moff.back();
                        }
                        const int nf = (int)fin_ids.size();
                        fin_res.resize((size_t)nf);
                        select_run(R, stream, PairSel{nf, fin_ids.data()}, fin_off.data(), fin_moff.data(),
                                   st_m.data(), nullptr, nullptr, fin_res.data(), nullptr, model_chunk, tile, false,
                                   stm);
                        for (int f = 0; f < nf; ++f) {
                            const SelectResult &W = fin_res[(size_t)f];
                            if (W.best_index < 0) continue;
                            const size_t e = (size_t)fin_first[(size_t)f] + (size_t)W.best_index;
                            const int j = lo_j[(size_t)st_i[e]];
                            if (lo_step_offer(track[(size_t)j], strack[(size_t)j], results[j].best_candidate, st_r[e],
                                              2 + Q, W.best_score, W.num_inliers)) {
                                models[j] = st_m[e];
                                if (weighted_stop) rule.dirty[(size_t)j] = 1;
                            }
                        }
                    }
                }
            }
            // ---- weighted_stop: one mass_run over the entries whose overall best was replaced
            // during this checkpoint, on the overall best as it stands at its end ----
            if (weighted_stop)
                rule.update(R, stream, weights, sel, active, models, [&](int j) { return track[(size_t)j].counts; });
            // ---- the rule, on the overall best's counts (weighted_stop: its masses) ----
            next.clear();
            for (int a = 0; a < na; ++a) {
                const int j = active[(size_t)a];
                const LoTrack &K = track[(size_t)j];
                uint32_t req[2];
                if (weighted_stop)
                    rule.required(j, kmd, kpt, R.n[sel[j]], K.source != 0, K.counts, so, req);
                else
                    for (int s = 0; s < 2; ++s)
                        req[s] = required_samples(s, kmd, kpt, R.n[sel[j]], K.source != 0 ? K.counts : nullptr, so);
                if (stop_reached(req, &drawn[2 * (size_t)j])) {
                    if (stopped) stopped[j] = 1;
                } else if (results[j].num_samples < budget) {
                    next.push_back(j);
                }
            }
            active.swap(next);
        }
    }
    for (int j = 0; j < num_sel; ++j) {
        RansacResult &Q = results[j];
        const LoTrack &K = track[(size_t)j];
        if (K.source != 0) Q.score_initial = Q.score_final = K.score;
        for (int t = 0; t < 3; ++t) Q.num_inliers[t] = K.counts[t];
        lo_info[j] = RansacLoInfo{K.lo_runs, K.lo_accepted, K.lo_index, 0};
        if (weighted_stop && rule_mass) rule_mass[j] = rule.rm[(size_t)j];
        if (steps_info) {
            const LoStepTrack &S = strack[(size_t)j];
            steps_info[j] = RansacLoStepsInfo{S.lo_step, S.lo_stage, S.offers, S.accepted};
        }
    }
    // rounds = 0: the lists of an overall best that came from a step are the ones select
    // returns for that single model (no stage of a step forms tight lists)
    if (lo_steps > 0 && rounds == 0 && inlier_idx) {
        std::vector<int32_t> one_ids;
        std::vector<int> one_j;
        std::vector<int64_t> one_off, one_moff(1, 0);
        std::vector<Model> one_models;
        for (int j = 0; j < num_sel; ++j) {
            if (track[(size_t)j].source != kLoSourceStep) continue;
            one_j.push_back(j);
            one_ids.push_back(sel[j]);
            one_off.push_back(set->out_off[(size_t)j]);
            one_moff.push_back((int64_t)one_j.size());
            one_models.push_back(models[j]);
        }
        if (!one_j.empty()) {
            const int no = (int)one_j.size();
            std::vector<SelectResult> one_res((size_t)no);
            SelectTiming stm;
            select_run(*set->R, stream, PairSel{no, one_ids.data()}, one_off.data(), one_moff.data(),
                       one_models.data(), nullptr, nullptr, one_res.data(), inlier_idx, model_chunk, tile, false, stm);
            for (int i = 0; i < no; ++i) {
                const LoTrack &K = track[(size_t)one_j[(size_t)i]];
                const SelectResult &W = one_res[(size_t)i];
                if (W.best_index != 0 || W.best_score != K.score || W.num_inliers[0] != K.counts[0] ||
                    W.num_inliers[1] != K.counts[1] || W.num_inliers[2] != K.counts[2])
                    throw std::logic_error("ransac_lo_steps: a step's model scored differently");
            }
        }
    }
    // ---- refine: once, the overall bests ----
    refine_winners(set, stream, sel, rounds, models, results, inlier_idx, stage.swept());
    stage.finish(set, sel, stream, models, results);
}
} // namespace

void ransac_lo_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step, uint64_t seed,
                   int32_t point_share, int32_t rounds, int32_t lo_rounds, Model *models, RansacResult *results,
                   int32_t *inlier_idx, int32_t *stopped, RansacLoInfo *lo_info, int64_t sample_chunk,
                   int64_t model_chunk, const DrawWeights *weights, bool weighted_stop, InlierMass *rule_mass,
                   const RansacOut *out) {
    ransac_lo_run(set, num_sel, pair_ids, budget, step, seed, point_share, rounds, lo_rounds, models, results,
                  inlier_idx, stopped, lo_info, sample_chunk, model_chunk, 0, nullptr, weights, weighted_stop,
                  rule_mass, out);
}

void ransac_lo_steps_set(PairSet *set, int32_t num_sel, const int32_t *pair_ids, int32_t budget, int32_t step,
                         uint64_t seed, int32_t point_share, int32_t rounds, int32_t lo_rounds, int32_t lo_steps,
                         Model *models, RansacResult *results, int32_t *inlier_idx, int32_t *stopped,
                         RansacLoInfo *lo_info, RansacLoStepsInfo *steps_info, int64_t sample_chunk,
                         int64_t model_chunk, const DrawWeights *weights, bool weighted_stop,
                         InlierMass *rule_mass, const RansacOut *out) {
    if (!set) throw std::invalid_argument("null pair set");
    if (lo_steps < 1 || lo_steps > kLoStepsMax) throw std::invalid_argument("lo_steps must be in 1..64");
    if (num_sel > 0 && !steps_info) throw std::invalid_argument("null steps_info");
    if (set->opts.num_lsq_iterations < 0 || set->opts.num_lsq_iterations > kLoStepLsqIterMax)
        throw std::invalid_argument("num_lsq_iterations must be in 0..254 with lo_steps");
    if (!(set->opts.threshold_multiplier > 0.0) || !(set->opts.threshold_multiplier <= DBL_MAX))
        throw std::invalid_argument("threshold_multiplier must be positive and finite with lo_steps");
    ransac_lo_run(set, num_sel, pair_ids, budget, step, seed, point_share, rounds, lo_rounds, models, results,
                  inlier_idx, stopped, lo_info, sample_chunk, model_chunk, lo_steps, steps_info, weights,
                  weighted_stop, rule_mass, out);
}

void ransac_out_set(PairSet *set, const DrawWeights *weights, int32_t num_sel, const int32_t *pair_ids, int32_t budget,
                    int32_t step, uint64_t seed, int32_t point_share, const int64_t *sample_offsets,
                    const int32_t *sample_types, const int32_t *sample_idx, int32_t rounds, int32_t lo_rounds,
                    int32_t lo_steps, bool weighted_stop, Model *models, RansacResult *results, int32_t *inlier_idx,
                    int32_t *stopped, RansacLoInfo *lo_info, RansacLoStepsInfo *steps_info, int64_t sample_chunk,
                    int64_t model_chunk, InlierMass *rule_mass, const RansacOut *out) {
    if (!set) throw std::invalid_argument("null pair set");
    // (a body told apart from its own entry by out != null: the caller's, or one with nothing in it)
    const RansacOut none;
    const RansacOut *O = out ? out : &none;
    RansacOutStage(O).check_args(rounds, lo_rounds); // (before the bodies' own checks: the refused combination)
    if (step < 0) throw std::invalid_argument("step must be 0 (a fixed budget) or at least 1");
    if (lo_rounds < 0 || lo_steps < 0) throw std::invalid_argument("lo_rounds and lo_steps must not be negative");
    if (step == 0 && (lo_rounds != 0 || lo_steps != 0))
        throw std::invalid_argument("lo_rounds and lo_steps need step: they run inside the adaptive rounds");
    if (lo_rounds == 0 && lo_steps != 0) throw std::invalid_argument("lo_steps needs lo_rounds");
    if (weighted_stop && !weights) throw std::invalid_argument("weighted_stop needs draw weights");
    if (weighted_stop && step < 1)
        throw std::invalid_argument("the weighted stop needs step >= 1: the rule is read at checkpoints");
    const bool given = sample_offsets || sample_types || sample_idx;
    if (given && step != 0) throw std::invalid_argument("given samples go with step 0: the adaptive rounds draw their own");
    if (step == 0)
        ransac_set(set, num_sel, pair_ids, budget, seed, point_share, sample_offsets, sample_types, sample_idx, rounds,
                   models, results, inlier_idx, sample_chunk, model_chunk, weights, O);
    else if (lo_rounds == 0)
        ransac_adaptive_set(set, num_sel, pair_ids, budget, step, seed, point_share, rounds, models, results, inlier_idx,
                            stopped, sample_chunk, model_chunk, weights, weighted_stop, rule_mass, O);
    else if (lo_steps == 0)
        ransac_lo_set(set, num_sel, pair_ids, budget, step, seed, point_share, rounds, lo_rounds, models, results,
                      inlier_idx, stopped, lo_info, sample_chunk, model_chunk, weights, weighted_stop, rule_mass, O);
    else
        ransac_lo_steps_set(set, num_sel, pair_ids, budget, step, seed, point_share, rounds, lo_rounds, lo_steps, models,
                            results, inlier_idx, stopped, lo_info, steps_info, sample_chunk, model_chunk, weights,
                            weighted_stop, rule_mass, O);
}

void ransac_lo_track(int32_t num_rounds, const double *min_score, const int32_t *min_counts, const int32_t *candidate,
                     const int32_t *lo_rounds_accepted, const double *lo_score, const int32_t *lo_counts,
                     double *score, int32_t *out) {
    if (num_rounds < 0) throw std::invalid_argument("negative round count");
    if (!score || !out) throw std::invalid_argument("null output");
    if (num_rounds > 0 && (!min_score || !min_counts || !candidate || !lo_rounds_accepted || !lo_score || !lo_counts))
        throw std::invalid_argument("null input");
    LoTrack K;
    for (int32_t r = 0; r < num_rounds; ++r) {
        lo_take_minimal(K, min_score[r], min_counts + 3 * (size_t)r);
        lo_take_refined(K, candidate[r], lo_rounds_accepted[r], lo_score[r], lo_counts + 3 * (size_t)r);
    }
    *score = K.score;
    for (int t = 0; t < 3; ++t) out[t] = K.counts[t];
    out[3] = K.lo_index;
    out[4] = K.lo_runs;
    out[5] = K.lo_accepted;
    out[6] = K.source;
}

int solve_md_direct(int variant, const double *x, const double *y, const double *dx, const double *dy, double *sols,
                    int max_sols, Model *poses, int max_poses, int *nposes, int device, int alt) {
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    const int k = variant == kCal ? 3 : 4;
    std::vector<double> in(8 * k);
    std::memcpy(in.data(), x, sizeof(double) * 3 * k);
    std::memcpy(in.data() + 3 * k, y, sizeof(double) * 3 * k);
    std::memcpy(in.data() + 6 * k, dx, sizeof(double) * k);
    std::memcpy(in.data() + 7 * k, dy, sizeof(double) * k);
    DevArray<double> d_in(in.size()), d_sols(8 * 6);
    DevArray<int> d_n(2);
    DevArray<Model> d_poses(8);
    MP_HIP(hipMemcpyAsync(d_in.p, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, X.stream));
    MP_HIP(launch_md_direct(X.stream, variant, alt, d_in.p, d_sols.p, d_n.p, d_poses.p, d_n.p + 1));
    double hs[48];
    int hn[2];
    Model hp[8];
    MP_HIP(hipMemcpyAsync(hs, d_sols.p, sizeof(hs), hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipMemcpyAsync(hn, d_n.p, sizeof(hn), hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipMemcpyAsync(hp, d_poses.p, sizeof(hp), hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipStreamSynchronize(X.stream));
    const int w = variant == kCal ? 4 : (variant == kSF ? 5 : 6);
    for (int i = 0; i < std::min(hn[0], max_sols); ++i)
        for (int c = 0; c < w; ++c) sols[i * w + c] = hs[i * w + c];
    for (int i = 0; i < std::min(hn[1], max_poses); ++i) poses[i] = hp[i];
    if (nposes) *nposes = hn[1];
    return hn[0];
}

int solve_point_direct(int kind, const double *x1, const double *x2, Model *poses, int max_poses, int device) {
    if (kind < 0 || kind > 2) throw std::invalid_argument("point solver kind must be 0, 1 or 2");
    if (kind == 1) {
        // the estimator's root stage (deflated eigenproblem) on this one sample, then
        // its poses
        double cand[kPtCandStride];
        int nc = 0;
        debug_pt_roots(kSF, 1, x1, x2, cand, &nc, device);
        CtxLease lease(device);
        DeviceCtx &X = *lease.c;
        double in[24];
        std::memcpy(in, x1, sizeof(double) * 12);
        std::memcpy(in + 12, x2, sizeof(double) * 12);
        constexpr int kCap = 16;
        DevArray<double> d_in(24), d_cand(kPtCandStride);
        DevArray<int> d_nc(1), d_n(1);
        DevArray<Model> d_poses(kCap);
        MP_HIP(hipMemcpyAsync(d_in.p, in, sizeof(in), hipMemcpyHostToDevice, X.stream));
        MP_HIP(hipMemcpyAsync(d_cand.p, cand, sizeof(cand), hipMemcpyHostToDevice, X.stream));
        MP_HIP(hipMemcpyAsync(d_nc.p, &nc, sizeof(int), hipMemcpyHostToDevice, X.stream));
        MP_HIP(launch_point_direct_6pt(X.stream, d_in.p, d_cand.p, d_nc.p, d_poses.p, d_n.p));
        int hn = 0;
        Model hp[kCap];
        MP_HIP(hipMemcpyAsync(&hn, d_n.p, sizeof(int), hipMemcpyDeviceToHost, X.stream));
        MP_HIP(hipMemcpyAsync(hp, d_poses.p, sizeof(hp), hipMemcpyDeviceToHost, X.stream));
        MP_HIP(hipStreamSynchronize(X.stream));
        for (int i = 0; i < std::min(std::min(hn, kCap), max_poses); ++i) poses[i] = hp[i];
        return hn;
    }
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    const int per = kind == 0 ? 15 : 14;
    double in[30];
    std::memcpy(in, x1, sizeof(double) * per);
    std::memcpy(in + per, x2, sizeof(double) * per);
    constexpr int kCap = 16;
    DevArray<double> d_in(30), d_cand(kPtCandStride);
    DevArray<int> d_n(1), d_nc(1);
    DevArray<Model> d_poses(kCap);
    MP_HIP(hipMemcpyAsync(d_in.p, in, sizeof(in), hipMemcpyHostToDevice, X.stream));
    MP_HIP(launch_point_direct(X.stream, kind, d_in.p, d_poses.p, d_n.p, d_cand.p, d_nc.p));
    int hn = 0;
    Model hp[kCap];
    MP_HIP(hipMemcpyAsync(&hn, d_n.p, sizeof(int), hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipMemcpyAsync(hp, d_poses.p, sizeof(hp), hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipStreamSynchronize(X.stream));
    for (int i = 0; i < std::min(std::min(hn, kCap), max_poses); ++i) poses[i] = hp[i];
    return hn;
}

// The pseudo-pair of ns point samples of K normalized 2-D points each (pts*: ns x K x 2),
// as launch_pt_roots reads a pair: one correspondence per sample point (host: the eight
// PairData arrays x0u x0v x1u x1v d0 d1 r0 r1 of np = K ns entries), sample s = points
// K s .. K s + K - 1 (smp, kSampleStride ints each), every sample listed.
static void pt_pseudo_pair(int K, int64_t ns, const double *pts0, const double *pts1, std::vector<double> &host,
                           std::vector<int> &smp, std::vector<int> &list) {
    const int64_t np = K * ns;
    host.resize(8 * (size_t)np);
    for (int64_t i = 0; i < np; ++i) {
        host[i] = pts0[2 * i];
        host[np + i] = pts0[2 * i + 1];
        host[2 * np + i] = pts1[2 * i];
        host[3 * np + i] = pts1[2 * i + 1];
        host[4 * np + i] = host[5 * np + i] = 1.0;
        host[6 * np + i] = 1.0 / std::sqrt(pts0[2 * i] * pts0[2 * i] + pts0[2 * i + 1] * pts0[2 * i + 1] + 1.0);
        host[7 * np + i] = 1.0 / std::sqrt(pts1[2 * i] * pts1[2 * i] + pts1[2 * i + 1] * pts1[2 * i + 1] + 1.0);
    }
    smp.assign(8 * (size_t)ns, 0);
    list.resize((size_t)ns);
    for (int64_t s = 0; s < ns; ++s) {
        list[s] = (int)s;
        for (int j = 0; j < K; ++j) smp[8 * s + j] = (int)(K * s + j);
    }
}
// its device views: identity intrinsics, the arrays at d_pair (8 np doubles)
static void pt_pseudo_views(int variant, int64_t np, double *d_pair, PairData *D, PairConst *C) {
    *D = PairData{d_pair, d_pair + np, d_pair + 2 * np, d_pair + 3 * np, d_pair + 4 * np, d_pair + 5 * np,
                  d_pair + 6 * np, d_pair + 7 * np};
    *C = PairConst{};
    C->variant = variant;
    C->n = (int)np;
    for (int k = 0; k < 9; ++k) C->K0[k] = C->K1[k] = C->K0i[k] = C->K1i[k] = (k % 4 == 0) ? 1.0 : 0.0;
}

void debug_pt_roots(int variant, int64_t ns, const double *pts0, const double *pts1, double *cand, int *ncand,
                    int device) {
    if (variant != kCal && variant != kSF && variant != kTF)
        throw std::invalid_argument("variant must be 0 (5pt), 1 (6pt) or 2 (7pt)");
    if (ns <= 0 || ns > (1 << 22)) throw std::invalid_argument("bad number of samples");
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    const int K = variant == kCal ? 5 : (variant == kSF ? 6 : 7);
    const int64_t np = K * ns;
    // one correspondence per sample point, identity intrinsics, sample s = points Ks..Ks+K-1
    std::vector<double> host;
    std::vector<int> smp, list;
    pt_pseudo_pair(K, ns, pts0, pts1, host, smp, list);
    DevArray<double> d_pair_a(host.size()), d_cand_a(kPtCandStride * (size_t)ns);
    DevArray<int> d_smp_a(smp.size()), d_list_a(list.size()), d_n_a((size_t)ns);
    double *d_pair = d_pair_a.p, *d_cand = d_cand_a.p;
    int *d_smp = d_smp_a.p, *d_list = d_list_a.p, *d_n = d_n_a.p;
    MP_HIP(hipMemcpyAsync(d_pair, host.data(), sizeof(double) * host.size(), hipMemcpyHostToDevice, X.stream));
    MP_HIP(hipMemcpyAsync(d_smp, smp.data(), sizeof(int) * smp.size(), hipMemcpyHostToDevice, X.stream));
    MP_HIP(hipMemcpyAsync(d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, X.stream));
    MP_HIP(hipMemsetAsync(d_cand, 0, sizeof(double) * kPtCandStride * (size_t)ns, X.stream));
    PairData D;
    PairConst C;
    pt_pseudo_views(variant, np, d_pair, &D, &C);
    DevArray<double> d_pen(variant == kSF ? (size_t)ns * kPtPenStride : 1);
    MP_HIP(launch_pt_roots(X.stream, D, C, d_list, (int)ns, d_smp, d_cand, d_n, d_pen.p));
    MP_HIP(hipMemcpyAsync(cand, d_cand, sizeof(double) * kPtCandStride * (size_t)ns, hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipMemcpyAsync(ncand, d_n, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, X.stream));
    MP_HIP(hipStreamSynchronize(X.stream));
}

// ---- the minimal solvers over many raw samples (mp_*_batch) ----
// A batch runs in rounds of at most `chunk` samples (host/solve_batch_pack.h); every
// round reuses the context's block (DeviceCtx::solve_block), carved below.
namespace {
struct Carver {
    char *base;
    size_t off = 0;
    template <class T> T *take(size_t n) {
        off = (off + 255) & ~size_t(255);
        T *r = reinterpret_cast<T *>(base + off);
        off += sizeof(T) * n;
        return r;
    }
};
void check_batch_args(int64_t ns, int64_t chunk) {
    if (ns < 0 || ns > kSolveBatchMax) throw std::invalid_argument("the number of samples must be in [0, 2^22]");
    if (chunk < 0) throw std::invalid_argument("chunk must not be negative (0: the default)");
}
} // namespace

void solve_md_batch(int variant, int alt, bool pose, int64_t ns, const double *x, const double *y, const double *dx,
                    const double *dy, double *sols, Model *poses, int32_t *counts, int64_t chunk, int device) {
    if (variant != kCal && variant != kSF && variant != kTF) throw std::invalid_argument("bad variant");
    if (alt < 0 || alt > 2 || (alt == 2 && variant != kTF))
        throw std::invalid_argument("alt must be 0, 1 (use_ours) or 2 (use_4p4d, two-focal only)");
    if (alt != 0 && !pose) throw std::invalid_argument("the alternates return poses only");
    check_batch_args(ns, chunk);
    if (ns == 0) return;
    if (!x || !y || !dx || !dy || !counts || (pose ? !poses : !sols)) throw std::invalid_argument("bad arguments");
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    const int K = variant == kCal ? 3 : 4, w = variant == kCal ? 4 : (variant == kSF ? 5 : 6);
    const int64_t cmax = solve_batch_chunk(ns, chunk), ldmax = solve_batch_ld(cmax);
    const size_t out_bytes = pose ? sizeof(Model) * 8 : sizeof(double) * 8 * w; // per sample
    double *d_in = nullptr;
    char *d_out = nullptr;
    int *d_n = nullptr;
    auto carve = [&](char *base) {
        Carver c{base};
        d_in = c.take<double>((size_t)md_rows(K) * ldmax);
        d_out = c.take<char>(out_bytes * cmax);
        d_n = c.take<int>((size_t)cmax);
        return c.off;
    };
    carve(X.solve_block(carve(nullptr)));
    std::vector<double> hin((size_t)md_rows(K) * ldmax, 0.0);
    char *out = pose ? reinterpret_cast<char *>(poses) : reinterpret_cast<char *>(sols);
    for (int64_t r = 0, nr = solve_batch_rounds(ns, chunk); r < nr; ++r) {
        int64_t s0, cnt;
        solve_batch_round(ns, chunk, r, &s0, &cnt);
        const int64_t ld = solve_batch_ld(cnt);
        pack_md_soa(K, s0, cnt, ld, x, y, dx, dy, hin.data());
        MP_HIP(hipMemcpyAsync(d_in, hin.data(), sizeof(double) * md_rows(K) * ld, hipMemcpyHostToDevice, X.stream));
        MP_HIP(hipMemsetAsync(d_out, 0, out_bytes * cnt, X.stream));
        MP_HIP(launch_sb_md(X.stream, variant, alt, pose, d_in, (int)ld, (int)cnt, reinterpret_cast<double *>(d_out),
                            reinterpret_cast<Model *>(d_out), d_n));
        MP_HIP(hipMemcpyAsync(out + out_bytes * s0, d_out, out_bytes * cnt, hipMemcpyDeviceToHost, X.stream));
        MP_HIP(hipMemcpyAsync(counts + s0, d_n, sizeof(int) * cnt, hipMemcpyDeviceToHost, X.stream));
        MP_HIP(hipStreamSynchronize(X.stream)); // (hin is packed again for the next round)
    }
}

void relpose_batch(int kind, int64_t ns, const double *x0, const double *x1, Model *poses, int32_t *counts,
                   int64_t chunk, int device) {
    if (kind < 0 || kind > 2) throw std::invalid_argument("point solver kind must be 0, 1 or 2");
    check_batch_args(ns, chunk);
    if (ns == 0) return;
    if (!x0 || !x1 || !poses || !counts) throw std::invalid_argument("bad arguments");
    CtxLease lease(device);
    DeviceCtx &X = *lease.c;
    const int K = kind == 0 ? 5 : (kind == 1 ? 6 : 7);
    const int per = kind == 0 ? 15 : 2 * K; // doubles of a sample per image
    const int64_t cmax = solve_batch_chunk(ns, chunk), ldmax = solve_batch_ld(cmax);
    double *d_in = nullptr, *d_cand = nullptr, *d_pen = nullptr, *d_pair = nullptr, *d_F = nullptr;
    int *d_ncand = nullptr, *d_n = nullptr, *d_smp = nullptr, *d_list = nullptr;
    Model *d_poses = nullptr;
    auto carve = [&](char *base) {
        Carver c{base};
        d_in = c.take<double>(kind == 2 ? 28 * (size_t)ldmax : 2 * (size_t)per * cmax);
        d_poses = c.take<Model>(16 * (size_t)cmax);
        d_n = c.take<int>((size_t)cmax);
        if (kind != 2) {
            d_cand = c.take<double>((size_t)kPtCandStride * cmax);
            d_ncand = c.take<int>((size_t)cmax);
        }
        if (kind == 1) {
            d_pen = c.take<double>((size_t)kPtPenStride * cmax);
            d_pair = c.take<double>(8 * (size_t)K * cmax);
            d_smp = c.take<int>(8 * (size_t)cmax);
            d_list = c.take<int>((size_t)cmax);
        }
        if (kind == 2) d_F = c.take<double>(27 * (size_t)ldmax);
        return c.off;
    };
    carve(X.solve_block(carve(nullptr)));
    std::vector<double> hin(kind == 2 ? 28 * (size_t)ldmax : 2 * (size_t)per * cmax, 0.0), hpair;
    std::vector<int> smp, list;
    for (int64_t r = 0, nr = solve_batch_rounds(ns, chunk); r < nr; ++r) {
        int64_t s0, cnt;
        solve_batch_round(ns, chunk, r, &s0, &cnt);
        const int64_t ld = solve_batch_ld(cnt);
        size_t in_doubles;
        if (kind == 2) {
            pack_soa(x0, 14, s0, cnt, ld, 0, hin.data());
            pack_soa(x1, 14, s0, cnt, ld, 14, hin.data());
            in_doubles = 28 * (size_t)ld;
        } else { // sample-major, image 0's points then image 1's (the single-sample layout)
            for (int64_t i = 0; i < cnt; ++i) {
                std::memcpy(hin.data() + 2 * per * i, x0 + (s0 + i) * per, sizeof(double) * per);
                std::memcpy(hin.data() + 2 * per * i + per, x1 + (s0 + i) * per, sizeof(double) * per);
            }
            in_doubles = 2 * (size_t)per * cnt;
        }
        MP_HIP(hipMemcpyAsync(d_in, hin.data(), sizeof(double) * in_doubles, hipMemcpyHostToDevice, X.stream));
        MP_HIP(hipMemsetAsync(d_poses, 0, sizeof(Model) * 16 * cnt, X.stream));
        if (kind == 0) {
            MP_HIP(launch_sb_pt5(X.stream, d_in, (int)cnt, d_cand, d_ncand, d_poses, d_n));
        } else if (kind == 1) {
            // the estimator's root stage on the chunk's pseudo-pair, as debug_pt_roots runs it
            pt_pseudo_pair(K, cnt, x0 + s0 * per, x1 + s0 * per, hpair, smp, list);
            MP_HIP(hipMemcpyAsync(d_pair, hpair.data(), sizeof(double) * hpair.size(), hipMemcpyHostToDevice, X.stream));
            MP_HIP(hipMemcpyAsync(d_smp, smp.data(), sizeof(int) * smp.size(), hipMemcpyHostToDevice, X.stream));
            MP_HIP(hipMemcpyAsync(d_list, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice, X.stream));
            MP_HIP(hipMemsetAsync(d_cand, 0, sizeof(double) * kPtCandStride * (size_t)cnt, X.stream));
            PairData D;
            PairConst C;
            pt_pseudo_views(kSF, K * cnt, d_pair, &D, &C);
            MP_HIP(launch_pt_roots(X.stream, D, C, d_list, (int)cnt, d_smp, d_cand, d_ncand, d_pen));
            MP_HIP(launch_sb_pt6_poses(X.stream, d_in, (int)cnt, d_cand, d_ncand, d_poses, d_n));
        } else {
            MP_HIP(launch_sb_pt7(X.stream, d_in, (int)ld, (int)cnt, d_F, d_poses, d_n));
        }
        MP_HIP(hipMemcpyAsync(poses + 16 * s0, d_poses, sizeof(Model) * 16 * cnt, hipMemcpyDeviceToHost, X.stream));
        MP_HIP(hipMemcpyAsync(counts + s0, d_n, sizeof(int) * cnt, hipMemcpyDeviceToHost, X.stream));
        MP_HIP(hipStreamSynchronize(X.stream)); // (the host staging is packed again for the next round)
    }
}

void bougnoux_batch(int64_t k, const double *F, double *out, int device) {
    if (k <= 0) return;
    CtxLease lease(device);
    hipStream_t s = lease.c->stream;
    DevArray<double> d_F(9 * (size_t)k), d_out(2 * (size_t)k);
    MP_HIP(hipMemcpyAsync(d_F.p, F, sizeof(double) * 9 * (size_t)k, hipMemcpyHostToDevice, s));
    MP_HIP(launch_bougnoux(s, d_F.p, k, d_out.p));
    MP_HIP(hipMemcpyAsync(out, d_out.p, sizeof(double) * 2 * (size_t)k, hipMemcpyDeviceToHost, s));
    MP_HIP(hipStreamSynchronize(s));
}

void pose_eval_batch(int64_t k, const double *R, const double *t, const double *T, double t_thres, double *err_t,
                     double *err_R, int nthr, const double *thr, double *aucs, int device) {
    if (k <= 0) {
        for (int b = 0; b < nthr; ++b) aucs[b] = NAN;
        return;
    }
    CtxLease lease(device);
    hipStream_t s = lease.c->stream;
    // one block: R (9k) t (3k) T (16k) | err_t err_R max(err_t, err_R) sorted (4k) | thr, aucs (2 nthr)
    const size_t in = 28 * (size_t)k, tot = in + 4 * (size_t)k + 2 * (size_t)std::max(nthr, 0);
    std::vector<double> host(in);
    std::memcpy(host.data(), R, sizeof(double) * 9 * k);
    std::memcpy(host.data() + 9 * k, t, sizeof(double) * 3 * k);
    std::memcpy(host.data() + 12 * k, T, sizeof(double) * 16 * k);
    DevArray<double> d_all(tot);
    double *d = d_all.p;
    double *d_et = d + in, *d_eR = d_et + k, *d_max = d_eR + k, *d_sorted = d_max + k, *d_thr = d_sorted + k,
           *d_auc = d_thr + nthr;
    MP_HIP(hipMemcpyAsync(d, host.data(), sizeof(double) * in, hipMemcpyHostToDevice, s));
    if (nthr > 0) MP_HIP(hipMemcpyAsync(d_thr, thr, sizeof(double) * nthr, hipMemcpyHostToDevice, s));
    MP_HIP(launch_pose_errors(s, k, d, d + 9 * k, d + 12 * k, t_thres, d_et, d_eR, nthr > 0 ? d_max : nullptr));
    MP_HIP(launch_pose_auc(s, k, d_max, d_sorted, nthr, d_thr, d_auc));
    MP_HIP(hipMemcpyAsync(err_t, d_et, sizeof(double) * k, hipMemcpyDeviceToHost, s));
    MP_HIP(hipMemcpyAsync(err_R, d_eR, sizeof(double) * k, hipMemcpyDeviceToHost, s));
    if (nthr > 0) MP_HIP(hipMemcpyAsync(aucs, d_auc, sizeof(double) * nthr, hipMemcpyDeviceToHost, s));
    MP_HIP(hipStreamSynchronize(s));
}

void pose_auc_batch(int64_t k, const double *errors, int nthr, const double *thr, double *aucs, int device) {
    if (nthr <= 0) return;
    if (k <= 0) {
        for (int b = 0; b < nthr; ++b) aucs[b] = NAN;
        return;
    }
    CtxLease lease(device);
    hipStream_t s = lease.c->stream;
    DevArray<double> d_all(2 * (size_t)k + 2 * (size_t)nthr); // errors (k) | sorted (k) | thresholds, aucs
    double *d = d_all.p;
    double *d_sorted = d + k, *d_thr = d_sorted + k, *d_auc = d_thr + nthr;
    MP_HIP(hipMemcpyAsync(d, errors, sizeof(double) * k, hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(d_thr, thr, sizeof(double) * nthr, hipMemcpyHostToDevice, s));
    MP_HIP(launch_pose_auc(s, k, d, d_sorted, nthr, d_thr, d_auc));
    MP_HIP(hipMemcpyAsync(aucs, d_auc, sizeof(double) * nthr, hipMemcpyDeviceToHost, s));
    MP_HIP(hipStreamSynchronize(s));
}

void get_depths_batch(int dtype, int32_t num, const void *maps, const int64_t *dims, const int64_t *pt_off,
                      const double *pts, void *out, int device) {
    if (dtype != 0 && dtype != 1) throw std::invalid_argument("dtype must be 0 (float32) or 1 (float64)");
    if (num <= 0) return;
    const size_t es = dtype == 0 ? sizeof(float) : sizeof(double);
    std::vector<int64_t> map_off(num + 1), hw(2 * (size_t)num);
    std::vector<double> fac(2 * (size_t)num);
    map_off[0] = 0;
    for (int p = 0; p < num; ++p) {
        const int64_t h = dims[4 * p], w = dims[4 * p + 1], ih = dims[4 * p + 2], iw = dims[4 * p + 3];
        if (h <= 0 || w <= 0 || ih <= 0 || iw <= 0) throw std::invalid_argument("bad depth-map or image size");
        if (pt_off[p + 1] < pt_off[p]) throw std::invalid_argument("keypoint offsets must not decrease");
        map_off[p + 1] = map_off[p] + h * w;
        hw[2 * p] = h;
        hw[2 * p + 1] = w;
        fac[2 * p] = (double)w / (double)iw; // factor = [dm_w / im_w, dm_h / im_h]
        fac[2 * p + 1] = (double)h / (double)ih;
    }
    const int64_t total = pt_off[num], cells = map_off[num];
    CtxLease lease(device);
    hipStream_t s = lease.c->stream;
    DevArray<char> d_maps_a(es * (size_t)std::max<int64_t>(cells, 1)), d_out_a(es * (size_t)std::max<int64_t>(total, 1));
    DevArray<int64_t> d_map_off_a(num + 1), d_hw_a(2 * (size_t)num), d_pt_off_a(num + 1);
    DevArray<double> d_fac_a(2 * (size_t)num), d_pts_a(2 * (size_t)std::max<int64_t>(total, 1));
    char *d_maps = d_maps_a.p, *d_out = d_out_a.p;
    int64_t *d_map_off = d_map_off_a.p, *d_hw = d_hw_a.p, *d_pt_off = d_pt_off_a.p;
    double *d_fac = d_fac_a.p, *d_pts = d_pts_a.p;
    MP_HIP(hipMemcpyAsync(d_maps, maps, es * (size_t)cells, hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(d_map_off, map_off.data(), sizeof(int64_t) * (num + 1), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(d_hw, hw.data(), sizeof(int64_t) * 2 * num, hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(d_pt_off, pt_off, sizeof(int64_t) * (num + 1), hipMemcpyHostToDevice, s));
    MP_HIP(hipMemcpyAsync(d_fac, fac.data(), sizeof(double) * 2 * num, hipMemcpyHostToDevice, s));
    if (total > 0) MP_HIP(hipMemcpyAsync(d_pts, pts, sizeof(double) * 2 * total, hipMemcpyHostToDevice, s));
    MP_HIP(launch_get_depths(s, dtype, d_maps, d_map_off, d_hw, d_fac, d_pt_off, num, total, d_pts, d_out));
    if (total > 0) MP_HIP(hipMemcpyAsync(out, d_out, es * (size_t)total, hipMemcpyDeviceToHost, s));
    MP_HIP(hipStreamSynchronize(s));
}

void scale_and_pose_direct(const double *X, const double *Y, const double *W, int64_t n, Model *out, int device) {
    CtxLease lease(device);
    DeviceCtx &C = *lease.c;
    std::vector<double> in(7 * (size_t)n);
    std::memcpy(in.data(), X, sizeof(double) * 3 * n);
    std::memcpy(in.data() + 3 * n, Y, sizeof(double) * 3 * n);
    std::memcpy(in.data() + 6 * n, W, sizeof(double) * n);
    DevArray<double> d_in(in.size());
    DevArray<Model> d_out(1);
    MP_HIP(hipMemcpyAsync(d_in.p, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, C.stream));
    MP_HIP(launch_scale_and_pose(C.stream, d_in.p, n, d_out.p));
    MP_HIP(hipMemcpyAsync(out, d_out.p, sizeof(Model), hipMemcpyDeviceToHost, C.stream));
    MP_HIP(hipStreamSynchronize(C.stream));
}

int device_count() {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

} // namespace mp
