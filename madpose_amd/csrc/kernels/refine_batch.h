// Refinement of given models over many resident pairs (mp_refine_batch; host side:
// engine.cpp refine_batch).  Included from kernels.hip after the estimator's kernels.
// The pairs of a run stay on the device (host/refine_plan.h); their PairData / PairConst
// records sit in device arrays and every work item names its pair, so one launch covers
// all pairs that are still running.
//
//  refine_sweep<V>  one workgroup per (pair, model): the three squared errors of every
//                   correspondence as sweep_kernel forms them (eval_corr<V>, no score-type
//                   gating), the MSAC sum of the gated values accumulated and reduced as
//                   score_models_kernel does (the same bits), and the three ascending
//                   inlier lists err < thr written by ballot + popcount ranks: a lane's
//                   rank inside its wave, the waves' counts scanned in LDS, a running
//                   base across trips.  No atomics; the lists are deterministic.
//  refine_sweep_relaxed<V>  the same pass with a second, relaxed threshold per term: the
//                   tight lists to the item's buffer, the relaxed lists to the other one
//  lm_pairs<V>      lm_device.h: the device LM, one workgroup per (pair, problem)
#pragma once

namespace mp {
namespace {

template <int V>
__global__ void __launch_bounds__(kBlock) refine_sweep_kernel(const PairData *Ds, const PairConst *Cs,
                                                              const RefineItem *items, const ScoreRec *recs,
                                                              const int64_t *list_off, int *lists, int64_t buf_stride,
                                                              RefineSweepOut *out) {
    const RefineItem it = items[blockIdx.x];
    const PairData &D = Ds[it.pair];
    const PairConst &C = Cs[it.pair];
    const ScoreRec r = recs[blockIdx.x];
    const int n = C.n;
    int *lst = lists + (int64_t)it.buf * buf_stride + list_off[it.pair]; // list t at lst + t n
    // EvaluateModelOnPoint's score-type gating replaces a term's error by DBL_MAX; the
    // inlier lists take the ungated errors -- both from the one evaluation
    const bool skip_md = C.score_type == 1, skip_epi = C.score_type == 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int s_cnt[3][kBlock / 64];
    __shared__ double part[kBlock / 64];
    int base[3] = {0, 0, 0};
    double acc = 0.0;
    const int ntrip = (n + kBlock - 1) / kBlock;
    for (int trip = 0; trip < ntrip; ++trip) {
        const int i = trip * kBlock + threadIdx.x;
        bool inl[3] = {false, false, false};
        if (i < n) {
            const Corr p = load_corr(C, D, i, V == kCal);
            double e0, e1, e2;
            bool flag = false; // (unused: nothing is screened here)
            eval_corr<V>(C, r, p, false, e0, e1, e2, flag);
            inl[0] = e0 < C.thr[0];
            inl[1] = e1 < C.thr[1];
            inl[2] = e2 < C.thr[2];
            if (skip_md) e0 = e1 = DBL_MAX;
            if (skip_epi) e2 = DBL_MAX;
            acc += msac(e0, C.thr[0], C.w[0]) + msac(e1, C.thr[1], C.w[1]) + msac(e2, C.thr[2], C.w[2]);
        }
        int rank[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const unsigned long long b = __ballot(inl[t]);
            rank[t] = __popcll(b & ((1ull << lane) - 1ull));
            if (lane == 0) s_cnt[t][wave] = __popcll(b);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            int before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) {
                const int c = s_cnt[t][w];
                before += w < wave ? c : 0;
                total += c;
            }
            // (base + before + rank < the inliers so far <= i < n: inside list t)
            if (inl[t]) lst[(int64_t)t * n + base[t] + before + rank[t]] = i;
            base[t] += total;
        }
        __syncthreads(); // s_cnt is rewritten by the next trip
    }
    const double v = wave_sum(acc);
    if (lane == 0) part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kBlock / 64; ++w) s += part[w];
        RefineSweepOut o;
        o.score = s;
        o.count[0] = base[0];
        o.count[1] = base[1];
        o.count[2] = base[2];
        o.pad = 0;
        out[blockIdx.x] = o;
    }
}

// refine_sweep_kernel with two thresholds per term in the one pass (the first sweep of a
// relaxed refinement, refine_run(relax)): the tight lists err < thr go to the item's list
// buffer as above, the relaxed lists err < thr * relax (one double product, rounded once)
// to the other buffer, each with its own ballot + popcount ranks and running bases.  The
// score is accumulated and reduced in refine_sweep_kernel's order: the same bits.
template <int V>
__global__ void __launch_bounds__(kBlock)
    refine_sweep_relaxed_kernel(const PairData *Ds, const PairConst *Cs, const RefineItem *items, const ScoreRec *recs,
                                const int64_t *list_off, int *lists, int64_t buf_stride, double relax,
                                RelaxedSweepOut *out) {
    const RefineItem it = items[blockIdx.x];
    const PairData &D = Ds[it.pair];
    const PairConst &C = Cs[it.pair];
    const ScoreRec r = recs[blockIdx.x];
    const int n = C.n;
    // list t of set q (0 tight, 1 relaxed) at lst[q] + t n
    int *lst[2] = {lists + (int64_t)it.buf * buf_stride + list_off[it.pair],
                   lists + (int64_t)(it.buf ^ 1) * buf_stride + list_off[it.pair]};
    const double rthr[3] = {C.thr[0] * relax, C.thr[1] * relax, C.thr[2] * relax};
    const bool skip_md = C.score_type == 1, skip_epi = C.score_type == 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int s_cnt[2][3][kBlock / 64];
    __shared__ double part[kBlock / 64];
    int base[2][3] = {{0, 0, 0}, {0, 0, 0}};
    double acc = 0.0;
    const int ntrip = (n + kBlock - 1) / kBlock;
    for (int trip = 0; trip < ntrip; ++trip) {
        const int i = trip * kBlock + threadIdx.x;
        bool inl[2][3] = {{false, false, false}, {false, false, false}};
        if (i < n) {
            const Corr p = load_corr(C, D, i, V == kCal);
            double e0, e1, e2;
            bool flag = false; // (unused: nothing is screened here)
            eval_corr<V>(C, r, p, false, e0, e1, e2, flag);
            inl[0][0] = e0 < C.thr[0];
            inl[0][1] = e1 < C.thr[1];
            inl[0][2] = e2 < C.thr[2];
            inl[1][0] = e0 < rthr[0];
            inl[1][1] = e1 < rthr[1];
            inl[1][2] = e2 < rthr[2];
            if (skip_md) e0 = e1 = DBL_MAX;
            if (skip_epi) e2 = DBL_MAX;
            acc += msac(e0, C.thr[0], C.w[0]) + msac(e1, C.thr[1], C.w[1]) + msac(e2, C.thr[2], C.w[2]);
        }
        int rank[2][3];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const unsigned long long b = __ballot(inl[q][t]);
                rank[q][t] = __popcll(b & ((1ull << lane) - 1ull));
                if (lane == 0) s_cnt[q][t][wave] = __popcll(b);
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                int before = 0, total = 0;
#pragma unroll
                for (int w = 0; w < kBlock / 64; ++w) {
                    const int c = s_cnt[q][t][w];
                    before += w < wave ? c : 0;
                    total += c;
                }
                // (base + before + rank < the set's inliers so far <= i < n: inside list t)
                if (inl[q][t]) lst[q][(int64_t)t * n + base[q][t] + before + rank[q][t]] = i;
                base[q][t] += total;
            }
        }
        __syncthreads(); // s_cnt is rewritten by the next trip
    }
    const double v = wave_sum(acc);
    if (lane == 0) part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < kBlock / 64; ++w) s += part[w];
        RelaxedSweepOut o;
        o.score = s;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            o.count[t] = base[0][t];
            o.relaxed[t] = base[1][t];
        }
        out[blockIdx.x] = o;
    }
}

} // namespace

hipError_t launch_refine_sweep_relaxed(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                                       const RefineItem *items, const ScoreRec *recs, int nitems,
                                       const int64_t *list_off, int *lists, int64_t buf_stride, double relax,
                                       RelaxedSweepOut *out) {
    if (nitems <= 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        refine_sweep_relaxed_kernel<decltype(V)::value>
            <<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, list_off, lists, buf_stride, relax, out);
        return hipGetLastError();
    });
}

hipError_t launch_refine_sweep(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                               const RefineItem *items, const ScoreRec *recs, int nitems, const int64_t *list_off,
                               int *lists, int64_t buf_stride, RefineSweepOut *out) {
    if (nitems <= 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        refine_sweep_kernel<decltype(V)::value>
            <<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, list_off, lists, buf_stride, out);
        return hipGetLastError();
    });
}

hipError_t launch_lm_pairs(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs, const LmJob *jobs,
                           const LmPairRef *refs, int njobs, const int *idx, Model *out, int *status) {
    if (njobs <= 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        lm_pairs_kernel<decltype(V)::value><<<njobs, kLmBlock, 0, s>>>(Ds, Cs, jobs, refs, idx, out, status);
        return hipGetLastError();
    });
}

} // namespace mp
