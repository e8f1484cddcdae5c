// The Gauss-Newton system of the estimators' cost over a model's inliers, and its inverse, per
// entry (mp_information_set; host side: engine.cpp information_set, plan:
// host/information_plan.h, finishing arithmetic: include/mp_information.h).  Included from
// kernels.hip after residuals.h.  Two kernels; nothing else is launched.
//
//  information_kernel<V>  one 256-lane workgroup per item (ResidItem: up to kInfoItemRows
//                   consecutive rows of one entry), one row per lane per trip.  Thread 0 sets
//                   the parameters up as lm_setup.inc does (lm_rot_to_quat, then
//                   lm_quat_to_rot) and, where Sampson blocks are not gated off, the Sampson
//                   constants once for the workgroup, as lm_evaluate does.  Per row: one
//                   load_corr and one eval_corr<V> on the entry's record, the three bits
//                   err_t < thr_t * factor (residuals_kernel's, so the blocks are exactly the
//                   set bits of mp_residuals_set), and for every set bit whose block type the
//                   LO type leaves, the matching lm_block_*<V, NA>(.., jac = true, acc) into
//                   the lane's LmAcc<NA>.  One pass with the whole accumulator: the Jacobians
//                   are the cost of a row, and a second pass (H, then g and the cost) would
//                   form them twice to save 12 of 78 accumulators.  Then lm_reduce's fixed
//                   order (wave butterflies, then the four waves in order) and the item's
//                   partial record in the full 11-parameter layout (entries the variant does
//                   not have: zero).  Counts: wave ballots' popcounts, as residuals_kernel.
//                   No atomics; no floating-point sum whose order depends on scheduling.
//  information_finish_kernel  one 128-lane workgroup per entry.  Thread q < 78 adds entry q
//                   of the entry's partial records in item order (threads 78 .. 80 the
//                   counts); thread 0 forms the gated block counts, the active columns
//                   (info_columns: lm_setup.inc's), zeroes the inactive rows and columns
//                   (info_mask) and inverts on the active set (info_covariance), all in LDS
//                   and registers; then all threads store H, g, the cost and cov (each
//                   nullable) to row out_row of the outputs and thread 0 the entry's record.
//                   An entry with one item, or none, takes the same path.
//
// LDS: information_kernel LmShared<NA> + 48 bytes of counts (5200 bytes for NA = 11);
// information_finish_kernel 78 + 121 doubles and a few ints.  Neither limits occupancy, which
// the registers set: one wave per SIMD (356 / 422 / 466 of 512 registers, no scratch, no vector
// spill; profiles/information/resource_usage.txt).
#pragma once
#include "../host/information_plan.h"

namespace mp {
namespace {

constexpr int kInfoFinishBlock = 128;
static_assert(kInfoFinishBlock >= kInfoRed + 3, "one reduced value per thread, and the counts");
static_assert(kInfoItemRows % kBlock == 0, "an item is whole trips");

template <int V>
__global__ void __launch_bounds__(kBlock) __attribute__((flatten))
    information_kernel(const PairData *__restrict__ Ds, const PairConst *__restrict__ Cs,
                       const ResidItem *__restrict__ items, const ScoreRec *__restrict__ recs,
                       const InfoJob *__restrict__ jobs, InfoPartial *__restrict__ part) {
    static_assert(kBlock == kLmBlock, "lm_reduce's workgroup");
    constexpr int NA = V == kCal ? kLF0 : (V == kSF ? kLF0 + 1 : kLNFull);
    constexpr int kPack = LmShared<NA>::kPack;
    __shared__ LmShared<NA> sh;
    __shared__ int s_cnt[3][kBlock / 64];
    const ResidItem it = items[blockIdx.x];
    const PairData &D = Ds[it.pair];
    const PairConst &C = Cs[it.pair];
    const ScoreRec r = recs[it.rec];
    const InfoJob &J = jobs[it.rec]; // (read in place: uniform)
    const bool use_reproj = J.use_reproj != 0, use_sampson = J.use_sampson != 0;
    const double w_sampson = J.w_sampson;
    const double rthr[3] = {C.thr[0] * it.factor, C.thr[1] * it.factor, C.thr[2] * it.factor};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) {
        // ---- setup (lm_setup.inc: lm_refine's in host/lm.cpp) ----
        LmParams &x = sh.x;
        lm_rot_to_quat(J.m, x.q);
        lm_quat_to_rot(x.q, x.R);
        for (int k = 0; k < 3; ++k) x.t[k] = J.m[9 + k];
        x.s = J.m[12];
        x.o0 = J.m[13];
        x.o1 = J.m[14];
        x.f0 = J.m[15];
        x.f1 = J.m[16];
        if (use_sampson) lm_sampson_const<V>(x, sh.K);
    }
    __syncthreads();
    LmAcc<NA> acc;
    acc.clear();
    int cnt[3] = {0, 0, 0}; // (this wave's, uniform over its lanes)
    const int ntrip = (it.count + kBlock - 1) / kBlock;
    for (int trip = 0; trip < ntrip; ++trip) {
        const int j = trip * kBlock + threadIdx.x; // row of the item
        bool inl[3] = {false, false, false};
        if (j < it.count) {
            const int i = it.first + j; // (< first + count <= n: a row of the pair)
            const Corr p = load_corr(C, D, i, V == kCal);
            double e0, e1, e2;
            bool flag = false; // (unused: nothing is screened here)
            eval_corr<V>(C, r, p, false, e0, e1, e2, flag);
            inl[0] = e0 < rthr[0];
            inl[1] = e1 < rthr[1];
            inl[2] = e2 < rthr[2];
            if (use_reproj && inl[0]) lm_block_reproj0<V, NA>(D, C, sh.x, i, true, acc);
            if (use_reproj && inl[1]) lm_block_reproj1<V, NA>(D, C, sh.x, i, true, acc);
            if (use_sampson && inl[2]) lm_block_sampson<V, NA>(D, C, sh.x, sh.K, w_sampson, i, true, acc);
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) cnt[t] += __popcll(__ballot(inl[t]));
    }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < 3; ++t) s_cnt[t][wave] = cnt[t];
    }
    lm_reduce<NA>(acc, sh, sh.red[0]); // (its barriers order s_cnt too)
    // the partial record, NA layout -> full layout: one entry per thread
    InfoPartial &o = part[blockIdx.x];
    if (threadIdx.x < kInfoRed) {
        const int q = threadIdx.x;
        double v = 0.0;
        if (q < kInfoPack) {
            // (a, b) of the full packed triangle
            int a = 0, rest = q;
            while (rest >= kInfoN - a) rest -= kInfoN - a, ++a;
            const int b = a + rest;
            if (b < NA) v = sh.red[0][lm_up(a, b, NA)];
        } else if (q < kInfoPack + kInfoN) {
            const int a = q - kInfoPack;
            if (a < NA) v = sh.red[0][kPack + a];
        } else {
            v = sh.red[0][kPack + NA];
        }
        o.v[q] = v;
    } else if (threadIdx.x < kInfoRed + 3) {
        const int t = threadIdx.x - kInfoRed;
        int k = 0;
        for (int w = 0; w < kBlock / 64; ++w) k += s_cnt[t][w];
        o.count[t] = k;
    } else if (threadIdx.x == kInfoRed + 3) {
        o.pad = 0;
    }
}

__global__ void __launch_bounds__(kInfoFinishBlock)
    information_finish_kernel(int variant, const InfoJob *__restrict__ jobs, const InfoPartial *__restrict__ part,
                              double *__restrict__ H, double *__restrict__ g, double *__restrict__ cost,
                              double *__restrict__ cov, InfoRecord *__restrict__ recs) {
    __shared__ double s_red[kInfoRed];
    __shared__ double s_cov[kInfoN * kInfoN];
    __shared__ int s_count[3];
    const InfoJob &J = jobs[blockIdx.x];
    const int q = threadIdx.x;
    if (q < kInfoRed) {
        double v = 0.0;
        for (int k = 0; k < J.nitems; ++k) v += part[J.first_item + k].v[q]; // (item order)
        s_red[q] = v;
    } else if (q < kInfoRed + 3) {
        int c = 0;
        for (int k = 0; k < J.nitems; ++k) c += part[J.first_item + k].count[q - kInfoRed];
        s_count[q - kInfoRed] = c;
    }
    for (int k = q; k < kInfoN * kInfoN; k += kInfoFinishBlock) s_cov[k] = 0.0;
    __syncthreads();
    if (q == 0) {
        InfoRecord rec;
        const int n0 = J.use_reproj ? s_count[0] : 0, n1 = J.use_reproj ? s_count[1] : 0;
        const int n2 = J.use_sampson ? s_count[2] : 0;
        info_columns(variant, n0, n1, n2, J.use_shift, rec.col, &rec.status, &rec.rows);
        for (int t = 0; t < 3; ++t) rec.counts[t] = s_count[t];
        if (rec.status == 0) {
            // nothing evaluated: every sum is an empty one already; pd -1
            for (int k = 0; k < kInfoRed; ++k) s_red[k] = 0.0;
            rec.pd = -1;
        } else {
            info_mask(s_red, s_red + kInfoPack, rec.col);
            rec.pd = info_covariance(s_red, rec.col, s_cov);
        }
        recs[blockIdx.x] = rec;
    }
    __syncthreads();
    const int64_t row = J.out_row;
    if (H && q < kInfoPack) H[row * kInfoPack + q] = s_red[q];
    if (g && q < kInfoN) g[row * kInfoN + q] = s_red[kInfoPack + q];
    if (cost && q == 0) cost[row] = s_red[kInfoPack + kInfoN];
    if (cov)
        for (int k = q; k < kInfoN * kInfoN; k += kInfoFinishBlock) cov[row * (kInfoN * kInfoN) + k] = s_cov[k];
}

} // namespace

hipError_t launch_information(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                              const ResidItem *items, int nitems, const ScoreRec *recs, const InfoJob *jobs,
                              InfoPartial *part) {
    if (nitems <= 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        information_kernel<decltype(V)::value><<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, jobs, part);
        return hipGetLastError();
    });
}

hipError_t launch_information_finish(hipStream_t s, int variant, const InfoJob *jobs, int nentries,
                                     const InfoPartial *part, double *H, double *g, double *cost, double *cov,
                                     InfoRecord *recs) {
    if (nentries <= 0) return hipSuccess;
    information_finish_kernel<<<nentries, kInfoFinishBlock, 0, s>>>(variant, jobs, part, H, g, cost, cov, recs);
    return hipGetLastError();
}

} // namespace mp
