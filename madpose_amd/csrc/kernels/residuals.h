// The three squared errors and the inlier mask of every correspondence under given models
// (mp_residuals_set; host side: engine.cpp residuals_set, plan: host/residuals_plan.h).
// Included from kernels.hip after inlier_mass.h.
//
//  residuals<V, ERR>  one workgroup per item (ResidItem: up to kResidItemRows consecutive rows
//                   of one entry), one row per lane per trip.  The errors are the sweep
//                   kernels': the same load_corr and eval_corr<V> call on the entry's record,
//                   no score-type gating -- the error bits refine_sweep_kernel and
//                   inlier_mass_kernel compare.  Row i of the item's entry gets the mask byte
//                   (bit t: err_t < thr_t * factor, the product formed once in double as
//                   refine_sweep_relaxed_kernel forms thr * relax; a NaN error compares false;
//                   bits 3 .. 7 zero) by an ordinary byte store -- entries start at arbitrary
//                   byte offsets, so nothing is widened across rows -- and, with ERR, its
//                   three errors as coalesced double stores into the term-major (3, stride)
//                   array.  The item's three inlier counts are wave ballots' popcounts, kept
//                   per wave over the trips (a wave-uniform integer) and added over the four
//                   waves through LDS once at the end: integer sums, order-free.  No atomics,
//                   no floating-point reduction, no list written; the set's list buffers are
//                   not touched.  Every store of an item lands in rows row .. row + count - 1
//                   of the outputs: inside its entry's rows.
//
// LDS: 48 bytes (3 x 4 ints), written once per wave by lane 0 and read by one thread: no bank
// conflict to speak of and no limit on occupancy, which the errors' registers set.
#pragma once

namespace mp {
namespace {

template <int V, bool ERR>
__global__ void __launch_bounds__(kBlock) residuals_kernel(const PairData *Ds, const PairConst *Cs,
                                                           const ResidItem *items, const ScoreRec *recs,
                                                           unsigned char *mask, double *errors, int64_t stride,
                                                           ResidCount *out) {
    const ResidItem it = items[blockIdx.x];
    const PairData &D = Ds[it.pair];
    const PairConst &C = Cs[it.pair];
    const ScoreRec r = recs[it.rec];
    const double rthr[3] = {C.thr[0] * it.factor, C.thr[1] * it.factor, C.thr[2] * it.factor};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ int s_cnt[3][kBlock / 64];
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
            // (j < count: row + j is one of the item's rows of the outputs)
            mask[it.row + j] = (unsigned char)((inl[0] ? 1 : 0) | (inl[1] ? 2 : 0) | (inl[2] ? 4 : 0));
            if (ERR) {
                errors[it.row + j] = e0;
                errors[stride + it.row + j] = e1;
                errors[2 * stride + it.row + j] = e2;
            }
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) cnt[t] += __popcll(__ballot(inl[t]));
    }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < 3; ++t) s_cnt[t][wave] = cnt[t];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ResidCount o;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            int k = 0;
            for (int w = 0; w < kBlock / 64; ++w) k += s_cnt[t][w];
            o.count[t] = k;
        }
        o.pad = 0;
        out[blockIdx.x] = o;
    }
}

} // namespace

hipError_t launch_residuals(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                            const ResidItem *items, int nitems, const ScoreRec *recs, unsigned char *mask,
                            double *errors, int64_t stride, ResidCount *out) {
    if (nitems <= 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        if (errors)
            residuals_kernel<decltype(V)::value, true>
                <<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, mask, errors, stride, out);
        else
            residuals_kernel<decltype(V)::value, false>
                <<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, mask, nullptr, 0, out);
        return hipGetLastError();
    });
}

} // namespace mp
