// ransac's results in the caller's device arrays (mp_ransac_out_set; host side: engine.cpp
// RansacOutStage, plan: host/residuals_plan.h).  Included from kernels.hip after residuals.h.
//
//  ransac_out<V, ERR>  one workgroup per item (ResidItem: up to kResidItemRows consecutive rows
//                   of one selected pair), one row per lane per trip.
//                   An evaluate item (rec >= 0) holds the pair's winner: the record is the one
//                   prepare_score_rec made of the problem-unit model the returned lists were
//                   swept from, and the errors are the sweep's -- the same load_corr and
//                   eval_corr<V> call, no score-type gating -- compared as the sweep compares
//                   them, err_t < C.thr[t].  So bit t of a row is set iff the row is in list t.
//                   A fill item (rec == kResidFill: a pair without a winner) reads nothing of the
//                   pair: mask 0 and a quiet NaN in the three errors.
//                   Stores per row: the mask byte by an ordinary byte store (pairs start at
//                   arbitrary byte offsets, so nothing is widened across rows) and, with ERR, the
//                   three errors as coalesced double stores into the term-major (3, stride)
//                   array.  The item's three counts are wave ballots' popcounts, kept per wave
//                   over the trips and added over the four waves through LDS once at the end:
//                   integer sums, order-free.  No atomics, no floating-point reduction, no list
//                   written; the set's list buffers are not read.  Every store of an item lands
//                   in rows row .. row + count - 1 of the outputs: inside its pair's rows.
//  ransac_out_pairs   one lane per selected pair: its uploaded RansacOutPair to row j of the
//                   caller's models (17 doubles), index and counts (3 ints), each array nullable.
//
// LDS: 48 bytes (3 x 4 ints), written once per wave by lane 0 and read by one thread.
#pragma once

namespace mp {
namespace {

template <int V, bool ERR>
__global__ void __launch_bounds__(kBlock) ransac_out_kernel(const PairData *Ds, const PairConst *Cs,
                                                            const ResidItem *items, const ScoreRec *recs,
                                                            unsigned char *mask, double *errors, int64_t stride,
                                                            ResidCount *out) {
    const ResidItem it = items[blockIdx.x];
    if (it.rec == kResidFill) { // (uniform over the workgroup: no barrier is skipped by a part of it)
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        for (int j = threadIdx.x; j < it.count; j += kBlock) {
            mask[it.row + j] = 0;
            if (ERR) {
                errors[it.row + j] = qnan;
                errors[stride + it.row + j] = qnan;
                errors[2 * stride + it.row + j] = qnan;
            }
        }
        if (threadIdx.x == 0) {
            ResidCount o;
            o.count[0] = o.count[1] = o.count[2] = o.pad = 0;
            out[blockIdx.x] = o;
        }
        return;
    }
    const PairData &D = Ds[it.pair];
    const PairConst &C = Cs[it.pair];
    const ScoreRec r = recs[it.rec];
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
            inl[0] = e0 < C.thr[0];
            inl[1] = e1 < C.thr[1];
            inl[2] = e2 < C.thr[2];
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

__global__ void __launch_bounds__(kBlock) ransac_out_pairs_kernel(const RansacOutPair *pairs, int npairs,
                                                                  double *models, int *index, int *counts) {
    const int j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= npairs) return;
    const RansacOutPair p = pairs[j];
    if (models) {
#pragma unroll
        for (int i = 0; i < 17; ++i) models[(int64_t)17 * j + i] = p.model[i];
    }
    if (index) index[j] = p.index;
    if (counts) {
#pragma unroll
        for (int t = 0; t < 3; ++t) counts[(int64_t)3 * j + t] = p.count[t];
    }
}

} // namespace

hipError_t launch_ransac_out(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                             const ResidItem *items, int nitems, const ScoreRec *recs, unsigned char *mask,
                             double *errors, int64_t stride, ResidCount *out) {
    if (nitems <= 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        if (errors)
            ransac_out_kernel<decltype(V)::value, true>
                <<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, mask, errors, stride, out);
        else
            ransac_out_kernel<decltype(V)::value, false>
                <<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, mask, nullptr, 0, out);
        return hipGetLastError();
    });
}

hipError_t launch_ransac_out_pairs(hipStream_t s, const RansacOutPair *pairs, int npairs, double *models, int *index,
                                   int *counts) {
    if (npairs <= 0) return hipSuccess;
    ransac_out_pairs_kernel<<<(npairs + kBlock - 1) / kBlock, kBlock, 0, s>>>(pairs, npairs, models, index, counts);
    return hipGetLastError();
}

} // namespace mp
