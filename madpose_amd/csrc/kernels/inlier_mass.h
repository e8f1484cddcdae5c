// The confidence mass of a model's inlier lists (mp_inlier_mass_set, the weighted stopping rule
// of mp_ransac_weighted_stop_set; host side: engine.cpp mass_run).  Included from kernels.hip
// after refine_batch.h.
//
//  inlier_mass<V>   one workgroup per item (pair, model record): the three squared errors of
//                   every correspondence as refine_sweep_kernel forms them (the same trips,
//                   load_corr and eval_corr<V> call: the error bits of select's winner
//                   sweep, no score-type gating), and per term t the number of rows with
//                   err_t < thr_t and the sum of their quantised weights q_i = c[i + 1] - c[i]
//                   from the pair's table of mp_draw_weights_create (include/mp_draw.h).
//                   An item of a pair that is not weighted takes q_i = 1 and total = n.
//                   Integer sums only: uint32 masses (distinct rows, so mass <= W = c[n] <
//                   2^32) and int counts, reduced in-wave by DPP row sums and across the four
//                   waves in LDS.  Integer addition is associative, so the record does not
//                   depend on the reduction order and a host sum over the same lists gives
//                   the same numbers.  No atomics, no lists written, no floating-point sum.
#pragma once

namespace mp {
namespace {

// Sum over the 64 lanes of a wave (all lanes active), returned uniformly: wave_sum's
// butterflies and row reads on one 32-bit integer (wrapping, as unsigned addition does)
__device__ inline uint32_t wave_sum_u32(uint32_t x) {
    const int v = gsum16((int)x);
    return ((uint32_t)__builtin_amdgcn_readlane(v, 0) + (uint32_t)__builtin_amdgcn_readlane(v, 16)) +
           ((uint32_t)__builtin_amdgcn_readlane(v, 32) + (uint32_t)__builtin_amdgcn_readlane(v, 48));
}

template <int V>
__global__ void __launch_bounds__(kBlock) inlier_mass_kernel(const PairData *Ds, const PairConst *Cs,
                                                             const MassItem *items, const ScoreRec *recs,
                                                             const uint32_t *cum, const int64_t *tab_off,
                                                             MassOut *out) {
    const MassItem it = items[blockIdx.x];
    const PairData &D = Ds[it.pair];
    const PairConst &C = Cs[it.pair];
    const ScoreRec r = recs[blockIdx.x];
    const int n = C.n;
    // the pair's table: n + 1 entries c[0 .. n] at cum + tab_off[pair] (weighted items only;
    // a handle without tables passes null and has no weighted item)
    const uint32_t *c = it.weighted ? cum + tab_off[it.pair] : nullptr;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ uint32_t s_part[6][kBlock / 64];
    uint32_t mass[3] = {0u, 0u, 0u};
    int count[3] = {0, 0, 0};
    const int ntrip = (n + kBlock - 1) / kBlock;
    for (int trip = 0; trip < ntrip; ++trip) {
        const int i = trip * kBlock + threadIdx.x;
        if (i < n) {
            const Corr p = load_corr(C, D, i, V == kCal);
            double e0, e1, e2;
            bool flag = false; // (unused: nothing is screened here)
            eval_corr<V>(C, r, p, false, e0, e1, e2, flag);
            // (i < n: entries i and i + 1 <= n, inside the pair's n + 1 entries)
            const uint32_t q = c ? c[i + 1] - c[i] : 1u;
            const bool inl[3] = {e0 < C.thr[0], e1 < C.thr[1], e2 < C.thr[2]};
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                mass[t] += inl[t] ? q : 0u;
                count[t] += inl[t] ? 1 : 0;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const uint32_t m = wave_sum_u32(mass[t]), k = wave_sum_u32((uint32_t)count[t]);
        if (lane == 0) {
            s_part[t][wave] = m;
            s_part[3 + t][wave] = k;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        MassOut o;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            uint32_t m = 0u, k = 0u;
            for (int w = 0; w < kBlock / 64; ++w) {
                m += s_part[t][w];
                k += s_part[3 + t][w];
            }
            o.mass[t] = m;
            o.count[t] = (int)k;
        }
        // (entry n: the last of the pair's n + 1)
        o.total = c ? c[n] : (uint32_t)n;
        o.pad = 0;
        out[blockIdx.x] = o;
    }
}

} // namespace

hipError_t launch_inlier_mass(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                              const MassItem *items, const ScoreRec *recs, int nitems, const uint32_t *cum,
                              const int64_t *tab_off, MassOut *out) {
    if (nitems <= 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        inlier_mass_kernel<decltype(V)::value><<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, cum, tab_off, out);
        return hipGetLastError();
    });
}

} // namespace mp
