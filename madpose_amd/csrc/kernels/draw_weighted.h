// The confidence-weighted sampler of mp_draw_weights_create / mp_draw_weighted_set /
// mp_ransac_weighted_set (host side: engine.cpp DrawWeights, draw_slab; the rule:
// include/mp_draw.h).  Included from kernels.hip.
//
// draw_weights_table: one workgroup per pair of the set, looping over tiles of
// kDrawTableBlock weights: load (float32 widened exactly, or float64), draw_quantise, a block
// scan (wave scans by shuffles, the four wave sums through LDS) with a running carry, and the
// pair's table c written at cum + off[p] + p (n + 1 entries), its #{q > 0} and W = c[n].  A
// weight draw_quantise refuses puts its row of the set into *bad_row by a vector atomic min
// (the host reads it and raises; that pair's table is then not used).  Pairs not given
// weights, and pairs above kDrawWeightMaxN (which the host refuses before the launch), are
// skipped.  Bounds: a workgroup reads weights[off[p] .. off[p] + n) -- the host checked that
// the array holds off[np - 1] + n[np - 1] = T elements -- and writes cum[off[p] + p .. off[p] +
// p + n], inside the T + np entries the host allocated; pos / total at p < np.
//
// draw_samples_weighted: draw_samples' items and stores.  The item's pair is weighted or not
// for the whole workgroup: an unweighted pair runs draw_sample, today's bytes; a weighted one
// runs draw_sample_weighted on its table, which is first copied to LDS by the workgroup when
// STAGE and its n + 1 entries fit kDrawStageEntries, and read from global memory otherwise
// (the result does not depend on which).  A weighted pair has n <= kDrawWeightMaxN, so the
// table reads stay inside cum_off[pair] .. + n.  Every index written is < n by construction:
// it is draw_cum_find's result (0 .. n - 1) or the fill's loop variable (< n); the lane writes
// only position out + lane < out + count of the launch's arrays, which the host sized for its
// items.
#pragma once
#include "../include/mp_draw_weights.h"

namespace mp {

constexpr int kDrawTableBlock = 256;

namespace {

template <class T>
__global__ void __launch_bounds__(kDrawTableBlock)
draw_weights_table(const T *__restrict__ weights, const int64_t *__restrict__ off, const int *__restrict__ pair_n,
                   const unsigned char *__restrict__ given, uint32_t *__restrict__ cum, int *__restrict__ pos,
                   uint32_t *__restrict__ total, int *bad_row) {
    const int p = blockIdx.x;
    if (given && !given[p]) return;
    const int n = pair_n[p];
    if (n > kDrawWeightMaxN) return;
    const int64_t o = off[p];
    uint32_t *c = cum + o + p;
    __shared__ uint32_t wave_sum[kDrawTableBlock / 64], wave_pos[kDrawTableBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t carry = 0, npos = 0; // (the same in every thread)
    if (threadIdx.x == 0) c[0] = 0;
    for (int base = 0; base < n; base += kDrawTableBlock) {
        const int i = base + (int)threadIdx.x;
        uint32_t q = 0;
        if (i < n && !draw_quantise((double)weights[o + i], &q)) atomicMin(bad_row, (int)(o + i));
        uint32_t x = q; // the wave's inclusive scan
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        const unsigned long long m = __ballot(q > 0);
        if (lane == 63) {
            wave_sum[wave] = x;
            wave_pos[wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        uint32_t before = carry;
        for (int k = 0; k < kDrawTableBlock / 64; ++k) {
            if (k < wave) before += wave_sum[k];
            carry += wave_sum[k];
            npos += wave_pos[k];
        }
        if (i < n) c[i + 1] = before + x;
        __syncthreads(); // (the wave sums are rewritten by the next tile)
    }
    if (threadIdx.x == 0) {
        pos[p] = (int)npos;
        total[p] = carry;
    }
}

template <int V, bool STAGE>
__global__ void __launch_bounds__(kDrawItemSamples)
draw_samples_weighted(const DrawItem *__restrict__ items, const int *__restrict__ pair_n,
                      const uint32_t *__restrict__ cum, const int64_t *__restrict__ cum_off,
                      const unsigned char *__restrict__ weighted, unsigned long long seed, int point_share,
                      int *__restrict__ samples, int *__restrict__ types) {
    __shared__ uint32_t tab[STAGE ? kDrawStageEntries : 1];
    const DrawItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    const int n = pair_n[it.pair];
    int idx[8];
    int type;
    if (!weighted[it.pair]) {
        if (lane >= it.count) return;
        type = draw_sample(n, draw_k_md(V), draw_k_pt(V), seed, point_share, (uint32_t)it.pair,
                           (uint32_t)(it.s0 + lane), idx);
    } else {
        const uint32_t *c = cum + cum_off[it.pair];
        if (STAGE && n + 1 <= kDrawStageEntries) { // (the same for the whole workgroup)
            for (int i = lane; i <= n; i += kDrawItemSamples) tab[i] = c[i];
            __syncthreads();
            c = tab;
        }
        if (lane >= it.count) return;
        type = draw_sample_weighted(n, draw_k_md(V), draw_k_pt(V), seed, point_share, (uint32_t)it.pair,
                                    (uint32_t)(it.s0 + lane), c, idx);
    }
    const size_t at = (size_t)it.out + lane;
    int4 *o = reinterpret_cast<int4 *>(samples + at * kSampleStride);
    o[0] = make_int4(idx[0], idx[1], idx[2], idx[3]);
    o[1] = make_int4(idx[4], idx[5], idx[6], idx[7]);
    types[at] = type;
}

} // namespace

hipError_t launch_draw_weights_table(hipStream_t s, const void *weights, int dtype, const int64_t *off,
                                     const int *pair_n, const unsigned char *given, int num_pairs, uint32_t *cum,
                                     int *pos, uint32_t *total, int *bad_row) {
    if (num_pairs < 0 || (dtype != 0 && dtype != 1)) return hipErrorInvalidValue;
    if (num_pairs == 0) return hipSuccess;
    if (dtype == 0)
        draw_weights_table<float><<<num_pairs, kDrawTableBlock, 0, s>>>(static_cast<const float *>(weights), off, pair_n,
                                                                       given, cum, pos, total, bad_row);
    else
        draw_weights_table<double><<<num_pairs, kDrawTableBlock, 0, s>>>(static_cast<const double *>(weights), off,
                                                                        pair_n, given, cum, pos, total, bad_row);
    return hipGetLastError();
}

hipError_t launch_draw_samples_weighted(hipStream_t s, int variant, const DrawItem *items, int nitems,
                                        const int *pair_n, const uint32_t *cum, const int64_t *cum_off,
                                        const unsigned char *weighted, bool stage, uint64_t seed, int point_share,
                                        int *samples, int *types) {
    if (nitems < 0 || point_share < 0 || point_share > kDrawShareMax) return hipErrorInvalidValue;
    if (nitems == 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        constexpr int v = decltype(V)::value;
        if (stage)
            draw_samples_weighted<v, true><<<nitems, kDrawItemSamples, 0, s>>>(items, pair_n, cum, cum_off, weighted,
                                                                               seed, point_share, samples, types);
        else
            draw_samples_weighted<v, false><<<nitems, kDrawItemSamples, 0, s>>>(items, pair_n, cum, cum_off, weighted,
                                                                                seed, point_share, samples, types);
        return hipGetLastError();
    });
}

} // namespace mp
