// The device sampler of mp_draw_set / mp_ransac_set (host side: engine.cpp draw_slab).
// Included from kernels.hip.
//
// One lane per sample; a workgroup reads its item (DrawItem, include/mp_draw.h; planned by
// host/candidates_plan.h draw_items), which names a pair of the set and up to
// kDrawItemSamples consecutive samples of it, as the hyp_* kernels' items do.  The lane runs
// draw_sample -- the function the host runs for the types -- and stores the sample's 8 index
// slots (two 16-byte vector stores) and its type.  The pair's size comes from a per-pair int
// array; no correspondence data is read.  Every index written is < n by construction
// (draw_sample), and the lane writes only position out + lane < out + count of the launch's
// arrays, which the host sized for its items.
#pragma once
#include "../include/mp_draw.h"

namespace mp {
namespace {

template <int V>
__global__ void __launch_bounds__(kDrawItemSamples)
draw_samples(const DrawItem *__restrict__ items, const int *__restrict__ pair_n, unsigned long long seed,
             int point_share, int *__restrict__ samples, int *__restrict__ types) {
    const DrawItem it = items[blockIdx.x];
    const int lane = threadIdx.x;
    if (lane >= it.count) return;
    int idx[8];
    const int type = draw_sample(pair_n[it.pair], draw_k_md(V), draw_k_pt(V), seed, point_share, (uint32_t)it.pair,
                                 (uint32_t)(it.s0 + lane), idx);
    const size_t at = (size_t)it.out + lane;
    int4 *o = reinterpret_cast<int4 *>(samples + at * kSampleStride);
    o[0] = make_int4(idx[0], idx[1], idx[2], idx[3]);
    o[1] = make_int4(idx[4], idx[5], idx[6], idx[7]);
    types[at] = type;
}

} // namespace

hipError_t launch_draw_samples(hipStream_t s, int variant, const DrawItem *items, int nitems, const int *pair_n,
                               uint64_t seed, int point_share, int *samples, int *types) {
    if (nitems < 0 || point_share < 0 || point_share > kDrawShareMax) return hipErrorInvalidValue;
    if (nitems == 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        draw_samples<decltype(V)::value><<<nitems, kDrawItemSamples, 0, s>>>(items, pair_n, seed, point_share, samples,
                                                                             types);
        return hipGetLastError();
    });
}

} // namespace mp
