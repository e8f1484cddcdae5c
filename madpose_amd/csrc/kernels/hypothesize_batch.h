// The estimator's minimal-solver stages over explicit samples of many resident pairs
// (mp_hypothesize_batch; host side: engine.cpp hypothesize_batch).  Included from
// kernels.hip after the estimator's kernels.
//
// The pairs of a run stay on the device (host/refine_plan.h); their PairData / PairConst
// records sit in device arrays, and a work item (HypItem, host/hypothesis_plan.h) names its
// pair and `count` consecutive entries of the slab's list of one solver type.  A workgroup
// reads its item -- uniform, so the pair's records go through the scalar cache -- and runs
// the estimator's own stage body on the item as if it were a launch of its own: the list
// is the item's part of the slab's list, nlist its count, and the stage's workspace
// (indexed by list position) starts at the item's first entry.  The bodies are the
// estimator's (md_exact_body, pt_roots5_group_body, pt_tail5_group_body, pt_pencil6_body,
// pt_tail6_group_body, pt_roots7_body, pt_tail7_group_body, pt_compact_body): one text for
// both, so a sample's models are the estimator's.  No arithmetic of a body depends on
// nlist or on the other samples of its workgroup (tests/test_switch_invariance_gpu.py
// holds the estimator to that), so the cut into items does not show in the results.
//
// A stage whose single-pair launch spreads a sample over several workgroups (the tails,
// root-major over the list: group = root * nlist + sample; the compaction) gives an item
// kVb workgroups, the number its cap-sized launch would have; workgroup blockIdx.x runs
// block blockIdx.x % kVb of item blockIdx.x / kVb.  Blocks past a short item's groups
// leave at once (their root index is past the last root).
//
// Models only: no score record is written (put_model<false>); select_batch prepares its
// records on the host.
#pragma once
#include "../host/hypothesis_plan.h"

namespace mp {
namespace {

template <int V> struct HypStage {
    using T = PtTraits<V>;
    static constexpr int kMdR = V == kSF ? 2 : 4; // md_lanes' defaults
    static constexpr int kMdCap = 64 / kMdR;
    static constexpr int kPtCap = V == kTF ? 64 : kGrpPerWg;
    static constexpr int kTailG = V == kSF ? kGrp : kTail; // lanes per (root, sample)
    static constexpr int kTailVb = (kPtCap * T::kRoots * kTailG + 63) / 64;
    static constexpr int kCompactG = T::kPosesPerRoot * T::kRoots <= 4 ? 4 : 32;
    static constexpr int kCompactVb = (kPtCap * kCompactG + 63) / 64;
    static_assert(kMdCap == hyp_md_cap(V) && kPtCap == hyp_pt_cap(V), "the plan's caps are the kernels'");
    static_assert(kS5 == kGrpPerWg, "5pt groups per workgroup");
};

// MD samples: md_exact_body on the item (one workgroup: kMdCap samples)
template <int V>
__global__ void __launch_bounds__(64) hyp_md_kernel(const PairData *__restrict__ Ds, const PairConst *__restrict__ Cs,
                                                    const HypItem *__restrict__ items, const int *list,
                                                    const int *samples, Model *models, int *counts, int maxm) {
    const HypItem it = items[blockIdx.x];
    md_exact_body<V, HypStage<V>::kMdR, false>(0, Ds[it.pair], Cs[it.pair], list + it.first, it.count, samples, models,
                                               nullptr, counts, maxm);
}

// root stages (one workgroup per item)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3)))
hyp_roots5_kernel(const PairData *__restrict__ Ds, const PairConst *__restrict__ Cs, const HypItem *__restrict__ items,
                  const int *list, const int *samples, double *cand, int *ncand) {
    const HypItem it = items[blockIdx.x];
    pt_roots5_group_body(0, Ds[it.pair], Cs[it.pair], list + it.first, it.count, samples,
                         cand + (size_t)it.first * kCandStride, ncand + it.first, kCandStride);
}

__global__ void __launch_bounds__(64) hyp_pencil6_kernel(const PairData *__restrict__ Ds,
                                                         const HypItem *__restrict__ items, const int *list,
                                                         const int *samples, double *cand, double *pen) {
    const HypItem it = items[blockIdx.x];
    pt_pencil6_body(0, Ds[it.pair], list + it.first, it.count, samples, cand + (size_t)it.first * kCandStride,
                    kCandStride, pen + (size_t)it.first * kPenStride);
}

__global__ void __launch_bounds__(64) hyp_roots7_kernel(const PairData *__restrict__ Ds,
                                                        const HypItem *__restrict__ items, const int *list,
                                                        const int *samples, double *cand, int *ncand) {
    const HypItem it = items[blockIdx.x];
    pt_roots7_body(0, Ds[it.pair], list + it.first, it.count, samples, cand + (size_t)it.first * kCandStride,
                   ncand + it.first);
}

// tails: kTailVb workgroups per item
template <int V>
__global__ void __launch_bounds__(64) hyp_tail_kernel(const PairData *__restrict__ Ds, const PairConst *__restrict__ Cs,
                                                      const HypItem *__restrict__ items, const int *list,
                                                      const int *samples, const double *cand, const int *ncand,
                                                      Model *slots, int *valid) {
    constexpr int kVb = HypStage<V>::kTailVb;
    const HypItem it = items[blockIdx.x / kVb];
    const int vb = blockIdx.x % kVb;
    const PairData &D = Ds[it.pair];
    const PairConst &C = Cs[it.pair];
    const int *l = list + it.first;
    const double *cd = cand + (size_t)it.first * kCandStride;
    const int *nc = ncand + it.first;
    Model *sl = slots + (size_t)it.first * kSlotStride;
    int *va = valid + (size_t)it.first * kSlotStride;
    if constexpr (V == kCal)
        pt_tail5_group_body(vb, D, C, l, it.count, cd, nc, samples, sl, va);
    else if constexpr (V == kSF)
        pt_tail6_group_body(vb, D, C, l, it.count, cd, nc, samples, sl, va);
    else
        pt_tail7_group_body<8>(vb, D, C, l, it.count, cd, nc, samples, sl, va);
}

// compaction: kCompactVb workgroups per item
template <int V>
__global__ void __launch_bounds__(64) hyp_compact_kernel(const PairConst *__restrict__ Cs,
                                                         const HypItem *__restrict__ items, const int *list,
                                                         const int *ncand, const Model *slots, const int *valid,
                                                         Model *models, int *counts, int maxm) {
    constexpr int kVb = HypStage<V>::kCompactVb;
    const HypItem it = items[blockIdx.x / kVb];
    pt_compact_body<V, false>(blockIdx.x % kVb, Cs[it.pair], list + it.first, it.count, ncand + it.first,
                              slots + (size_t)it.first * kSlotStride, valid + (size_t)it.first * kSlotStride, models,
                              nullptr, counts, maxm);
}

// ---- the hand-over to select (mp_candidates_set): only the models that exist leave ----
// After a slab's solve launches, sample b holds counts[b] models at models[b * maxm ..].
// hyp_scan_counts: base[b] = the models of the samples before b (exclusive scan in sample
// order), base[ns] their total; one workgroup, thread t owns a contiguous run of samples.  A
// count outside 0 .. maxm counts as 0 here and in the gather (the host refuses such a slab).
constexpr int kScanThreads = 1024;
__global__ void __launch_bounds__(kScanThreads)
hyp_scan_counts(const int *__restrict__ counts, int ns, int maxm, int *__restrict__ base) {
    __shared__ int part[kScanThreads];
    const int t = threadIdx.x;
    const int per = (ns + kScanThreads - 1) / kScanThreads;
    const int b0 = min(ns, t * per), b1 = min(ns, b0 + per);
    auto count_of = [&](int b) {
        const int c = counts[b];
        return c < 0 || c > maxm ? 0 : c;
    };
    int sum = 0;
    for (int b = b0; b < b1; ++b) sum += count_of(b);
    part[t] = sum;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const int add = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int run = part[t] - sum;
    for (int b = b0; b < b1; ++b) {
        base[b] = run;
        run += count_of(b);
    }
    if (t == kScanThreads - 1) base[ns] = part[t];
}

// hyp_gather_models: a wave per sample copies its counts[b] models (17 doubles each,
// contiguous from slot 0) to compact[base[b] ..], a lane per double, and tags each with
// (slab position, slot).  Reads stay inside the sample's maxm slots (count <= maxm), writes
// below base[ns] <= ns * maxm, the size of compact and tags.
constexpr int kGatherWaves = 4;
__global__ void __launch_bounds__(64 * kGatherWaves)
hyp_gather_models(const Model *__restrict__ models, const int *__restrict__ counts, const int *__restrict__ base,
                  int ns, int maxm, Model *__restrict__ compact, int2 *__restrict__ tags) {
    const int b = blockIdx.x * kGatherWaves + threadIdx.x / 64;
    const int lane = threadIdx.x % 64;
    if (b >= ns) return;
    const int c = counts[b];
    if (c <= 0 || c > maxm) return;
    constexpr int kD = (int)(sizeof(Model) / sizeof(double));
    const double *src = reinterpret_cast<const double *>(models + (size_t)b * maxm);
    double *dst = reinterpret_cast<double *>(compact + base[b]);
    for (int i = lane; i < c * kD; i += 64) dst[i] = src[i];
    if (lane < c) tags[base[b] + lane] = make_int2(b, lane);
}

} // namespace

hipError_t launch_hyp_compact(hipStream_t s, int variant, const Model *models, const int *counts, int ns, int *base,
                              Model *compact, int *tags) {
    if (ns < 0 || ns > kHypSlabSamplesMax) return hipErrorInvalidValue;
    if (ns == 0) return hipSuccess;
    const int maxm = max_models(variant);
    hyp_scan_counts<<<1, kScanThreads, 0, s>>>(counts, ns, maxm, base);
    hyp_gather_models<<<(ns + kGatherWaves - 1) / kGatherWaves, 64 * kGatherWaves, 0, s>>>(
        models, counts, base, ns, maxm, compact, reinterpret_cast<int2 *>(tags));
    return hipGetLastError();
}

hipError_t launch_hyp_solve(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                            const HypItem *md_items, int nmd_items, const int *md_list, const HypItem *pt_items,
                            int npt_items, const int *pt_list, int npt, const int *samples, const PtWorkspace &W,
                            Model *models, int *counts) {
    if (nmd_items < 0 || npt_items < 0 || npt < 0) return hipErrorInvalidValue;
    return by_variant(variant, [&](auto V) {
        constexpr int v = decltype(V)::value;
        using H = HypStage<v>;
        const int maxm = max_models(v);
        if (nmd_items > 0)
            hyp_md_kernel<v><<<nmd_items, 64, 0, s>>>(Ds, Cs, md_items, md_list, samples, models, counts, maxm);
        if (npt_items > 0) {
            if constexpr (v == kCal) {
                hyp_roots5_kernel<<<npt_items, 64, 0, s>>>(Ds, Cs, pt_items, pt_list, samples, W.cand, W.ncand);
            } else if constexpr (v == kSF) {
                // the pencils per item; the deflation and the QR read only the pencils and run
                // over the slab's point samples as they do over a batch's (launch_sf_eig)
                hyp_pencil6_kernel<<<npt_items, 64, 0, s>>>(Ds, pt_items, pt_list, samples, W.cand, W.pen);
                pt_defl6_grp_kernel<<<(npt + 3) / 4, 64, 0, s>>>(W.pen, npt);
                const int spw = eig_spw(npt);
                if (spw == 1)
                    pt_eig6_reg_kernel<true><<<npt, 64, 0, s>>>(W.pen, npt, 1, W.cand, W.ncand, kCandStride);
                else
                    pt_eig6_reg_kernel<false>
                        <<<(npt + spw - 1) / spw, 64, 0, s>>>(W.pen, npt, spw, W.cand, W.ncand, kCandStride);
            } else {
                hyp_roots7_kernel<<<npt_items, 64, 0, s>>>(Ds, pt_items, pt_list, samples, W.cand, W.ncand);
            }
            hyp_tail_kernel<v><<<npt_items * H::kTailVb, 64, 0, s>>>(Ds, Cs, pt_items, pt_list, samples, W.cand,
                                                                    W.ncand, W.slots, W.valid);
            hyp_compact_kernel<v><<<npt_items * H::kCompactVb, 64, 0, s>>>(Cs, pt_items, pt_list, W.ncand, W.slots,
                                                                          W.valid, models, counts, maxm);
        }
        return hipGetLastError();
    });
}

} // namespace mp
