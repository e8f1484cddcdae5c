// Least-squares fits on random subsets of a model's inliers, many entries per launch
// (mp_lsq_fit_set; host side: engine.cpp lsq_fit_run).  Included from kernels.hip after
// refine_batch.h.  A launch takes entries (LsqEntry): an entry names its pair, has its own
// score record and owns a slice of the call's workspace, so a pair may occur in several entries
// of one launch; the pair's two refine_list buffers are never touched.
//
//  lsq_sweep<V>   one workgroup per entry: refine_sweep_relaxed_kernel's pass with the entry's
//                 own factor.  The MSAC sum in refine_sweep_kernel's accumulation and reduction
//                 order (the bits of score_models), the three tight counts err < thr (no tight
//                 lists), and the three wide ascending lists err < thr * factor (one double
//                 product, rounded once: factor 1 gives the tight lists) written to the entry's
//                 slice by ballot + popcount ranks.  No atomics.
//  lsq_subset     one workgroup per entry: the subset of include/mp_subset.h of the entry's
//                 wide lists.  k by the shared size rule; M <= k copies the lists.  Otherwise a
//                 radix select over the masked 64-bit key, most significant byte first: eight
//                 passes, each a 256-bin histogram in LDS (integer LDS atomics: a count does
//                 not depend on their order) of the elements that match the prefix so far, and
//                 a scan that picks the byte of the k-th smallest key.  That leaves the k-th
//                 key K and the number of elements with key K to take; those are the first in
//                 (t, i) order, which is list order.  The last pass walks the lists in that
//                 order and writes the chosen elements by ballot + popcount ranks.  Integer
//                 only; the keys are recomputed per pass (no scratch, no global atomics).
#pragma once

#include "../include/mp_subset.h"

namespace mp {
namespace {

static_assert(kBlock == 256, "lsq_subset_kernel: one histogram bin per thread");

template <int V>
__global__ void __launch_bounds__(kBlock) lsq_sweep_kernel(const PairData *Ds, const PairConst *Cs,
                                                           const LsqEntry *entries, const ScoreRec *recs, int *ws,
                                                           LsqOut *out) {
    const LsqEntry it = entries[blockIdx.x];
    const PairData &D = Ds[it.pair];
    const PairConst &C = Cs[it.pair];
    const ScoreRec r = recs[blockIdx.x];
    const int n = C.n;
    int *lst = ws + it.ws_off; // wide list t at lst + t n (it.stride == n)
    const double rthr[3] = {C.thr[0] * it.factor, C.thr[1] * it.factor, C.thr[2] * it.factor};
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
        int rank[3];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const unsigned long long b = __ballot(inl[q][t]);
                if (q == 1) rank[t] = __popcll(b & ((1ull << lane) - 1ull));
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
                // (base + before + rank < the wide inliers so far <= i < n: inside list t)
                if (q == 1 && inl[1][t]) lst[(int64_t)t * n + base[1][t] + before + rank[t]] = i;
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
        LsqOut &o = out[blockIdx.x]; // (sub and k are lsq_subset_kernel's)
        o.score = s;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            o.tight[t] = base[0][t];
            o.wide[t] = base[1][t];
        }
    }
}

__global__ void __launch_bounds__(kBlock) lsq_subset_kernel(const LsqEntry *entries, int *ws, LsqOut *out, int v,
                                                            int mu, int nu, uint64_t seed, uint64_t key_mask) {
    const LsqEntry e = entries[blockIdx.x];
    LsqOut &o = out[blockIdx.x];
    const int M[3] = {o.wide[0], o.wide[1], o.wide[2]};
    const int total = M[0] + M[1] + M[2]; // (<= 3 n < 2^30)
    const int64_t stride = e.stride;
    const int *src = ws + e.ws_off;
    int *dst = ws + e.ws_off + 3 * stride;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int64_t k64;
    bool ok = true;
    if (e.rule < 0) {
        k64 = e.k < 0 ? 0 : (e.k > total ? total : e.k);
    } else {
        ok = subset_size(e.rule, e.stype, v, mu, nu, M, &k64);
    }
    // (uniform over the workgroup from here on: every branch below depends on the entry alone)
    if (!ok) {
        if (tid == 0) {
            o.sub[0] = o.sub[1] = o.sub[2] = 0;
            o.k = -1;
        }
        return;
    }
    const int k = (int)k64; // (<= total)
    if (total <= k) {       // everything: the lists as they are
        for (int t = 0; t < 3; ++t)
            for (int j = tid; j < M[t]; j += kBlock) dst[t * stride + j] = src[t * stride + j];
        if (tid == 0) {
            o.sub[0] = M[0];
            o.sub[1] = M[1];
            o.sub[2] = M[2];
            o.k = k;
        }
        return;
    }
    if (k == 0) {
        if (tid == 0) {
            o.sub[0] = o.sub[1] = o.sub[2] = 0;
            o.k = 0;
        }
        return;
    }
    // element g of the concatenated lists (g < total): its type, index and masked key
    auto element = [&](int g, int &t, int &i) {
        t = (g >= M[0]) + (g >= M[0] + M[1]);
        const int j = g - (t > 0 ? M[0] : 0) - (t > 1 ? M[1] : 0);
        i = src[t * stride + j];
    };
    auto key_of = [&](int t, int i) {
        return subset_key(seed, (uint32_t)e.pair, e.stream, e.substream, t, (uint32_t)i) & key_mask;
    };

    // ---- the k-th smallest key: 1 <= k < total ----
    __shared__ unsigned hist[256];
    __shared__ int s_wave[kBlock / 64];
    __shared__ uint64_t s_prefix;
    __shared__ int s_rem;
    uint64_t prefix = 0; // the bytes of the k-th key found so far (the rest 0)
    int rem = k;         // its rank among the elements that match the prefix (1-based)
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[tid] = 0u;
        __syncthreads();
        for (int g = tid; g < total; g += kBlock) {
            int t, i;
            element(g, t, i);
            const uint64_t key = key_of(t, i);
            const bool match = pass == 0 || ((key ^ prefix) >> (shift + 8)) == 0;
            if (match) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        // bin tid's count and the counts before it: an inclusive scan inside the wave, the
        // waves' totals through LDS
        const int c = (int)hist[tid];
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int ex = incl - c;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) ex += w < wave ? s_wave[w] : 0;
        // (the matching elements number at least rem >= 1, so exactly one bin holds rank rem)
        if (ex < rem && rem <= ex + c) {
            s_prefix = prefix | ((uint64_t)tid << shift);
            s_rem = rem - ex;
        }
        __syncthreads();
        prefix = s_prefix;
        rem = s_rem;
    }
    // prefix: the k-th key; rem: how many of the elements with that key are taken (the first
    // in list order); everything below it is taken

    // ---- the chosen elements, in list order ----
    __shared__ int s_eq[kBlock / 64], s_sel[kBlock / 64];
    int eq_base = 0; // elements with the k-th key before this trip, over all types
    int z[3] = {0, 0, 0};
    for (int t = 0; t < 3; ++t) {
        const int ntrip = (M[t] + kBlock - 1) / kBlock;
        for (int trip = 0; trip < ntrip; ++trip) {
            const int j = trip * kBlock + tid;
            int i = 0;
            bool lt = false, eq = false;
            if (j < M[t]) {
                i = src[t * stride + j];
                const uint64_t key = key_of(t, i);
                lt = key < prefix;
                eq = key == prefix;
            }
            const unsigned long long be = __ballot(eq);
            if (lane == 0) s_eq[wave] = __popcll(be);
            __syncthreads();
            int eq_before = eq_base + __popcll(be & ((1ull << lane) - 1ull)), eq_total = 0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) {
                const int c = s_eq[w];
                eq_before += w < wave ? c : 0;
                eq_total += c;
            }
            eq_base += eq_total;
            const bool sel = lt || (eq && eq_before < rem);
            const unsigned long long bs = __ballot(sel);
            if (lane == 0) s_sel[wave] = __popcll(bs);
            __syncthreads();
            int before = __popcll(bs & ((1ull << lane) - 1ull)), sel_total = 0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; ++w) {
                const int c = s_sel[w];
                before += w < wave ? c : 0;
                sel_total += c;
            }
            // (z + before < the chosen of type t so far <= j < M[t] <= stride: inside list t)
            if (sel) dst[t * stride + z[t] + before] = i;
            z[t] += sel_total;
            // (s_eq is next written after the next trip's ballot, which every wave reaches only
            // after this trip's second barrier; s_sel after its first barrier)
        }
    }
    if (tid == 0) {
        o.sub[0] = z[0];
        o.sub[1] = z[1];
        o.sub[2] = z[2];
        o.k = k;
    }
}

} // namespace

hipError_t launch_lsq_sweep(hipStream_t s, int variant, const PairData *Ds, const PairConst *Cs,
                            const LsqEntry *entries, const ScoreRec *recs, int nentries, int *ws, LsqOut *out) {
    if (nentries <= 0) return hipSuccess;
    return by_variant(variant, [&](auto V) {
        lsq_sweep_kernel<decltype(V)::value><<<nentries, kBlock, 0, s>>>(Ds, Cs, entries, recs, ws, out);
        return hipGetLastError();
    });
}

hipError_t launch_lsq_subset(hipStream_t s, const LsqEntry *entries, int nentries, int *ws, LsqOut *out, int variant,
                             int mu, int nu, uint64_t seed, uint64_t key_mask) {
    if (nentries <= 0) return hipSuccess;
    lsq_subset_kernel<<<nentries, kBlock, 0, s>>>(entries, ws, out, variant, mu, nu, seed, key_mask);
    return hipGetLastError();
}

} // namespace mp
