// Ranking of candidate models over many resident pairs (mp_select_batch; host side:
// engine.cpp select_batch, host/select_plan.h).  Included from kernels.hip after
// refine_batch.h: the pairs' PairData / PairConst records sit in device arrays as there.
//
//  select_score<V, TILE>  one workgroup per work item = up to TILE consecutive candidates
//                   of one pair.  A lane loads its correspondence once per 256-correspondence
//                   trip and evaluates every model of the item on it exactly as
//                   refine_sweep_kernel does (eval_corr<V>, no score-type gating): the
//                   ungated errors give the three counts err < thr, the same values with
//                   the gated terms replaced by DBL_MAX the MSAC term, accumulated per lane
//                   and reduced as score_models_kernel does.  At TILE = 1, the shipped
//                   size, the scores are score_models_kernel's bit for bit; the larger
//                   sizes exist for the timing record (mp_debug_select_tile) and may
//                   differ from them in the last bits (other fused pairs).  The records
//                   are read at uniform addresses through const __restrict__ pointers
//                   (scalar loads, as lm_pairs_kernel reads its pair records).
//  select_argmin    one wave per pair: GetBestEstimatedModelId's walk (start at DBL_MAX,
//                   strict <, so the first of equal scores wins and NaN / inf never do)
//                   over the pair's scores -- each lane over its strided candidates in
//                   ascending order, then a lexicographic (score, index) reduction in
//                   which a lane without a winner loses to any lane with one.
//  select_argmin_seeded  the same walk started from a per-pair prior score.
#pragma once

namespace mp {
namespace {

// sum of an int over the 64 lanes of a wave (all lanes active), returned uniformly
__device__ inline int wave_sum_int(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The evaluation of model M of the item on the lane's correspondence, as plain text and
// not a lambda or a function: the scores are pinned to score_models_kernel's bits, and a
// body that reaches the optimiser in another shape can come out with other fused pairs
// (DESIGN.md 2.1, 2.2).
#define MP_SELECT_MODEL(M)                                                                                            \
    if (TILE > (M) && (M) < it.count) {                                                                               \
        const ScoreRec &r = rv[TILE > (M) ? (M) : 0];                                                                 \
        double e0, e1, e2;                                                                                            \
        bool flag = false; /* (unused: nothing is screened here) */                                                   \
        eval_corr<V>(C, r, p, false, e0, e1, e2, flag);                                                               \
        c0[TILE > (M) ? (M) : 0] += e0 < C.thr[0] ? 1 : 0;                                                            \
        c1[TILE > (M) ? (M) : 0] += e1 < C.thr[1] ? 1 : 0;                                                            \
        c2[TILE > (M) ? (M) : 0] += e2 < C.thr[2] ? 1 : 0;                                                            \
        if (skip_md) e0 = e1 = DBL_MAX;                                                                               \
        if (skip_epi) e2 = DBL_MAX;                                                                                   \
        acc[TILE > (M) ? (M) : 0] +=                                                                                  \
            msac(e0, C.thr[0], C.w[0]) + msac(e1, C.thr[1], C.w[1]) + msac(e2, C.thr[2], C.w[2]);                     \
    }

template <int V, int TILE>
__global__ void __launch_bounds__(kBlock)
    select_score_kernel(const PairData *__restrict__ Ds, const PairConst *__restrict__ Cs,
                        const SelectItem *__restrict__ items, const ScoreRec *__restrict__ recs, int64_t base,
                        double *__restrict__ scores, int *__restrict__ counts) {
    static_assert(TILE == 1 || TILE == 2 || TILE == 4 || TILE == 8, "work items of 1, 2, 4 or 8 candidates");
    const SelectItem it = items[blockIdx.x];
    const PairData &D = Ds[it.pair];
    const PairConst &C = Cs[it.pair];
    const ScoreRec *__restrict__ rs = recs + it.rec;
    // The records by value, before the loop, as score_models_kernel and refine_sweep_kernel
    // hold theirs: where an operand is defined decides the operand order of the optimised
    // additions and with it which product is fused into which sum.  A slot
    // past the item's count repeats the first record and is not used.
    ScoreRec rv[TILE];
#pragma unroll
    for (int m = 0; m < TILE; ++m) rv[m] = rs[m < it.count ? m : 0];
    const int n = C.n;
    // (as refine_sweep_kernel: the counts take the ungated errors, the score the gated)
    const bool skip_md = C.score_type == 1, skip_epi = C.score_type == 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc[TILE];
    int c0[TILE], c1[TILE], c2[TILE];
#pragma unroll
    for (int m = 0; m < TILE; ++m) {
        acc[m] = 0.0;
        c0[m] = c1[m] = c2[m] = 0;
    }
    for (int i = threadIdx.x; i < n; i += kBlock) {
        const Corr p = load_corr(C, D, i, V == kCal);
        MP_SELECT_MODEL(0)
        MP_SELECT_MODEL(1)
        MP_SELECT_MODEL(2)
        MP_SELECT_MODEL(3)
        MP_SELECT_MODEL(4)
        MP_SELECT_MODEL(5)
        MP_SELECT_MODEL(6)
        MP_SELECT_MODEL(7)
    }
    __shared__ double part[TILE][kBlock / 64];
    __shared__ int cpart[TILE][3][kBlock / 64];
#pragma unroll
    for (int m = 0; m < TILE; ++m) {
        if (m < it.count) { // (uniform over the workgroup)
            const double v = wave_sum(acc[m]);
            const int s0 = wave_sum_int(c0[m]), s1 = wave_sum_int(c1[m]), s2 = wave_sum_int(c2[m]);
            if (lane == 0) {
                part[m][wave] = v;
                cpart[m][0][wave] = s0;
                cpart[m][1][wave] = s1;
                cpart[m][2][wave] = s2;
            }
        }
    }
    __syncthreads();
    // (it.count <= TILE <= kBlock: one lane per model, the wave partials in wave order)
    if ((int)threadIdx.x < it.count) {
        const int m = threadIdx.x;
        double s = 0.0;
        int c[3] = {0, 0, 0};
        for (int w = 0; w < kBlock / 64; ++w) {
            s += part[m][w];
            c[0] += cpart[m][0][w];
            c[1] += cpart[m][1][w];
            c[2] += cpart[m][2][w];
        }
        const int64_t at = base + it.rec + m; // the candidate's position in the run
        scores[at] = s;
        counts[3 * at] = c[0];
        counts[3 * at + 1] = c[1];
        counts[3 * at + 2] = c[2];
    }
}
#undef MP_SELECT_MODEL

constexpr int kArgminPairs = kBlock / 64; // pairs per workgroup, one wave each

__global__ void __launch_bounds__(kBlock)
    select_argmin_kernel(const int64_t *__restrict__ moff, int np, const double *__restrict__ scores,
                         SelectBest *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * kArgminPairs + (threadIdx.x >> 6);
    if (k >= np) return; // (the whole wave)
    const int64_t o = moff[k];
    const int K = (int)(moff[k + 1] - o);
    double best = DBL_MAX;
    int idx = -1;
    for (int j = lane; j < K; j += 64) {
        const double s = scores[o + j];
        if (s < best) {
            best = s;
            idx = j;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        // a lane that holds an index has a score below DBL_MAX (not NaN): a total order
        const bool take = oi >= 0 && (idx < 0 || ob < best || (ob == best && oi < idx));
        if (take) {
            best = ob;
            idx = oi;
        }
    }
    if (lane == 0) {
        SelectBest b;
        b.score = idx >= 0 ? best : DBL_MAX;
        b.index = idx;
        b.pad = 0;
        out[k] = b;
    }
}

// The walk continued from an earlier one (mp_ransac_adaptive_set): pair k's walk and the
// reduction start from prior[k], the score its running best already holds, instead of
// DBL_MAX.  A lane takes a candidate only strictly below the prior, so a lane that holds an
// index holds a score below the prior (not NaN) and the reduction's order is total as above.
// No candidate strictly below the prior (an equal one, a NaN one, a NaN prior): index -1 and
// the prior's own bits as the score -- "unchanged".  A kernel of its own, so the unseeded
// launch stays the code it was.
__global__ void __launch_bounds__(kBlock)
    select_argmin_seeded_kernel(const int64_t *__restrict__ moff, int np, const double *__restrict__ scores,
                                const double *__restrict__ prior, SelectBest *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * kArgminPairs + (threadIdx.x >> 6);
    if (k >= np) return; // (the whole wave)
    const int64_t o = moff[k];
    const int K = (int)(moff[k + 1] - o);
    const double seed = prior[k];
    double best = seed;
    int idx = -1;
    for (int j = lane; j < K; j += 64) {
        const double s = scores[o + j];
        if (s < best) {
            best = s;
            idx = j;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(idx, off, 64);
        const bool take = oi >= 0 && (idx < 0 || ob < best || (ob == best && oi < idx));
        if (take) {
            best = ob;
            idx = oi;
        }
    }
    if (lane == 0) {
        SelectBest b;
        b.score = idx >= 0 ? best : seed;
        b.index = idx;
        b.pad = 0;
        out[k] = b;
    }
}

} // namespace

hipError_t launch_select_argmin_seeded(hipStream_t s, const int64_t *moff, int np, const double *scores,
                                       const double *prior, SelectBest *out) {
    if (np <= 0) return hipSuccess;
    if (!prior) return hipErrorInvalidValue;
    select_argmin_seeded_kernel<<<(np + kArgminPairs - 1) / kArgminPairs, kBlock, 0, s>>>(moff, np, scores, prior, out);
    return hipGetLastError();
}

hipError_t launch_select_score(hipStream_t s, int variant, int tile, const PairData *Ds, const PairConst *Cs,
                               const SelectItem *items, int nitems, const ScoreRec *recs, int64_t base,
                               double *scores, int *counts) {
    if (nitems <= 0) return hipSuccess;
    if (tile != 1 && tile != 2 && tile != 4 && tile != 8) return hipErrorInvalidValue;
    return by_variant(variant, [&](auto V) {
        constexpr int v = decltype(V)::value;
        if (tile == 1)
            select_score_kernel<v, 1><<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, base, scores, counts);
        else if (tile == 2)
            select_score_kernel<v, 2><<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, base, scores, counts);
        else if (tile == 4)
            select_score_kernel<v, 4><<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, base, scores, counts);
        else
            select_score_kernel<v, 8><<<nitems, kBlock, 0, s>>>(Ds, Cs, items, recs, base, scores, counts);
        return hipGetLastError();
    });
}

hipError_t launch_select_argmin(hipStream_t s, const int64_t *moff, int np, const double *scores, SelectBest *out) {
    if (np <= 0) return hipSuccess;
    select_argmin_kernel<<<(np + kArgminPairs - 1) / kArgminPairs, kBlock, 0, s>>>(moff, np, scores, out);
    return hipGetLastError();
}

} // namespace mp
