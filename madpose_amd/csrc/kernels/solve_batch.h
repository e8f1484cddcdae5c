// The minimal solvers over many raw samples per launch (mp_solve_scale_and_shift_batch,
// mp_solve_scale_shift_pose_batch, mp_relpose_batch; host side: engine.cpp solve_*_batch).
// Included from kernels.hip after the estimator's kernels: the per-sample arithmetic is
// the device functions the single-sample entries call (md_direct_kernel,
// point_direct_*_kernel), so a batch row is that entry's result to the bit; only the
// mapping of samples to lanes differs.
//
//  sb_md<V, R, POSE>  default MD solvers, R = 2 lanes per sample as md_exact_body: every lane
//                     of a group runs the setup, lane r the roots r, r + R, ...; rows
//                     compacted in root order by ballot + popcount.  No PairData, no
//                     K^-1 product and no md_accept (the single-sample entries filter
//                     nothing).  Inputs structure of arrays (host/solve_batch_pack.h).
//  sb_md_alt<V, ALT>  use_ours / use_4p4d: one lane per sample
//  sb_pt5_pose        16 lanes per sample, lane e the essential matrix e of the root
//                     stage (pt_roots5_bearings_kernel over the chunk)
//  sb_pt6_pose        16 lanes per sample, lane r the root r of the estimator's root
//                     stage (launch_pt_roots on the chunk's pseudo-pair), the sample's
//                     pencil (sixpt_matrices) formed once in LDS; concatenation, cap and
//                     keep-the-first duplicate rule of sixpt_poses_for_roots
//  sb_pt7_F, _pose    relpose_7pt_F with one lane per sample, then one lane per
//                     (sample, F) through twofocal_pose_from_F
#pragma once

namespace mp {
namespace {

constexpr int kSbMdSlots = 8, kSbPtSlots = 16; // output slots per sample

// an MD sample of the chunk (structure of arrays: value k of sample i at in[k * ld + i])
template <int K>
__device__ __forceinline__ void sb_md_inputs(const double *in, int ld, int i, double (&x)[K][3], double (&y)[K][3],
                                             double (&dx)[K], double (&dy)[K]) {
    static_for<3 * K>([&](auto k) {
        x[k / 3][k % 3] = in[(size_t)k * ld + i];
        y[k / 3][k % 3] = in[(size_t)(3 * K + k) * ld + i];
    });
    static_for<K>([&](auto k) {
        dx[k] = in[(size_t)(6 * K + k) * ld + i];
        dy[k] = in[(size_t)(7 * K + k) * ld + i];
    });
}

// POSE = false: rows = every solution the solver emits (ns x 8 rows of width 4 / 5 / 6);
// POSE = true: rows = the models of the solutions md_pose_exact accepts (ns x 8 Models).
// The slots past a sample's count are left as the host zeroed them.
template <int V, int R, bool POSE>
__global__ void __launch_bounds__(64) sb_md_kernel(const double *in, int ld, int ns, double *sols, Model *poses,
                                                   int *counts) {
    using Sys = typename MdxSys<V>::S;
    constexpr int K = MdxSys<V>::K, NR = Sys::NR, W = V == kCal ? 4 : (V == kSF ? 5 : 6);
    static_assert(R == 1 || R == 2 || R == 4 || R == 8, "1, 2, 4 or 8 lanes per sample");
    static_assert(NR % R == 0 && NR <= kSbMdSlots, "a sample's lanes take its roots in equal turns");
    const int g = threadIdx.x / R, r = threadIdx.x % R;
    const int idx = blockIdx.x * (64 / R) + g;
    const bool active = idx < ns;
    const int ia = active ? idx : ns - 1;
    double x[K][3], y[K][3], dx[K], dy[K];
    sb_md_inputs<K>(in, ld, ia, x, y, dx, dy);
    Sys sys;
    double roots[NR];
    const int nr = sys.setup(x, y, dx, dy, roots);
    const int g0 = (threadIdx.x & 63) & ~(R - 1);
    int n = 0; // the sample's rows so far (root order: turn j, then lane r)
#pragma unroll
    for (int j = 0; j < NR / R; ++j) {
        const int q = j * R + r;
        double root = 0.0;
#pragma unroll
        for (int c = 0; c < R; ++c)
            if (c == r) root = opaque(roots[j * R + c]);
        double sol[6], X[K][3], Y[K][3];
        bool keep = false;
        if (active && q < nr && sys.root(root, sol))
            keep = POSE ? md_pose_points<K>(x, y, dx, dy, sol, sol[4], sol[5], X, Y) : true;
        const unsigned long long ball = __ballot(keep);
        const unsigned long long mine = (ball >> g0) & ((1ull << R) - 1);
        const int pos = n + __popcll(mine & ((1ull << r) - 1));
        if (keep) { // (pos < NR <= kSbMdSlots: at most one row per root)
            if constexpr (POSE) {
                Model m;
                m.focal0 = sol[4];
                m.focal1 = sol[5];
                mdx::procrustes<K>(X, Y, m);
                m.scale = sol[2];
                m.offset0 = sol[1];
                m.offset1 = sol[3];
                poses[(size_t)idx * kSbMdSlots + pos] = m;
            } else {
                double *o = sols + ((size_t)idx * kSbMdSlots + pos) * W;
#pragma unroll
                for (int c = 0; c < W; ++c) o[c] = sol[c];
            }
        }
        n += __popcll(mine);
        if (!__any(active && (j + 1) * R < nr)) break; // (uniform) no sample of the wave has more roots
    }
    if (active && r == 0) counts[idx] = n;
}

template <int V, int ALT>
__global__ void __launch_bounds__(64) sb_md_alt_kernel(const double *in, int ld, int ns, Model *poses, int *counts) {
    constexpr int K = MdxSys<V>::K;
    const int idx = blockIdx.x * 64 + (int)threadIdx.x;
    if (idx >= ns) return;
    double x[K][3], y[K][3], dx[K], dy[K];
    sb_md_inputs<K>(in, ld, idx, x, y, dx, dy);
    Model *out = poses + (size_t)idx * kSbMdSlots; // (as md_direct_kernel: the solver writes its at most 8 models)
    int n;
    if constexpr (V == kCal)
        n = md_pose_cal_ours(x, y, dx, dy, out);
    else if constexpr (V == kSF)
        n = md_pose_sf_ours(x, y, dx, dy, out);
    else if constexpr (ALT == 1)
        n = md_pose_tf_ours(x, y, dx, dy, out);
    else
        n = md_pose_tf_4p4d(x, y, dx, dy, out);
    counts[idx] = n < kSbMdSlots ? n : kSbMdSlots;
}

// the models before a lane's in its 16-lane group: the sum of cnt over the lower lanes
__device__ __forceinline__ int sb_group16_before(int cnt, int *total) {
    const int base = (int)(threadIdx.x & 63) & ~15, e = (int)threadIdx.x & 15;
    int off = 0, tot = 0;
#pragma unroll
    for (int l = 0; l < 16; ++l) {
        const int c = __shfl(cnt, base + l);
        off += l < e ? c : 0;
        tot += c;
    }
    *total = tot;
    return off;
}

// in: ns x 30 doubles (image 0's five unit bearings, then image 1's); cand / ncand: the
// root stage's essential matrices.  The sequential loop of point_direct_5pt_kernel
// appends candidate e's poses while slots remain, so slot p of the concatenation in
// candidate order is kept for p < kMaxModelsCal.
__global__ void __launch_bounds__(64) sb_pt5_pose_kernel(const double *in, int ns, const double *cand,
                                                         const int *ncand, Model *poses, int *counts) {
    const int g = threadIdx.x / 16, e = threadIdx.x % 16;
    const int idx = blockIdx.x * 4 + g;
    const bool active = idx < ns;
    const int ia = active ? idx : ns - 1;
    double b1[5][3], b2[5][3];
    const double *p = in + (size_t)ia * 30;
#pragma unroll
    for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            b1[j][c] = p[3 * j + c];
            b2[j][c] = p[15 + 3 * j + c];
        }
    const int nc = ncand[ia] < 10 ? ncand[ia] : 10;
    Model loc[4];
    int cnt = 0;
    if (active && e < nc) cnt = motion_from_essential<5>(cand + (size_t)ia * kCandStride + 9 * e, b1, b2, loc, 0, 4);
    int total;
    const int off = sb_group16_before(cnt, &total);
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (q < cnt && off + q < kMaxModelsCal) poses[(size_t)idx * kSbPtSlots + off + q] = loc[q];
    if (active && e == 0) counts[idx] = total < kMaxModelsCal ? total : kMaxModelsCal;
}

// in: ns x 24 doubles (image 0's six normalized 2-D points, then image 1's); cand: the
// null space N (27) and the roots u of the estimator's root stage.  Lane r runs
// sixpt_poses_for_root on root r; the poses are concatenated in root order up to
// kMaxModelsSF in LDS, where the group's first lane applies the duplicate rule of
// sixpt_poses_for_roots (the same comparisons, in place, keeping the first).
__global__ void __launch_bounds__(64) sb_pt6_pose_kernel(const double *in, int ns, const double *cand,
                                                         const int *ncand, Model *poses, int *counts) {
    __shared__ Model stage[4][kMaxModelsSF];
    __shared__ double Msh[4][3][10][10]; // the sample's pencil, formed once by the group's first lane
    __shared__ int kept[4];
    const int g = threadIdx.x / 16, r = threadIdx.x % 16;
    const int idx = blockIdx.x * 4 + g;
    const bool active = idx < ns;
    const int ia = active ? idx : ns - 1;
    const double *p = in + (size_t)ia * 24, *cd = cand + (size_t)ia * kCandStride;
    const int nr = ncand[ia] < 15 ? ncand[ia] : 15;
    double N[3][9];
    for (int e = 0; e < 27; ++e) N[e / 9][e % 9] = cd[e];
    if (active && r == 0 && nr > 0) sixpt_matrices(N, Msh[g]);
    __syncthreads();
    Model loc[4];
    int cnt = 0;
    if (active && r < nr) {
        double b0[6][3], b1[6][3];
        for (int j = 0; j < 6; ++j) {
            const double a[3] = {p[2 * j], p[2 * j + 1], 1.0}, c[3] = {p[12 + 2 * j], p[12 + 2 * j + 1], 1.0};
            const double na = 1.0 / sqrt(dot3(a, a)), nc = 1.0 / sqrt(dot3(c, c));
            for (int q = 0; q < 3; ++q) {
                b0[j][q] = a[q] * na;
                b1[j][q] = c[q] * nc;
            }
        }
        cnt = sixpt_poses_for_root(Msh[g], N, cd[27 + r], b0, b1, loc, 0, 4);
    }
    int total;
    const int off = sb_group16_before(cnt, &total);
    for (int q = 0; q < cnt; ++q)
        if (off + q < kMaxModelsSF) stage[g][off + q] = loc[q];
    __syncthreads();
    if (r == 0) {
        Model *out = stage[g];
        const int nout = total < kMaxModelsSF ? total : kMaxModelsSF;
        int n = 0;
        for (int q = 0; q < nout; ++q) {
            bool dup = false;
            for (int pp = 0; pp < n && !dup; ++pp) {
                bool same = fabs(out[pp].focal0 - out[q].focal0) <= 1e-8 * fabs(out[q].focal0);
                for (int e = 0; e < 9 && same; ++e) same = fabs(out[pp].R[e] - out[q].R[e]) <= 1e-6;
                for (int e = 0; e < 3 && same; ++e)
                    same = fabs(out[pp].t[e] - out[q].t[e]) <= 1e-6 * (1.0 + fabs(out[q].t[e]));
                dup = same;
            }
            if (!dup) out[n++] = out[q];
        }
        kept[g] = n;
        if (active) counts[idx] = n;
    }
    __syncthreads();
    if (active && r < kept[g]) poses[(size_t)idx * kSbPtSlots + r] = stage[g][r];
}

// in: 28 rows of the chunk (structure of arrays): image 0's seven normalized 2-D points,
// then image 1's.  The bearings are formed as point_direct_kernel forms them.
__global__ void __launch_bounds__(64) sb_pt7_F_kernel(const double *in, int ld, int ns, double *Fws, int *counts) {
    const int idx = blockIdx.x * 64 + (int)threadIdx.x;
    if (idx >= ns) return;
    double b0[7][3], b1[7][3];
    for (int j = 0; j < 7; ++j) {
        const double a[3] = {in[(size_t)(2 * j) * ld + idx], in[(size_t)(2 * j + 1) * ld + idx], 1.0};
        const double c[3] = {in[(size_t)(14 + 2 * j) * ld + idx], in[(size_t)(14 + 2 * j + 1) * ld + idx], 1.0};
        const double na = 1.0 / sqrt(dot3(a, a)), nc = 1.0 / sqrt(dot3(c, c));
        for (int q = 0; q < 3; ++q) {
            b0[j][q] = a[q] * na;
            b1[j][q] = c[q] * nc;
        }
    }
    double F[3][9];
    const int nf = relpose_7pt_F(b0, b1, F);
    static_for<3>([&](auto k) {
        if (k < nf) static_for<9>([&](auto e) { Fws[(size_t)(9 * k + e) * ld + idx] = F[k][e]; });
    });
    counts[idx] = nf;
}

// lane (k, i): candidate k of sample i -- the grid covers 3 x ld lanes, k = lane / ld
__global__ void __launch_bounds__(64) sb_pt7_pose_kernel(const double *in, int ld, int ns, const double *Fws,
                                                         const int *counts, Model *poses) {
    const int t = blockIdx.x * 64 + (int)threadIdx.x;
    const int k = t / ld, idx = t % ld;
    if (k >= 3 || idx >= ns || k >= counts[idx]) return;
    double p0[7][2], p1[7][2], F[9];
    static_for<7>([&](auto j) {
        p0[j][0] = in[(size_t)(2 * j) * ld + idx];
        p0[j][1] = in[(size_t)(2 * j + 1) * ld + idx];
        p1[j][0] = in[(size_t)(14 + 2 * j) * ld + idx];
        p1[j][1] = in[(size_t)(14 + 2 * j + 1) * ld + idx];
    });
    for (int e = 0; e < 9; ++e) F[e] = Fws[(size_t)(9 * k + e) * ld + idx];
    Model m;
    twofocal_pose_from_F<7>(F, p0, p1, m);
    poses[(size_t)idx * kSbPtSlots + k] = m;
}

} // namespace

// lanes per sample of sb_md: two for every variant, by measurement at 32768 samples per
// launch (pose kernels; profiles/solver_batch/md_lanes.txt): cal 1 / 2 / 4 lanes 157 /
// 125 / 146 us, tf 170 / 141 / 176 us, sf 2 / 4 / 8 lanes 344 / 528 / 919 us.  With full
// launches the repeated setup of wider groups costs more than the shorter root loop saves.
hipError_t launch_sb_md(hipStream_t s, int variant, int alt, bool pose, const double *in, int ld, int ns, double *sols,
                        Model *poses, int *counts) {
    if (ns <= 0) return hipSuccess;
    if (alt != 0) {
        const int grid = (ns + 63) / 64;
        if (variant == kCal)
            sb_md_alt_kernel<kCal, 1><<<grid, 64, 0, s>>>(in, ld, ns, poses, counts);
        else if (variant == kSF)
            sb_md_alt_kernel<kSF, 1><<<grid, 64, 0, s>>>(in, ld, ns, poses, counts);
        else if (alt == 1)
            sb_md_alt_kernel<kTF, 1><<<grid, 64, 0, s>>>(in, ld, ns, poses, counts);
        else
            sb_md_alt_kernel<kTF, 2><<<grid, 64, 0, s>>>(in, ld, ns, poses, counts);
        return hipGetLastError();
    }
    return by_variant(variant, [&](auto V) {
        constexpr int v = decltype(V)::value, R = 2;
        const int grid = (ns + 64 / R - 1) / (64 / R);
        if (pose)
            sb_md_kernel<v, R, true><<<grid, 64, 0, s>>>(in, ld, ns, sols, poses, counts);
        else
            sb_md_kernel<v, R, false><<<grid, 64, 0, s>>>(in, ld, ns, sols, poses, counts);
        return hipGetLastError();
    });
}

hipError_t launch_sb_pt5(hipStream_t s, const double *in, int ns, double *cand, int *ncand, Model *poses,
                         int *counts) {
    if (ns <= 0) return hipSuccess;
    pt_roots5_bearings_kernel<<<(ns + kS5 - 1) / kS5, 64, 0, s>>>(in, ns, cand, ncand, kCandStride);
    sb_pt5_pose_kernel<<<(ns + 3) / 4, 64, 0, s>>>(in, ns, cand, ncand, poses, counts);
    return hipGetLastError();
}

hipError_t launch_sb_pt6_poses(hipStream_t s, const double *in, int ns, const double *cand, const int *ncand,
                               Model *poses, int *counts) {
    if (ns <= 0) return hipSuccess;
    sb_pt6_pose_kernel<<<(ns + 3) / 4, 64, 0, s>>>(in, ns, cand, ncand, poses, counts);
    return hipGetLastError();
}

hipError_t launch_sb_pt7(hipStream_t s, const double *in, int ld, int ns, double *Fws, Model *poses, int *counts) {
    if (ns <= 0) return hipSuccess;
    sb_pt7_F_kernel<<<(ns + 63) / 64, 64, 0, s>>>(in, ld, ns, Fws, counts);
    sb_pt7_pose_kernel<<<(3 * ld + 63) / 64, 64, 0, s>>>(in, ld, ns, Fws, counts, poses);
    return hipGetLastError();
}

} // namespace mp
