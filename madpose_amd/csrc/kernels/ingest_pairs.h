// The device ingest of mp_pair_set_create_device (host side: host/resident_pairs.h
// ResidentPairs' second constructor; plan and records: host/ingest_plan.h).  Included from
// kernels.hip.
//
// What make_problem + refine_pack_pair + pair_magnitudes (and get_depths) do on the host for
// a host-built set, on arrays that are already on the device, with their bits:
//   * ingest_scale_kernel (shared / two focal): one workgroup per pair.  All lanes form the
//     square-root terms sqrt(a0^2 + a1^2), sqrt(b0^2 + b1^2) of kIngestChunk correspondences
//     and stage them in LDS in make_problem's order (two per correspondence); lane 0 adds the
//     staged terms into ONE accumulator in that order -- no tree, no per-lane partial sums: the
//     sum is not associative and the scale, hence every normalized coordinate, is pinned to
//     the host's bits.  Two LDS buffers: the other lanes stage chunk k + 1 while lane 0 still
//     adds chunk k (one barrier per chunk).  No FMA contraction, plain / and sqrt (correctly
//     rounded), as include/mp_md_exact.h.
//   * ingest_rows_kernel: one workgroup per item (a pair and up to kIngestSpan consecutive
//     correspondences of it, kIngestBlock per trip).  A lane widens its correspondence
//     (float32 -> double is exact), centres and divides it (shared / two focal: (x - pp) /
//     scale, make_problem's two operations), takes the depths from the arrays or looks them up
//     in the pair's maps with get_depths_kernel's arithmetic, writes rows 0 .. 5 and keeps the
//     running maxima of pair_magnitudes (a < b ? b : a as std::max: a NaN is never taken, so
//     any order gives the same maxima) and the non-finite flag.  Maxima and flag are reduced
//     over the workgroup (wave shuffles, then LDS) and lane 0 writes the item's IngestStats.
// Inputs are only read, through element-typed scalar loads (element alignment is all the host
// checks).  Every index is below the pair's n, which the host checked against the allocations'
// address ranges before the launch; a map index is clipped to the map.  Every store is an
// ordinary vector store; no atomics, no scratch.
#pragma once
#include "../host/ingest_plan.h"

namespace mp {
namespace {

static_assert(kIngestChunk == kIngestBlock, "one staged correspondence per lane");
static_assert(kIngestSpan % kIngestBlock == 0, "whole trips per item");

__device__ inline double ingest_ld(const void *p, int type, int64_t i) {
    return type ? static_cast<const double *>(p)[i] : (double)static_cast<const float *>(p)[i];
}

// get_depths_kernel's lookup of keypoint (x, y) in side s's map of the pair
__device__ inline double ingest_depth(const IngestPair &P, int s, double x, double y, int mtype) {
    const int64_t h = P.h[s], w = P.w[s];
    int64_t c = (int64_t)rint(x * P.fx[s]), r = (int64_t)rint(y * P.fy[s]);
    c = c < 0 ? 0 : (c > w - 1 ? w - 1 : c);
    r = r < 0 ? 0 : (r > h - 1 ? h - 1 : r);
    return ingest_ld(P.map[s], mtype, r * w + c);
}

__device__ inline double ingest_wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = ingest_max(v, __shfl_xor(v, d, 64));
    return v;
}

__global__ void __launch_bounds__(kIngestBlock)
ingest_scale_kernel(IngestArgs A, const IngestPair *__restrict__ Ps, double *__restrict__ scale) {
#pragma clang fp contract(off)
    __shared__ double term[2][2 * kIngestChunk];
    const IngestPair &P = Ps[blockIdx.x];
    const int n = P.n, tid = threadIdx.x;
    const int64_t off = P.off;
    const double p0u = P.cam0[0], p0v = P.cam0[1], p1u = P.cam1[0], p1v = P.cam1[1];
    double acc = 0.0;
    for (int c0 = 0, k = 0; c0 < n; c0 += kIngestChunk, ++k) {
        double *buf = term[k & 1];
        const int i = c0 + tid;
        if (i < n) {
            const int64_t g = off + i;
            const double a0 = ingest_ld(A.x0, A.xtype, 2 * g) - p0u, a1 = ingest_ld(A.x0, A.xtype, 2 * g + 1) - p0v;
            const double b0 = ingest_ld(A.x1, A.xtype, 2 * g) - p1u, b1 = ingest_ld(A.x1, A.xtype, 2 * g + 1) - p1v;
            buf[2 * tid] = sqrt(a0 * a0 + a1 * a1);
            buf[2 * tid + 1] = sqrt(b0 * b0 + b1 * b1);
        }
        __syncthreads();
        if (tid == 0) {
            const int cnt = n - c0 < kIngestChunk ? n - c0 : kIngestChunk;
            for (int j = 0; j < 2 * cnt; ++j) acc += buf[j];
        }
    }
    if (tid == 0) scale[blockIdx.x] = n > 0 ? acc / (sqrt(2.0) * n) : 1.0;
}

__global__ void __launch_bounds__(kIngestBlock)
ingest_rows_kernel(IngestArgs A, const IngestItem *__restrict__ items, const IngestPair *__restrict__ Ps,
                   const PairData *__restrict__ Ds, const double *__restrict__ scale,
                   IngestStats *__restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double red[kIngestBlock / 64][kIngestStatValues + 1];
    const IngestItem it = items[blockIdx.x];
    const IngestPair &P = Ps[it.pair];
    const PairData D = Ds[it.pair];
    const int n = P.n, tid = threadIdx.x;
    const bool cal = A.cal != 0;
    const double s = cal ? 1.0 : scale[it.pair];
    double *r0u = const_cast<double *>(D.x0u), *r0v = const_cast<double *>(D.x0v);
    double *r1u = const_cast<double *>(D.x1u), *r1v = const_cast<double *>(D.x1v);
    double *rd0 = const_cast<double *>(D.d0), *rd1 = const_cast<double *>(D.d1);
    double ea = 0, eap = 0, exi = 0, eb = 0, ebp = 0, exj = 0, ed0 = 0, ed1 = 0, ex0 = 0, ex1 = 0, eab2 = 0;
    double bad = 0.0;
    for (int t = tid; t < it.count; t += kIngestBlock) {
        const int i = it.first + t;
        if (i >= n) break;
        const int64_t g = P.off + i;
        const double q0u = ingest_ld(A.x0, A.xtype, 2 * g), q0v = ingest_ld(A.x0, A.xtype, 2 * g + 1);
        const double q1u = ingest_ld(A.x1, A.xtype, 2 * g), q1v = ingest_ld(A.x1, A.xtype, 2 * g + 1);
        double d0, d1;
        if (A.d0) {
            d0 = ingest_ld(A.d0, A.dtype, g);
            d1 = ingest_ld(A.d1, A.dtype, g);
        } else {
            d0 = ingest_depth(P, 0, q0u, q0v, A.mtype);
            d1 = ingest_depth(P, 1, q1u, q1v, A.mtype);
        }
        double u0 = q0u, v0 = q0v, u1 = q1u, v1 = q1v;
        if (!cal) { // make_problem: centred on the principal point, then divided by the scale
            u0 = (q0u - P.cam0[0]) / s;
            v0 = (q0v - P.cam0[1]) / s;
            u1 = (q1u - P.cam1[0]) / s;
            v1 = (q1v - P.cam1[1]) / s;
        }
        r0u[i] = u0;
        r0v[i] = v0;
        r1u[i] = u1;
        r1v[i] = v1;
        rd0[i] = d0;
        rd1[i] = d1;
        // pair_magnitudes, statement for statement
        ex0 = ingest_max(ex0, ingest_max(fabs(u0), fabs(v0)));
        ex1 = ingest_max(ex1, ingest_max(fabs(u1), fabs(v1)));
        ed0 = ingest_max(ed0, fabs(d0));
        ed1 = ingest_max(ed1, fabs(d1));
        if (cal) {
            auto ray = [](const double *Ki, double u, double v, double &abs1, double &absp, double &xi, double &o0,
                          double &o1) {
                const double a0 = Ki[0] * u + Ki[1] * v + Ki[2], a1 = Ki[3] * u + Ki[4] * v + Ki[5],
                             a2 = Ki[6] * u + Ki[7] * v + Ki[8];
                double p = 0.0;
                p += fabs(Ki[0] * u) + fabs(Ki[1] * v) + fabs(Ki[2]);
                p += fabs(Ki[3] * u) + fabs(Ki[4] * v) + fabs(Ki[5]);
                p += fabs(Ki[6] * u) + fabs(Ki[7] * v) + fabs(Ki[8]);
                abs1 = ingest_max(abs1, fabs(a0) + fabs(a1) + fabs(a2));
                absp = ingest_max(absp, p);
                xi = ingest_max(xi, p / (fabs(a0) + fabs(a1) + 1.0));
                o0 = a0;
                o1 = a1;
            };
            double a0, a1, b0, b1;
            ray(P.cam0, u0, v0, ea, eap, exi, a0, a1);
            ray(P.cam1, u1, v1, eb, ebp, exj, b0, b1);
            const double ab = (fabs(a0) + fabs(a1) + 1.0) * (fabs(b0) + fabs(b1) + 1.0);
            eab2 = ingest_max(eab2, ab * ab);
        } else {
            ea = ingest_max(ea, fabs(u0) + fabs(v0));
            eb = ingest_max(eb, fabs(u1) + fabs(v1));
            const double ab = (fabs(u0) + fabs(v0) + 1.0) * (fabs(u1) + fabs(v1) + 1.0);
            eab2 = ingest_max(eab2, ab * ab);
        }
        const bool fin = __builtin_isfinite(u0) && __builtin_isfinite(v0) && __builtin_isfinite(u1) &&
                         __builtin_isfinite(v1) && __builtin_isfinite(d0) && __builtin_isfinite(d1);
        if (!fin) bad = 1.0;
    }
    if (!cal) {
        eap = ea;
        ebp = eb;
    }
    double m[kIngestStatValues + 1] = {ea, eap, exi, eb, ebp, exj, ed0, ed1, ex0, ex1, eab2, bad};
    const int wave = tid >> 6, lane = tid & 63;
    static_for<kIngestStatValues + 1>([&](auto I) {
        const double v = ingest_wave_max(m[I.value]);
        if (lane == 0) red[wave][I.value] = v;
    });
    __syncthreads();
    if (tid <= kIngestStatValues) {
        double v = red[0][tid];
#pragma unroll
        for (int w = 1; w < kIngestBlock / 64; ++w) v = ingest_max(v, red[w][tid]);
        IngestStats &S = stats[blockIdx.x];
        if (tid < kIngestStatValues)
            S.m[tid] = v;
        else
            S.nonfinite = v != 0.0 ? 1 : 0;
    }
}

} // namespace

hipError_t launch_ingest_scale(hipStream_t s, const IngestArgs &A, const IngestPair *Ps, int np, double *scale) {
    if (np <= 0) return hipSuccess;
    if (A.cal) return hipErrorInvalidValue;
    ingest_scale_kernel<<<np, kIngestBlock, 0, s>>>(A, Ps, scale);
    return hipGetLastError();
}

hipError_t launch_ingest_rows(hipStream_t s, const IngestArgs &A, const IngestItem *items, int nitems,
                              const IngestPair *Ps, const PairData *Ds, const double *scale, IngestStats *stats) {
    if (nitems <= 0) return hipSuccess;
    if (!A.cal && !scale) return hipErrorInvalidValue;
    ingest_rows_kernel<<<nitems, kIngestBlock, 0, s>>>(A, items, Ps, Ds, scale, stats);
    return hipGetLastError();
}

} // namespace mp
