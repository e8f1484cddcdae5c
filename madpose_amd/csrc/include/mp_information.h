// The finishing arithmetic of the information stage (mp_information_set; kernels/information.h
// information_finish_kernel, and the host-only test hook mp_debug_information_finish): one
// text for device and host.
//
// Input: the Gauss-Newton system of one entry in the full 11-parameter layout of LmSystem
// (rotation tangent 3, t 3, scale, offset0, offset1, focal0, focal1) -- H the packed upper
// triangle of J^T J, g = J^T r -- and the active mask col.
//
//   * info_mask zeroes every entry of H and g that belongs to an inactive parameter, which
//     makes the full layout equal the compacted system of the host LM.
//   * info_covariance inverts H on the active set.  With D_a = 1 / sqrt(H_aa) and A = D H D
//     (unit diagonal up to rounding): one Cholesky factorisation A = L L^T, then for every
//     active k the two triangular solves of A x = e_k, and cov[a][k] = D_a x_a D_k.  Inactive
//     parameters are carried as identity rows, as lm_step carries them (kernels/lm_device.h):
//     their terms in every inner product are exact zeros, so the operations on the active
//     parameters are those of the compacted system; their rows and columns of cov are zero.
//     Returns 1 when it was done; 0 when an active H_aa or a pivot is not positive and finite
//     (cov all zero then).  A completed factorisation says nothing about conditioning: a
//     gauge direction (|t| under Sampson blocks alone) has a pivot at rounding level, which
//     is usually still positive.
//
// All loops have compile-time bounds and indices (lm_step's form), so on the device L, D and
// the solve vector stay in registers; the column loop is a loop (its index only selects e_k).
#pragma once
#include <cmath>

#include "mp_types.h"

namespace mp {

constexpr int kInfoN = 11;                          // parameters of the full layout
constexpr int kInfoPack = kInfoN * (kInfoN + 1) / 2; // 66: packed upper triangle
constexpr int kInfoRed = kInfoPack + kInfoN + 1;     // H, g, cost

// (a, b), a <= b, of the packed upper triangle (lm_up with na = 11)
MP_HD int info_up(int a, int b) { return a * kInfoN - a * (a - 1) / 2 + (b - a); }

MP_HD bool info_pos_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

// exact zeros on the inactive parameters' entries of H (66) and g (11)
MP_HD void info_mask(double *H, double *g, const int *col) {
    for (int a = 0; a < kInfoN; ++a) {
        if (!col[a]) g[a] = 0.0;
        for (int b = a; b < kInfoN; ++b)
            if (!col[a] || !col[b]) H[info_up(a, b)] = 0.0;
    }
}

// cov (121, row-major) = the inverse of H on the active set, zero elsewhere; 1 done, 0 not
// positive definite (cov all zero)
MP_HD int info_covariance(const double *H, const int *col, double *cov) {
    double L[kInfoPack]; // lower triangle, row-major packed: (i, j) at i (i + 1) / 2 + j
    double D[kInfoN], y[kInfoN];
    bool act[kInfoN];
    bool ok = true;
    for (int q = 0; q < kInfoN * kInfoN; ++q) cov[q] = 0.0;
#pragma unroll
    for (int a = 0; a < kInfoN; ++a) {
        act[a] = col[a] != 0;
        const double h = act[a] ? H[info_up(a, a)] : 1.0;
        ok = ok && info_pos_finite(h);
        D[a] = act[a] ? 1.0 / sqrt(h) : 1.0;
    }
    if (!ok) return 0;
#pragma unroll
    for (int i = 0; i < kInfoN; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double h = (act[i] && act[j]) ? H[info_up(j, i)] : (i == j ? 1.0 : 0.0);
            L[i * (i + 1) / 2 + j] = h * D[i] * D[j];
        }
#pragma unroll
    for (int j = 0; j < kInfoN; ++j) {
        double dj = L[j * (j + 1) / 2 + j];
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= L[j * (j + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        ok = ok && info_pos_finite(dj);
        dj = sqrt(dj);
        L[j * (j + 1) / 2 + j] = dj;
#pragma unroll
        for (int i = j + 1; i < kInfoN; ++i) {
            double s2 = L[i * (i + 1) / 2 + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s2 -= L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
            L[i * (i + 1) / 2 + j] = s2 / dj;
        }
    }
    if (!ok) return 0;
    for (int k = 0; k < kInfoN; ++k) {
        if (!col[k]) continue;
#pragma unroll
        for (int i = 0; i < kInfoN; ++i) {
            double s2 = i == k ? 1.0 : 0.0;
#pragma unroll
            for (int m = 0; m < i; ++m) s2 -= L[i * (i + 1) / 2 + m] * y[m];
            y[i] = s2 / L[i * (i + 1) / 2 + i];
        }
#pragma unroll
        for (int i = kInfoN - 1; i >= 0; --i) {
            double s2 = y[i];
#pragma unroll
            for (int m = i + 1; m < kInfoN; ++m) s2 -= L[m * (m + 1) / 2 + i] * y[m];
            y[i] = s2 / L[i * (i + 1) / 2 + i];
        }
        const double dk = D[k];
#pragma unroll
        for (int a = 0; a < kInfoN; ++a) cov[a * kInfoN + k] = act[a] ? y[a] * D[a] * dk : 0.0;
    }
    return 1;
}

} // namespace mp
