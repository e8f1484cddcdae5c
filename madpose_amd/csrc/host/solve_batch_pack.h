// Chunk planning and host packing of the batched minimal solvers (mp_*_batch): plain
// C++, no HIP, so the index arithmetic is checked on the CPU under a sanitizer
// (tests/solve_batch_pack_check.cpp).
//
// A batch of ns samples runs in rounds of at most `chunk` samples; a round's inputs are
// transposed on the host to structure of arrays: value k of the round's sample i at
// out[k * ld + i], ld = the round's samples rounded up to a wave (64), so that lane i of
// a kernel reads consecutive doubles (the layout of the MD workspace, kernels.h).
#pragma once
#include <cstdint>

namespace mp {

constexpr int64_t kSolveBatchMax = int64_t(1) << 22; // samples per call
constexpr int64_t kSolveBatchChunk = 32768;          // samples per round when chunk == 0

// samples per round: the caller's chunk, the default for 0, never more than the batch
inline int64_t solve_batch_chunk(int64_t ns, int64_t chunk) {
    const int64_t c = chunk > 0 ? chunk : kSolveBatchChunk;
    return c < ns ? c : (ns > 0 ? ns : 1);
}
inline int64_t solve_batch_rounds(int64_t ns, int64_t chunk) {
    if (ns <= 0) return 0;
    const int64_t c = solve_batch_chunk(ns, chunk);
    return (ns + c - 1) / c;
}
// first sample and sample count of round r
inline void solve_batch_round(int64_t ns, int64_t chunk, int64_t r, int64_t *s0, int64_t *cnt) {
    const int64_t c = solve_batch_chunk(ns, chunk);
    *s0 = r * c;
    *cnt = ns - *s0 < c ? ns - *s0 : c;
}
// leading dimension of a round of cnt samples
inline int64_t solve_batch_ld(int64_t cnt) { return (cnt + 63) & ~int64_t(63); }

// src: sample-major, `per` doubles per sample; samples s0 .. s0 + cnt - 1 go to rows
// row0 .. row0 + per - 1 of out (leading dimension ld >= cnt).  The padding columns
// cnt .. ld - 1 are left alone.
inline void pack_soa(const double *src, int64_t per, int64_t s0, int64_t cnt, int64_t ld, int64_t row0, double *out) {
    for (int64_t i = 0; i < cnt; ++i) {
        const double *p = src + (s0 + i) * per;
        for (int64_t k = 0; k < per; ++k) out[(row0 + k) * ld + i] = p[k];
    }
}

// rows of an MD sample of K points: x (3K), y (3K), depth_x (K), depth_y (K)
inline int64_t md_rows(int K) { return 8 * (int64_t)K; }
inline void pack_md_soa(int K, int64_t s0, int64_t cnt, int64_t ld, const double *x, const double *y, const double *dx,
                        const double *dy, double *out) {
    pack_soa(x, 3 * K, s0, cnt, ld, 0, out);
    pack_soa(y, 3 * K, s0, cnt, ld, 3 * K, out);
    pack_soa(dx, K, s0, cnt, ld, 6 * K, out);
    pack_soa(dy, K, s0, cnt, ld, 7 * K, out);
}

} // namespace mp
