// The minimal-sample generator of mp_draw_set / mp_ransac_set: one integer-only function for
// host and device, so a sample's bits agree by construction (no floating point anywhere).
//
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) with
// the standard constants.  The key is (seed low 32 bits, seed high 32 bits); the counter of a
// block is (s, block, pair, 0): s the sample's index within its pair, pair the pair's index
// in the set, block = 0, 1, ...  A sample's word stream is the four outputs of block 0 in
// order, then block 1, and so on; kDrawBlocks blocks (64 words) at most are read.
//
// The rule for a pair of n correspondences (k_md = 3 calibrated, 4 otherwise; k_pt = 5 / 6 /
// 7):  word 0 decides the type: 1 (the point solver) iff (w0 >> 24) < point_share, with
// point_share in 0 .. 256; n < k_pt forces type 0; n < k_md gives the pair no samples.  From
// word 1 on each word w proposes the index (uint64(w) * n) >> 32 (< n); slot a takes the next
// proposal that differs from slots 0 .. a - 1.  After the 64 words any slot still open is
// filled with the smallest unused indices in ascending order (all < k <= n), so the loop is
// bounded.  The slots past the sample's size are 0, the form mp_hypothesize_set takes.
#pragma once
#include "mp_types.h"

namespace mp {

constexpr int kDrawBlocks = 16;      // Philox blocks per sample at most (64 words)
constexpr int kDrawShareMax = 256;   // point_share: 0 .. 256
constexpr int kDrawItemSamples = 64; // samples per work item of draw_samples (one per lane)

constexpr int draw_k_md(int v) { return v == kCal ? 3 : 4; }
constexpr int draw_k_pt(int v) { return v == kCal ? 5 : (v == kSF ? 6 : 7); }
// point_share = -1: the default of the set's solver_type (0 hybrid, 1 point solver only, 2 MD
// solver only)
constexpr int draw_default_share(int solver_type) { return solver_type == 1 ? 256 : (solver_type == 2 ? 0 : 128); }

// One workgroup of draw_samples (kernels/draw_batch.h; planned by host/candidates_plan.h):
// samples s0 .. s0 + count - 1 (count <= kDrawItemSamples) of pair `pair` of the set, written
// to the positions out .. out + count - 1 of the launch's sample array.
struct DrawItem {
    int pair, s0, count, out;
};

MP_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                         uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// the type word 0 gives a sample of a pair of n >= k_md correspondences
MP_HD int draw_type_of(uint32_t w0, int64_t n, int k_pt, int point_share) {
    return (n >= k_pt && (int)(w0 >> 24) < point_share) ? 1 : 0;
}

// The type alone (the host's planning: hyp_items needs no index).  n >= k_md.
MP_HD int draw_type(int64_t n, int k_pt, uint64_t seed, int point_share, uint32_t pair, uint32_t s) {
    uint32_t w[4];
    philox4x32_10(s, 0u, pair, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
    return draw_type_of(w[0], n, k_pt, point_share);
}

// Sample s of pair `pair`: its type (the return value) and its 8 index slots; -1 and zeros
// for n < k_md.  Every index written is < n.  idx is only ever indexed by constants, so it
// stays in registers on the device.  *fill (nullable): whether the ascending fill was needed.
MP_HD int draw_sample(int64_t n, int k_md, int k_pt, uint64_t seed, int point_share, uint32_t pair, uint32_t s,
                      int idx[8], bool *fill = nullptr) {
    static_for<8>([&](auto I) { idx[I.value] = 0; });
    if (fill) *fill = false;
    if (n < k_md) return -1;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint32_t w[4];
    philox4x32_10(s, 0u, pair, 0u, k0, k1, w);
    const int type = draw_type_of(w[0], n, k_pt, point_share);
    const int k = type ? k_pt : k_md;
    int filled = 0;
    // one proposal: taken by slot `filled` unless an earlier slot holds it
    auto propose = [&](int p) {
        bool dup = false;
        static_for<8>([&](auto I) { dup = dup || (I.value < filled && idx[I.value] == p); });
        if (dup) return;
        static_for<8>([&](auto I) {
            if (I.value == filled) idx[I.value] = p;
        });
        ++filled;
    };
    for (int block = 0; block < kDrawBlocks && filled < k; ++block) {
        if (block > 0) philox4x32_10(s, (uint32_t)block, pair, 0u, k0, k1, w);
        for (int j = block == 0 ? 1 : 0; j < 4 && filled < k; ++j) propose((int)(((uint64_t)w[j] * (uint64_t)n) >> 32));
    }
    if (filled < k) {
        if (fill) *fill = true;
        // (of 0 .. k - 1 at most `filled` are used: the k - filled smallest unused are < k <= n)
        for (int c = 0; c < k && filled < k; ++c) propose(c);
    }
    return type;
}

// ---- the confidence-weighted draw (mp_draw_weights_create, mp_draw_weighted_set) ----
// A pair given weights has the integer table q_i in 0 .. 65535 (the quantisation of the weights
// is include/mp_draw_weights.h's; this header stays integer-only), c[0] = 0, c[i + 1] = c[i] +
// q_i in uint32 and W = c[n]; n <= kDrawWeightMaxN, so W <= 65535^2 < 2^32.  q_i = 0 masks
// correspondence i.  The pair is weighted iff #{q_i > 0} >= k_pt (n >= k_pt) or
// k_md (n < k_pt); otherwise it draws by draw_sample.  The type is word 0's, unchanged.  From
// word 1 on each word w proposes t = (uint64(w) * W) >> 32 (< W) and then the unique i with
// c[i] <= t < c[i + 1] (so q_i > 0); slots and duplicates as draw_sample; the fill takes the
// smallest unused indices with q_i > 0 in ascending order (there are at least k of them).
// With all q_i equal to some q > 0: i = floor(floor(w n q / 2^32) / q) = floor(w n / 2^32),
// draw_sample's proposal, so equal weights give draw_sample's bytes, fill included.
constexpr int kDrawWeightMaxN = 65535;   // the largest pair that may be given weights
constexpr uint32_t kDrawWeightQMax = 65535u;
// draw_samples_weighted reads a table of at most this many entries (n + 1) through LDS: 16 KiB
constexpr int kDrawStageEntries = 4096;

// the pair's k_max: what #{q_i > 0} must reach for the pair to draw by its weights
MP_HD int draw_weighted_need(int64_t n, int k_md, int k_pt) { return n >= k_pt ? k_pt : k_md; }

// the i in 0 .. n - 1 with c[i] <= t < c[i + 1], for t < c[n] (c[0] = 0, c non-decreasing)
MP_HD int draw_cum_find(const uint32_t *c, int n, uint32_t t) {
    int lo = 0, hi = n; // c[lo] <= t < c[hi] throughout
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (c[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// draw_sample for a weighted pair: c its table of n + 1 entries (k_md <= n <= kDrawWeightMaxN,
// at least draw_weighted_need of the q_i positive).  Every index written is < n.
MP_HD int draw_sample_weighted(int n, int k_md, int k_pt, uint64_t seed, int point_share, uint32_t pair, uint32_t s,
                               const uint32_t *c, int idx[8], bool *fill = nullptr) {
    static_for<8>([&](auto I) { idx[I.value] = 0; });
    if (fill) *fill = false;
    if (n < k_md) return -1;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const uint64_t W = c[n];
    uint32_t w[4];
    philox4x32_10(s, 0u, pair, 0u, k0, k1, w);
    const int type = draw_type_of(w[0], n, k_pt, point_share);
    const int k = type ? k_pt : k_md;
    int filled = 0;
    auto propose = [&](int p) {
        bool dup = false;
        static_for<8>([&](auto I) { dup = dup || (I.value < filled && idx[I.value] == p); });
        if (dup) return;
        static_for<8>([&](auto I) {
            if (I.value == filled) idx[I.value] = p;
        });
        ++filled;
    };
    for (int block = 0; block < kDrawBlocks && filled < k; ++block) {
        if (block > 0) philox4x32_10(s, (uint32_t)block, pair, 0u, k0, k1, w);
        for (int j = block == 0 ? 1 : 0; j < 4 && filled < k; ++j)
            propose(draw_cum_find(c, n, (uint32_t)(((uint64_t)w[j] * W) >> 32)));
    }
    if (filled < k) {
        if (fill) *fill = true;
        for (int i = 0; i < n && filled < k; ++i)
            if (c[i + 1] != c[i]) propose(i);
    }
    return type;
}

} // namespace mp
