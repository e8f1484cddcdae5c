// Plan, pointer-extent arithmetic and record finishing of the device ingest
// (mp_pair_set_create_device; kernels/ingest_pairs.h): plain C++, no HIP, so all three are
// checked on the CPU under a sanitizer (tests/pair_set_ingest_check.cpp).
//
// The ingest builds a pair set from arrays that are already on the device.  Two launches:
//   * ingest_scale_kernel (shared- and two-focal sets): one workgroup per pair forms the
//     normalization scale -- the square-root terms of kIngestChunk correspondences at a time
//     staged in LDS by all lanes, added by one lane into one accumulator in index order;
//   * ingest_rows_kernel: one workgroup per item -- `count` (1 .. kIngestSpan) consecutive
//     correspondences of one pair from `first` on, kIngestBlock per trip -- writes rows 0 .. 5
//     and the item's statistics (IngestStats: order-free maxima and the non-finite flag).
// An item never crosses a pair and a pair without correspondences gives none.  The host takes
// the maximum over a pair's items (one item for a pair of up to kIngestSpan correspondences)
// and finishes the pair's record with ingest_finish, make_problem's tail restated.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../include/mp_score.h"

namespace mp {

constexpr int kIngestBlock = 256;  // threads per workgroup of both kernels
constexpr int kIngestChunk = 256;  // correspondences per staged chunk of the scale's sum
constexpr int kIngestSpan = 4096;  // correspondences per item of ingest_rows_kernel
constexpr int kIngestStatValues = 11;

struct IngestItem {
    int pair, first, count, pad;
};

// One item's (device) or one pair's (host, after the maximum over its items) statistics:
// m = the maxima of pair_magnitudes in PairConst's order (ea eap exi eb ebp exj ed0 ed1 ex0
// ex1 eab2) before the paddings; nonfinite: some coordinate (as stored in rows 0 .. 3) or
// depth is not finite.
struct IngestStats {
    double m[kIngestStatValues];
    int nonfinite, pad;
};

// What the kernels read of a pair beside its PairData: where its correspondences start in
// the caller's arrays, its size, the cameras (calibrated: K0^-1, K1^-1 row-major; else the
// principal points in cam[0], cam[1]) and, for the map source, side s's depth map (h x w
// row-major at map[s]) with the factors fx = w / image_w, fy = h / image_h.
struct IngestPair {
    int64_t off;
    int n, pad;
    double cam0[9], cam1[9];
    const void *map[2];
    int64_t h[2], w[2];
    double fx[2], fy[2];
};

// The caller's device arrays (uniform over a launch): x0, x1 T x 2 interleaved pixels of
// element type xtype, d0, d1 T depths of type dtype (both null: the maps of IngestPair, of
// element type mtype); types 0 float32, 1 float64.  cal: calibrated geometry (variants 0, 3).
struct IngestArgs {
    const void *x0, *x1, *d0, *d1;
    int xtype, dtype, mtype, cal;
};

// n[k]: the correspondences of pair k (0 .. np - 1, each below 2^31); first_item (np + 1
// values): the items of pair k are first_item[k] .. first_item[k + 1] - 1
inline void ingest_items(int np, const int64_t *n, std::vector<IngestItem> &items, std::vector<int64_t> &first_item) {
    items.clear();
    first_item.assign((size_t)np + 1, 0);
    for (int k = 0; k < np; ++k) {
        first_item[(size_t)k] = (int64_t)items.size();
        for (int64_t first = 0; first < n[k]; first += kIngestSpan) {
            const int64_t left = n[k] - first;
            items.push_back(IngestItem{k, (int)first, (int)(left < kIngestSpan ? left : kIngestSpan), 0});
        }
    }
    first_item[(size_t)np] = (int64_t)items.size();
}

// count * per * elem bytes, or -1 when a factor is negative or the product leaves int64
inline int64_t ingest_bytes(int64_t count, int64_t per, int64_t elem) {
    if (count < 0 || per <= 0 || elem <= 0) return -1;
    const int64_t lim = std::numeric_limits<int64_t>::max();
    if (count > lim / per) return -1;
    const int64_t c = count * per;
    if (c > lim / elem) return -1;
    return c * elem;
}

// Why `bytes` bytes (>= 0) at address `ptr`, elements of `elem` (4, 8) bytes, may not be read
// from the allocation [base, base + size): null (all well) or a short reason.  All in
// unsigned arithmetic on the addresses: no sum that could wrap is formed.
inline const char *ingest_extent_error(uint64_t ptr, uint64_t base, uint64_t size, int64_t bytes, int64_t elem) {
    if (bytes < 0) return "its byte count overflows";
    if (ptr % (uint64_t)elem != 0) return "is not aligned to its element type";
    if (ptr < base) return "lies before its allocation";
    const uint64_t into = ptr - base;
    if (into > size) return "lies past its allocation";
    if ((uint64_t)bytes > size - into) return "is shorter than the correspondences need";
    return nullptr;
}

// max of make_problem's std::max chain: a NaN on the right is never taken
MP_HD double ingest_max(double a, double b) { return a < b ? b : a; }
inline void ingest_merge(IngestStats &a, const IngestStats &b) {
    for (int i = 0; i < kIngestStatValues; ++i) a.m[i] = ingest_max(a.m[i], b.m[i]);
    a.nonfinite |= b.nonfinite;
}

// make_problem's data-dependent tail on a record whose data-independent part (variant, n,
// cameras, inverses, kstd, flags, loss_scale, md_alt, min_depth) is set: thr0, thr1 / w0, w1 the
// options' squared thresholds and weights, scale the pair's normalization scale (1 for a
// calibrated record), tie the screening scale of a finite pair (MADPOSE_TIE_SCALE).  Returns
// the Sampson weight (HostPair::sampson_squared_weight).
inline double ingest_finish(PairConst &C, const IngestStats &S, double scale, double thr0, double thr1, double w0,
                            double w1, double tie) {
    // (no FMA contraction, as make_problem)
#pragma clang fp contract(off)
    if (C.variant != kCal) {
        thr0 /= scale * scale;
        thr1 /= scale * scale;
    }
    // pair_magnitudes' paddings
    C.ea = S.m[0] * (1 + 1e-12);
    C.eap = S.m[1] * (1 + 1e-12);
    C.exi = S.m[2] * (1 + 1e-12);
    C.eb = S.m[3] * (1 + 1e-12);
    C.ebp = S.m[4] * (1 + 1e-12);
    C.exj = S.m[5] * (1 + 1e-12);
    C.ed0 = S.m[6];
    C.ed1 = S.m[7];
    C.ex0 = S.m[8];
    C.ex1 = S.m[9];
    C.eab2 = S.m[10] * (1 + 1e-12);
    C.tie_scale = S.nonfinite ? std::numeric_limits<double>::infinity() : tie;
    // data_type_weights_[1] *= 2 * thr0 / thr1 (src/hybrid_pose_estimator.cpp:16-17)
    const double ws = w1 * (2 * thr0 / thr1);
    C.thr[0] = C.thr[1] = thr0;
    C.thr[2] = thr1;
    C.w[0] = C.w[1] = w0;
    C.w[2] = ws;
    margin_consts(C);
    return ws;
}

// mp_debug_pair_set_record's values (MP_PAIR_RECORD_VALUES), in the header's order
constexpr int kPairRecordValues = 30;
inline void pair_record_values(const PairConst &C, double norm_scale, double *out) {
    const double v[kPairRecordValues] = {
        C.thr[0],   C.thr[1],   C.thr[2],   C.w[0],     C.w[1],     C.w[2],     C.loss_scale, C.tie_scale,
        norm_scale, C.ea,       C.eap,      C.exi,      C.eb,       C.ebp,      C.exj,        C.ed0,
        C.ed1,      C.ex0,      C.ex1,      C.eab2,     C.mg_s2[0], C.mg_s2[1], C.mg_U[0],    C.mg_U[1],
        C.mg_c0[0], C.mg_c0[1], C.mg_c1[0], C.mg_c1[1], C.mg_tau2,  C.mg_fixed};
    for (int i = 0; i < kPairRecordValues; ++i) out[i] = v[i];
}

} // namespace mp
