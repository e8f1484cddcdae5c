// Stand-alone check of madpose_amd/csrc/host/ingest_plan.h (the work items of the device
// ingest, the byte-extent arithmetic behind the device pointers' checks, and the finishing of a
// pair's record from its statistics), built with -fsanitize=address,undefined and run as a
// program by tests/test_pair_set_ingest_cpu.py.  Prints "ok" and returns 0, or says what failed
// and returns 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "ingest_plan.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// the items cover every correspondence of every pair exactly once, in order, never cross a
// pair, never exceed kIngestSpan, a pair without correspondences gives none, and first_item
// brackets each pair's items
static void check_items(const std::vector<int64_t> &n) {
    std::vector<IngestItem> items(3, IngestItem{-1, -1, -1, -1}); // (stale contents must go)
    std::vector<int64_t> first_item(1, 99);
    ingest_items((int)n.size(), n.data(), items, first_item);
    CHECK(first_item.size() == n.size() + 1);
    size_t at = 0;
    for (size_t k = 0; k < n.size(); ++k) {
        CHECK(first_item[k] == (int64_t)at);
        int64_t next = 0;
        while (next < n[k]) {
            CHECK(at < items.size());
            const IngestItem &it = items[at++];
            CHECK(it.pair == (int)k && it.pad == 0);
            CHECK((int64_t)it.first == next);
            CHECK(it.count >= 1 && it.count <= kIngestSpan);
            CHECK(it.first % kIngestSpan == 0);
            // only a pair's last item is short
            CHECK(it.count == kIngestSpan || next + it.count == n[k]);
            next += it.count;
        }
        CHECK(next == n[k]);
    }
    CHECK(at == items.size());
    CHECK(first_item[n.size()] == (int64_t)items.size());
}

static void check_bytes_and_extents() {
    const int64_t big = std::numeric_limits<int64_t>::max();
    CHECK(ingest_bytes(0, 2, 8) == 0);
    CHECK(ingest_bytes(7, 2, 4) == 56);
    CHECK(ingest_bytes(int64_t(1) << 26, 2, 8) == int64_t(1) << 30);
    CHECK(ingest_bytes(-1, 2, 8) == -1);
    CHECK(ingest_bytes(1, 0, 8) == -1);
    CHECK(ingest_bytes(1, 1, 0) == -1);
    CHECK(ingest_bytes(big, 1, 1) == big);
    CHECK(ingest_bytes(big, 2, 1) == -1);
    CHECK(ingest_bytes(big / 2, 2, 1) == big - 1);
    CHECK(ingest_bytes(big / 2 + 1, 2, 1) == -1);
    CHECK(ingest_bytes(big / 8, 1, 8) == big - 7);
    CHECK(ingest_bytes(big / 8 + 1, 1, 8) == -1);
    CHECK(ingest_bytes(int64_t(1) << 31, int64_t(1) << 31, 2) == -1); // 2^63
    CHECK(ingest_bytes(int64_t(1) << 31, int64_t(1) << 31, 1) == int64_t(1) << 62);
    CHECK(ingest_bytes(int64_t(1) << 40, int64_t(1) << 40, 4) == -1);

    const uint64_t base = 0x7f0000000000ull, size = 4096;
    CHECK(!ingest_extent_error(base, base, size, 4096, 8));
    CHECK(!ingest_extent_error(base, base, size, 0, 8));
    CHECK(!ingest_extent_error(base + 4096, base, size, 0, 8)); // nothing read at the very end
    CHECK(ingest_extent_error(base, base, size, 4097, 1));
    CHECK(ingest_extent_error(base, base, size, 4104, 8));
    CHECK(!ingest_extent_error(base + 16, base, size, 4080, 8));
    CHECK(ingest_extent_error(base + 16, base, size, 4088, 8)); // two elements short
    CHECK(ingest_extent_error(base + 4, base, size, 8, 8));     // not aligned to a double
    CHECK(!ingest_extent_error(base + 4, base, size, 8, 4));    // ... but to a float
    CHECK(ingest_extent_error(base + 2, base, size, 4, 4));
    CHECK(ingest_extent_error(base - 8, base, size, 8, 8));     // before the allocation
    CHECK(ingest_extent_error(base + 4104, base, size, 0, 8));  // past it
    CHECK(ingest_extent_error(base, base, size, -1, 8));        // an overflowed byte count
    CHECK(ingest_extent_error(base, base, size, big, 1));
    // the int64 / uint64 edges: no sum of address and length is ever formed
    const uint64_t top = std::numeric_limits<uint64_t>::max();
    CHECK(ingest_extent_error(top - 7, top - 4095, 4096, 16, 8));
    CHECK(!ingest_extent_error(top - 7, top - 4095, 4095, 7, 1));
    CHECK(ingest_extent_error(top - 7, top - 4095, 4095, 8, 1));
    CHECK(ingest_extent_error(8, 0, 16, big, 8));
    CHECK(!ingest_extent_error(0, 0, top, big, 1));
    CHECK(!ingest_extent_error(8, 0, top, big - 7, 8));
    CHECK(ingest_extent_error(top - 15, 0, top, big, 8));
    CHECK(ingest_extent_error(16, 32, top - 32, 8, 8));
}

static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

// make_problem's tail, written out from its formulas on fixed statistics
static void check_finish(int variant, double scale, bool nonfinite, int n) {
    PairConst C;
    std::memset(&C, 0, sizeof(C));
    C.variant = variant;
    C.n = n;
    const double K[9] = {525.0, 0.5, 319.5, 0.0, 530.0, 239.5, 0.0, 0.0, 1.0};
    const double Ki[9] = {1.0 / 525.0, -0.5 / (525.0 * 530.0), -0.6, 0.0, 1.0 / 530.0, -0.45, 0.0, 0.0, 1.0};
    for (int i = 0; i < 9; ++i) {
        C.K0[i] = C.K1[i] = variant == kCal ? K[i] : (i % 4 == 0 ? 1.0 : 0.0);
        C.K0i[i] = C.K1i[i] = variant == kCal ? Ki[i] : (i % 4 == 0 ? 1.0 : 0.0);
    }
    C.loss_scale = variant == kCal ? 1.0 / ((2.0 / 1055.0) * (2.0 / 1055.0)) : 1.0;
    IngestStats S;
    const double m[kIngestStatValues] = {1.9, 2.3, 1.7, 2.1, 2.6, 1.4, 9.25, 11.5, 640.0, 700.5, 37.0};
    for (int i = 0; i < kIngestStatValues; ++i) S.m[i] = m[i];
    S.nonfinite = nonfinite ? 1 : 0;
    S.pad = 0;
    const double thr0 = 16.0, thr1 = 4.0, w0 = 1.0, w1 = 1.5, tie = 3.0;
    const PairConst before = C;
    const double ws = ingest_finish(C, S, scale, thr0, thr1, w0, w1, tie);

    PairConst E = before;
    double t0 = thr0, t1 = thr1;
    if (variant != kCal) {
        const volatile double s2 = scale * scale; // (one rounding, as the header's own division)
        t0 = t0 / s2;
        t1 = t1 / s2;
    }
    const double pad = 1 + 1e-12;
    E.ea = m[0] * pad, E.eap = m[1] * pad, E.exi = m[2] * pad, E.eb = m[3] * pad, E.ebp = m[4] * pad, E.exj = m[5] * pad;
    E.ed0 = m[6], E.ed1 = m[7], E.ex0 = m[8], E.ex1 = m[9], E.eab2 = m[10] * pad;
    E.tie_scale = nonfinite ? std::numeric_limits<double>::infinity() : tie;
    const double ews = w1 * (2 * t0 / t1);
    E.thr[0] = E.thr[1] = t0;
    E.thr[2] = t1;
    E.w[0] = E.w[1] = w0;
    E.w[2] = ews;
    margin_consts(E);
    CHECK(same(ws, ews));
    CHECK(std::memcmp(&C, &E, sizeof(PairConst)) == 0);
    // the data-independent part was not touched, the thresholds are the options' over scale^2
    CHECK(C.variant == variant && C.n == n && same(C.loss_scale, before.loss_scale));
    CHECK(std::memcmp(C.K0i, before.K0i, sizeof(C.K0i)) == 0);
    if (variant == kCal) CHECK(same(C.thr[0], 16.0) && same(C.thr[2], 4.0));
    if (variant != kCal && scale == 2.0) CHECK(same(C.thr[0], 4.0) && same(C.thr[2], 1.0) && same(C.w[2], 12.0));
    CHECK(std::isinf(C.tie_scale) == nonfinite);
    // the record hook's order
    double rec[kPairRecordValues];
    pair_record_values(C, scale, rec);
    CHECK(same(rec[0], C.thr[0]) && same(rec[2], C.thr[2]) && same(rec[5], C.w[2]) && same(rec[6], C.loss_scale));
    CHECK(same(rec[7], C.tie_scale) && same(rec[8], scale) && same(rec[9], C.ea) && same(rec[19], C.eab2));
    CHECK(same(rec[20], C.mg_s2[0]) && same(rec[25], C.mg_c0[1]) && same(rec[28], C.mg_tau2) &&
          same(rec[29], C.mg_fixed));
}

static void check_merge() {
    IngestStats a, b;
    std::memset(&a, 0, sizeof(a));
    std::memset(&b, 0, sizeof(b));
    a.m[0] = 2.0, b.m[0] = 3.0;
    a.m[1] = 5.0, b.m[1] = std::nan("");
    a.m[2] = 1.0, b.m[2] = std::numeric_limits<double>::infinity();
    b.nonfinite = 1;
    ingest_merge(a, b);
    CHECK(a.m[0] == 3.0 && a.m[1] == 5.0 && std::isinf(a.m[2]) && a.m[3] == 0.0 && a.nonfinite == 1);
    CHECK(ingest_max(0.0, std::nan("")) == 0.0);
}

int main() {
    const int c[3] = {kIngestBlock, kIngestChunk, kIngestSpan};
    std::vector<int64_t> n = {0, 1, 5, 7, 63, 64, 65, 255, 256, 257, 1100};
    for (int v : c)
        for (int64_t s : {(int64_t)v - 1, (int64_t)v, (int64_t)v + 1, 2 * (int64_t)v + 1}) n.push_back(s);
    check_items(n);
    check_items({});
    check_items({0, 0, 0});
    check_items({kIngestSpan, 0, kIngestSpan});
    // 2^28-scale: the largest pair (kRefinePairMax), alone and between neighbours
    const int64_t big = int64_t(1) << 28;
    check_items({big});
    check_items({3, big - 1, 0, big, 1});
    check_bytes_and_extents();
    for (int variant : {0, 1, 2})
        for (double scale : {1.0, 2.0, 173.20508075688772})
            for (bool nf : {false, true}) check_finish(variant, variant == kCal ? 1.0 : scale, nf, 1100);
    check_finish(1, 1.0, false, 0);
    check_merge();
    std::printf("ok\n");
    return 0;
}
