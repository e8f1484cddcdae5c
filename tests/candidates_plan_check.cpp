// Stand-alone check of madpose_amd/csrc/host/candidates_plan.h (the sampler's work items, the
// candidates' offsets and tags across slabs, a winner's way back to its sample and slot) and
// of the host side of include/mp_draw.h, built with -fsanitize=address,undefined and run as a
// program by tests/test_ransac_set_cpu.py.  Prints "ok" and returns 0, or says what failed
// and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "candidates_plan.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// nsamp: samples per entry; counts: models per sample of the call; first: soff[0]
static void check_plan(const std::vector<int64_t> &nsamp, const std::vector<int32_t> &counts, int maxm,
                       int64_t sample_chunk, int64_t first) {
    const int32_t np = (int32_t)nsamp.size();
    std::vector<int64_t> soff(1, first);
    for (int64_t c : nsamp) soff.push_back(soff.back() + c);
    const int64_t S = soff.back() - first;
    CHECK((int64_t)counts.size() == S);
    const std::vector<HypSlab> slabs = hyp_slabs(S, sample_chunk);

    // ---- the sampler's items: every sample once, in order, inside its entry and its slab ----
    std::vector<DrawItem> items;
    std::vector<int> seen((size_t)S, 0);
    for (const HypSlab &s : slabs) {
        draw_items(np, soff.data(), s, items);
        CHECK((int64_t)items.size() <= s.s1 - s.s0);
        int64_t next = 0; // slab position
        for (const DrawItem &it : items) {
            CHECK(it.count >= 1 && it.count <= kDrawItemSamples);
            CHECK(it.pair >= 0 && it.pair < np);
            CHECK(it.out == next && (int64_t)it.out + it.count <= s.s1 - s.s0);
            CHECK(it.s0 >= 0 && (int64_t)it.s0 + it.count <= nsamp[(size_t)it.pair]);
            for (int i = 0; i < it.count; ++i) {
                const int64_t g = soff[(size_t)it.pair] - first + it.s0 + i; // the sample of the call
                CHECK(g == s.s0 + it.out + i);
                CHECK(seen[(size_t)g]++ == 0);
            }
            next += it.count;
        }
        CHECK(next == s.s1 - s.s0);
    }
    for (int64_t g = 0; g < S; ++g) CHECK(seen[(size_t)g] == 1);

    // ---- the candidates: the plan fed slab by slab against the direct enumeration ----
    CandPlan P;
    P.begin(np, soff.data(), maxm);
    int64_t total = 0;
    for (const HypSlab &s : slabs) {
        const int64_t nm = P.add_slab(s, counts.data() + s.s0);
        CHECK(nm == (int64_t)P.slab_pos.size());
        int64_t m = 0;
        for (int64_t b = 0; b < s.s1 - s.s0; ++b)
            for (int32_t i = 0; i < counts[(size_t)(s.s0 + b)]; ++i, ++m) {
                CHECK(P.slab_pos[(size_t)m] == b);
                CHECK(P.slot[(size_t)(total + m)] == i);
            }
        CHECK(m == nm);
        total += nm;
    }
    P.finish();
    CHECK((int64_t)P.sample.size() == total && (int64_t)P.slot.size() == total);
    CHECK((int32_t)P.moff.size() == np + 1 && P.moff[0] == 0 && P.moff[(size_t)np] == total);
    int64_t at = 0;
    for (int32_t j = 0; j < np; ++j) {
        CHECK(P.moff[(size_t)j] == at);
        int32_t index = 0;
        for (int64_t k = 0; k < nsamp[(size_t)j]; ++k)
            for (int32_t i = 0; i < counts[(size_t)(soff[(size_t)j] - first + k)]; ++i, ++at, ++index) {
                CHECK(P.sample[(size_t)at] == k && P.slot[(size_t)at] == i);
                int32_t bs = -2, bl = -2;
                cand_origin(P, j, index, &bs, &bl);
                CHECK(bs == k && bl == i);
            }
        CHECK(P.moff[(size_t)j + 1] == at);
        // (one past the entry's last candidate is refused)
        bool threw = false;
        try {
            int32_t a, b;
            cand_origin(P, j, index, &a, &b);
        } catch (const std::logic_error &) {
            threw = true;
        }
        CHECK(threw);
    }
    CHECK(at == total);
}

static void check_refusals() {
    const int64_t soff[3] = {0, 2, 5};
    CandPlan P;
    P.begin(2, soff, 4);
    const int32_t bad[5] = {0, 5, 0, 0, 0};
    bool threw = false;
    try {
        P.add_slab(HypSlab{0, 5}, bad); // a count above maxm
    } catch (const std::runtime_error &) {
        threw = true;
    }
    CHECK(threw);
    P.begin(2, soff, 4);
    const int32_t ok[5] = {1, 0, 4, 0, 2};
    threw = false;
    try {
        P.add_slab(HypSlab{2, 5}, ok + 2); // a gap
    } catch (const std::logic_error &) {
        threw = true;
    }
    CHECK(threw);
    P.begin(2, soff, 4);
    P.add_slab(HypSlab{0, 3}, ok);
    threw = false;
    try {
        P.finish(); // samples missing
    } catch (const std::logic_error &) {
        threw = true;
    }
    CHECK(threw);
    P.add_slab(HypSlab{3, 5}, ok + 3);
    P.finish();
    CHECK(P.moff[1] == 1 && P.moff[2] == 7);
}

// the host side of draw_sample: distinct indices below n, zero past the sample, the type rule
static void check_draw() {
    for (int v = 0; v < 3; ++v) {
        const int kmd = draw_k_md(v), kpt = draw_k_pt(v);
        for (int64_t n : {int64_t(0), int64_t(kmd - 1), int64_t(kmd), int64_t(kpt - 1), int64_t(kpt), int64_t(kpt + 1),
                          int64_t(64), int64_t(700), int64_t(1) << 28}) {
            for (int share : {0, 1, 128, 256}) {
                for (uint32_t s = 0; s < 300; ++s) {
                    int idx[8];
                    bool fill = false;
                    const int t = draw_sample(n, kmd, kpt, 0x0123456789abcdefull + (uint64_t)v, share, 7u, s, idx, &fill);
                    if (n < kmd) {
                        CHECK(t == -1);
                        for (int a = 0; a < 8; ++a) CHECK(idx[a] == 0);
                        continue;
                    }
                    CHECK(t == 0 || t == 1);
                    CHECK(t == draw_type(n, kpt, 0x0123456789abcdefull + (uint64_t)v, share, 7u, s));
                    if (n < kpt || share == 0) CHECK(t == 0);
                    if (n >= kpt && share == 256) CHECK(t == 1);
                    const int k = t ? kpt : kmd;
                    for (int a = 0; a < 8; ++a) {
                        if (a >= k) {
                            CHECK(idx[a] == 0);
                            continue;
                        }
                        CHECK(idx[a] >= 0 && idx[a] < n);
                        for (int b = 0; b < a; ++b) CHECK(idx[a] != idx[b]);
                    }
                    if (n > 64) CHECK(!fill); // (63 proposals of which k - 1 repeat: not at this size)
                }
            }
        }
    }
}

int main() {
    std::mt19937 rng(20260101u);
    const int64_t chunks[] = {0, 1, 16, 37, 64, 65, 1000};
    for (int rep = 0; rep < 200; ++rep) {
        const int np = 1 + (int)(rng() % 12);
        const int maxm = (rep % 3 == 0) ? 10 : (rep % 3 == 1 ? 16 : 4);
        std::vector<int64_t> nsamp;
        for (int k = 0; k < np; ++k) {
            const int kind = (int)(rng() % 6);
            nsamp.push_back(kind == 0 ? 0 : (kind == 1 ? 1 : (kind == 2 ? 64 : (kind == 3 ? 65 : rng() % 200))));
        }
        int64_t S = 0;
        for (int64_t c : nsamp) S += c;
        std::vector<int32_t> counts((size_t)S);
        for (auto &c : counts) c = (rng() % 4 == 0) ? (int32_t)(rng() % (uint32_t)(maxm + 1)) : 0;
        for (int64_t chunk : chunks) check_plan(nsamp, counts, maxm, chunk, rep % 2 ? 0 : 1234);
    }
    // no entries with samples at all, and a single entry
    check_plan({0, 0, 0}, {}, 4, 0, 0);
    check_plan({3}, {4, 0, 4}, 4, 2, 9);
    check_refusals();
    check_draw();
    std::printf("ok\n");
    return 0;
}
