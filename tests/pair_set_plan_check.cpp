// Stand-alone check of madpose_amd/csrc/host/pair_set_plan.h (the work items of the
// multi-pair preparation launch and the selection check of the pair-set calls), built with
// -fsanitize=address,undefined and run as a program by tests/test_pair_set_cpu.py.  Prints
// "ok" and returns 0, or says what failed and returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "pair_set_plan.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// the items cover every correspondence of every pair exactly once, in order, never cross a
// pair, never exceed kPrepItemMax, and a pair without correspondences gives none
static void check_items(const std::vector<int64_t> &n) {
    std::vector<PrepItem> items(3, PrepItem{-1, -1, -1, -1}); // (stale contents must go)
    prep_items((int)n.size(), n.data(), items);
    std::vector<std::vector<int>> hits(n.size());
    for (size_t k = 0; k < n.size(); ++k) hits[k].assign((size_t)n[k], 0);
    int last_pair = -1, next_first = 0;
    size_t expected = 0;
    for (int64_t v : n) expected += (size_t)((v + kPrepItemMax - 1) / kPrepItemMax);
    CHECK(items.size() == expected);
    for (const PrepItem &it : items) {
        CHECK(it.pair >= 0 && it.pair < (int)n.size());
        CHECK(it.count >= 1 && it.count <= kPrepItemMax);
        CHECK(it.first >= 0 && (int64_t)it.first + it.count <= n[(size_t)it.pair]);
        CHECK(it.pad == 0);
        // ascending pairs, and inside a pair back to back from 0
        if (it.pair != last_pair) {
            CHECK(it.pair > last_pair);
            if (last_pair >= 0) CHECK(next_first == n[(size_t)last_pair]);
            last_pair = it.pair;
            next_first = 0;
        }
        CHECK(it.first == next_first);
        next_first += it.count;
        // only the last item of a pair is short
        if ((int64_t)it.first + it.count < n[(size_t)it.pair]) CHECK(it.count == kPrepItemMax);
        for (int i = 0; i < it.count; ++i) ++hits[(size_t)it.pair][(size_t)(it.first + i)];
    }
    if (last_pair >= 0) CHECK(next_first == n[(size_t)last_pair]);
    for (size_t k = 0; k < n.size(); ++k)
        for (int h : hits[k]) CHECK(h == 1);
}

// check_selection throws std::invalid_argument whose text holds `what`, or passes (what null)
static void check_sel(int32_t num_pairs, int32_t num_sel, const std::vector<int32_t> *ids, const char *what) {
    std::vector<char> seen(7, 1); // (stale contents must go)
    bool threw = false;
    std::string msg;
    try {
        check_selection(num_pairs, num_sel, ids ? ids->data() : nullptr, seen);
    } catch (const std::invalid_argument &e) {
        threw = true;
        msg = e.what();
    }
    if (!what) {
        if (threw) std::printf("unexpected: %s\n", msg.c_str());
        CHECK(!threw);
    } else {
        CHECK(threw);
        if (msg.find(what) == std::string::npos) std::printf("message: %s (wanted %s)\n", msg.c_str(), what);
        CHECK(msg.find(what) != std::string::npos);
    }
}

int main() {
    static_assert(kPrepItemMax == 256, "one 256-thread workgroup per item");
    static_assert(kPairSetMaxCorr == (int64_t(1) << 26), "MP_PAIR_SET_MAX_CORRESPONDENCES");
    check_items({});
    check_items({0});
    check_items({1});
    check_items({255});
    check_items({256});
    check_items({257});
    check_items({0, 1, 255, 256, 257, 700});
    check_items({0, 0, 0, 0, 0, 0, 0, 0, 0});
    check_items({0, 0, 0, 5, 0, 0, 0, 0, 512, 0, 0, 513, 0});
    check_items({700, 0, 257, 256, 255, 1, 0});
    check_items({100000, 3, 0, 65536});
    {
        std::vector<int64_t> n;
        uint64_t s = 12345;
        for (int k = 0; k < 500; ++k) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const int r = (int)((s >> 33) % 8);
            n.push_back(r == 0 ? 0 : (int64_t)((s >> 40) % 1200));
        }
        check_items(n);
    }

    // ---- the selection ----
    const std::vector<int32_t> all{0, 1, 2, 3}, perm{3, 0, 2}, one{2}, rep{1, 3, 1}, high{0, 4}, neg{2, -1},
        rep_first{0, 0};
    check_sel(4, 4, nullptr, nullptr);
    check_sel(0, 0, nullptr, nullptr);
    check_sel(4, 3, nullptr, "num_sel must equal");
    check_sel(4, 0, nullptr, "num_sel must equal");
    check_sel(4, 5, nullptr, "num_sel must equal");
    check_sel(0, 1, nullptr, "num_sel must equal");
    check_sel(4, -1, nullptr, "negative");
    check_sel(4, -1, &all, "negative");
    check_sel(4, 4, &all, nullptr);
    check_sel(4, 3, &perm, nullptr);
    check_sel(4, 1, &one, nullptr);
    check_sel(4, 0, &all, nullptr); // (an empty selection with an address: nothing is read)
    check_sel(4, 3, &rep, "pair_ids[2] = 1 occurs twice");
    check_sel(4, 2, &rep, nullptr); // (the repeat lies past num_sel)
    check_sel(4, 2, &rep_first, "pair_ids[1] = 0 occurs twice");
    check_sel(4, 2, &high, "pair_ids[1] = 4 is outside");
    check_sel(5, 2, &high, nullptr);
    check_sel(4, 2, &neg, "pair_ids[1] = -1 is outside");
    check_sel(0, 1, &one, "pair_ids[0] = 2 is outside");
    // a check after a failed one starts clean
    check_sel(4, 3, &rep, "occurs twice");
    check_sel(4, 3, &perm, nullptr);
    std::printf("ok\n");
    return 0;
}
