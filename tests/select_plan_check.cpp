// Stand-alone check of madpose_amd/csrc/host/select_plan.h (the slabs and work items of
// mp_select_batch), built with -fsanitize=address,undefined and run as a program by
// tests/test_select_batch_cpu.py.  Prints "ok" and returns 0, or says what failed and
// returns 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "select_plan.h"

using namespace mp;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                               \
        }                                                               \
    } while (0)

// counts: candidates per pair; first: the value of moff[0] (a run in the middle of a call)
static void check_plan(const std::vector<int64_t> &counts, int64_t model_chunk, int tile, int64_t first) {
    const int32_t np = (int32_t)counts.size();
    std::vector<int64_t> moff(1, first);
    for (int64_t c : counts) moff.push_back(moff.back() + c);
    const int64_t M = moff.back() - first;
    const std::vector<SelectSlab> slabs = select_slabs(M, model_chunk);
    const int64_t cap = model_chunk > 0 ? model_chunk : kSelectSlabModels;
    std::vector<int> seen((size_t)M, 0);
    std::vector<SelectItem> items;
    int64_t next = 0; // the slabs, and the items inside them, are in candidate order
    for (size_t si = 0; si < slabs.size(); ++si) {
        const SelectSlab &s = slabs[si];
        CHECK(s.m0 == next && s.m1 > s.m0 && s.m1 <= M);
        CHECK(s.m1 - s.m0 <= cap);
        CHECK(s.m1 - s.m0 == cap || si + 1 == slabs.size()); // only the last may be short
        CHECK(s.m1 - s.m0 <= slabs[0].m1 - slabs[0].m0);     // the first is the largest (buffer sizes)
        select_items(np, moff.data(), s, tile, items);
        CHECK((int64_t)items.size() <= s.m1 - s.m0);
        for (const SelectItem &it : items) {
            CHECK(it.count >= 1 && it.count <= tile);                        // none is empty
            CHECK(it.pair >= 0 && it.pair < np);
            CHECK(it.rec >= 0 && (int64_t)it.rec + it.count <= s.m1 - s.m0); // none spans a slab
            const int64_t m = s.m0 + it.rec;
            CHECK(m == next);                                                // in order, no gap
            // none spans a pair
            CHECK(m >= moff[it.pair] - first && m + it.count <= moff[it.pair + 1] - first);
            for (int j = 0; j < it.count; ++j) CHECK(seen[(size_t)(m + j)]++ == 0);
            next = m + it.count;
        }
        CHECK(next == s.m1);
    }
    CHECK(next == M);
    for (int v : seen) CHECK(v == 1);
}

int main() {
    // nothing to do: no slabs, no items
    {
        CHECK(select_slabs(0, 0).empty());
        CHECK(select_slabs(0, 5).empty());
        const int64_t moff[3] = {4, 4, 4};
        std::vector<SelectItem> items(3);
        select_items(2, moff, SelectSlab{0, 0}, 4, items);
        CHECK(items.empty());
    }
    std::mt19937 rng(12345);
    std::vector<std::vector<int64_t>> cases = {
        {0}, {1}, {0, 0, 0}, {0, 1, 0}, {5, 0, 0, 7}, {0, 5, 7}, {5, 7, 0}, {37, 1, 2, 3, 4, 5, 8, 9, 0, 16},
    };
    for (int c = 0; c < 40; ++c) {
        std::vector<int64_t> counts(1 + rng() % 12);
        for (int64_t &v : counts) v = (rng() % 3 == 0) ? 0 : (int64_t)(rng() % 40);
        cases.push_back(counts);
    }
    for (const auto &counts : cases)
        for (int64_t model_chunk : {int64_t(1), int64_t(3), int64_t(7), int64_t(0)})
            for (int tile : {1, 2, 4, 8})
                for (int64_t first : {int64_t(0), int64_t(17)}) check_plan(counts, model_chunk, tile, first);
    // more candidates than the default slab: three slabs, the items of one large pair
    check_plan({10, 2 * kSelectSlabModels + 5, 3}, 0, 8, 0);
    check_plan({10, 2 * kSelectSlabModels + 5, 3}, 0, 1, 3);
    {
        const auto slabs = select_slabs(2 * kSelectSlabModels + 18, 0);
        CHECK(slabs.size() == 3 && slabs[2].m1 - slabs[2].m0 == 18);
    }
    // the exact items of one plan: pairs of 3, 0, 5 candidates, slabs of 4, tile 2
    {
        const int64_t moff[4] = {0, 3, 3, 8};
        std::vector<SelectItem> items;
        select_items(3, moff, SelectSlab{0, 4}, 2, items);
        CHECK(items.size() == 3);
        CHECK(items[0].pair == 0 && items[0].rec == 0 && items[0].count == 2);
        CHECK(items[1].pair == 0 && items[1].rec == 2 && items[1].count == 1);
        CHECK(items[2].pair == 2 && items[2].rec == 3 && items[2].count == 1);
        select_items(3, moff, SelectSlab{4, 8}, 2, items);
        CHECK(items.size() == 2);
        CHECK(items[0].pair == 2 && items[0].rec == 0 && items[0].count == 2);
        CHECK(items[1].pair == 2 && items[1].rec == 2 && items[1].count == 2);
    }
    CHECK(kSelectTile == 1 || kSelectTile == 2 || kSelectTile == 4 || kSelectTile == 8);
    std::printf("ok\n");
    return 0;
}
