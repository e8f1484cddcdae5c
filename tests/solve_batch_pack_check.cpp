// Stand-alone check of the batched solvers' host packing (madpose_amd/csrc/host/
// solve_batch_pack.h), built with -fsanitize=address,undefined by
// tests/test_solver_batch_cpu.py: for ns in {0, 1, chunk - 1, chunk, chunk + 1,
// 3 chunk + 7} at K = 3 and 4 every round is planned and packed into buffers of exactly
// the size the engine allocates, and every packed value is compared with the direct
// index formula.  Exit status 0: all equal and the rounds cover the batch once.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "solve_batch_pack.h"

namespace {

int fails = 0;
#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            if (++fails < 20) std::printf("line %d: %s\n", __LINE__, #c); \
        }                                                                  \
    } while (0)

// distinct value of entry k of array a of sample s
double val(int a, int64_t s, int64_t k) { return (double)(a * 1000003 + s * 64 + k); }

void run(int K, int64_t ns, int64_t chunk) {
    std::vector<double> x((size_t)ns * 3 * K), y((size_t)ns * 3 * K), dx((size_t)ns * K), dy((size_t)ns * K);
    for (int64_t s = 0; s < ns; ++s) {
        for (int k = 0; k < 3 * K; ++k) {
            x[s * 3 * K + k] = val(0, s, k);
            y[s * 3 * K + k] = val(1, s, k);
        }
        for (int k = 0; k < K; ++k) {
            dx[s * K + k] = val(2, s, k);
            dy[s * K + k] = val(3, s, k);
        }
    }
    const int64_t rounds = mp::solve_batch_rounds(ns, chunk);
    CHECK(ns > 0 ? rounds == (ns + chunk - 1) / chunk : rounds == 0);
    const int64_t cmax = mp::solve_batch_chunk(ns, chunk), ldmax = mp::solve_batch_ld(cmax);
    CHECK(cmax >= 1 && cmax <= chunk && ldmax >= cmax && ldmax % 64 == 0 && ldmax < cmax + 64);
    const double kPad = -7.0;
    int64_t next = 0;
    for (int64_t r = 0; r < rounds; ++r) {
        int64_t s0, cnt;
        mp::solve_batch_round(ns, chunk, r, &s0, &cnt);
        CHECK(s0 == next && cnt >= 1 && cnt <= cmax && s0 + cnt <= ns);
        next = s0 + cnt;
        const int64_t ld = mp::solve_batch_ld(cnt);
        CHECK(ld <= ldmax && ld >= cnt);
        // exactly the round's extent: an index past it is a heap overflow under ASan
        std::vector<double> out((size_t)(mp::md_rows(K) * ld), kPad);
        mp::pack_md_soa(K, s0, cnt, ld, x.data(), y.data(), dx.data(), dy.data(), out.data());
        for (int64_t i = 0; i < ld; ++i) {
            for (int k = 0; k < 3 * K; ++k) {
                CHECK(out[(size_t)(k * ld + i)] == (i < cnt ? val(0, s0 + i, k) : kPad));
                CHECK(out[(size_t)((3 * K + k) * ld + i)] == (i < cnt ? val(1, s0 + i, k) : kPad));
            }
            for (int k = 0; k < K; ++k) {
                CHECK(out[(size_t)((6 * K + k) * ld + i)] == (i < cnt ? val(2, s0 + i, k) : kPad));
                CHECK(out[(size_t)((7 * K + k) * ld + i)] == (i < cnt ? val(3, s0 + i, k) : kPad));
            }
        }
        // the 7pt layout: two arrays of 14 values per sample (reusing x, y as the source
        // would need 3K = 14; pack a source of its own)
        if (K == 4 && r == rounds - 1) {
            std::vector<double> p((size_t)ns * 14), o((size_t)(14 * ld), kPad);
            for (int64_t s = 0; s < ns; ++s)
                for (int k = 0; k < 14; ++k) p[s * 14 + k] = val(4, s, k);
            mp::pack_soa(p.data(), 14, s0, cnt, ld, 0, o.data());
            for (int64_t i = 0; i < cnt; ++i)
                for (int k = 0; k < 14; ++k) CHECK(o[(size_t)(k * ld + i)] == val(4, s0 + i, k));
        }
    }
    CHECK(next == ns);
}

} // namespace

int main() {
    const int64_t chunk = 192; // a multiple of the wave and a small one beside it
    for (int64_t c : {chunk, (int64_t)37})
        for (int K : {3, 4})
            for (int64_t ns : {(int64_t)0, (int64_t)1, c - 1, c, c + 1, 3 * c + 7}) run(K, ns, c);
    // chunk 0: the default
    CHECK(mp::solve_batch_chunk(10, 0) == 10);
    CHECK(mp::solve_batch_chunk(mp::kSolveBatchMax, 0) == mp::kSolveBatchChunk);
    CHECK(mp::solve_batch_rounds(mp::kSolveBatchChunk + 3, 0) == 2);
    CHECK(mp::kSolveBatchChunk <= 65536);
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
