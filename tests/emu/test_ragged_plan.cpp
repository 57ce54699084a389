// Host check of the plan of a ragged batch on the wide route (gpsig_amd/csrc/ragged_plan.hpp): the offsets are the prefix sums of the lengths and of
// their squares, the chunks partition 0 .. N in order, no chunk exceeds the budget unless it is a single sequence, and the cut is greedy (a chunk
// could not have taken its successor's first sequence).  Over random length vectors, all ones, one sequence over the budget, N = 1 and N = 0; a
// length outside [1, L] is refused with its index.  Prints "<failed checks> <plans>".
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>
#include "ragged_plan.hpp"

using namespace gpsig;

static int bad = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            if (++bad <= 10) std::printf("line %d: %s\n", __LINE__, #cond);                          \
        }                                                                                            \
    } while (0)

static long plans = 0;

static void check_chunks(const std::vector<int64_t>& pre, size_t unit, size_t budget) {
    const int64_t N = int64_t(pre.size()) - 1;
    std::vector<int64_t> b;
    ragged_chunks(pre, unit, budget, &b);
    ++plans;
    CHECK(!b.empty() && b.front() == 0 && b.back() == (N > 0 ? N : 0));
    int64_t most = 0;
    for (size_t k = 0; k + 1 < b.size(); ++k) {
        CHECK(b[k] < b[k + 1]);                                            // at least one sequence, in order: a partition of 0 .. N
        const unsigned __int128 cost = (unsigned __int128)(pre[size_t(b[k + 1])] - pre[size_t(b[k])]) * unit;
        CHECK(cost <= budget || b[k + 1] - b[k] == 1);                     // within the budget, or a single sequence
        if (b[k + 1] < N) {                                                // greedy: the next sequence would not have fitted
            const unsigned __int128 more = (unsigned __int128)(pre[size_t(b[k + 1]) + 1] - pre[size_t(b[k])]) * unit;
            CHECK(more > budget);
        }
        if (pre[size_t(b[k + 1])] - pre[size_t(b[k])] > most) most = pre[size_t(b[k + 1])] - pre[size_t(b[k])];
    }
    CHECK(ragged_chunk_max(pre, b) == most);
}

static void check_batch(const std::vector<int32_t>& len, int32_t L) {
    const int64_t N = int64_t(len.size());
    RaggedPlan pl;
    int64_t at = -1;
    CHECK(ragged_offsets(len.data(), N, L, &pl, &at));
    CHECK(int64_t(pl.off.size()) == N + 1 && int64_t(pl.doff.size()) == N + 1 && int64_t(pl.len.size()) == N);
    int64_t rows = 0, cells = 0;
    int32_t longest = 0;
    for (int64_t n = 0; n < N; ++n) {
        CHECK(pl.off[size_t(n)] == rows && pl.doff[size_t(n)] == cells && pl.len[size_t(n)] == len[size_t(n)]);
        rows += len[size_t(n)];
        cells += int64_t(len[size_t(n)]) * len[size_t(n)];
        if (len[size_t(n)] > longest) longest = len[size_t(n)];
    }
    CHECK(pl.rows() == rows && pl.cells() == cells && pl.max_len == longest);
    // budgets around the sizes at hand: below one row, one sequence, a few, everything, the default 4 GB; units: a lattice cell, a row of 2,560 / 1e6 columns
    const size_t units[] = {8, 8 * 2560, size_t(8) * 1000000};
    for (size_t unit : units) {
        const size_t budgets[] = {1, unit, unit * size_t(longest > 0 ? longest : 1), unit * size_t(rows / 3 + 1), unit * size_t(cells + 1), size_t(1) << 20, size_t(4096) << 20};
        for (size_t budget : budgets) {
            check_chunks(pl.off, unit, budget);
            check_chunks(pl.doff, unit, budget);
        }
    }
}

int main() {
    std::mt19937_64 rng(12345);
    for (int trial = 0; trial < 3000; ++trial) {
        const int32_t L = int32_t(1 + rng() % 600);
        const int64_t N = trial % 50 == 0 ? 1 : int64_t(1 + rng() % 300);
        std::vector<int32_t> len(size_t(N), 1);
        const int kind = trial % 5;                                        // uniform, all ones, all L, mostly short with one long, 4 .. L
        for (int64_t n = 0; n < N; ++n) {
            if (kind == 0) len[size_t(n)] = int32_t(1 + rng() % uint64_t(L));
            else if (kind == 2) len[size_t(n)] = L;
            else if (kind == 3) len[size_t(n)] = int32_t(1 + rng() % uint64_t(L < 4 ? L : 4));
            else if (kind == 4) len[size_t(n)] = L < 4 ? L : int32_t(4 + rng() % uint64_t(L - 3));
        }
        if (kind == 3) len[size_t(rng() % uint64_t(N))] = L;              // one sequence alone over a budget sized for the others
        check_batch(len, L);
    }
    check_batch(std::vector<int32_t>(), 7);                                // N = 0: one empty partition
    check_batch(std::vector<int32_t>(1, 500), 500);
    check_batch(std::vector<int32_t>(1024, 4096), 4096);                   // 2^34 cells: beyond 32 bits
    {   // lengths outside [1, L]
        RaggedPlan pl;
        int64_t at = -1;
        const int32_t a[] = {3, 0, 2}, b[] = {3, 2, 8}, c[] = {-1};
        CHECK(!ragged_offsets(a, 3, 7, &pl, &at) && at == 1);
        CHECK(!ragged_offsets(b, 3, 7, &pl, &at) && at == 2);
        CHECK(!ragged_offsets(c, 1, 7, &pl, &at) && at == 0);
    }
    {   // a sequence alone larger than the budget is a chunk of its own, its neighbours are packed around it
        const std::vector<int64_t> pre = {0, 2, 4, 104, 106, 108};
        std::vector<int64_t> b;
        ragged_chunks(pre, 8, 8 * 4, &b);
        CHECK((b == std::vector<int64_t>{0, 2, 3, 5}));
    }
    std::printf("%d %ld\n", bad, plans);
    return bad != 0;
}
