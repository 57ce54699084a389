// ragged_plan.hpp -- the host-side plan of a ragged batch on the wide route (wide_ragged_api.hip): where every sequence's rows and its argument
// lattice start in the packed arrays, and how the batch is cut into chunks of whole sequences that fit the argument budget.  Plain C++, no HIP:
// tests/emu/test_ragged_plan.cpp runs it on the host under the sanitizers.
//
// Sequence n of a batch (N, L, d) with lengths len[n] in [1, L] is its first len[n] rows.  The packed table holds those rows back to back:
//     off[n]  = sum_{m<n} len[m]        first packed row of sequence n             (off[N]  = all rows)
//     doff[n] = sum_{m<n} len[m]^2      first cell of its len[n] x len[n] lattice  (doff[N] = all cells of the block diagonal)
// both int64: 2^20 sequences of 4,096 rows have 2^44 cells.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace gpsig {

struct RaggedPlan {
    std::vector<int32_t> len;        // (N)
    std::vector<int64_t> off, doff;  // (N + 1) each
    int32_t max_len = 0;
    int64_t rows() const { return off.empty() ? 0 : off.back(); }
    int64_t cells() const { return doff.empty() ? 0 : doff.back(); }
};

// false: a length outside [1, L] (*bad: the first such sequence) -- nothing of the plan may be used then
inline bool ragged_offsets(const int32_t* len, int64_t N, int32_t L, RaggedPlan* pl, int64_t* bad = nullptr) {
    pl->len.assign(len, len + (N > 0 ? N : 0));
    pl->off.assign(size_t(N > 0 ? N : 0) + 1, 0);
    pl->doff.assign(size_t(N > 0 ? N : 0) + 1, 0);
    pl->max_len = 0;
    for (int64_t n = 0; n < N; ++n) {
        const int32_t l = len[n];
        if (l < 1 || l > L) {
            if (bad) *bad = n;
            return false;
        }
        pl->off[n + 1] = pl->off[n] + l;
        pl->doff[n + 1] = pl->doff[n] + int64_t(l) * l;
        if (l > pl->max_len) pl->max_len = l;
    }
    return true;
}

// Chunks of whole sequences.  `pre` (N + 1): a prefix sum over the sequences (off: rows, doff: lattice cells); a chunk [a, b) costs
// (pre[b] - pre[a]) * unit_bytes.  bounds: b_0 = 0 < b_1 < ... < b_k = N, every chunk within `budget` bytes unless it is ONE sequence (a sequence
// alone beyond the budget is still served).  Greedy from the front: the cut depends on the lengths and the budget alone.
inline void ragged_chunks(const std::vector<int64_t>& pre, size_t unit_bytes, size_t budget, std::vector<int64_t>* bounds) {
    const int64_t N = int64_t(pre.size()) - 1;
    bounds->clear();
    bounds->push_back(0);
    if (N <= 0) return;
    const uint64_t units = unit_bytes ? uint64_t(budget) / uint64_t(unit_bytes) : ~uint64_t(0);       // (no product that could overflow)
    int64_t a = 0;
    while (a < N) {
        int64_t b = a + 1;
        while (b < N && uint64_t(pre[b + 1] - pre[a]) <= units) ++b;
        bounds->push_back(b);
        a = b;
    }
}

// the largest chunk's cost in units of `pre` (what the argument buffer has to hold)
inline int64_t ragged_chunk_max(const std::vector<int64_t>& pre, const std::vector<int64_t>& bounds) {
    int64_t m = 0;
    for (size_t k = 0; k + 1 < bounds.size(); ++k) {
        const int64_t u = pre[size_t(bounds[k + 1])] - pre[size_t(bounds[k])];
        if (u > m) m = u;
    }
    return m;
}

}  // namespace gpsig
