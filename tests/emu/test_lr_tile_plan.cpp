// Host check of the time-tile plan of the low-rank sequence feature kernels (gpsig_amd/csrc/lr_tile_plan.hpp): tiles cover the steps of
// a sequence exactly once with their halo inside it, the footprints fit the LDS, the tile length is a multiple of 64, the plan says
// "untiled" exactly where the whole-sequence footprints fit, and the grid keeps the reverse pass's scratch within its budget.
#include <cstdio>
#include <vector>
#include "lr_tile_plan.hpp"

using namespace gpsig;

static int bad = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            if (++bad <= 10) std::printf("line %d: %s\n", __LINE__, #cond);                          \
        }                                                                                            \
    } while (0)

static void check_dir(const LrTileDir& D, bool reverse, int c, int r, int d, int L, int l, int halo, int pad) {
    const size_t whole = reverse ? lr_grad_lds_bytes(c, r, d, L, pad) : lr_fused_lds_bytes(c, r, d, L, pad);
    CHECK(D.untiled == (whole <= LR_FUSED_MAX_LDS));
    CHECK(D.TL % LR_TILE_STEP == 0);
    if (D.untiled) {
        CHECK(D.lds == whole && D.lp == lr_fused_stride(L, pad));
        return;
    }
    if (D.TL == 0) {                                         // refused: not even the smallest tile fits
        CHECK((reverse ? lr_tiled_grad_lds_bytes(c, r, d, LR_TILE_STEP, pad) : lr_tiled_fused_lds_bytes(c, r, d, LR_TILE_STEP, pad)) > LR_FUSED_MAX_LDS);
        return;
    }
    CHECK(D.TL >= LR_TILE_STEP && D.lds <= LR_FUSED_MAX_LDS);
    CHECK(D.lds == (reverse ? lr_tiled_grad_lds_bytes(c, r, d, D.TL, pad) : lr_tiled_fused_lds_bytes(c, r, d, D.TL, pad)));
    // the largest multiple of 64 that fits
    CHECK((reverse ? lr_tiled_grad_lds_bytes(c, r, d, D.TL + LR_TILE_STEP, pad) : lr_tiled_fused_lds_bytes(c, r, d, D.TL + LR_TILE_STEP, pad)) > LR_FUSED_MAX_LDS);
    CHECK(D.lp >= D.TL + halo && D.lp == lr_tile_stride(D.TL, pad));
    CHECK(D.ntiles == lr_tile_count(l, D.TL) && D.ntiles >= 1);
    std::vector<int> seen(size_t(l > 0 ? l : 0), 0);
    for (int k = 0; k < D.ntiles; ++k) {
        const int t0 = lr_tile_first(k, D.TL), tl = lr_tile_steps(l, k, D.TL);
        CHECK(tl >= (l > 0 ? 1 : 0) && tl <= D.TL);
        CHECK(t0 >= 0 && t0 + tl + halo <= L);               // the points the tile reads, halo included, lie inside the sequence
        CHECK(tl + halo <= D.lp);
        for (int t = t0; t < t0 + tl && t < l; ++t) ++seen[size_t(t)];
    }
    for (int t = 0; t < l; ++t) CHECK(seen[size_t(t)] == 1);
}

int main() {
    const int widths[] = {5, 16, 50, 64}, ds[] = {1, 6, 32};
    const int64_t Ns[] = {0, 1, 3, 511, 600, 100000};
    long plans = 0;
    for (int c : widths)
        for (int r : widths)
            for (int d : ds)
                for (int L = 1; L <= 600; ++L)
                    for (int difference = 0; difference < 2; ++difference)
                        for (int pad = 0; pad <= 1; ++pad) {
                            const int halo = difference, l = L - halo;
                            for (int M : {1, 2, 4, 8})
                                for (int64_t N : Ns) {
                                    const LrTilePlan P = lr_tile_plan(c, r, d, L, M, difference, pad, N);
                                    ++plans;
                                    CHECK(P.l == l && P.halo == halo);
                                    CHECK(P.grid >= 0 && P.grid <= LR_TILE_MAX_GRID && int64_t(P.grid) <= N);
                                    CHECK(P.escr_stride >= (int64_t(c) + int64_t(M > 2 ? M - 2 : 0) * r) * l);
                                    if (!P.rev.untiled)
                                        CHECK(size_t(P.grid) * size_t(P.escr_stride) * sizeof(double) <= LR_TILE_SCRATCH_BUDGET);
                                    else
                                        CHECK(P.grid == (N < LR_TILE_MAX_GRID ? N : LR_TILE_MAX_GRID));     // whole sequences: the grid as it was
                                    if (N > 0 && P.escr_stride * int64_t(sizeof(double)) <= int64_t(LR_TILE_SCRATCH_BUDGET)) CHECK(P.grid >= 1);
                                    // SignatureSpectral's reverse pass keeps kxs (c, L) per workgroup too.  Where the plan of a chunk of N sequences is a
                                    // whole-sequence one, it is the numbers gpsig_lr_seq_features_spectral_grad was written with: kxs behind the E_i, eight
                                    // doubles of slack, min(N, 512) workgroups, the whole-sequence footprint
                                    const LrTilePlan K = lr_tile_plan(c, r, d, L, M, difference, pad, N, int64_t(c) * L);
                                    CHECK(K.rev.untiled == P.rev.untiled);
                                    if (K.rev.untiled) {
                                        const int64_t kxs_off = (int64_t(c) + int64_t(M > 2 ? M - 2 : 0) * r) * (l > 0 ? l : 1);
                                        CHECK(K.escr_stride - int64_t(c) * L - 8 == kxs_off && K.escr_stride == kxs_off + int64_t(c) * L + 8);
                                        CHECK(K.grid == (N < 512 ? N : 512));
                                        CHECK(K.rev.lds == lr_grad_lds_bytes(c, r, d, L, pad));
                                    }
                                    if (M == 4 && N == 3) {
                                        check_dir(P.fwd, false, c, r, d, L, l, halo, pad);
                                        check_dir(P.rev, true, c, r, d, L, l, halo, pad);
                                    }
                                }
                        }
    // the shapes the design document quotes: 64 steps at 64 rows, 256 at 16 rows (reverse); c = r = 50 whole up to L = 64 (reverse), 128 (forward)
    CHECK(lr_tile_plan(64, 64, 3, 130, 4, 1, 1, 3).rev.TL == 64 && lr_tile_plan(64, 64, 3, 130, 4, 1, 1, 3).fwd.TL == 64);
    CHECK(lr_tile_plan(16, 16, 3, 330, 4, 1, 1, 3).rev.TL == 256);
    CHECK(lr_tile_plan(50, 50, 6, 64, 4, 1, 1, 3).rev.untiled && !lr_tile_plan(50, 50, 6, 65, 4, 1, 1, 3).rev.untiled);
    CHECK(lr_tile_plan(50, 50, 6, 128, 4, 1, 1, 3).fwd.untiled && !lr_tile_plan(50, 50, 6, 129, 4, 1, 1, 3).fwd.untiled);
    // the grid cap: c = r = 64, M = 8, L = 500 takes 1.8 MB of scratch per workgroup
    {
        const LrTilePlan P = lr_tile_plan(64, 64, 6, 500, 8, 1, 1, 1024);
        CHECK(P.grid < LR_TILE_MAX_GRID && P.grid >= 128);
        CHECK(size_t(P.grid + 1) * size_t(P.escr_stride) * sizeof(double) > LR_TILE_SCRATCH_BUDGET);
    }
    // a shape whose single 64-step tile does not fit is refused in both directions
    CHECK(lr_tile_plan(64, 100, 6, 500, 4, 1, 1, 3).rev.TL == 0 && !lr_tile_plan(64, 100, 6, 500, 4, 1, 1, 3).rev.untiled);
    std::printf("%d %ld\n", bad, plans);
    return bad != 0;
}
