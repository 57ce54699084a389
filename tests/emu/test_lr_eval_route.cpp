// Host check of the route predicates of the low-rank evaluation entry points (gpsig_amd/csrc/lr_tile_plan.hpp: lr_eval_route,
// lr_eval_tens_route).  The conditions under which gpsig_lr_seq_features / _ragged / gpsig_lr_tens_features picked the fused kernels, the tiled
// kernels, the multi-pass route or a refusal BEFORE the wide route existed are restated here from the footprints alone; the predicate has to
// agree with them wherever it does not answer "wide", and "wide" may only replace "passes" or "refuse".
#include <cstdio>
#include <cstdint>
#include <initializer_list>
#include "lr_tile_plan.hpp"

using namespace gpsig;

static int bad = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) {                                                                               \
            if (++bad <= 10) std::printf("line %d: %s\n", __LINE__, #cond);                          \
        }                                                                                            \
    } while (0)

static size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// ---- the rules as they were (sequences): footprints in bytes, written out
static size_t stride_whole(int L, int pad) { return size_t((L + 63) / 64 * 64 + pad); }
static size_t whole3(int c, int r, int d, int L, int pad) { return 8 * stride_whole(L, pad) * (size_t(c) + 2 * max3(c, r, d)); }
static size_t whole2(int c, int r, int d, int L, int pad) { return 8 * stride_whole(L, pad) * 2 * max3(c, r, d); }
static size_t tile64(bool f32, int c, int r, int d, int pad) {
    const size_t rows = max3(c, r, d);
    return (f32 ? 4 : 8) * (size_t(64 + (pad > 0 ? pad : 1)) * (size_t(c) + 2 * rows) + 8 * rows);
}
static const size_t LDS = 156 * 1024;

static LrEvalRoute old_seq(bool f32, int c, int r, int d, int L, int M, bool ragged, int lr_fused, bool spectral, int pad) {
    const bool two = lr_fused == 1 && L <= 64 && c <= 64 && r <= 64;
    const size_t lds = !f32 ? whole3(c, r, d, L, pad) : two ? whole2(c, r, d, L, pad) / 2 : whole3(c, r, d, L, pad) / 2;
    const bool levels_ok = M <= 8;
    const bool fused = !ragged && lr_fused != 0 && lds <= LDS && levels_ok;
    const bool tiled = !fused && (ragged || lr_fused != 0) && tile64(f32, c, r, d, pad) <= LDS && levels_ok && !(f32 && spectral);
    if (fused) return LR_EVAL_FUSED;
    if (tiled) return LR_EVAL_TILED;
    if (ragged || f32) return LR_EVAL_REFUSE;
    return LR_EVAL_PASSES;
}
// ... and where the wide route takes a call that was "passes" or "refuse"
static bool wide_seq(bool f32, int c, int r, int d, int M, bool ragged, int lr_fused, bool spectral, int pad) {
    return (ragged || lr_fused != 0) && !spectral && c <= 64 && M <= 8 && d <= 4096 && tile64(f32, c, r, 0, pad) <= LDS;
}

// ---- tensors
static size_t tens_bytes(bool f32, int c, int r, int d, int lt, int E) {
    const size_t b = 8 * (size_t(lt) * E * (size_t(d) + 2 * size_t(c)) + size_t(lt) * c + 2 * size_t(c > r ? c : r));
    return f32 ? b / 2 : b;
}
static LrEvalRoute old_tens(bool f32, int c, int r, int d, int M, int E, int lr_fused, int64_t T) {
    const bool fused = lr_fused != 0 && tens_bytes(f32, c, r, d, M * (M + 1) / 2, E) <= 64 * 1024 && M <= 8 && T <= 0x7fffffff;
    if (fused) return LR_EVAL_FUSED;
    return f32 ? LR_EVAL_REFUSE : LR_EVAL_PASSES;
}
static bool wide_tens(bool f32, int c, int r, int d, int M, int E, int lr_fused, bool spectral, int64_t T) {
    return lr_fused != 0 && !spectral && c <= 64 && M <= 8 && d <= 4096 && T <= 0x7fffffff && tens_bytes(f32, c, r, 0, M * (M + 1) / 2, E) <= 64 * 1024;
}

int main() {
    long cases = 0, wides = 0;
    const int cs[] = {8, 16, 50, 64, 65, 100}, ds[] = {3, 32, 121, 122, 126, 160, 320, 1928, 4096, 4097};
    const int Ls[] = {1, 64, 65, 70, 130, 500}, Ms[] = {1, 4, 8, 9};
    for (int f32 = 0; f32 < 2; ++f32)
        for (int c : cs)
            for (int r : cs)
                for (int d : ds)
                    for (int L : Ls)
                        for (int M : Ms)
                            for (int ragged = 0; ragged < 2; ++ragged)
                                for (int lr_fused = 0; lr_fused <= 2; ++lr_fused)
                                    for (int spectral = 0; spectral < 2; ++spectral)
                                        for (int difference = 0; difference < 2; ++difference)
                                            for (int pad = 0; pad <= 1; ++pad) {
                                                ++cases;
                                                const LrEvalRoute got = lr_eval_route(f32, c, r, d, L, M, difference, ragged, lr_fused, spectral, pad);
                                                const LrEvalRoute was = old_seq(f32, c, r, d, L, M, ragged, lr_fused, spectral, pad);
                                                if (was == LR_EVAL_FUSED || was == LR_EVAL_TILED) {
                                                    CHECK(got == was);                  // a shape a fused or tiled kernel serves keeps it
                                                } else if (wide_seq(f32, c, r, d, M, ragged, lr_fused, spectral, pad)) {
                                                    CHECK(got == LR_EVAL_WIDE);
                                                    ++wides;
                                                } else {
                                                    CHECK(got == was);
                                                }
                                                if (!ragged && lr_fused == 0) CHECK(got == (f32 ? LR_EVAL_REFUSE : LR_EVAL_PASSES));
                                            }
    // the shapes the issue names: CMUsubject16, the smallest float64 / float32 shapes beyond the tiled kernels, PEMS
    const struct { bool f32; int c, r, d; } named[] = {{false, 50, 50, 126}, {false, 8, 8, 160}, {true, 8, 8, 320}, {false, 50, 50, 1928}};
    for (const auto& s : named)
        for (int L : {70, 130, 500}) {
            CHECK(lr_eval_route(s.f32, s.c, s.r, s.d, L, 4, 1, false, 1, false, 1) == LR_EVAL_WIDE);
            CHECK(lr_eval_route(s.f32, s.c, s.r, s.d, L, 4, 1, false, 2, false, 1) == LR_EVAL_WIDE);
            for (int lr_fused = 0; lr_fused <= 2; ++lr_fused) CHECK(lr_eval_route(s.f32, s.c, s.r, s.d, L, 4, 1, true, lr_fused, false, 1) == LR_EVAL_WIDE);
            CHECK(lr_eval_route(s.f32, s.c, s.r, s.d, L, 4, 1, false, 0, false, 1) == (s.f32 ? LR_EVAL_REFUSE : LR_EVAL_PASSES));
        }
    // one column fewer than the bound is the tiled kernels' still: 65 c + 138 max(c, r, d) <= 19,968 doubles
    CHECK(lr_eval_route(false, 50, 50, 121, 500, 4, 1, false, 1, false, 1) == LR_EVAL_TILED);
    CHECK(lr_eval_route(false, 50, 50, 122, 500, 4, 1, false, 1, false, 1) == LR_EVAL_WIDE);
    CHECK(lr_eval_route(false, 8, 8, 3, 70, 4, 1, false, 1, false, 1) == LR_EVAL_FUSED);
    CHECK(lr_eval_route(false, 64, 64, 3, 130, 4, 1, false, 1, false, 1) == LR_EVAL_TILED);
    // what stays as it was: SignatureSpectral and c > 64, dense (multi-pass) and ragged (refused)
    CHECK(lr_eval_route(false, 8, 8, 160, 70, 4, 1, false, 1, true, 1) == LR_EVAL_PASSES);
    CHECK(lr_eval_route(false, 8, 8, 160, 70, 4, 1, true, 1, true, 1) == LR_EVAL_REFUSE);
    CHECK(lr_eval_route(false, 65, 65, 160, 70, 4, 1, false, 1, false, 1) == LR_EVAL_PASSES);
    CHECK(lr_eval_route(false, 65, 65, 160, 70, 4, 1, true, 1, false, 1) == LR_EVAL_REFUSE);
    CHECK(lr_eval_route(true, 65, 65, 320, 70, 4, 1, false, 1, false, 1) == LR_EVAL_REFUSE);

    // ---- tensors
    const int64_t Ts[] = {3, 500, int64_t(1) << 31};
    for (int f32 = 0; f32 < 2; ++f32)
        for (int c : cs)
            for (int r : cs)
                for (int d : ds)
                    for (int M : Ms)
                        for (int E = 1; E <= 2; ++E)
                            for (int lr_fused = 0; lr_fused <= 2; ++lr_fused)
                                for (int spectral = 0; spectral < 2; ++spectral)
                                    for (int64_t T : Ts) {
                                        ++cases;
                                        const LrEvalRoute got = lr_eval_tens_route(f32, c, r, d, M, E, lr_fused, spectral, T);
                                        const LrEvalRoute was = old_tens(f32, c, r, d, M, E, lr_fused, T);
                                        if (was == LR_EVAL_FUSED) CHECK(got == was);
                                        else if (wide_tens(f32, c, r, d, M, E, lr_fused, spectral, T)) { CHECK(got == LR_EVAL_WIDE); ++wides; }
                                        else CHECK(got == was);
                                        CHECK(got != LR_EVAL_TILED);
                                    }
    CHECK(lr_eval_tens_route(false, 16, 16, 240, 5, 2, 1, false, 3) == LR_EVAL_WIDE);
    CHECK(lr_eval_tens_route(true, 16, 16, 512, 5, 2, 1, false, 3) == LR_EVAL_WIDE);
    CHECK(lr_eval_tens_route(false, 50, 50, 1928, 4, 2, 1, false, 500) == LR_EVAL_WIDE);
    CHECK(lr_eval_tens_route(false, 50, 50, 145, 5, 2, 1, false, 500) == LR_EVAL_WIDE);
    CHECK(lr_eval_tens_route(false, 50, 50, 144, 5, 2, 1, false, 500) == LR_EVAL_FUSED);
    CHECK(lr_eval_tens_route(false, 16, 16, 240, 5, 2, 0, false, 3) == LR_EVAL_PASSES);
    CHECK(lr_eval_tens_route(true, 16, 16, 512, 5, 2, 0, false, 3) == LR_EVAL_REFUSE);
    CHECK(lr_eval_tens_route(false, 16, 16, 240, 5, 2, 1, true, 3) == LR_EVAL_PASSES);
    CHECK(lr_eval_tens_route(false, 16, 16, 3, 5, 2, 1, false, 3) == LR_EVAL_FUSED);
    std::printf("%d %ld %ld\n", bad, cases, wides);
    return bad != 0;
}
