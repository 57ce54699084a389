// Host check of the predicates that send SignatureSpectral's low-rank evaluation calls beyond 32 columns to the wide route
// (gpsig_amd/csrc/lr_tile_plan.hpp: lr_spectral_eval_wide, lr_spectral_eval_tens_wide), over the grid of tests/emu/test_lr_eval_route.cpp.  The
// bounds are restated here from the footprints alone: float64, c <= 64, M <= 8, d <= 4096, and a 64-step tile of max(c, r) rows in the LDS
// (sequences) or a tensor's kzs arrays within 64 KB and T <= 2^31 - 1 (tensors) -- whatever `ragged` and lr_fused say, which the predicates do
// not even take.  And lr_eval_route / lr_eval_tens_route, which serve every call without the kernel object's opt-in, answer for spectral = true
// what they answered before the opt-in existed: fused, tiled, passes or refuse, never wide.
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
static size_t stride_whole(int L, int pad) { return size_t((L + 63) / 64 * 64 + pad); }
static size_t whole3(int c, int r, int d, int L, int pad) { return 8 * stride_whole(L, pad) * (size_t(c) + 2 * max3(c, r, d)); }
static size_t whole2(int c, int r, int d, int L, int pad) { return 8 * stride_whole(L, pad) * 2 * max3(c, r, d); }
static size_t tile64(bool f32, int c, int r, int d, int pad) {
    const size_t rows = max3(c, r, d);
    return (f32 ? 4 : 8) * (size_t(64 + (pad > 0 ? pad : 1)) * (size_t(c) + 2 * rows) + 8 * rows);
}
static const size_t LDS = 156 * 1024;
static size_t tens_bytes(bool f32, int c, int r, int d, int lt, int E) {
    const size_t b = 8 * (size_t(lt) * E * (size_t(d) + 2 * size_t(c)) + size_t(lt) * c + 2 * size_t(c > r ? c : r));
    return f32 ? b / 2 : b;
}

// the spectral answers of lr_eval_route / lr_eval_tens_route as they were
static LrEvalRoute spectral_seq(bool f32, int c, int r, int d, int L, int M, bool ragged, int lr_fused, int pad) {
    const bool two = lr_fused == 1 && L <= 64 && c <= 64 && r <= 64;
    const size_t lds = !f32 ? whole3(c, r, d, L, pad) : two ? whole2(c, r, d, L, pad) / 2 : whole3(c, r, d, L, pad) / 2;
    if (!ragged && lr_fused != 0 && lds <= LDS && M <= 8) return LR_EVAL_FUSED;
    if ((ragged || lr_fused != 0) && tile64(f32, c, r, d, pad) <= LDS && M <= 8 && !f32) return LR_EVAL_TILED;
    return ragged || f32 ? LR_EVAL_REFUSE : LR_EVAL_PASSES;
}
static LrEvalRoute spectral_tens(bool f32, int c, int r, int d, int M, int E, int lr_fused, int64_t T) {
    if (lr_fused != 0 && tens_bytes(f32, c, r, d, M * (M + 1) / 2, E) <= 64 * 1024 && M <= 8 && T <= 0x7fffffff) return LR_EVAL_FUSED;
    return f32 ? LR_EVAL_REFUSE : LR_EVAL_PASSES;
}

int main() {
    long cases = 0, wides = 0;
    const int cs[] = {8, 16, 50, 64, 65, 100}, ds[] = {3, 32, 33, 63, 64, 65, 121, 122, 126, 160, 320, 1928, 4096, 4097};
    const int Ls[] = {1, 64, 65, 70, 130, 500}, Ms[] = {1, 4, 8, 9};
    for (int f32 = 0; f32 < 2; ++f32)
        for (int c : cs)
            for (int r : cs)
                for (int d : ds)
                    for (int L : Ls)
                        for (int M : Ms)
                            for (int difference = 0; difference < 2; ++difference)
                                for (int pad = 0; pad <= 1; ++pad) {
                                    ++cases;
                                    const bool want = !f32 && c <= 64 && M <= 8 && d <= 4096 && tile64(false, c, r, 0, pad) <= LDS;
                                    const LrSpectralWide got = lr_spectral_eval_wide(f32, c, r, d, L, M, difference, pad);
                                    CHECK((got == LR_SPX_WIDE) == want);
                                    wides += want;
                                    // the refusal names the first bound that fails
                                    if (f32) CHECK(got == LR_SPX_F32);
                                    else if (c > 64) CHECK(got == LR_SPX_COMPONENTS);
                                    else if (M > 8) CHECK(got == LR_SPX_LEVELS);
                                    else if (d > 4096) CHECK(got == LR_SPX_COLUMNS);
                                    else if (!want) CHECK(got == LR_SPX_TILE);
                                    for (int ragged = 0; ragged < 2; ++ragged)
                                        for (int lr_fused = 0; lr_fused <= 2; ++lr_fused)
                                            CHECK(lr_eval_route(f32, c, r, d, L, M, difference, ragged, lr_fused, true, pad) ==
                                                  spectral_seq(f32, c, r, d, L, M, ragged, lr_fused, pad));
                                }
    // the shapes the issue names: one past the line, the tile, a second pass, three passes, CMUsubject16's spectral form, the widest
    for (int d : {33, 64, 65, 160, 63, 4096})
        for (int L : {70, 130, 500}) {
            CHECK(lr_spectral_eval_wide(false, 8, 8, d, L, 3, 1, 1) == LR_SPX_WIDE);
            CHECK(lr_spectral_eval_wide(false, 50, 50, d, L, 4, 1, 1) == LR_SPX_WIDE);
        }
    CHECK(lr_spectral_eval_wide(false, 65, 8, 160, 70, 3, 1, 1) == LR_SPX_COMPONENTS);
    CHECK(lr_spectral_eval_wide(false, 8, 8, 160, 70, 9, 1, 1) == LR_SPX_LEVELS);
    CHECK(lr_spectral_eval_wide(false, 8, 8, 4097, 70, 3, 1, 1) == LR_SPX_COLUMNS);
    CHECK(lr_spectral_eval_wide(true, 8, 8, 160, 70, 3, 1, 1) == LR_SPX_F32);
    CHECK(lr_spectral_eval_wide(false, 16, 160, 40, 70, 3, 1, 1) == LR_SPX_TILE);      // 65 c + 138 r doubles exceed the LDS
    // what the existing tests pin of lr_eval_route for a spectral kernel object
    CHECK(lr_eval_route(false, 8, 8, 160, 70, 4, 1, false, 1, true, 1) == LR_EVAL_PASSES);
    CHECK(lr_eval_route(false, 8, 8, 160, 70, 4, 1, true, 1, true, 1) == LR_EVAL_REFUSE);

    // ---- tensors
    const int64_t Ts[] = {3, 500, int64_t(1) << 31};
    for (int f32 = 0; f32 < 2; ++f32)
        for (int c : cs)
            for (int r : cs)
                for (int d : ds)
                    for (int M : Ms)
                        for (int E = 1; E <= 2; ++E)
                            for (int64_t T : Ts) {
                                ++cases;
                                const bool want = !f32 && c <= 64 && M <= 8 && d <= 4096 && T <= 0x7fffffff &&
                                                  tens_bytes(false, c, r, 0, M * (M + 1) / 2, E) <= 64 * 1024;
                                const LrSpectralWide got = lr_spectral_eval_tens_wide(f32, c, r, d, M, E, T);
                                CHECK((got == LR_SPX_WIDE) == want);
                                wides += want;
                                for (int lr_fused = 0; lr_fused <= 2; ++lr_fused)
                                    CHECK(lr_eval_tens_route(f32, c, r, d, M, E, lr_fused, true, T) == spectral_tens(f32, c, r, d, M, E, lr_fused, T));
                            }
    CHECK(lr_spectral_eval_tens_wide(false, 8, 8, 160, 3, 2, 3) == LR_SPX_WIDE);
    CHECK(lr_spectral_eval_tens_wide(false, 50, 50, 63, 4, 2, 500) == LR_SPX_WIDE);
    CHECK(lr_spectral_eval_tens_wide(false, 8, 8, 160, 3, 2, int64_t(1) << 31) == LR_SPX_TENSORS);
    CHECK(lr_spectral_eval_tens_wide(false, 64, 64, 160, 8, 2, 3) == LR_SPX_TILE);      // 72 (2 c) + 36 c + 2 c doubles exceed 64 KB
    CHECK(lr_eval_tens_route(false, 16, 16, 240, 5, 2, 1, true, 3) == LR_EVAL_PASSES);
    std::printf("%d %ld %ld\n", bad, cases, wides);
    return bad != 0;
}
