// lr_tile_plan.hpp -- LDS footprints of the low-rank sequence feature kernels and the time-tile plan of their tiled forms.
// Also: the footprints of the other evaluation kernels and the predicates that pick an evaluation call's route (lr_eval_route, lr_eval_tens_route;
// SignatureSpectral beyond 32 columns: lr_spectral_eval_wide, lr_spectral_eval_tens_wide, tests/emu/test_lr_spectral_eval_route.cpp).
// HIP-free (constexpr helpers are usable on the device): read by lr_fused_args.hpp / lr_grad_kernel.hpp (the whole-sequence kernels),
// lr_tiled_kernel.hpp, lr_eval_tiled_inst.hip, the host paths of lr_grad_api.hip and lr_api.hip, tests/emu/test_lr_tile_plan.cpp and
// tests/emu/test_lr_eval_route.cpp.
//
// The whole-sequence kernels keep (width, L) arrays of a sequence in LDS: three in the forward direction (lr_fused_lds_bytes), four in the
// reverse pass (lr_grad_lds_bytes).  Where those exceed LR_FUSED_MAX_LDS, the tiled kernels walk the sequence in tiles of TL time steps
// of U: everything in the feature map is elementwise in time except the running sums, which carry one column vector per level from
// tile to tile.  With `difference`, U[t] = feat[t+1] - feat[t]: a tile of TL steps reads TL + 1 points (a halo of one).
//   TL       the largest multiple of 64 whose arrays ([column][time], row stride TL + pad >= TL + halo) and carry rows fit the LDS
//   scratch  the reverse pass keeps E_2 .. E_M of a whole sequence per workgroup, (c + (M-2) r) l doubles: the grid shrinks below
//            LR_TILE_MAX_GRID workgroups until the launch's scratch is within LR_TILE_SCRATCH_BUDGET (workgroups stride over sequences)
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace gpsig {

constexpr size_t LR_FUSED_MAX_LDS = 156 * 1024;     // of the 160 KB a CU has (one workgroup per CU at that size)

constexpr int lr_fused_stride(int L, int pad) { return (L + 63) / 64 * 64 + pad; }
// rows of the work arrays: forward max(c, r, d), reverse also a row per wavefront for the per-wave partial sums (up to 1024 threads)
constexpr int lr_fused_rows(int c, int r, int d) { return (c > r ? c : r) > d ? (c > r ? c : r) : d; }
constexpr int lr_grad_rows(int c, int r, int d) { return lr_fused_rows(c, r, d) > 16 ? lr_fused_rows(c, r, d) : 16; }
constexpr size_t lr_fused_lds_bytes(int c, int r, int d_eff, int L, int pad = 1) {
    return sizeof(double) * size_t(lr_fused_stride(L, pad)) * (size_t(c) + 2 * size_t(lr_fused_rows(c, r, d_eff)));
}
constexpr size_t lr_grad_lds_bytes(int c, int r, int d, int L, int pad = 1) {
    return sizeof(double) * size_t(lr_fused_stride(L, pad)) * 4 * size_t(lr_grad_rows(c, r, d));
}

// ---- the tiled forms
constexpr int LR_TILE_STEP = 64;                                    // tile lengths are multiples of the wavefront (lane = time)
constexpr int LR_TILE_LEVELS = 8;                                   // carry rows per direction: levels 1 .. 8
constexpr int LR_TILE_MAX_GRID = 512;                               // as the whole-sequence reverse pass
constexpr size_t LR_TILE_SCRATCH_BUDGET = size_t(256) << 20;        // bytes of per-workgroup E_i scratch per launch

constexpr int lr_tile_stride(int TL, int pad) { return TL + (pad > 0 ? pad : 1); }       // holds the halo point
// carry rows behind the arrays.  Forward: sum of U / P_i over earlier tiles per level.  Reverse: those, the column sums of dE_i over
// later tiles per level, and the later tile's first dU.
constexpr size_t lr_tiled_fused_carry(int c, int r, int d) { return size_t(LR_TILE_LEVELS) * size_t(lr_fused_rows(c, r, d)); }
constexpr size_t lr_tiled_grad_carry(int c, int r, int d) { return size_t(2 * LR_TILE_LEVELS + 1) * size_t(lr_grad_rows(c, r, d)); }
constexpr size_t lr_tiled_fused_lds_bytes(int c, int r, int d, int TL, int pad = 1) {
    return sizeof(double) * (size_t(lr_tile_stride(TL, pad)) * (size_t(c) + 2 * size_t(lr_fused_rows(c, r, d))) + lr_tiled_fused_carry(c, r, d));
}
constexpr size_t lr_tiled_grad_lds_bytes(int c, int r, int d, int TL, int pad = 1) {
    return sizeof(double) * (size_t(lr_tile_stride(TL, pad)) * 4 * size_t(lr_grad_rows(c, r, d)) + lr_tiled_grad_carry(c, r, d));
}

// tile k of a sequence of l steps: steps [t0, t0 + tl); it reads the points [t0, t0 + tl + halo)
constexpr int lr_tile_count(int l, int TL) { return l > 0 ? (l + TL - 1) / TL : 1; }
constexpr int lr_tile_first(int k, int TL) { return k * TL; }
constexpr int lr_tile_steps(int l, int k, int TL) { return l - k * TL < TL ? (l - k * TL > 0 ? l - k * TL : 0) : TL; }

struct LrTileDir {
    bool untiled;           // the whole sequence fits: the whole-sequence kernel serves the call
    int TL;                 // tile length in steps of U (0: not even a 64-step tile fits); the tiled form's, also where `untiled`
    int ntiles;
    int lp;                 // row stride of the tile arrays
    size_t lds;             // footprint of the form that serves the call
};
struct LrTilePlan {
    int l, halo;            // steps of U; points a tile reads beyond its steps
    LrTileDir fwd, rev;
    int64_t escr_stride;    // doubles of E_i scratch per workgroup (reverse)
    int grid;               // workgroups of the reverse launch (0: one workgroup's scratch exceeds the budget)
};

inline LrTileDir lr_tile_dir(bool reverse, int c, int r, int d, int L, int l, int pad) {
    LrTileDir D{};
    const size_t whole = reverse ? lr_grad_lds_bytes(c, r, d, L, pad) : lr_fused_lds_bytes(c, r, d, L, pad);
    D.untiled = whole <= LR_FUSED_MAX_LDS;
    int TL = 0;
    while ((reverse ? lr_tiled_grad_lds_bytes(c, r, d, TL + LR_TILE_STEP, pad) : lr_tiled_fused_lds_bytes(c, r, d, TL + LR_TILE_STEP, pad)) <=
               LR_FUSED_MAX_LDS &&
           TL < (1 << 20))
        TL += LR_TILE_STEP;
    D.TL = TL;
    D.ntiles = TL ? lr_tile_count(l, TL) : 0;
    D.lp = D.untiled ? lr_fused_stride(L, pad) : lr_tile_stride(TL, pad);
    D.lds = D.untiled ? whole : TL ? (reverse ? lr_tiled_grad_lds_bytes(c, r, d, TL, pad) : lr_tiled_fused_lds_bytes(c, r, d, TL, pad)) : 0;
    return D;
}

// ---- the evaluation side's tiled forward family (lr_eval_tiled.hpp): the forward layout -- U [c], two work arrays [rows], one carry row per
// level -- in the element type of the call.  float32 keeps arrays and carries in float: its own footprint, about twice the tile length.
constexpr size_t lr_eval_tiled_lds_bytes_f32(int c, int r, int d, int TL, int pad = 1) {
    return sizeof(float) * (size_t(lr_tile_stride(TL, pad)) * (size_t(c) + 2 * size_t(lr_fused_rows(c, r, d))) + lr_tiled_fused_carry(c, r, d));
}
constexpr size_t lr_eval_tiled_lds_bytes(bool f32, int c, int r, int d, int TL, int pad = 1) {
    return f32 ? lr_eval_tiled_lds_bytes_f32(c, r, d, TL, pad) : lr_tiled_fused_lds_bytes(c, r, d, TL, pad);
}
// the family's plan for sequences of l steps (as lr_tile_dir's tiled half: TL the largest multiple of 64 that fits, 0 where none does);
// `untiled` is left false -- whether a whole-sequence kernel serves the call is the caller's decision
inline LrTileDir lr_eval_tile_dir(bool f32, int c, int r, int d, int l, int pad) {
    LrTileDir D{};
    int TL = 0;
    while (lr_eval_tiled_lds_bytes(f32, c, r, d, TL + LR_TILE_STEP, pad) <= LR_FUSED_MAX_LDS && TL < (1 << 20)) TL += LR_TILE_STEP;
    D.TL = TL;
    D.ntiles = TL ? lr_tile_count(l, TL) : 0;
    D.lp = lr_tile_stride(TL, pad);
    D.lds = TL ? lr_eval_tiled_lds_bytes(f32, c, r, d, TL, pad) : 0;
    return D;
}

// ---- the other evaluation kernels' footprints (their argument blocks: lr_fused_args.hpp)
constexpr int LR_FUSED_MAX_SKETCHES = 7;            // levels 2 .. 8
// two-array form (lr_seq_features_fused2_kernel): usable for L <= 64 and at most 8 output columns per wavefront of the 512-thread workgroup
inline bool lr_fused2_ok(int c, int r, int L) { return L <= 64 && c <= 64 && r <= 64; }
inline size_t lr_fused2_lds_bytes(int c, int r, int d_eff, int L, int pad = 1) {
    int kb = c > r ? c : r;
    if (d_eff > kb) kb = d_eff;
    return sizeof(double) * size_t(lr_fused_stride(L, pad)) * 2 * size_t(kb);
}
// the fused tensor kernel: a tensor's lt E points (d_eff), their kxs and features (c each), U (lt, c) and two chain rows
inline size_t lr_tens_fused_lds_bytes(int c, int r, int d_eff, int lt, int E) {
    const size_t rows = size_t(lt) * E, w = size_t(c > r ? c : r);
    return sizeof(double) * (rows * (size_t(d_eff) + 2 * size_t(c)) + size_t(lt) * c + 2 * w);
}
inline size_t lr_fused_lds_bytes_f32(int c, int r, int d_eff, int L, int pad = 1) { return lr_fused_lds_bytes(c, r, d_eff, L, pad) / 2; }
inline size_t lr_fused2_lds_bytes_f32(int c, int r, int d_eff, int L, int pad = 1) { return lr_fused2_lds_bytes(c, r, d_eff, L, pad) / 2; }
inline size_t lr_tens_fused_lds_bytes_f32(int c, int r, int d_eff, int lt, int E) { return lr_tens_fused_lds_bytes(c, r, d_eff, lt, E) / 2; }
constexpr size_t LR_TENS_FUSED_MAX_LDS = 64 * 1024; // what the evaluation side gives the fused tensor kernel (several workgroups per CU)

// ---- which route serves an evaluation call (lr_api.hip: lr_seq_features_t, lr_tens_features_t; tests/emu/test_lr_eval_route.cpp)
//   FUSED    the whole-sequence kernels (lr_fused_kernel.hpp) / the fused tensor kernel: the object's arrays, points included, in LDS
//   TILED    the time-tiled kernels on raw points (lr_eval_tiled.hpp): a 64-step tile of max(c, r, d) rows fits
//   WIDE     beyond those: the Nystrom cross matrix on the float64 matrix cores from the raw points (lr_cross_kernel.hpp, evaluation form), then
//            the feature kernels that take it from memory (lr_kx.hpp; float32: the kx instances of the evaluation kernels).  The width d
//            enters no LDS plan: the kx plan is that of d = 0.  Families of base_eval, c <= 64, d <= 4096.
//   PASSES   the multi-pass route (float64): lr_fused = 0 at every shape, and what none of the above serves
//   REFUSE   GPSIG_ERR_UNSUPPORTED: float32 or ragged where only the multi-pass route is left
// A shape a fused or tiled kernel serves keeps it; WIDE only takes calls that were PASSES or REFUSE before it existed.
enum LrEvalRoute { LR_EVAL_FUSED = 0, LR_EVAL_TILED = 1, LR_EVAL_WIDE = 2, LR_EVAL_PASSES = 3, LR_EVAL_REFUSE = 4 };
constexpr int LR_EVAL_WIDE_MAX_C = 64;               // the cross kernel's four 16-landmark accumulator tiles
constexpr int LR_EVAL_WIDE_MAX_D = 4096;             // MAX_FEATURES_WIDE

inline bool lr_eval_wide_common(int c, int d, int M, bool spectral) {
    return !spectral && c <= LR_EVAL_WIDE_MAX_C && M - 1 <= LR_FUSED_MAX_SKETCHES && d <= LR_EVAL_WIDE_MAX_D;
}
// sequences: (N, L) points of d columns after lags; `ragged`: the call carries lengths; `spectral`: GPSIG_BASE_SPECTRAL
inline LrEvalRoute lr_eval_route(bool f32, int c, int r, int d, int L, int M, int difference, bool ragged, int lr_fused, bool spectral, int pad) {
    // two arrays in LDS instead of three where a wavefront can hold its output columns in registers: float32 tests the footprint of the
    // form it picks, float64 the three-array footprint before it may pick either
    const bool two = lr_fused == 1 && lr_fused2_ok(c, r, L);
    const size_t lds = !f32 ? lr_fused_lds_bytes(c, r, d, L, pad) : two ? lr_fused2_lds_bytes_f32(c, r, d, L, pad) : lr_fused_lds_bytes_f32(c, r, d, L, pad);
    const bool levels_ok = M - 1 <= LR_FUSED_MAX_SKETCHES;
    if (!ragged && lr_fused != 0 && lds <= LR_FUSED_MAX_LDS && levels_ok) return LR_EVAL_FUSED;
    const bool beyond = ragged || lr_fused != 0;     // ragged batches take the tiled forms whatever lr_fused says: there is no multi-pass form
    const int l = L - (difference ? 1 : 0);
    if (beyond && levels_ok && !(f32 && spectral) && lr_eval_tile_dir(f32, c, r, d, l, pad).TL > 0) return LR_EVAL_TILED;
    if (beyond && lr_eval_wide_common(c, d, M, spectral) && lr_eval_tile_dir(f32, c, r, 0, l, pad).TL > 0) return LR_EVAL_WIDE;
    return ragged || f32 ? LR_EVAL_REFUSE : LR_EVAL_PASSES;
}
// inducing tensors: T tensors of lt = M (M + 1) / 2 components of E points
inline LrEvalRoute lr_eval_tens_route(bool f32, int c, int r, int d, int M, int E, int lr_fused, bool spectral, int64_t T) {
    const int lt = M * (M + 1) / 2;
    const bool ok = lr_fused != 0 && M - 1 <= LR_FUSED_MAX_SKETCHES && T <= 0x7fffffff;
    if (ok && (f32 ? lr_tens_fused_lds_bytes_f32(c, r, d, lt, E) : lr_tens_fused_lds_bytes(c, r, d, lt, E)) <= LR_TENS_FUSED_MAX_LDS) return LR_EVAL_FUSED;
    if (ok && lr_eval_wide_common(c, d, M, spectral) &&
        (f32 ? lr_tens_fused_lds_bytes_f32(c, r, 0, lt, E) : lr_tens_fused_lds_bytes(c, r, 0, lt, E)) <= LR_TENS_FUSED_MAX_LDS)
        return LR_EVAL_WIDE;
    return f32 ? LR_EVAL_REFUSE : LR_EVAL_PASSES;
}

// ---- SignatureSpectral beyond the 32 columns of its packed table, for a kernel object that opts in (gpsig_params.base_params[2] != 0).  lr_api.hip
// asks these two only for GPSIG_BASE_SPECTRAL with the flag set and d > 32; every other call is lr_eval_route's / lr_eval_tens_route's, which
// answer as they did.  There is one route at these widths -- the evaluation form of the spectral cross kernel (lr_eval_spectral_wide_inst.hip),
// then the feature kernels that take kxs / kzs from memory, as WIDE above -- for dense and ragged calls and at any lr_fused, 0 included: the
// multi-pass route has no form here.  LR_SPX_WIDE: the call takes it; any other value names the bound that refuses it (GPSIG_ERR_UNSUPPORTED).
enum LrSpectralWide {
    LR_SPX_WIDE = 0,
    LR_SPX_F32,          // float64 only (the Python layer computes a float32 call in float64 and rounds)
    LR_SPX_COMPONENTS,   // c <= 64: the cross kernel's four accumulator tiles
    LR_SPX_LEVELS,       // M <= 8
    LR_SPX_COLUMNS,      // d <= 4096
    LR_SPX_TILE,         // sequences: a 64-step tile of max(c, r) rows in the LDS; tensors: the kx footprint within 64 KB
    LR_SPX_TENSORS       // T <= 2^31 - 1
};
inline LrSpectralWide lr_spectral_eval_common(bool f32, int c, int d, int M) {
    if (f32) return LR_SPX_F32;
    if (c > LR_EVAL_WIDE_MAX_C) return LR_SPX_COMPONENTS;
    if (M - 1 > LR_FUSED_MAX_SKETCHES) return LR_SPX_LEVELS;
    if (d > LR_EVAL_WIDE_MAX_D) return LR_SPX_COLUMNS;
    return LR_SPX_WIDE;
}
inline LrSpectralWide lr_spectral_eval_wide(bool f32, int c, int r, int d, int L, int M, int difference, int pad) {
    const LrSpectralWide w = lr_spectral_eval_common(f32, c, d, M);
    if (w != LR_SPX_WIDE) return w;
    return lr_eval_tile_dir(false, c, r, 0, L - (difference ? 1 : 0), pad).TL > 0 ? LR_SPX_WIDE : LR_SPX_TILE;
}
inline LrSpectralWide lr_spectral_eval_tens_wide(bool f32, int c, int r, int d, int M, int E, int64_t T) {
    const LrSpectralWide w = lr_spectral_eval_common(f32, c, d, M);
    if (w != LR_SPX_WIDE) return w;
    if (lr_tens_fused_lds_bytes(c, r, 0, M * (M + 1) / 2, E) > LR_TENS_FUSED_MAX_LDS) return LR_SPX_TILE;
    return T <= 0x7fffffff ? LR_SPX_WIDE : LR_SPX_TENSORS;
}

// the reverse pass's E_i scratch per workgroup, in doubles (what the whole-sequence kernel takes as well)
constexpr int64_t lr_escr_stride(int c, int r, int M, int l) { return (int64_t(c) + int64_t(M > 2 ? M - 2 : 0) * r) * (l > 0 ? l : 1) + 8; }

// (`extra`: further doubles of scratch per workgroup, under the same budget -- SignatureSpectral's reverse pass keeps kxs (c, L) there)
inline LrTilePlan lr_tile_plan(int c, int r, int d, int L, int M, int difference, int pad, int64_t N, int64_t extra = 0) {
    LrTilePlan P{};
    P.halo = difference ? 1 : 0;
    P.l = L - P.halo;
    P.fwd = lr_tile_dir(false, c, r, d, L, P.l, pad);
    P.rev = lr_tile_dir(true, c, r, d, L, P.l, pad);
    P.escr_stride = lr_escr_stride(c, r, M, P.l) + extra;
    int64_t g = N < LR_TILE_MAX_GRID ? N : LR_TILE_MAX_GRID;
    if (!P.rev.untiled) {                               // (whole sequences are short: their scratch stays small)
        const int64_t fit = int64_t(LR_TILE_SCRATCH_BUDGET / (sizeof(double) * size_t(P.escr_stride)));
        if (fit < g) g = fit;
    }
    P.grid = int(g);
    return P;
}

}  // namespace gpsig
