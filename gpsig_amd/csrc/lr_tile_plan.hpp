// lr_tile_plan.hpp -- LDS footprints of the low-rank sequence feature kernels and the time-tile plan of their tiled forms.
// HIP-free (constexpr helpers are usable on the device): read by lr_fused_args.hpp / lr_grad_kernel.hpp (the whole-sequence kernels),
// lr_tiled_kernel.hpp, lr_eval_tiled_inst.hip, the host paths of lr_grad_api.hip and api.hip, and tests/emu/test_lr_tile_plan.cpp.
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
