// grad_plan.hpp -- which compiled instance of the sequence-gradient sweeps a call runs: the lists of compiled shapes and the shape decisions of
// wave_plan, wave2_plan, lam_undo_plan and ho_sweeps_plan (grad_api.hip), as plain integer functions.  No HIP in here: the instantiation lists
// (grad_wave_inst.hpp, grad_wave_ho_inst.hpp) and the planners read the same lists, and tests/emu/test_grad_plan.cpp compiles this header with g++
// alone (tests/test_grad_plan_host.py).
#pragma once
#include <cstddef>

namespace gpsig {

// ---- compiled shapes ---------------------------------------------------------------------------------------------------------------
// first order -- seq_grad_wave_kernel, seq_grad_wave2_kernel, seq_lam_undo_kernel -- (G, C, DP): lanes per pair, columns per lane, padded
// feature count.  C * DP bounded by the register file.
#define GPSIG_WAVE_SHAPES(X) \
    X(16, 2, 4) X(16, 2, 8) X(16, 2, 16) X(16, 4, 4) X(16, 4, 8) X(16, 4, 16) \
    X(64, 2, 4) X(64, 2, 8) X(64, 2, 16) X(64, 4, 4) X(64, 4, 8) X(64, 4, 16) X(64, 8, 4) X(64, 8, 8)

// higher order, scratch-free (seq_grad_wave_ho_undo_kernel; the forward seq_levels_wave_ho_kernel has the same forms): (G, C) and (num_levels, order)
#define GPSIG_HO_UNDO_FORMS(X) X(16, 2) X(16, 4) X(32, 2) X(64, 2) X(64, 4) X(64, 8)
#define GPSIG_HO_UNDO_LEVELS(X) X(2, 2) X(3, 2) X(3, 3) X(4, 2) X(4, 3) X(4, 4) X(5, 2) X(5, 3) X(5, 4)
// higher order, prefixes in an HBM slot (seq_grad_wave_ho_kernel): (G, C) and the order; num_levels 2 .. 5 at run time
#define GPSIG_HO_SLOT_FORMS(X) X(16, 2) X(16, 4) X(64, 2) X(64, 4) X(64, 8)
#define GPSIG_HO_SLOT_ORDERS(X) X(2) X(3) X(4)
constexpr int HO_SLOT_MIN_LEVELS = 2, HO_SLOT_MAX_LEVELS = 5;

// lattice modes (seq_core.hpp: MODE_INC, MODE_PT_DIFF, MODE_PT_NODIFF) restated for the host tests; grad_api.hip asserts they are the same numbers
enum : int { GRAD_MODE_INC = 0, GRAD_MODE_PT_DIFF = 1, GRAD_MODE_PT_NODIFF = 2 };

enum GradFamily : int { GRAD_NONE = 0, GRAD_WAVE = 1, GRAD_WAVE2 = 2, GRAD_LAM_UNDO = 3, GRAD_HO_UNDO = 4, GRAD_HO_SLOT = 5 };

// Level variants of the scratch-free first-order kernels (template arguments LQ, MX): num_levels 4 and 5 at compile time (LQ = 3, 4), otherwise
// LQ = 4 (num_levels <= 3) or 7 (num_levels 6 .. 8) at run time.  lq = num_levels - 1.
enum GradLevelVariant : int { GRAD_LV_CT3 = 0, GRAD_LV_CT4 = 1, GRAD_LV_RT4 = 2, GRAD_LV_RT7 = 3 };
constexpr GradLevelVariant grad_w2_variant(int lq) { return lq == 3 ? GRAD_LV_CT3 : (lq == 4 ? GRAD_LV_CT4 : (lq < 3 ? GRAD_LV_RT4 : GRAD_LV_RT7)); }
constexpr int grad_variant_lq(GradLevelVariant v) { return v == GRAD_LV_CT3 ? 3 : (v == GRAD_LV_RT7 ? 7 : 4); }
constexpr bool grad_variant_ct(GradLevelVariant v) { return v == GRAD_LV_CT3 || v == GRAD_LV_CT4; }
// the stored-lattice kernel keeps 4 or 7 levels, both at run time
constexpr GradLevelVariant grad_wave_variant(int lq) { return lq <= 4 ? GRAD_LV_RT4 : GRAD_LV_RT7; }

// One compiled instance.  First order: family, mode, G, C, DP, variant (GRAD_LAM_UNDO: rbf = the RBF instances, otherwise the base kernel at run
// time).  Higher order: family, G, C, order, and num_levels for GRAD_HO_UNDO (0 for GRAD_HO_SLOT, whose num_levels is a run-time argument).
struct GradInstance {
    int family = GRAD_NONE, mode = 0, G = 0, C = 0, DP = 0, variant = 0, rbf = 0, num_levels = 0, order = 0;
};

constexpr bool grad_wave_shape_compiled(int G, int C, int DP) {
#define X_GP(G_, C_, D_) if (G == G_ && C == C_ && DP == D_) return true;
    GPSIG_WAVE_SHAPES(X_GP)
#undef X_GP
    return false;
}
constexpr bool grad_ho_undo_form_compiled(int G, int C) {
#define X_GP(G_, C_) if (G == G_ && C == C_) return true;
    GPSIG_HO_UNDO_FORMS(X_GP)
#undef X_GP
    return false;
}
constexpr bool grad_ho_undo_levels_compiled(int num_levels, int order) {
#define X_GP(M_, O_) if (num_levels == M_ && order == O_) return true;
    GPSIG_HO_UNDO_LEVELS(X_GP)
#undef X_GP
    return false;
}
constexpr bool grad_ho_slot_form_compiled(int G, int C) {
#define X_GP(G_, C_) if (G == G_ && C == C_) return true;
    GPSIG_HO_SLOT_FORMS(X_GP)
#undef X_GP
    return false;
}
constexpr bool grad_ho_slot_order_compiled(int order) {
#define X_GP(O_) if (order == O_) return true;
    GPSIG_HO_SLOT_ORDERS(X_GP)
#undef X_GP
    return false;
}

// ---- lane shapes in planning order: the first whose G * C columns hold the lattice side ---------------------------------------------
constexpr int GRAD_LANE_SHAPES[5][2] = {{16, 2}, {16, 4}, {64, 2}, {64, 4}, {64, 8}};
// seq_grad_wave2_kernel: (64, 4) is not listed
constexpr int GRAD_WAVE2_LANE_SHAPES[4][2] = {{16, 2}, {16, 4}, {64, 2}, {64, 8}};
constexpr int GRAD_WAVE2_MAX_TILE = 32;                    // C * DP: larger per-lane tiles spill

// dynamic LDS of the scratch-free first-order kernels: the row totals of 64 / G streamed sequences (R1 rows each)
inline size_t wave2_lds(int G, int R1, int M) { return sizeof(double) * size_t(64 / G) * size_t(R1 > 0 ? R1 : 1) * size_t(M - 1 == 3 ? 3 : (M - 1 <= 4 ? 4 : 7)); }
constexpr size_t WAVE2_LDS_MAX = 64 * 1024;

// dynamic LDS of seq_grad_wave_ho_undo_kernel: the row totals of every level's grids, 64 / G pairs
inline size_t wave_ho_undo_lds(int G, int R1, int order, int M) {
    int w = 0;
    for (int j = 1; j < M; ++j) w += 1 + (((j + 1) < order ? (j + 1) : order) - 1);
    return sizeof(double) * size_t(64 / G) * size_t(R1) * size_t(w);
}
constexpr size_t WAVE_HO_UNDO_LDS_MAX = 64 * 1024;

// ---- stored lattice (seq_grad_wave_kernel): R2 lattice columns on the lanes -----------------------------------------------------------
inline GradInstance wave_plan_shape(int mode, int R2, int DP, int M) {
    GradInstance g;
    if (DP > 16 || M - 1 > 7) return g;
    for (auto& sh : GRAD_LANE_SHAPES) {
        if (sh[0] * sh[1] < R2) continue;
        if (!grad_wave_shape_compiled(sh[0], sh[1], DP)) continue;
        g.family = GRAD_WAVE; g.mode = mode; g.G = sh[0]; g.C = sh[1]; g.DP = DP; g.variant = grad_wave_variant(M - 1);
        return g;
    }
    return g;
}

// ---- scratch-free, gradient formed in the sweep (seq_grad_wave2_kernel): Rreg points of the register-resident side on the lanes --------
// The linear kernel on increments only: the point kernels would carry the derivative coefficients of a whole row on top of the recursion
// state; they run through seq_lam_undo_kernel + lam_contract_kernel.
inline GradInstance wave2_plan_shape(int mode, int Rreg, int DP, int M) {
    GradInstance g;
    if (mode != GRAD_MODE_INC || DP > 16 || M - 1 > 7) return g;
    for (auto& sh : GRAD_WAVE2_LANE_SHAPES) {
        if (sh[0] * sh[1] < Rreg) continue;
        if (sh[1] * DP > GRAD_WAVE2_MAX_TILE) continue;
        if (!grad_wave_shape_compiled(sh[0], sh[1], DP)) continue;
        g.family = GRAD_WAVE2; g.mode = mode; g.G = sh[0]; g.C = sh[1]; g.DP = DP; g.variant = grad_w2_variant(M - 1);
        return g;
    }
    return g;
}

// Both launches of a call (R1 x R2 lattice): x resp. y on the lanes, the other side streamed through LDS.  one_side: a diagonal or a symmetric
// Gram, whose single launch has x in both roles.  Both instances or none.
inline bool wave2_plan_call(int mode, int R1, int R2, int DP, int M, bool one_side, GradInstance* gx, GradInstance* gy) {
    *gx = *gy = GradInstance();
    if (R1 <= 0 || R2 <= 0) return false;
    const GradInstance x = wave2_plan_shape(mode, R1, DP, M);
    const GradInstance y = one_side ? x : wave2_plan_shape(mode, R2, DP, M);
    if (!x.family || !y.family) return false;
    if (wave2_lds(x.G, R2, M) > WAVE2_LDS_MAX || (!one_side && wave2_lds(y.G, R1, M) > WAVE2_LDS_MAX)) return false;
    *gx = x; *gy = y;
    return true;
}

// ---- scratch-free with Lam out (seq_lam_undo_kernel): R2 columns on the lanes, the row totals of R1 rows in LDS ------------------------
// (the linear kernel on increments runs faster through seq_grad_wave2_kernel: 44 ms against 66 ms for a 1024 x 1024 Gram)
inline GradInstance lam_undo_plan_shape(int mode, bool rbf, int R1, int R2, int DP, int M) {
    GradInstance g;
    if (mode == GRAD_MODE_INC || DP > 16 || M - 1 > 7) return g;
    for (auto& sh : GRAD_LANE_SHAPES) {
        if (sh[0] * sh[1] < R2) continue;
        if (wave2_lds(sh[0], R1, M) > WAVE2_LDS_MAX) continue;
        if (!grad_wave_shape_compiled(sh[0], sh[1], DP)) continue;
        g.family = GRAD_LAM_UNDO; g.mode = mode; g.G = sh[0]; g.C = sh[1]; g.DP = DP; g.variant = grad_w2_variant(M - 1); g.rbf = rbf ? 1 : 0;
        return g;
    }
    return g;
}

// ---- higher order: both sweeps of a pair in one wavefront (grad_wave_ho_kernel.hpp) ---------------------------------------------------
// order: the kernel's order as given (cut to num_levels here).  *lds: the dynamic LDS of the scratch-free kernel, 0 for the slot kernel.
inline GradInstance ho_sweeps_plan_shape(int grad_impl, int ho_g32, int num_levels, int order_in, int R1, int R2, size_t* lds) {
    GradInstance g;
    const int M = num_levels, order = order_in < M ? order_in : M;
    *lds = 0;
    if ((grad_impl != 0 && grad_impl != 3) || order < 2 || R1 < 1 || R2 < 1) return g;
    for (auto& sh : GRAD_LANE_SHAPES) {
        if (sh[0] * sh[1] < R2) continue;
        int G = sh[0], C = sh[1];
        // 33 .. 64 columns at order >= 3: two columns per lane and two pairs per wavefront instead of four and four -- the four-column instances of
        // orders 3 / 4 spill (312 B .. 1.6 KB of scratch at one wavefront per SIMD): K(X) N = 512 order 4 64.7 -> 39.3 ms; at order 2 they do not (25.8 against 27.0).
        // Option ho_g32: -1 this rule, 0 never, 1 always
        if (G == 16 && C == 4 && grad_impl == 0 && (ho_g32 > 0 || (ho_g32 < 0 && order >= 3))) { G = 32; C = 2; }
        const size_t need = wave_ho_undo_lds(G, R1, order, M);
        if (grad_impl == 0 && need <= WAVE_HO_UNDO_LDS_MAX && grad_ho_undo_form_compiled(G, C) && grad_ho_undo_levels_compiled(M, order)) {
            g.family = GRAD_HO_UNDO; g.G = G; g.C = C; g.num_levels = M; g.order = order;
            *lds = need;
            return g;
        }
        if (G == 32) { G = 16; C = 4; }
        if (M >= HO_SLOT_MIN_LEVELS && M <= HO_SLOT_MAX_LEVELS && grad_ho_slot_form_compiled(G, C) && grad_ho_slot_order_compiled(order)) {
            g.family = GRAD_HO_SLOT; g.G = G; g.C = C; g.order = order;
        }
        return g;
    }
    return g;
}

}  // namespace gpsig
