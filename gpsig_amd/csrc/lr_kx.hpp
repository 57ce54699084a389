// lr_kx.hpp -- instances of the low-rank feature kernels that take kappa(points, landmarks) from MEMORY (lr_kx_inst.hip): argument blocks, traits
// and launchers, for lr_grad_api.hip.
//
// The feature map sees the state-space width d only in kxs = kappa(x, S) and its adjoint.  With kxs computed by the cross op on the matrix cores
// (lr_cross_kernel.hpp) the instances here begin behind it: no points, no landmarks, d in neither the LDS plan nor a per-thread table.  Float64,
// order 1, every family of base_eval (the kernels never see which).  Two callers: the training path (lr_grad_api.hip: gpsig_lr_*_kx_dev / _kx_grad
// behind gpsig_lr_cross) and the evaluation side's wide route (lr_api.hip through lr_eval_wide.hpp: the forward instances behind the evaluation
// form of the cross kernel; its float32 calls take LrTensKxArgsF32 here and the kx instance of lr_eval_tiled.hpp for sequences).
//   sequences   the time-tiled bodies (lr_tiled_fwd_body.inc, lr_tiled_rev_body.inc) on a lengths-aware block (`lengths` may be NULL: L points
//               each); a sequence that fits the LDS is one tile.  The bodies step through A.X in rows of A.d values per point: here X is
//               kxs (N, L, c) and d = c, so that the tile pointer they hand to the overloaded phases is the tile's first kxs row.  The plan has
//               max(c, r) rows (lr_tile_plan with d = 0).  Reverse: the kernel stops at dkxs (N, L, c), the rows of a sequence's padded points
//               exact zeros, each row written by exactly one tile, and sums dWh alone -- SignatureSpectral's shape (lr_spectral_tiled.hpp), but
//               kxs is read again where it is needed instead of kept in the workgroup's scratch: it is in memory already.
//   tensors     the fused tensor bodies with kzs (lt T E, c) in Z's flat point order (lr_tens_kx, lr_fused_args.hpp); reverse: the SPEC shape
//               of lr_tens_features_grad_body, dkzs in the same order (one launch over all tensors), dWh alone.
#pragma once

#include "lr_tens_grad_kernel.hpp"
#include "lr_tiled_kernel.hpp"

namespace gpsig {

struct LrTiledKxArgs : LrTiledRaggedArgs { double* dkxs; };        // X: kxs (N, L, c), d = c; dkxs: reverse only
template <> struct lr_ragged<LrTiledKxArgs> { static constexpr bool value = true; };
template <> struct lr_ragged_nullable<LrTiledKxArgs> { static constexpr bool value = true; };

struct LrTensKxArgs : LrTensFusedArgs { const double* kzs; };      // Z unused, P.d_in = 0
struct LrTensGradKxArgs : LrTensGradSpectralArgs { const double* kzs; };   // Z, alpha, omega, gamma unused, d = 0; dkx: dkzs
struct LrTensKxArgsF32 : LrTensFusedArgsF32 { const float* kzs; };  // the evaluation side's float32 calls (lr_api.hip, the wide route)
template <> struct lr_tens_kx<LrTensKxArgs> { static constexpr bool value = true; };
template <> struct lr_tens_kx<LrTensKxArgsF32> { static constexpr bool value = true; };
template <> struct lr_tens_kx<LrTensGradKxArgs> { static constexpr bool value = true; };

// the tile plan of the sequence instances, from max(c, r) rows alone: always the tiled form (TL = 0: not even a 64-step tile fits), tiles no
// longer than the sequence needs
inline LrTileDir lr_kx_tile_dir(bool reverse, int c, int r, int L, int l, int pad) {
    LrTileDir D = lr_tile_dir(reverse, c, r, 0, L, l, pad);
    const int need = (l > 0 ? l + LR_TILE_STEP - 1 : LR_TILE_STEP) / LR_TILE_STEP * LR_TILE_STEP;
    if (D.TL > need) D.TL = need;
    D.untiled = false;
    D.ntiles = D.TL ? lr_tile_count(l, D.TL) : 0;
    D.lp = lr_tile_stride(D.TL, pad);
    D.lds = D.TL ? (reverse ? lr_tiled_grad_lds_bytes(c, r, 0, D.TL, pad) : lr_tiled_fused_lds_bytes(c, r, 0, D.TL, pad)) : 0;
    return D;
}

// Launchers; each returns the hipError_t of the launch.  Sequences: grid and LDS bytes of the plan, forward 1024 threads, reverse 512 (the
// sizes of the other tiled instances).  Tensors: forward one workgroup per tensor (F derived), reverse `grid` workgroups that stride over them.
int lr_kx_tiled_launch(hipStream_t stream, const LrTiledKxArgs& A, unsigned grid, size_t lds);
int lr_kx_grad_tiled_launch(hipStream_t stream, const LrTiledKxArgs& A, unsigned grid, size_t lds);
int lr_kx_tens_launch(hipStream_t stream, LrTensKxArgs A);
int lr_kx_tens_launch(hipStream_t stream, LrTensKxArgsF32 A);
int lr_kx_tens_grad_launch(hipStream_t stream, const LrTensGradKxArgs& A, unsigned grid);

}  // namespace gpsig
