// lr_eval_tiled.hpp -- the evaluation side's time-tiled, lengths-aware low-rank sequence feature kernels (lr_eval_tiled_inst.hip): argument
// blocks and launchers, for lr_api.hip (gpsig_lr_seq_features beyond the whole-sequence kernels, gpsig_lr_seq_features_ragged).
//
// The forward walk of lr_tiled_kernel.hpp -- tiles of TL time steps in increasing time, one carried column vector per level, the additions in
// the whole-sequence kernel's order -- on the evaluation side's block: the caller's RAW points, scaled in the kernel as
// lr_seq_features_fused_kernel scales them (lengthscales, lags and lag weights by scaled_point on the sequence's own time axis; a tile's halo
// point comes from global memory), in float64 and in float32 (arrays and carries in float: lr_eval_tiled_lds_bytes_f32, lr_tile_plan.hpp).
// `lengths` (N int32 on the device) may be NULL: every sequence then has L points (lr_ragged_nullable, one wave-uniform branch).  Otherwise
// sequence n has lengths[n] points, clamped to [1, L] in the kernel: that bounds its points, steps, 64-lane chunks and tiles, and the rows
// beyond are never read.  Lags with lengths (gpsig_lr_seq_features_ragged_lagged; gpsig_lr_seq_features_ragged refuses them) are interpolated
// on the sequence's own axis i / (lengths[n] - 1), halo point included: the features of the truncated sequence evaluated on its own.  A
// sequence of one point has no axis; its lagged copies are the point itself (scaled_point, aux_kernels.hpp).
// Families: every family of base_eval at run-time kind, in both element types; SignatureSpectral in float64 only.
#pragma once

#include "lr_fused_args.hpp"

namespace gpsig {

template <typename V, typename Entry>
struct LrEvalTiledFields : LrFusedFields<V, Entry> {
    int TL, ntiles;                 // tile length in steps of U; tiles of a sequence of L points
    const int32_t* lengths;         // NULL: L points each
};
struct LrEvalTiledArgs : LrEvalTiledFields<double, LrEntry> {};
struct LrEvalTiledArgsF32 : LrEvalTiledFields<float, LrEntryF32> {};
template <> struct lr_ragged<LrEvalTiledArgs> { static constexpr bool value = true; };
template <> struct lr_ragged<LrEvalTiledArgsF32> { static constexpr bool value = true; };
template <> struct lr_ragged_nullable<LrEvalTiledArgs> { static constexpr bool value = true; };
template <> struct lr_ragged_nullable<LrEvalTiledArgsF32> { static constexpr bool value = true; };

// The float32 kernel BEHIND the Nystrom cross matrix (the wide route of lr_api.hip; float64 takes lr_seq_features_tiled_kx_kernel, lr_kx.hpp): X is
// kxs (N, L, c) in float, from lr_cross_eval_kernel; phases 0 and 1 are a load, the rest is the kernel above.  S and kind are not read.
struct LrEvalTiledKxArgsF32 : LrEvalTiledArgsF32 {};
template <typename Args> struct lr_eval_kx { static constexpr bool value = false; };
template <> struct lr_eval_kx<LrEvalTiledKxArgsF32> { static constexpr bool value = true; };
template <> struct lr_ragged<LrEvalTiledKxArgsF32> { static constexpr bool value = true; };
template <> struct lr_ragged_nullable<LrEvalTiledKxArgsF32> { static constexpr bool value = true; };

// The caller fills the arguments except F, rows_b, lp, TL and ntiles, which the launcher derives from lr_eval_tile_dir (with the LDS row
// padding `pad`); one workgroup of 1024 threads per sequence (at most 2^20: the kernel strides over the rest).  A.kind == BASE_SPECTRAL
// launches the spectral instance (float64 only: the float32 launcher returns hipErrorInvalidValue for it, as both do where not even a
// 64-step tile fits the LDS -- callers test lr_eval_tile_dir(...).TL first).  Return the hipError_t of the launch.
int lr_eval_tiled_launch(hipStream_t stream, LrEvalTiledArgs A, int pad);
int lr_eval_tiled_launch(hipStream_t stream, LrEvalTiledArgsF32 A, int pad);
// ... and the kx instance: P is set here (d_in = c, no scaling), the plan is lr_eval_tile_dir's with max(c, r) rows
int lr_eval_tiled_kx_launch(hipStream_t stream, LrEvalTiledKxArgsF32 A, int pad);

}  // namespace gpsig
