// lr_spectral_tiled.hpp -- SignatureSpectral's instances of the low-rank sequence feature kernels that know per-sequence lengths, whole
// sequence and time-tiled (lr_spectral_tiled_inst.hip): argument blocks, traits and launchers, for lr_grad_api.hip.
//
// The bodies are those of lr_fused_kernel.hpp, lr_grad_kernel.hpp and lr_tiled_kernel.hpp.  Every block here carries `lengths` (N int32 on the
// device, sequence n has lengths[n] of its L points) and is lr_ragged_nullable: a NULL pointer means that every sequence has L points, so one
// set of instances serves long dense batches and ragged ones.  Float64, order 1, no lags.
//   forward   phase 1 by spectral_pair on the packed table (alpha[Q], omega[Q][SPECTRAL_STRIDE], gamma[Q][SPECTRAL_STRIDE])
//   reverse   phase 1 on the trainable parameters as they lie in memory (ld = d); the kernels stop at dkxs (N, L, c), rows beyond a
//             sequence's length exact zeros, and sum dWh alone -- the spectral cross op's reverse kernels take dkxs from there
//             (spectral_cross_grad_len_launch).  kxs of the WHOLE sequence is kept in the workgroup's scratch next to the E_i (c L doubles
//             at kxs_off, rows of the sequence's own number of points): the tiled form evaluates kappa -- Q exponentials and cosines per
//             (point, landmark), the costly phase of this family -- once per point in pass A and reads it back twice in pass B, where the
//             other families' form evaluates their kappa three times.
// In the forward and the tiled instances one component of kappa is a function of its own (lr_spectral_term_val): see lr_spectral_tiled_inst.hip.
#pragma once

#include "lr_tiled_kernel.hpp"

namespace gpsig {

struct LrFusedSpectralLenArgs : LrFusedArgs { const int32_t* lengths; };
struct LrGradSpectralLenArgs : LrGradSpectralArgs { const int32_t* lengths; };
// the tiled forms': the parameters with their row stride (forward: the packed table's, reverse: d); dkxs, kxs_off: reverse only
struct LrTiledSpectralArgs : LrTiledArgs {
    const double* alpha; const double* omega; const double* gamma; int ld;
    double* dkxs; int64_t kxs_off;
    const int32_t* lengths;
};
template <> struct lr_ragged<LrFusedSpectralLenArgs> { static constexpr bool value = true; };
template <> struct lr_ragged<LrGradSpectralLenArgs> { static constexpr bool value = true; };
template <> struct lr_ragged<LrTiledSpectralArgs> { static constexpr bool value = true; };
template <> struct lr_ragged_nullable<LrFusedSpectralLenArgs> { static constexpr bool value = true; };
template <> struct lr_ragged_nullable<LrGradSpectralLenArgs> { static constexpr bool value = true; };
template <> struct lr_ragged_nullable<LrTiledSpectralArgs> { static constexpr bool value = true; };
template <> struct lr_keeps_kxs<LrTiledSpectralArgs> { static constexpr bool value = true; };

// Launchers; each returns the hipError_t of the launch.  The whole-sequence forward form: three arrays, 512 threads, 8 entries per scalar-load
// batch; F, lp, rows_b and the grid derived as lr_fused_launch derives them.  The others take the grid and the LDS bytes of the plan:
// whole-sequence reverse 512 threads, tiled forward 1024, tiled reverse 512 (the sizes of their twins in lr_ragged_inst.hip, for their reasons).
int lr_spectral_len_fused_launch(hipStream_t stream, LrFusedSpectralLenArgs A, int pad);
int lr_spectral_len_grad_launch(hipStream_t stream, const LrGradSpectralLenArgs& A, unsigned grid, size_t lds);
int lr_spectral_tiled_launch(hipStream_t stream, const LrTiledSpectralArgs& A, unsigned grid, size_t lds);
int lr_spectral_grad_tiled_launch(hipStream_t stream, const LrTiledSpectralArgs& A, unsigned grid, size_t lds);

}  // namespace gpsig
