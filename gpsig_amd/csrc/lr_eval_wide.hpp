// lr_eval_wide.hpp -- the evaluation side's wide route (lr_api.hip: lr_seq_features_t, lr_tens_features_t; which calls take it: lr_eval_route,
// lr_tile_plan.hpp): argument block and launchers of the evaluation form of the Nystrom cross kernel (lr_cross_kernel.hpp, instances in
// lr_eval_wide_inst.hip).  The feature kernels that follow it take kxs / kzs from memory: float64 lr_kx.hpp, float32 lr_eval_tiled.hpp
// (sequences) and lr_kx.hpp (tensors).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"
#include "lr_fused_args.hpp"

namespace gpsig {

template <typename In>
struct LrCrossEvalArgs {
    const In* X;                                   // sequences: the launch's first one, (., L, P.d_in); tensors: Z (lt, T, E, d)
    int64_t n;                                     // points of the launch: sequences x L, or lt nt E
    int L;                                         // points per sequence (tensors: unused)
    const int32_t* lengths;                        // sequences: the launch's lengths on the device, or NULL (L points each)
    int64_t T, t0, nt; int E;                      // tensors
    ScaleParams P;                                 // d = P.d_eff()
    const double* S; int c;
    int kind; double p0, p1;
    const double* sn;                              // |S_i|^2 (c), lr_cross_norms_kernel
    In* K;                                         // (n, c)
};

// what the feature kernels behind the cross matrix take of a call, in the call's element type: kxs (N, L, c) of N sequences (`lengths` on the
// device or NULL), or kzs (lt, N, E, c) of N inducing tensors (L = lt); whitening and projections as lr_state_args leaves them
template <typename V, typename Entry>
struct LrEvalWideFeat {
    const V* kxs; int64_t N; int L, E;
    const int32_t* lengths;
    const V* Wh;
    int c, r, M, difference;
    LrSketch<Entry> sk[LR_FUSED_MAX_SKETCHES];
    V* Phi;
};

// |S_i|^2 (c) of float64 landmarks (c, d), by the walk the cross kernels take (lr_cross_inst.hip).  Return the hipError_t of the launch.
int lr_cross_norms_launch(hipStream_t stream, const double* S, int c, int d, double* sn);
// kxs of the points of sequences / of inducing tensors, min(blocks of 64 points, 1024) workgroups that stride over them
int lr_cross_eval_seq_launch(hipStream_t stream, const LrCrossEvalArgs<double>& A);
int lr_cross_eval_seq_launch(hipStream_t stream, const LrCrossEvalArgs<float>& A);
int lr_cross_eval_tens_launch(hipStream_t stream, const LrCrossEvalArgs<double>& A);
int lr_cross_eval_tens_launch(hipStream_t stream, const LrCrossEvalArgs<float>& A);
// the feature maps from kxs / kzs in memory.  Sequences: float64 lr_seq_features_tiled_kx_kernel on the plan of lr_kx_tile_dir, float32 the kx
// instance of the evaluation side's tiled kernel on lr_eval_tile_dir's with d = 0 (`pad`: the LDS row padding); hipErrorInvalidValue where not
// even a 64-step tile of max(c, r) rows fits.  Tensors: the kx instances of the fused tensor kernel, one workgroup per tensor.
int lr_eval_wide_seq_launch(hipStream_t stream, const LrEvalWideFeat<double, LrEntry>& W, int pad);
int lr_eval_wide_seq_launch(hipStream_t stream, const LrEvalWideFeat<float, LrEntryF32>& W, int pad);
int lr_eval_wide_tens_launch(hipStream_t stream, const LrEvalWideFeat<double, LrEntry>& W);
int lr_eval_wide_tens_launch(hipStream_t stream, const LrEvalWideFeat<float, LrEntryF32>& W);

}  // namespace gpsig
