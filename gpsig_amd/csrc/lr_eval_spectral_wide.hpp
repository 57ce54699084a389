// lr_eval_spectral_wide.hpp -- the evaluation side's wide route for SignatureSpectral (lr_api.hip: lr_seq_features_t, lr_tens_features_t; which calls
// take it: lr_spectral_eval_wide / lr_spectral_eval_tens_wide, lr_tile_plan.hpp): argument block and launchers of the evaluation form of the
// spectral cross kernel and of the landmark Gram at more than 32 columns (kernels and instances: lr_eval_spectral_wide_inst.hip).  The feature
// kernels that follow the cross matrix take kxs / kzs from memory (lr_eval_wide.hpp: lr_eval_wide_seq_launch / _tens_launch).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpsig {

struct LrSpxEvalArgs {
    const double* X;                               // sequences: the launch's first one, (., L, d); tensors: Z (lt, T, E, d)
    int64_t n;                                     // points of the launch: sequences x L, or lt nt E
    int L;                                         // points per sequence (tensors: unused)
    const int32_t* lengths;                        // sequences: the launch's lengths on the device, or NULL (L points each)
    int64_t T, t0, nt; int E;                      // tensors
    int d;                                         // no lengthscales, no lags: the points are read raw
    const double* S; int c;
    int Q, family;
    const double* alpha; const double* omega;      // (Q), (Q, d): the device copy of the kernel object's table
    const double* g2;                              // gamma^2 (Q, d)
    const double* ss;                              // sum_f g2_qf s_if^2 (Q, c)
    const double* phS;                             // phi_q(S_i) (Q, c)
    double* K;                                     // (n, c)
};

// kxs of the points of sequences / of inducing tensors, min(blocks of 64 points, 1024) workgroups that stride over them.  Return the hipError_t
// of the launch.
int lr_spx_eval_seq_launch(hipStream_t stream, const LrSpxEvalArgs& A);
int lr_spx_eval_tens_launch(hipStream_t stream, const LrSpxEvalArgs& A);
// out (na, nb) = kappa(A_i, B_j) of rows of d columns, one thread per pair, in the difference form (spectral_pair.hpp) on the table in its
// (Q, d) layout: alpha = tab, omega = tab + Q, gamma = tab + Q + Q d
int lr_spx_gram_launch(hipStream_t stream, const double* A, const double* B, int64_t na, int64_t nb, int d, int Q, int family, const double* tab,
                       double* out);

}  // namespace gpsig
