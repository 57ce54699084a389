// lr_eval_wide_inst.hip -- the instances of the evaluation form of the Nystrom cross kernel (lr_cross_kernel.hpp: lr_cross_eval_kernel) and their
// launchers (own translation unit: the training kernels of lr_cross_inst.hip stay the code they were).  Element type of the caller's table x
// sequences / inducing tensors; what they compute and the argument block: lr_cross_kernel.hpp, lr_eval_wide.hpp.
// Also here, host code alone: the launches of the feature kernels that follow the cross matrix (lr_eval_wide_*_launch), from the plain fields of
// lr_eval_wide.hpp -- so that lr_api.hip sees neither the training path's argument blocks nor its kernels' headers.
#define GPSIG_LR_CROSS_TEMPLATES_ONLY     // the header's kernels that are no templates belong to lr_cross_inst.hip
#define GPSIG_LR_BODIES_ONLY              // ... and those of the training path's headers to lr_grad_api.hip
#include "lr_cross_kernel.hpp"
#include "lr_eval_tiled.hpp"
#include "lr_kx.hpp"

namespace gpsig {

namespace {
template <typename In, bool TENS>
int launch(hipStream_t stream, const LrCrossEvalArgs<In>& A) {
    if (A.n <= 0) return int(hipSuccess);
    const int64_t nblk = (A.n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    hipLaunchKernelGGL((lr_cross_eval_kernel<In, TENS>), dim3(unsigned(nblk < LR_CROSS_MAX_GRID ? nblk : LR_CROSS_MAX_GRID)), dim3(LR_CROSS_THREADS), 0,
                       stream, A);
    return int(hipGetLastError());
}
}  // namespace

int lr_cross_eval_seq_launch(hipStream_t stream, const LrCrossEvalArgs<double>& A) { return launch<double, false>(stream, A); }
int lr_cross_eval_seq_launch(hipStream_t stream, const LrCrossEvalArgs<float>& A) { return launch<float, false>(stream, A); }
int lr_cross_eval_tens_launch(hipStream_t stream, const LrCrossEvalArgs<double>& A) { return launch<double, true>(stream, A); }
int lr_cross_eval_tens_launch(hipStream_t stream, const LrCrossEvalArgs<float>& A) { return launch<float, true>(stream, A); }

int lr_eval_wide_seq_launch(hipStream_t stream, const LrEvalWideFeat<double, LrEntry>& W, int pad) {
    const LrTileDir D = lr_kx_tile_dir(false, W.c, W.r, W.L, W.difference ? W.L - 1 : W.L, pad);
    if (D.TL == 0 || W.M - 1 > LR_FUSED_MAX_SKETCHES) return int(hipErrorInvalidValue);
    LrTiledKxArgs A{};
    A.X = W.kxs; A.d = W.c; A.N = W.N; A.L = W.L;    // (the bodies step through X in rows of d: lr_kx.hpp)
    A.Wh = W.Wh;
    A.c = W.c; A.r = W.r; A.M = W.M; A.difference = W.difference;
    for (int i = 0; i < W.M - 1; ++i) A.sk[i] = LrGradSketch{W.sk[i].colptr, W.sk[i].ent, nullptr, nullptr, nullptr, nullptr};
    A.F = 1 + W.c + (W.M - 1) * W.r;
    A.lp = D.lp; A.TL = D.TL; A.ntiles = D.ntiles; A.rows_b = lr_fused_rows(W.c, W.r, 0);
    A.Phi = W.Phi;
    A.lengths = W.lengths;
    return lr_kx_tiled_launch(stream, A, unsigned(W.N < (1 << 20) ? W.N : (1 << 20)), D.lds);
}

int lr_eval_wide_seq_launch(hipStream_t stream, const LrEvalWideFeat<float, LrEntryF32>& W, int pad) {
    LrEvalTiledKxArgsF32 A{};
    A.X = W.kxs; A.N = W.N; A.L = W.L;
    A.Wh = W.Wh;
    A.c = W.c; A.r = W.r; A.M = W.M; A.difference = W.difference;
    for (int i = 0; i < W.M - 1 && i < LR_FUSED_MAX_SKETCHES; ++i) A.sk[i] = W.sk[i];
    A.Phi = W.Phi;
    A.lengths = W.lengths;
    return lr_eval_tiled_kx_launch(stream, A, pad);
}

namespace {
template <typename Args, typename V, typename Entry>
int tens_launch(hipStream_t stream, const LrEvalWideFeat<V, Entry>& W) {
    if (W.M - 1 > LR_FUSED_MAX_SKETCHES) return int(hipErrorInvalidValue);
    Args A{};                                        // (P.d_in = 0: no point is read)
    A.T = W.N; A.lt = W.L; A.E = W.E;
    A.Wh = W.Wh;
    A.c = W.c; A.r = W.r; A.M = W.M;
    for (int i = 0; i < W.M - 1; ++i) A.sk[i] = W.sk[i];
    A.Phi = W.Phi;
    A.kzs = W.kxs;
    return lr_kx_tens_launch(stream, A);
}
}  // namespace
int lr_eval_wide_tens_launch(hipStream_t stream, const LrEvalWideFeat<double, LrEntry>& W) { return tens_launch<LrTensKxArgs>(stream, W); }
int lr_eval_wide_tens_launch(hipStream_t stream, const LrEvalWideFeat<float, LrEntryF32>& W) { return tens_launch<LrTensKxArgsF32>(stream, W); }

}  // namespace gpsig
