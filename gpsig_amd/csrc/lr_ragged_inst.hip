// lr_ragged_inst.hip -- the ragged instances of the low-rank sequence feature kernels and their launchers (own translation unit: the
// instances of lr_fused_inst.hip and lr_grad_api.hip stay the code they were).  Sequence n of a batch has lengths[n] of the L points its
// rows have room for; the bodies are those of lr_fused_kernel.hpp, lr_grad_kernel.hpp and lr_tiled_kernel.hpp on argument blocks that
// carry the pointer (lr_fused_args.hpp: lr_ragged, lr_seq_points).  Float64, the families of base_eval.
//   forward, whole sequence   the three-array form, 512 threads, 8 entries per scalar-load batch (the default of lr_fused_variant)
//   reverse, whole sequence   512 threads, whatever lr_grad_threads says: at 1024, 128 registers a thread, the ragged instance keeps 208 bytes
//                             of scratch memory a thread (the existing instance fits exactly), and an instance with scratch is not built
//   forward, tiled            1024 threads
//   reverse, tiled            512 threads (at 1024, 128 registers a thread, it would keep scratch memory -- as the existing instance)
#define GPSIG_LR_BODIES_ONLY         // the headers' kernels that are no templates belong to lr_fused_inst.hip and lr_grad_api.hip
#include "lr_fused_kernel.hpp"
#include "lr_tiled_kernel.hpp"

namespace gpsig {

__global__ __launch_bounds__(512) void lr_seq_features_ragged_kernel(LrFusedRaggedArgs A) { lr_seq_features_fused_body<512, 8, false>(A); }
__global__ __launch_bounds__(512) void lr_seq_features_grad_ragged_kernel(LrGradRaggedArgs A) { lr_seq_features_grad_body<512, false>(A); }
// (the tiled kernels take their argument block by value and their bodies are shared as texts: lr_tiled_kernel.hpp)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_tiled_ragged_kernel(LrTiledRaggedArgs A) {
#include "lr_tiled_fwd_body.inc"
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_grad_tiled_ragged_kernel(LrTiledRaggedArgs A) {
#include "lr_tiled_rev_body.inc"
}

// (F, lp, rows_b and the grid as lr_fused_launch derives them)
int lr_ragged_fused_launch(hipStream_t stream, LrFusedRaggedArgs A, int pad) {
    A.F = 1 + A.c + (A.M - 1) * A.r;
    A.lp = lr_fused_stride(A.L, pad);
    A.rows_b = lr_fused_rows(A.c, A.r, A.P.d_eff());
    const unsigned grid = unsigned(A.N < (int64_t(1) << 20) ? A.N : (int64_t(1) << 20));
    return lr_launch(lr_seq_features_ragged_kernel, grid, 512, lr_fused_lds_bytes(A.c, A.r, A.P.d_eff(), A.L, pad), stream, A);
}

int lr_ragged_grad_launch(hipStream_t stream, const LrGradRaggedArgs& A, unsigned grid, size_t lds) {
    return lr_launch(lr_seq_features_grad_ragged_kernel, grid, 512, lds, stream, A);
}

int lr_ragged_tiled_launch(hipStream_t stream, const LrTiledRaggedArgs& A, unsigned grid, size_t lds) {
    return lr_launch(lr_seq_features_tiled_ragged_kernel<1024>, grid, 1024, lds, stream, A);
}

int lr_ragged_grad_tiled_launch(hipStream_t stream, const LrTiledRaggedArgs& A, unsigned grid, size_t lds) {
    return lr_launch(lr_seq_features_grad_tiled_ragged_kernel<512>, grid, 512, lds, stream, A);
}

}  // namespace gpsig
