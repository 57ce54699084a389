// lr_kx_inst.hip -- the instances of the low-rank feature kernels that take kappa(points, landmarks) from memory, and their launchers (own
// translation unit: the instances of the other units stay the code they were).  Argument blocks and what the instances compute: lr_kx.hpp.  The
// bodies are the shared ones; what differs is overloaded on the argument block below, as in lr_spectral_tiled_inst.hip: the tile's kxs rows
// loaded instead of evaluated, dkxs out instead of the base-kernel phase, dWh partials alone.
#define GPSIG_LR_BODIES_ONLY         // the headers' kernels that are no templates belong to lr_fused_inst.hip and lr_grad_api.hip
#include "lr_fused_kernel.hpp"
#include "lr_kx.hpp"

namespace gpsig {

// a tile's kxs -> kx[i][t] from its np rows of c at Xt (lr_load_points with c columns), feat -> ft, U -> u.  Ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void lr_tile_u(const LrTiledKxArgs& A, const double* Xt, int tl, int np, double*, double* kx, double* ft, double* u, int lane,
                                          int wave) {
    lr_load_points<THREADS>(Xt, np, A.c, A.lp, kx);
    __syncthreads();
    lr_tile_feat_u<THREADS>(A, tl, np, kx, ft, u, lane, wave);
}

// ---- the reverse body's family phases (lr_tiled_kernel.hpp has the other families')
// the dkxs rows of the sequence's padded points are zeros
template <int THREADS>
__device__ __forceinline__ void lr_tile_zero_padded(const LrTiledKxArgs& A, int64_t n, int Lp) {
    lr_zero_padded_rows<THREADS>(A.dkxs + n * int64_t(A.L) * A.c, Lp, A.L, A.c);
}
// pass B: the tile's kxs from memory again, then feat and U
template <int THREADS>
__device__ __forceinline__ void lr_tile_u_again(const LrTiledKxArgs& A, const double* Xt, int tl, int np, double* xb, double* kx, double* ft, double* u,
                                                int lane, int wave, const double*, int, int) {
    lr_tile_u<THREADS>(A, Xt, tl, np, xb, kx, ft, u, lane, wave);
}
// ... and once more for the dWh sums
template <int THREADS>
__device__ __forceinline__ void lr_tile_kxs_again(const LrTiledKxArgs& A, lr_const_ptr<double>, const double* Xt, int np, int, double*, double* kb,
                                                  const double*, int, int, int, int) {
    lr_load_points<THREADS>(Xt, np, A.c, A.lp, kb);
    __syncthreads();
}
// instead of the base-kernel phase: the rows [q0, np) of the tile's dkxs (in Y) out, each row of the sequence by exactly one tile
template <int THREADS, int KS>
__device__ __forceinline__ void lr_grad_base_phase(const LrTiledKxArgs& A, lr_const_ptr<double>, int64_t n, int t0, int q0, int np, double*, const double*,
                                                   double*, double* Y, double (&)[KS], double&, int, int) {
    const int c = A.c;
    double* const dk = A.dkxs + (n * int64_t(A.L) + t0) * c;
    for (int q = q0 * c + threadIdx.x; q < np * c; q += THREADS) {
        const int t = q / c, i = q - t * c;
        dk[q] = Y[i * A.lp + t];
    }
}
// this workgroup's partial sums: dWh alone, [c c]
template <int THREADS, int KW, int KS>
__device__ __forceinline__ void lr_grad_write_partials(const LrTiledKxArgs& A, const double (&accW)[KW], const double (&)[KS], double, double*, int, int) {
    double* part = A.part + int64_t(blockIdx.x) * (int64_t(A.c) * A.c);
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int q = k * THREADS + threadIdx.x;
        if (q < A.c * A.c) part[q] = accW[k];
    }
}

// (the tiled kernels take their argument block by value and their bodies are shared as texts: lr_tiled_kernel.hpp)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_tiled_kx_kernel(LrTiledKxArgs A) {
#include "lr_tiled_fwd_body.inc"
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_grad_tiled_kx_kernel(LrTiledKxArgs A) {
#include "lr_tiled_rev_body.inc"
}
__global__ __launch_bounds__(LR_TENS_THREADS) void lr_tens_features_kx_kernel(LrTensKxArgs A) { lr_tens_features_fused_body<false>(A); }
__global__ __launch_bounds__(LR_TENS_THREADS) void lr_tens_features_kx_f32_kernel(LrTensKxArgsF32 A) { lr_tens_features_fused_body<false>(A); }
__global__ __launch_bounds__(LR_TENS_GRAD_THREADS) void lr_tens_features_grad_kx_kernel(LrTensGradKxArgs A) { lr_tens_features_grad_body<true>(A); }

int lr_kx_tiled_launch(hipStream_t stream, const LrTiledKxArgs& A, unsigned grid, size_t lds) {
    return lr_launch(lr_seq_features_tiled_kx_kernel<1024>, grid, 1024, lds, stream, A);
}

int lr_kx_grad_tiled_launch(hipStream_t stream, const LrTiledKxArgs& A, unsigned grid, size_t lds) {
    return lr_launch(lr_seq_features_grad_tiled_kx_kernel<512>, grid, 512, lds, stream, A);
}

int lr_kx_tens_launch(hipStream_t stream, LrTensKxArgs A) {
    A.F = 1 + A.c + (A.M - 1) * A.r;
    return lr_launch(lr_tens_features_kx_kernel, unsigned(A.T), LR_TENS_THREADS, lr_tens_fused_lds_bytes(A.c, A.r, 0, A.lt, A.E), stream, A);
}

int lr_kx_tens_launch(hipStream_t stream, LrTensKxArgsF32 A) {
    A.F = 1 + A.c + (A.M - 1) * A.r;
    return lr_launch(lr_tens_features_kx_f32_kernel, unsigned(A.T), LR_TENS_THREADS, lr_tens_fused_lds_bytes_f32(A.c, A.r, 0, A.lt, A.E), stream, A);
}

int lr_kx_tens_grad_launch(hipStream_t stream, const LrTensGradKxArgs& A, unsigned grid) {
    return lr_launch(lr_tens_features_grad_kx_kernel, grid, LR_TENS_GRAD_THREADS, lr_tens_grad_lds_bytes(A.c, A.r, 0, A.lt, A.E, A.M), stream, A);
}

}  // namespace gpsig
