// lr_spectral_tiled_inst.hip -- SignatureSpectral's lengths-aware instances of the low-rank sequence feature kernels, whole sequence and
// time-tiled, and their launchers (own translation unit: the instances of lr_fused_inst.hip, lr_grad_api.hip and lr_ragged_inst.hip stay the
// code they were).  Argument blocks and what the instances compute: lr_spectral_tiled.hpp.  The bodies are the shared ones; what differs for
// this family is overloaded on the argument block below: the tile's cross phase (spectral_pair), kxs kept in and read back from the
// workgroup's scratch, dkxs out instead of the base-kernel phase, dWh partials alone.
#define GPSIG_LR_BODIES_ONLY         // the headers' kernels that are no templates belong to lr_fused_inst.hip and lr_grad_api.hip
#include "lr_fused_kernel.hpp"
#include "lr_spectral_tiled.hpp"

namespace gpsig {

// One component of kappa, OUT OF LINE on purpose.  Inlined into the loops over landmarks and sequences, the two dozen float64 coefficients of the
// exponential and the cosine are hoisted into registers for the whole kernel: the forward instances then take 102 / 108 registers (occupancy 4,
// their twins of the other families 5) and, held to 96, spill.  As a function of its own the term takes 30 registers, its coefficients live
// only inside it, and a call costs a few instructions next to the ~200 of the term.  The arithmetic is spectral_term's.
__device__ __attribute__((noinline)) double lr_spectral_term_val(double alpha, double w1, double w2, bool gauss) {
    return spectral_term(alpha, w1, w2, gauss).val;
}
// spectral_pair (spectral_pair.hpp) on that term
template <typename TP, class FX, class FY>
__device__ __forceinline__ double lr_spectral_pair_ool(TP alpha, TP omega, TP gamma, int ld, int Q, int family, int d, FX&& xf, FY&& yf) {
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) {
        double w1 = 0.0, w2 = 0.0;
        for (int f = 0; f < d; ++f) {
            const double diff = xf(f) - yf(f);
            const double gd = gamma[q * ld + f] * diff;
            w1 = fma(gd, gd, w1);
            w2 = fma(omega[q * ld + f], diff, w2);
        }
        acc += lr_spectral_term_val(alpha[q], w1, w2, spectral_gauss(family, q, Q));
    }
    return acc;
}
// phase 1 of the whole-sequence forward body for this unit's instance (lr_fused_kernel.hpp: lr_spectral_kappa)
template <class FX, class FY>
__device__ __forceinline__ double lr_spectral_kappa(const LrFusedSpectralLenArgs& A, lr_const_ptr<double> tab, int Q, int d_eff, FX&& xf, FY&& yf) {
    return lr_spectral_pair_ool(tab, tab + Q, tab + Q + Q * SPECTRAL_STRIDE, SPECTRAL_STRIDE, Q, int(A.p1), d_eff, xf, yf);
}

// kb[i][t] = kappa(x_t, S_i) for the n points of xb (lr_cross_base's loop)
template <int NW>
__device__ __forceinline__ void lr_cross_spectral(const LrTiledSpectralArgs& A, const double* xb, double* kb, int n, int nchunk, int lane, int wave) {
    const lr_const_ptr<double> al = lr_as_const(A.alpha), om = lr_as_const(A.omega), ga = lr_as_const(A.gamma), Sg = lr_as_const(A.S);
    const int lp = A.lp, c = A.c, d = A.d, Q = int(A.p0), family = int(A.p1), ld = A.ld;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int t = ch * 64 + lane;
        if (t < n)
            for (int i = wave; i < c; i += NW)
                kb[i * lp + t] = lr_spectral_pair_ool(al, om, ga, ld, Q, family, d, [&](int f) { return xb[f * lp + t]; },
                                                      [&](int f) { return Sg[size_t(i) * d + f]; });
    }
}

// lr_tile_u with the spectral cross phase
template <int THREADS>
__device__ __forceinline__ void lr_tile_u(const LrTiledSpectralArgs& A, const double* Xt, int tl, int np, double* xb, double* kx, double* ft, double* u,
                                          int lane, int wave) {
    lr_load_points<THREADS>(Xt, np, A.d, A.lp, xb);
    __syncthreads();
    lr_cross_spectral<THREADS / 64>(A, xb, kx, np, (np + 63) / 64, lane, wave);
    __syncthreads();
    lr_tile_feat_u<THREADS>(A, tl, np, kx, ft, u, lane, wave);
}

// ---- the reverse body's family phases (lr_tiled_kernel.hpp has the other families').  kxs of the sequence lies at escr + kxs_off, [c][Lp]
// the dkxs rows of the sequence's padded points are zeros
template <int THREADS>
__device__ __forceinline__ void lr_tile_zero_padded(const LrTiledSpectralArgs& A, int64_t n, int Lp) {
    lr_zero_padded_rows<THREADS>(A.dkxs + n * int64_t(A.L) * A.c, Lp, A.L, A.c);
}
// pass A: the tile's kxs -> scratch (the halo point is written by both of its tiles, with the same value); kx is rewritten after the barrier
template <int THREADS>
__device__ __forceinline__ void lr_tile_keep_kxs(const LrTiledSpectralArgs& A, const double* kx, double* escr, int Lp, int t0, int np) {
    double* const ks = escr + A.kxs_off + t0;
    for (int q = threadIdx.x; q < A.c * np; q += THREADS) {
        const int i = q / np, t = q - i * np;
        ks[size_t(i) * Lp + t] = kx[i * A.lp + t];
    }
    __syncthreads();
}
template <int THREADS>
__device__ __forceinline__ void lr_tile_load_kxs(const LrTiledSpectralArgs& A, double* kx, const double* escr, int Lp, int t0, int np) {
    const double* const ks = escr + A.kxs_off + t0;
    for (int q = threadIdx.x; q < A.c * np; q += THREADS) {
        const int i = q / np, t = q - i * np;
        kx[i * A.lp + t] = ks[size_t(i) * Lp + t];
    }
    __syncthreads();
}
// pass B: kxs from the scratch instead of a second evaluation, then feat and U
template <int THREADS>
__device__ __forceinline__ void lr_tile_u_again(const LrTiledSpectralArgs& A, const double*, int tl, int np, double*, double* kx, double* ft, double* u,
                                                int lane, int wave, const double* escr, int Lp, int t0) {
    lr_tile_load_kxs<THREADS>(A, kx, escr, Lp, t0, np);
    lr_tile_feat_u<THREADS>(A, tl, np, kx, ft, u, lane, wave);
}
// ... and once more for the dWh sums (the points themselves are not needed: there is no base-kernel phase)
template <int THREADS>
__device__ __forceinline__ void lr_tile_kxs_again(const LrTiledSpectralArgs& A, lr_const_ptr<double>, const double*, int np, int, double*, double* kb,
                                                  const double* escr, int Lp, int t0, int, int) {
    lr_tile_load_kxs<THREADS>(A, kb, escr, Lp, t0, np);
}
// instead of the base-kernel phase: the rows [q0, np) of the tile's dkxs (in Y) out, each row of the sequence by exactly one tile
template <int THREADS, int KS>
__device__ __forceinline__ void lr_grad_base_phase(const LrTiledSpectralArgs& A, lr_const_ptr<double>, int64_t n, int t0, int q0, int np, double*,
                                                   const double*, double*, double* Y, double (&)[KS], double&, int, int) {
    const int c = A.c;
    double* const dk = A.dkxs + (n * int64_t(A.L) + t0) * c;
    for (int q = q0 * c + threadIdx.x; q < np * c; q += THREADS) {
        const int t = q / c, i = q - t * c;
        dk[q] = Y[i * A.lp + t];
    }
}
// this workgroup's partial sums: dWh alone, [c c]
template <int THREADS, int KW, int KS>
__device__ __forceinline__ void lr_grad_write_partials(const LrTiledSpectralArgs& A, const double (&accW)[KW], const double (&)[KS], double, double*, int,
                                                       int) {
    double* part = A.part + int64_t(blockIdx.x) * (int64_t(A.c) * A.c);
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int q = k * THREADS + threadIdx.x;
        if (q < A.c * A.c) part[q] = accW[k];
    }
}

__global__ __launch_bounds__(512) void lr_seq_features_spectral_len_kernel(LrFusedSpectralLenArgs A) { lr_seq_features_fused_body<512, 8, true>(A); }
__global__ __launch_bounds__(512) void lr_seq_features_grad_spectral_len_kernel(LrGradSpectralLenArgs A) { lr_seq_features_grad_body<512, true>(A); }
// (the tiled kernels take their argument block by value and their bodies are shared as texts: lr_tiled_kernel.hpp)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_tiled_spectral_kernel(LrTiledSpectralArgs A) {
#include "lr_tiled_fwd_body.inc"
}
template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_grad_tiled_spectral_kernel(LrTiledSpectralArgs A) {
#include "lr_tiled_rev_body.inc"
}

int lr_spectral_len_fused_launch(hipStream_t stream, LrFusedSpectralLenArgs A, int pad) {
    A.F = 1 + A.c + (A.M - 1) * A.r;
    A.lp = lr_fused_stride(A.L, pad);
    A.rows_b = lr_fused_rows(A.c, A.r, A.P.d_eff());
    const unsigned grid = unsigned(A.N < (int64_t(1) << 20) ? A.N : (int64_t(1) << 20));
    return lr_launch(lr_seq_features_spectral_len_kernel, grid, 512, lr_fused_lds_bytes(A.c, A.r, A.P.d_eff(), A.L, pad), stream, A);
}

int lr_spectral_len_grad_launch(hipStream_t stream, const LrGradSpectralLenArgs& A, unsigned grid, size_t lds) {
    return lr_launch(lr_seq_features_grad_spectral_len_kernel, grid, 512, lds, stream, A);
}

int lr_spectral_tiled_launch(hipStream_t stream, const LrTiledSpectralArgs& A, unsigned grid, size_t lds) {
    return lr_launch(lr_seq_features_tiled_spectral_kernel<1024>, grid, 1024, lds, stream, A);
}

int lr_spectral_grad_tiled_launch(hipStream_t stream, const LrTiledSpectralArgs& A, unsigned grid, size_t lds) {
    return lr_launch(lr_seq_features_grad_tiled_spectral_kernel<512>, grid, 512, lds, stream, A);
}

}  // namespace gpsig
