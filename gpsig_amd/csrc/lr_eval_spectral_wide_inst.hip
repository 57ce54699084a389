// lr_eval_spectral_wide_inst.hip -- SignatureSpectral's evaluation side on state spaces of 33 .. 4096 columns (own translation unit: the training
// kernels of lr_cross_spectral_inst.hip stay the code they were).  Argument block and launchers: lr_eval_spectral_wide.hpp.
//
// lr_spx_eval_kernel: the evaluation form of the spectral cross kernel, K (n, c) = sum_q alpha_q E_q cos(theta_q) of the CALLER'S points against
// c <= 64 landmarks on the float64 matrix cores.  The walk is lr_spx_kernel<false>'s (lr_cross_spectral_kernel.hpp): a wavefront owns 16 points
// against up to four 16-landmark accumulator tiles, the point tile sits in LDS, rows of d <= 64 are loaded once for all components, wider rows are
// walked 64 columns at a time.  What differs:
//   rows     in the caller's layout, as lr_cross_eval_kernel's (lr_cross_kernel.hpp): sequences X (N, L, d) with optional lengths (clamped to
//            [1, L]) -- a point beyond its sequence's length is never read (zeros in the operand, NaN allowed in X) and its K row is not written --;
//            tensors Z (lt, T, E, d), of which the chunk [t0, t0 + nt) is written as kzs (lt, nt, E, c).  Spectral has no lengthscales and no
//            lags: the points are read raw.
//   phases   phi_q(p) = sum_f omega_qf p_f inside the same walk: the same contraction with Omega (ceil(Q / 16) tiles) in place of the landmarks,
//            once per 16-point block, in the accumulation order of lr_spx_phase_kernel (lr_cross_inner: steps of four columns in column order);
//            the lane of row g fetches component q's phase by a shuffle.  The landmarks' phases are that kernel's on S: a landmark that is one
//            of the points is at phase exactly 0, and at squared distance exactly 0 by the three-product argument of the training kernels' header.
//   padding  a wavefront whose 16 rows are all padding (or beyond n) skips the arithmetic; it still takes every barrier of the workgroup's round.
// lr_spx_gram_kernel: the landmark Gram at these widths, one thread per pair in the difference form of spectral_pair.hpp -- symmetric, and the reference's formulation.
#include "lr_cross_spectral_kernel.hpp"
#include "lr_eval_spectral_wide.hpp"

namespace gpsig {

namespace {

// column k0 + lane of the wavefront's 16 rows into its LDS tile: zeros beyond d and for a row that is not read (off < 0)
__device__ __forceinline__ void lr_spx_eval_load(const double* __restrict__ X, const int64_t* roff, int d, int k0, double* pt, int lane) {
    const int col = k0 + lane;
    for (int rr = 0; rr < 16; ++rr) {
        const int64_t off = roff[rr];
        pt[rr * LR_CROSS_LD + lane] = (off >= 0 && col < d) ? X[off + col] : 0.0;
    }
}

// one component's value at (point, landmark): out of line, so that its coefficients are not hoisted into registers for the whole kernel
__device__ __attribute__((noinline)) double lr_spx_eval_term(double alpha, double ip, double xs, double ss, double dph, bool gauss) {
    const double sq = fmax(fma(-2.0, ip, xs + ss), 0.0);
    return spectral_term(alpha, sq, dph, gauss).val;
}

}  // namespace

template <bool TENS>
__global__ __launch_bounds__(LR_CROSS_THREADS) void lr_spx_eval_kernel(LrSpxEvalArgs A) {
    __shared__ double tiles[LR_CROSS_WAVES][16 * LR_CROSS_LD];
    __shared__ int64_t roff[LR_CROSS_WAVES][16];                            // a row's first element in X; -1: the row is not read
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    double* const pt = tiles[wave];
    const int c = A.c, d = A.d, Q = A.Q, nt = (c + 15) / 16, nqt = (Q + 15) / 16;
    const bool whole = d <= LR_CROSS_KC;                                    // the whole rows: loaded once for the phases and all components
    const int64_t nblk = (A.n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    const double* __restrict__ S = A.S;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {                // (the same number of rounds for every wavefront: barriers inside)
        const int64_t row0 = (b * LR_CROSS_WAVES + wave) * 16;
        __syncthreads();                                                    // (the previous round's readers of the row table and the tile are done)
        if (lane < 16) {
            const int64_t row = row0 + lane;
            int64_t off = -1;
            if (row < A.n) {
                if constexpr (TENS) {
                    const int64_t per = A.nt * A.E, k = row / per;
                    off = ((k * A.T + A.t0) * A.E + (row - k * per)) * d;
                } else {
                    const int64_t nq = row / A.L;
                    const int tt = int(row - nq * A.L);
                    int len = A.L;
                    if (A.lengths) {
                        len = A.lengths[nq];
                        len = len < 1 ? 1 : (len > A.L ? A.L : len);
                    }
                    if (tt < len) off = (nq * int64_t(A.L) + tt) * d;
                }
            }
            roff[wave][lane] = off;
        }
        __syncthreads();
        const bool work = __any(roff[wave][m] >= 0) != 0;                   // (wavefront-uniform)
        bool live[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) live[g] = roff[wave][kq + 4 * g] >= 0;
        if (whole) {
            lr_spx_eval_load(A.X, roff[wave], d, 0, pt, lane);
            __syncthreads();
        }
        // ---- the phases of the 16 points: ph[j][g] = phi_{16 j + m}(row kq + 4 g)
        lr_cross_f64x4 ph[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ph[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < d; k0 += LR_CROSS_KC) {
            if (!whole) {
                __syncthreads();                    // (the previous columns' readers are done)
                lr_spx_eval_load(A.X, roff[wave], d, k0, pt, lane);
                __syncthreads();
            }
            if (work) {
                const int steps = (d - k0 < LR_CROSS_KC ? d - k0 + 3 : LR_CROSS_KC) / 4;
                for (int kk = 0; kk < steps; ++kk) {
                    const int f = k0 + kk * 4 + kq;
                    const double a = pt[m * LR_CROSS_LD + kk * 4 + kq];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < nqt) {
                            const int qi = j * 16 + m;
                            const double w = (qi < Q && f < d) ? A.omega[size_t(qi) * d + f] : 0.0;
                            ph[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, w, ph[j], 0, 0, 0);
                        }
                    }
                }
            }
        }
        double kacc[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) kacc[j][g] = 0.0;
        for (int q = 0; q < Q; ++q) {
            const double* __restrict__ g2 = A.g2 + size_t(q) * d;
            lr_cross_f64x4 ip[4], xx = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 4; ++j) ip[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < d; k0 += LR_CROSS_KC) {
                if (!whole) {
                    __syncthreads();
                    lr_spx_eval_load(A.X, roff[wave], d, k0, pt, lane);
                    __syncthreads();
                }
                if (work) {
                    const int steps = (d - k0 < LR_CROSS_KC ? d - k0 + 3 : LR_CROSS_KC) / 4;
                    for (int kk = 0; kk < steps; ++kk) {
                        const int f = k0 + kk * 4 + kq;
                        const double p = pt[m * LR_CROSS_LD + kk * 4 + kq];
                        const double a = p * (f < d ? g2[f] : 0.0);
                        xx = __builtin_amdgcn_mfma_f64_16x16x4f64(a, p, xx, 0, 0, 0);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (j < nt) {
                                const int i = j * 16 + m;
                                const double s = (i < c && f < d) ? S[size_t(i) * d + f] : 0.0;
                                ip[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, s, ip[j], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            if (work) {
                double xs[4];
                lr_spx_diag(xx, xs, lane);
                const int jq = q >> 4, src = (kq << 4) | (q & 15);          // the lane that holds phi_q of this lane's rows
                const double alpha = A.alpha[q];
                const bool gauss = spectral_gauss(A.family, q, Q);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    double pv = ph[0][g];
                    if (jq == 1) pv = ph[1][g];
                    if (jq == 2) pv = ph[2][g];
                    if (jq == 3) pv = ph[3][g];
                    const double php = __shfl(pv, src, 64);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = j * 16 + m;
                        if (j < nt && live[g] && i < c)
                            kacc[j][g] += lr_spx_eval_term(alpha, ip[j][g], xs[g], A.ss[size_t(q) * c + i], php - A.phS[size_t(q) * c + i], gauss);
                    }
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t row = row0 + kq + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = j * 16 + m;
                if (j < nt && live[g] && i < c) A.K[row * c + i] = kacc[j][g];
            }
        }
    }
}

__global__ __launch_bounds__(256) void lr_spx_gram_kernel(const double* __restrict__ A, const double* __restrict__ B, int64_t na, int64_t nb, int d, int Q,
                                                          int family, const double* __restrict__ tab, double* __restrict__ out) {
    const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= na * nb) return;
    const int64_t i = e / nb, j = e - i * nb;
    const double* __restrict__ x = A + i * d;
    const double* __restrict__ y = B + j * d;
    const double* alpha = tab;
    const double* omega = tab + Q;
    const double* gamma = omega + size_t(Q) * d;
    out[e] = spectral_pair(alpha, omega, gamma, d, Q, family, d, [&](int f) { return x[f]; }, [&](int f) { return y[f]; });
}

namespace {
template <bool TENS>
int launch(hipStream_t stream, const LrSpxEvalArgs& A) {
    if (A.n <= 0) return int(hipSuccess);
    const int64_t nblk = (A.n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    hipLaunchKernelGGL((lr_spx_eval_kernel<TENS>), dim3(unsigned(nblk < LR_CROSS_MAX_GRID ? nblk : LR_CROSS_MAX_GRID)), dim3(LR_CROSS_THREADS), 0, stream, A);
    return int(hipGetLastError());
}
}  // namespace

int lr_spx_eval_seq_launch(hipStream_t stream, const LrSpxEvalArgs& A) { return launch<false>(stream, A); }
int lr_spx_eval_tens_launch(hipStream_t stream, const LrSpxEvalArgs& A) { return launch<true>(stream, A); }

int lr_spx_gram_launch(hipStream_t stream, const double* A, const double* B, int64_t na, int64_t nb, int d, int Q, int family, const double* tab,
                       double* out) {
    if (na <= 0 || nb <= 0) return int(hipSuccess);
    hipLaunchKernelGGL(lr_spx_gram_kernel, dim3(unsigned((na * nb + 255) / 256)), dim3(256), 0, stream, A, B, na, nb, d, Q, family, tab, out);
    return int(hipGetLastError());
}

}  // namespace gpsig
