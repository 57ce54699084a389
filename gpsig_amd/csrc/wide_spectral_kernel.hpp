// wide_spectral_kernel.hpp -- SignatureSpectral's kernel-ARGUMENT array of the wide-state-space route (wide_api.hip) in exact (non-low-rank) mode,
// state spaces of 33 .. 4096 columns: for a strided batch b
//     C_b[i][j] = kappa(A_b[i], B_b[j]) = sum_q alpha_q E_q(A_b[i] - B_b[j]) cos(2 pi <omega_q, A_b[i] - B_b[j]>)          (spectral_pair.hpp)
// with A_b (m, lda), B_b (n, ldb), C_b (m, ldc) row-major -- what the dgemm of the other families leaves in `arg`, except that the entries ARE kappa:
// the chain, lattice and tensor kernels of wide_kernels.hpp read them in their identity kind (WIDE_KD_ID), differences taken on these values.
//
// The d-deep contractions run on the float64 matrix cores (v_mfma_f64_16x16x4_f64) in the formulation of lr_cross_spectral_kernel.hpp.  Per component q
// (g2 = gamma^2, written once per call by wide_spx_prep_kernel):
//     ip_q[i][j] = sum_f (g2_qf a_if) b_jf        nrm_q(x) = sum_f (g2_qf x_f) x_f        sq_q = max(nrm_q(a_i) + nrm_q(b_j) - 2 ip_q, 0)
//     theta_q = phi_q(a_i) - phi_q(b_j),   phi_q(x) = sum_f x_f omega_qf
// wide_spx_side_kernel is the one pre-pass per side: the norms as the diagonal of the 16 x 16 product of a row block with itself, the phases as the
// product of the row block with Omega.  All three sums of a component walk the columns in steps of four from column 0, each entry one accumulation
// chain of the matrix core's: where a_i == b_j bitwise, ip_q, nrm_q(a_i) and nrm_q(b_j) are the same products in the same order, and so are the two
// phases -- sq_q and theta_q are EXACTLY 0 and the entry is sum_q alpha_q.  (An exponential component takes the square root of sq_q: rounding noise of
// 1e-16 there would come out as 1e-8 in kappa at every self-pair of K(X), Kdiag and K_tens.)
//
// wide_spx_kernel: a workgroup of four wavefronts owns 64 rows x 64 columns; a wavefront 16 rows against four 16-column accumulator tiles.  Both operand
// tiles (64 x 32 columns of d each) are staged in LDS per 32 columns of d, the row stride of 34 doubles keeps the operand reads of a half wavefront on
// distinct banks.  Every entry depends on its own row and column alone -- no sum across workgroups, no atomics: a call returns the same bits however the
// host chunks it.  Rows beyond m, columns beyond n and features beyond d are zeros in the operands and are neither read nor written.
#pragma once

#include <hip/hip_runtime.h>

#include "launchers.hpp"
#include "spectral_pair.hpp"

namespace gpsig {

constexpr int WIDE_SPX_MAX_Q = 64;
constexpr int WIDE_SPX_KC = 32;                      // columns of d per LDS tile
constexpr int WIDE_SPX_LD = WIDE_SPX_KC + 2;         // its row stride
constexpr int WIDE_SPX_TILE = 64;                    // rows and columns of C per workgroup
constexpr int WIDE_SPX_THREADS = 256;

struct WideSpxArgs {
    const double* A; const double* B; double* C;
    int64_t m, n, lda, ldb, ldc;
    int64_t sa, sb, sc, batch;                       // strides between the batch's matrices, in doubles
    int d, Q, family;
    const double* alpha;                             // (Q)
    const double* g2;                                // gamma^2 (Q, d)
    // the sides' pre-pass (wide_spx_side_kernel): component q of row i of matrix b at [q * plane + b * rows + i]
    const double* nrmA; const double* phA; int64_t planeA, rowsA;
    const double* nrmB; const double* phB; int64_t planeB, rowsB;
};

// (the launchers of wide_spectral_inst.hip: launchers.hpp)

#ifdef GPSIG_WIDE_SPX_KERNELS      // defined once, in wide_spectral_inst.hip

typedef double wide_spx_f64x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void wide_spx_prep_kernel(const double* __restrict__ gamma, int64_t count, double* __restrict__ g2) {
    const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e < count) g2[e] = gamma[e] * gamma[e];
}

// A wavefront takes 16 rows: the phases of all components (ceil(Q / 16) accumulator tiles against Omega), then component by component the norms.
// The matrix core's operand layout: lane l gives row l & 15 at column 4 k + (l >> 4) of the step; its accumulator register g is the entry
// (row (l >> 4) + 4 g, column l & 15).
__global__ __launch_bounds__(WIDE_SPX_THREADS) void wide_spx_side_kernel(const double* __restrict__ X, int64_t rows, int64_t ld, int d, int Q,
                                                                         const double* __restrict__ omega, const double* __restrict__ g2,
                                                                         double* __restrict__ nrm, double* __restrict__ ph) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    const int nqt = (Q + 15) / 16;
    const int64_t nblk = (rows + 63) / 64;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {                // (no barriers in this kernel)
        const int64_t row0 = (b * 4 + wave) * 16;
        if (row0 >= rows) continue;
        const int64_t row = row0 + m;
        const double* __restrict__ x = X + (row < rows ? row : 0) * ld;
        const bool on = row < rows;
        wide_spx_f64x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = wide_spx_f64x4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < d; k0 += 4) {
            const int f = k0 + kq;
            const double a = (on && f < d) ? x[f] : 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nqt) {
                    const int qi = j * 16 + m;
                    const double w = (qi < Q && f < d) ? omega[size_t(qi) * d + f] : 0.0;
                    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, w, acc[j], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t r = row0 + kq + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int qi = j * 16 + m;
                if (j < nqt && r < rows && qi < Q) ph[int64_t(qi) * rows + r] = acc[j][g];
            }
        }
        for (int q = 0; q < Q; ++q) {
            const double* __restrict__ gq = g2 + size_t(q) * d;
            wide_spx_f64x4 xx = {0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < d; k0 += 4) {
                const int f = k0 + kq;
                const double p = (on && f < d) ? x[f] : 0.0;
                const double a = p * (f < d ? gq[f] : 0.0);
                xx = __builtin_amdgcn_mfma_f64_16x16x4f64(a, p, xx, 0, 0, 0);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g)                                     // the diagonal: entry (m, m) sits in register g of the lane with m == kq + 4 g
                if (m == kq + 4 * g && on) nrm[int64_t(q) * rows + row] = xx[g];
        }
    }
}

// one component's value at an entry: out of line, so that the library's exp / cos keep their registers to themselves
__device__ __attribute__((noinline)) double wide_spx_term(double alpha, double ip, double na, double nb, double dph, bool gauss) {
    const double sq = fmax(fma(-2.0, ip, na + nb), 0.0);
    return spectral_term(alpha, sq, dph, gauss).val;
}

// grid: (column blocks, row blocks (grid-stride), matrices of the batch (grid-stride)); every wavefront of a workgroup runs the same rounds (barriers inside)
__global__ __launch_bounds__(WIDE_SPX_THREADS) void wide_spx_kernel(const WideSpxArgs S) {
    __shared__ double at[WIDE_SPX_TILE * WIDE_SPX_LD];
    __shared__ double bt[WIDE_SPX_TILE * WIDE_SPX_LD];
    __shared__ double gt[WIDE_SPX_KC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
    const int d = S.d, Q = S.Q;
    const int lk = tid & (WIDE_SPX_KC - 1), lr = tid / WIDE_SPX_KC;        // this thread's column and first row of a tile load (8 rows per pass)
    const int64_t col0 = int64_t(blockIdx.x) * WIDE_SPX_TILE;
    const int64_t rblocks = (S.m + WIDE_SPX_TILE - 1) / WIDE_SPX_TILE;
    for (int64_t bi = blockIdx.z; bi < S.batch; bi += gridDim.z) {
        const double* __restrict__ A = S.A + bi * S.sa;
        const double* __restrict__ B = S.B + bi * S.sb;
        double* __restrict__ C = S.C + bi * S.sc;
        const double* __restrict__ nrmA = S.nrmA + bi * S.rowsA;
        const double* __restrict__ phA = S.phA + bi * S.rowsA;
        const double* __restrict__ nrmB = S.nrmB + bi * S.rowsB;
        const double* __restrict__ phB = S.phB + bi * S.rowsB;
        for (int64_t rb = blockIdx.y; rb < rblocks; rb += gridDim.y) {
            const int64_t row0 = rb * WIDE_SPX_TILE, wrow0 = row0 + wave * 16;
            double kacc[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) kacc[j][g] = 0.0;
            for (int q = 0; q < Q; ++q) {
                const double* __restrict__ gq = S.g2 + size_t(q) * d;
                wide_spx_f64x4 ip[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) ip[j] = wide_spx_f64x4{0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < d; k0 += WIDE_SPX_KC) {
                    __syncthreads();                        // (the previous tiles' readers are done)
                    const int f = k0 + lk;
#pragma unroll
                    for (int rr = 0; rr < WIDE_SPX_TILE; rr += WIDE_SPX_THREADS / WIDE_SPX_KC) {
                        const int r = rr + lr;
                        const int64_t ar = row0 + r, bc = col0 + r;
                        at[r * WIDE_SPX_LD + lk] = (ar < S.m && f < d) ? A[ar * S.lda + f] : 0.0;
                        bt[r * WIDE_SPX_LD + lk] = (bc < S.n && f < d) ? B[bc * S.ldb + f] : 0.0;
                    }
                    if (tid < WIDE_SPX_KC) gt[tid] = (k0 + tid < d) ? gq[k0 + tid] : 0.0;
                    __syncthreads();
                    const int steps = (d - k0 < WIDE_SPX_KC ? d - k0 + 3 : WIDE_SPX_KC) / 4;
                    for (int kk = 0; kk < steps; ++kk) {
                        const int k = kk * 4 + kq;
                        const double a = at[(wave * 16 + m) * WIDE_SPX_LD + k] * gt[k];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const double bv = bt[(j * 16 + m) * WIDE_SPX_LD + k];
                            ip[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, ip[j], 0, 0, 0);
                        }
                    }
                }
                const double alpha = S.alpha[q];
                const bool gauss = spectral_gauss(S.family, q, Q);
                double nb[4], pb[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t col = col0 + j * 16 + m;
                    nb[j] = col < S.n ? nrmB[int64_t(q) * S.planeB + col] : 0.0;
                    pb[j] = col < S.n ? phB[int64_t(q) * S.planeB + col] : 0.0;
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int64_t row = wrow0 + kq + 4 * g;
                    if (row < S.m) {
                        const double na = nrmA[int64_t(q) * S.planeA + row], pa = phA[int64_t(q) * S.planeA + row];
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (col0 + j * 16 + m < S.n) kacc[j][g] += wide_spx_term(alpha, ip[j][g], na, nb[j], pa - pb[j], gauss);
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t row = wrow0 + kq + 4 * g;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t col = col0 + j * 16 + m;
                    if (row < S.m && col < S.n) C[row * S.ldc + col] = kacc[j][g];
                }
            }
        }
    }
}

#endif  // GPSIG_WIDE_SPX_KERNELS

}  // namespace gpsig
