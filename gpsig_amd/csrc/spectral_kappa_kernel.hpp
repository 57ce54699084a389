// spectral_kappa_kernel.hpp -- the reverse pass of the batched SignatureSpectral kappa op (gpsig_spectral_kappa_grad, spectral_kappa_api.hip):
//     K_b[i][j] = kappa(A_b[i], B_b[j]) = sum_q alpha_q E_q cos(2 pi theta_q)          A (batch, m, d), B (batch, n, d), K and G = dL/dK (batch, m, n)
// in the formulation of wide_spectral_kernel.hpp (the forward pass IS that header's kernels): per component q, g2 = gamma^2,
//     ip_q = sum_f (g2_qf a_if) b_jf      sq_q = max(nrm_q(a_i) + nrm_q(b_j) - 2 ip_q, 0)      theta_q = phi_q(a_i) - phi_q(b_j)
// with the norms and phases of the sides' pre-pass (wide_spx_side_kernel) and ip_q on the float64 matrix cores by wide_spx_kernel's walk: where a_i == b_j
// bitwise, sq_q and theta_q are exactly 0 here as they are there, and an exponential component passes no gradient (spectral_pair.hpp).
//
// With spectral_term's pieces: U_q = G o d_w1, V_q = G o d_w2; ru, rv their row sums, cu, cv their column sums.  Then
//     dalpha_q = sum G o d_alpha
//     dA_i     = sum_q [ 2 g2_q o (ru_qi a_i - (U_q B)_i) + rv_qi omega_q ]
//     dB_j     = sum_q [ 2 g2_q o (cu_qj b_j) - cv_qj omega_q ] - 2 (sum_q U_q^T (g2_q o A))_j
//     domega_qf = sum_i rv_qi a_if - sum_j cv_qj b_jf
//     dgamma_qf = 2 gamma_qf [ sum_i ru_qi a_if^2 + sum_j cu_qj b_jf^2 - 2 sum_i a_if (U_q B)_if ]
// A call works in chunks (spectral_kappa_api.hip): `nb` whole batch members, or `nr` rows (a multiple of 64 but for the last) of one.  Per chunk:
//   spk_weights_kernel   wide_spx_kernel's tiling -- 64 x 64 entries per workgroup of four wavefronts, both operand tiles in LDS per 32 columns of d, a
//                        wavefront 16 rows against four 16-column accumulator tiles.  Writes U_q [b][q][nr][n]; of V_q only the sums are needed.  A row
//                        of a tile lies in one wavefront: its sums over the tile's 64 columns go to the slot of the tile's column block.  A column's sums
//                        over the 64 rows -- 16 per wavefront, the wavefronts added in order through LDS -- go to the slot of the tile's row block, and
//                        the tile's sum of G o d_alpha to the tile's own slot.  No slot is written twice: no atomics.
//   spk_reduce_kernel    adds slots (and partial sums of any kind) in their order
//   the products         U B (all components of a member: one GEMM) and sum_q U_q^T (g2_q o A) (one GEMM, depth Q nr, added over the row chunks in chunk
//                        order) are left to rocBLAS by the host; spk_scale_kernel writes g2_q o A
//   spk_rows_kernel      dA of the chunk's rows;     spk_cols_kernel   dB of a finished batch member, in place on the GEMM's sum
//   spk_param_kernel     the sums of domega, dgamma over slices of 64 rows of a side, one partial per slice;   spk_finish_kernel   the three outputs
#pragma once

#include <hip/hip_runtime.h>

#include "launchers.hpp"
#include "spectral_pair.hpp"

namespace gpsig {

constexpr int SPK_MAX_Q = 64;
constexpr int SPK_MAX_D = 4096;
constexpr int SPK_KC = 32;                       // columns of d per LDS tile
constexpr int SPK_LD = SPK_KC + 2;               // its row stride (wide_spectral_kernel.hpp)
constexpr int SPK_TILE = 64;                     // rows and columns per workgroup
constexpr int SPK_THREADS = 256;
constexpr int SPK_SLICE = 64;                    // rows per partial sum of domega, dgamma

// one chunk: batch members b < nb (the pointers A, B, G, dA, dB are those of the chunk's first member), rows r0 + i, i < nr, of each
struct SpecKappaArgs {
    const double* A; const double* B; const double* G;
    double* dA; double* dB;
    int64_t m, n, nb, nr, r0;
    int d, Q, family;
    const double* alpha; const double* omega; const double* gamma; const double* g2;      // (Q), (Q, d), (Q, d), (Q, d)
    const double* nrmA; const double* phA;       // component q of row i of member b at [q * nb * nr + b * nr + i]
    const double* nrmB; const double* phB;       // ... of column j at [q * nb * n + b * n + j]
    int64_t ncb, nrb;                            // column blocks of n, row blocks of nr
    double* U;                                   // [b][q][nr][n]
    double* rus; double* rvs;                    // row-sum slots [cb][b][q][nr]
    double* cus; double* cvs;                    // column-sum slots [rb][b][q][n]
    double* das;                                 // sums of G o d_alpha [cb][b][rb][q]
    double* ru; double* rv;                      // [b][q][nr]
    double* cu; double* cv;                      // [b][q][n]
    double* UB; double* AS;                      // [b][q][nr][d]: U_q B, g2_q o A
    double* ppart;                               // [slice][2][q][d]
    double* tot;                                 // dalpha (Q), then the sums of domega (Q, d) and of dgamma / (2 gamma) (Q, d)
};

#ifdef GPSIG_SPK_KERNELS         // defined once, in spectral_kappa_inst.hip

typedef double spk_f64x4 __attribute__((ext_vector_type(4)));

struct SpkWeights { double u, v, a; };

// one component's weights at an entry with upstream gradient g: out of line, so that the library's exp / sin / cos keep their registers to themselves
__device__ __attribute__((noinline)) SpkWeights spk_term(double alpha, double ip, double na, double nb, double dph, bool gauss, double g) {
    const double sq = fmax(fma(-2.0, ip, na + nb), 0.0);
    const SpectralTerm t = spectral_term(alpha, sq, dph, gauss);
    return SpkWeights{g * t.d_w1, g * t.d_w2, g * t.d_alpha};
}

// grid: (column blocks, row blocks (grid-stride), batch members of the chunk (grid-stride)); every wavefront of a workgroup runs the same rounds
__global__ __launch_bounds__(SPK_THREADS) void spk_weights_kernel(const SpecKappaArgs S) {
    __shared__ double at[SPK_TILE * SPK_LD];
    __shared__ double bt[SPK_TILE * SPK_LD];
    __shared__ double gt[SPK_KC];
    __shared__ double cs[2][4][SPK_TILE];            // column sums of U_q, V_q per wavefront
    __shared__ double ds[4];                         // a wavefront's sum of G o d_alpha
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
    const int d = S.d, Q = S.Q;
    const int lk = tid & (SPK_KC - 1), lr = tid / SPK_KC;
    const int64_t cb = blockIdx.x, col0 = cb * SPK_TILE;
    const int64_t n = S.n, nr = S.nr;
    const int64_t planeA = S.nb * nr, planeB = S.nb * n;
    for (int64_t bi = blockIdx.z; bi < S.nb; bi += gridDim.z) {
        const double* __restrict__ A = S.A + (bi * S.m + S.r0) * d;
        const double* __restrict__ B = S.B + bi * n * d;
        const double* __restrict__ G = S.G + (bi * S.m + S.r0) * n;
        for (int64_t rb = blockIdx.y; rb < S.nrb; rb += gridDim.y) {
            const int64_t row0 = rb * SPK_TILE, wrow0 = row0 + wave * 16;
            double gk[4][4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t row = wrow0 + kq + 4 * g;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t col = col0 + j * 16 + m;
                    gk[j][g] = (row < nr && col < n) ? G[row * n + col] : 0.0;
                }
            }
            for (int q = 0; q < Q; ++q) {
                const double* __restrict__ gq = S.g2 + size_t(q) * d;
                spk_f64x4 ip[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) ip[j] = spk_f64x4{0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < d; k0 += SPK_KC) {
                    __syncthreads();                        // (the previous tiles' readers, and the readers of cs and ds, are done)
                    const int f = k0 + lk;
#pragma unroll
                    for (int rr = 0; rr < SPK_TILE; rr += SPK_THREADS / SPK_KC) {
                        const int r = rr + lr;
                        const int64_t ar = row0 + r, bc = col0 + r;
                        at[r * SPK_LD + lk] = (ar < nr && f < d) ? A[ar * d + f] : 0.0;
                        bt[r * SPK_LD + lk] = (bc < n && f < d) ? B[bc * d + f] : 0.0;
                    }
                    if (tid < SPK_KC) gt[tid] = (k0 + tid < d) ? gq[k0 + tid] : 0.0;
                    __syncthreads();
                    const int steps = (d - k0 < SPK_KC ? d - k0 + 3 : SPK_KC) / 4;
                    for (int kk = 0; kk < steps; ++kk) {
                        const int k = kk * 4 + kq;
                        const double a = at[(wave * 16 + m) * SPK_LD + k] * gt[k];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const double bv = bt[(j * 16 + m) * SPK_LD + k];
                            ip[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, ip[j], 0, 0, 0);
                        }
                    }
                }
                const double alpha = S.alpha[q];
                const bool gauss = spectral_gauss(S.family, q, Q);
                double nb[4], pb[4], cu[4], cv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t col = col0 + j * 16 + m;
                    nb[j] = col < n ? S.nrmB[int64_t(q) * planeB + bi * n + col] : 0.0;
                    pb[j] = col < n ? S.phB[int64_t(q) * planeB + bi * n + col] : 0.0;
                    cu[j] = 0.0; cv[j] = 0.0;
                }
                double* __restrict__ Uq = S.U + (bi * Q + q) * nr * n;
                double da = 0.0;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int64_t row = wrow0 + kq + 4 * g;
                    double su = 0.0, sv = 0.0;
                    if (row < nr) {
                        const double na = S.nrmA[int64_t(q) * planeA + bi * nr + row], pa = S.phA[int64_t(q) * planeA + bi * nr + row];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int64_t col = col0 + j * 16 + m;
                            if (col < n) {
                                const SpkWeights w = spk_term(alpha, ip[j][g], na, nb[j], pa - pb[j], gauss, gk[j][g]);
                                Uq[row * n + col] = w.u;
                                su += w.u; sv += w.v;
                                cu[j] += w.u; cv[j] += w.v;
                                da += w.a;
                            }
                        }
                    }
                    // the row's sums over the 16 lanes that hold its columns
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) {
                        su += __shfl_xor(su, o, 64);
                        sv += __shfl_xor(sv, o, 64);
                    }
                    if (m == 0 && row < nr) {
                        const int64_t at_ = ((cb * S.nb + bi) * Q + q) * nr + row;
                        S.rus[at_] = su;
                        S.rvs[at_] = sv;
                    }
                }
                // the columns' sums over the wavefront's 16 rows: the four lanes that hold a column
#pragma unroll
                for (int j = 0; j < 4; ++j) {
#pragma unroll
                    for (int o = 32; o > 8; o >>= 1) {
                        cu[j] += __shfl_xor(cu[j], o, 64);
                        cv[j] += __shfl_xor(cv[j], o, 64);
                    }
                    if (kq == 0) {
                        cs[0][wave][j * 16 + m] = cu[j];
                        cs[1][wave][j * 16 + m] = cv[j];
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) da += __shfl_xor(da, o, 64);
                if (lane == 0) ds[wave] = da;
                __syncthreads();
                if (tid < 2 * SPK_TILE) {
                    const int w = tid >> 6, c = tid & 63;
                    const double s = ((cs[w][0][c] + cs[w][1][c]) + cs[w][2][c]) + cs[w][3][c];
                    const int64_t col = col0 + c;
                    if (col < n) (w ? S.cvs : S.cus)[((rb * S.nb + bi) * Q + q) * n + col] = s;
                } else if (tid == 2 * SPK_TILE) {
                    S.das[((cb * S.nb + bi) * S.nrb + rb) * Q + q] = ((ds[0] + ds[1]) + ds[2]) + ds[3];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void spk_reduce_kernel(const double* __restrict__ part, int64_t count, int64_t width, int first, double* __restrict__ out) {
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < width; e += int64_t(gridDim.x) * blockDim.x) {
        double s = first ? 0.0 : out[e];
        for (int64_t k = 0; k < count; ++k) s += part[k * width + e];
        out[e] = s;
    }
}

// AS[b][q][i][f] = g2[q][f] A[b][r0 + i][f]
__global__ __launch_bounds__(256) void spk_scale_kernel(const SpecKappaArgs S) {
    const int d = S.d, Q = S.Q;
    const int64_t total = S.nb * Q * S.nr * d;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += int64_t(gridDim.x) * blockDim.x) {
        const int f = int(e % d);
        const int64_t t = e / d, i = t % S.nr, bq = t / S.nr;
        const int q = int(bq % Q);
        const int64_t b = bq / Q;
        S.AS[e] = S.g2[size_t(q) * d + f] * S.A[(b * S.m + S.r0 + i) * d + f];
    }
}

// dA[b][r0 + i][f] = sum_q [ 2 g2_qf (ru_qi a_if - (U_q B)_if) + rv_qi omega_qf ]
__global__ __launch_bounds__(256) void spk_rows_kernel(const SpecKappaArgs S) {
    const int d = S.d, Q = S.Q;
    const int64_t nr = S.nr, total = S.nb * nr * d;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += int64_t(gridDim.x) * blockDim.x) {
        const int f = int(e % d);
        const int64_t t = e / d, i = t % nr, b = t / nr;
        const int64_t at_ = (b * S.m + S.r0 + i) * d + f;
        const double a = S.A[at_];
        double acc = 0.0;
        for (int q = 0; q < Q; ++q) {
            const int64_t w = (b * Q + q) * nr + i;
            acc += 2.0 * S.g2[size_t(q) * d + f] * (S.ru[w] * a - S.UB[w * d + f]) + S.rv[w] * S.omega[size_t(q) * d + f];
        }
        S.dA[at_] = acc;
    }
}

// dB[b][j][f] = sum_q [ 2 g2_qf cu_qj b_jf - cv_qj omega_qf ] - 2 T_jf, T = sum_q U_q^T (g2_q o A) as the products left it in dB
__global__ __launch_bounds__(256) void spk_cols_kernel(const SpecKappaArgs S) {
    const int d = S.d, Q = S.Q;
    const int64_t n = S.n, total = S.nb * n * d;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < total; e += int64_t(gridDim.x) * blockDim.x) {
        const int f = int(e % d);
        const int64_t t = e / d, j = t % n, b = t / n;
        const double bv = S.B[e];
        double acc = 0.0;
        for (int q = 0; q < Q; ++q) {
            const int64_t w = (b * Q + q) * n + j;
            acc += 2.0 * S.g2[size_t(q) * d + f] * (S.cu[w] * bv) - S.cv[w] * S.omega[size_t(q) * d + f];
        }
        S.dB[e] = fma(-2.0, S.dB[e], acc);
    }
}

// workgroup (slice, q): the rows e = b R + i of the slice, thread = column f.  side 0: the chunk's rows of A (R = nr; sums of rv a, ru a^2 - 2 a (U_q B));
// side 1: the rows of B (R = n; sums of -cv b, cu b^2)
__global__ __launch_bounds__(64) void spk_param_kernel(const SpecKappaArgs S, int side) {
    const int d = S.d, Q = S.Q, q = blockIdx.y;
    const int64_t R = side ? S.n : S.nr, rows = S.nb * R;
    const double* __restrict__ X = side ? S.B : S.A;
    const double* __restrict__ W1 = side ? S.cu : S.ru;
    const double* __restrict__ W2 = side ? S.cv : S.rv;
    const int64_t stride = side ? S.n : S.m, off = side ? 0 : S.r0;
    const double sign = side ? -1.0 : 1.0;
    const int64_t nsl = (rows + SPK_SLICE - 1) / SPK_SLICE;
    for (int64_t sl = blockIdx.x; sl < nsl; sl += gridDim.x) {
        const int64_t e0 = sl * SPK_SLICE, e1 = e0 + SPK_SLICE < rows ? e0 + SPK_SLICE : rows;
        for (int f = threadIdx.x; f < d; f += 64) {
            double so = 0.0, sg = 0.0;
            for (int64_t e = e0; e < e1; ++e) {
                const int64_t b = e / R, i = e - b * R;
                const int64_t w = (b * Q + q) * R + i;
                const double x = X[(b * stride + off + i) * d + f];
                so = fma(W2[w], x, so);
                sg = fma(W1[w] * x, x, sg);
                if (!side) sg = fma(-2.0 * x, S.UB[w * d + f], sg);
            }
            S.ppart[((sl * 2 + 0) * Q + q) * d + f] = sign * so;
            S.ppart[((sl * 2 + 1) * Q + q) * d + f] = sg;
        }
    }
}

__global__ __launch_bounds__(256) void spk_finish_kernel(const SpecKappaArgs S, double* __restrict__ dalpha, double* __restrict__ domega,
                                                         double* __restrict__ dgamma) {
    const int64_t qd = int64_t(S.Q) * S.d;
    for (int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < S.Q + 2 * qd; e += int64_t(gridDim.x) * blockDim.x) {
        if (e < S.Q) dalpha[e] = S.tot[e];
        else if (e < S.Q + qd) domega[e - S.Q] = S.tot[e];
        else dgamma[e - S.Q - qd] = 2.0 * S.gamma[e - S.Q - qd] * S.tot[e];
    }
}

#endif  // GPSIG_SPK_KERNELS

}  // namespace gpsig
