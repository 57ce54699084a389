// lr_cross_spectral_kernel.hpp -- SignatureSpectral's Nystrom cross matrix K[t][i] = kappa(P_t, S_i) = sum_q alpha_q E_q cos(theta_q) of n points
// (n, d) against c <= 64 landmarks (c, d) on state spaces of 33 .. 4096 columns, and its reverse pass, with the d-deep contractions on the float64
// matrix cores (v_mfma_f64_16x16x4_f64).  Layout and walk are lr_cross_kernel.hpp's: a wavefront owns 16 points against up to four 16-landmark
// accumulator tiles, A operand = the point rows from the wavefront's LDS tile, B operand = the landmark rows from L2.
//
// Per component q (g2 = gamma^2, written once per call by lr_spx_prep_kernel):
//   ip_q = sum_f (g2_qf p_f) s_f     xs_q = sum_f (g2_qf p_f) p_f (the diagonal of the tile's own product)     ss_q likewise, once per call
//   sq_q = max(xs_q + ss_q - 2 ip_q, 0)       theta_q = 2 pi (phi_q(p) - phi_q(s)),   phi_q(x) = sum_f omega_qf x_f
// The phases are the same d-deep contraction with Omega (Q <= 64 rows) in place of the landmarks: lr_spx_phase_kernel is lr_cross_inner on
// (points, Omega), for the landmarks once per call and for the points once per chunk.  Where P_t == S_i bitwise the three sums of a component
// are the same products in the same order, and so are the two phases: sq_q and theta_q are exactly 0 there (the argument of lr_cross_kernel.hpp's
// header); an exponential component's square root passes no gradient at sq = 0 (spectral_pair.hpp).  A tile of 16 points x 64 columns stays in
// the LDS for all Q components where d <= 64; wider rows are walked 64 columns at a time, per component, from L2.
//
// Reverse pass, G = dL/dK (n, c).  With A_q = G o alpha_q cos(theta_q) dE_q/dsq and B_q = -2 pi G o alpha_q E_q sin(theta_q):
//   lr_spx_weights_kernel    the forward walk again; A_q, B_q (Q, n, c) and, per point, rowsum(A_q), rowsum(B_q), sum_i G E_q cos (Q, n) and
//                            whether it carries any gradient (n) go to scratch.  An element with G == 0 is a select, not a product.
//   lr_spx_points_kernel     dP = sum_q [2 g2_q o (rowsum(A_q) o P - A_q S) + omega_q (x) rowsum(B_q)]: A_q S by a c-deep MFMA per 16 columns and
//                            component, the two row-sum terms by Q-deep ones; every dP row written once, exact zeros for a point without gradient
//   lr_spx_landmarks_kernel  the sums over the points, with the points as the contraction index: workgroup (x, y, q) owns 64 of the d + 1 columns
//                            [P | 1] and the y-th share of the points.  A_q^T [P | 1] gives A_q^T P and colsum(A_q); B_q^T 1 = colsum(B_q);
//                            rowsum(B_q)^T P, rowsum(A_q)^T P^2 and the sum of the alpha rows ride along as one more operand row.  One partial
//                            block per (share, q); a point without gradient is not read.
//   lr_spx_reduce_kernel     the shares' blocks added in their order (and onto the earlier chunks' sums)
//   lr_spx_finish_kernel     dS, dalpha, domega, dgamma from the summed blocks
// Every sum over the points is one accumulation chain in point order per share, shares and chunks are added in order: no floating-point atomics,
// two calls return the same bits, and zero rows between the live ones change no bit of the chain.
#pragma once

#define GPSIG_LR_CROSS_TEMPLATES_ONLY     // the header's kernels that are no templates belong to lr_cross_inst.hip
#include "lr_cross_kernel.hpp"
#include "spectral_pair.hpp"

namespace gpsig {

constexpr int LR_SPX_MAX_Q = 64;

struct LrSpxArgs {
    const double* P; int64_t n; int d;             // the points of this launch (a chunk of the call's)
    const double* S; int c;
    int Q, family;
    const double* alpha; const double* omega;      // (Q), (Q, d)
    const double* g2;                              // gamma^2 (Q, d)
    const double* ss;                              // sum_f g2_qf s_if^2 (Q, c)
    const double* phS;                             // phi_q(S_i) (Q, c)
    const double* phP;                             // phi_q(P_t) (Q, n)
    double* K;                                     // forward: (n, c)
    // reverse
    const double* G;                               // (n, c)
    double* dP;                                    // (n, d)
    double* WA; double* WB;                        // scratch (Q, n, c): A_q, B_q
    double* RA; double* RB; double* RL;            // scratch (Q, n): rowsum(A_q), rowsum(B_q), sum_i G E_q cos
    double* live;                                  // scratch (n): 1 where a point has a non-zero G, else 0
    double* part;                                  // [shares][Q][lr_spx_block(c, d)]
    int64_t share;                                 // points per share (a multiple of 4)
    int shares;
};

// a (share, q) block of the landmark sums: rows 0 .. c-1 of d + 1 columns (A_q^T P | colsum A_q), a row rowsum(B_q)^T P, a row
// rowsum(A_q)^T P^2, then colsum(B_q) (c) and the sum of the alpha rows
__host__ __device__ inline int64_t lr_spx_block(int c, int d) { return int64_t(c + 2) * (d + 1) + c + 1; }

// the diagonal of a wavefront's 16 x 16 tile: xs[g] = the entry of row (l >> 4) + 4 g, from the lane that holds it
__device__ __forceinline__ void lr_spx_diag(const lr_cross_f64x4& xx, double (&xs)[4], int lane) {
    const int kq = lane >> 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) xs[g] = __shfl(xx[g], (kq << 4) | (kq + 4 * g), 64);
}

// the wavefront's LDS tile: columns k0 .. k0 + 63 of its 16 points, zeros beyond n and d (between two workgroup barriers of the caller's)
__device__ __forceinline__ void lr_spx_load(const double* __restrict__ P, int64_t n, int d, int64_t row0, int k0, double* pt, int lane) {
    const int col = k0 + lane;
    for (int rr = 0; rr < 16; ++rr) {
        const int64_t row = row0 + rr;
        pt[rr * LR_CROSS_LD + lane] = (row < n && col < d) ? P[row * d + col] : 0.0;
    }
}

// component q of the wavefront's 16 points: ip[j][g] and the squared norms xs[g] of row (l >> 4) + 4 g.  Every wavefront of the workgroup calls it
// (d > 64: two barriers per 64 columns; d <= 64: the caller has loaded the tile, no barrier)
__device__ __forceinline__ void lr_spx_component(const LrSpxArgs& A, int q, int nt, int64_t row0, double* pt, lr_cross_f64x4 (&ip)[4], double (&xs)[4],
                                                 int lane) {
    const int m = lane & 15, kq = lane >> 4, d = A.d, c = A.c;
    const double* __restrict__ g2 = A.g2 + size_t(q) * d;
    const double* __restrict__ S = A.S;
    lr_cross_f64x4 xx = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) ip[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += LR_CROSS_KC) {
        if (d > LR_CROSS_KC) {
            __syncthreads();                        // (the previous columns' readers are done)
            lr_spx_load(A.P, A.n, d, row0, k0, pt, lane);
            __syncthreads();
        }
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
                    const double b = (i < c && f < d) ? S[size_t(i) * d + f] : 0.0;
                    ip[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, ip[j], 0, 0, 0);
                }
            }
        }
    }
    lr_spx_diag(xx, xs, lane);
}

// the term of component q at (row g, landmark tile j) of this lane
__device__ __forceinline__ SpectralTerm lr_spx_term(const LrSpxArgs& A, int q, double ip, double xs, double ss, double php, double phs) {
    const double sq = fmax(fma(-2.0, ip, xs + ss), 0.0);
    return spectral_term(A.alpha[q], sq, php - phs, spectral_gauss(A.family, q, A.Q));
}

#ifdef GPSIG_LR_SPX_KERNELS      // defined once, in lr_cross_spectral_inst.hip

// g2 = gamma^2 (Q, d)
__global__ __launch_bounds__(256) void lr_spx_prep_kernel(const double* __restrict__ gamma, int64_t count, double* __restrict__ g2) {
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q < count) g2[q] = gamma[q] * gamma[q];
}

// ss[q][i] = sum_f (g2_qf s_if) s_if by the walk of lr_spx_component on S itself: wavefront (x, q) takes 16 landmarks
__global__ __launch_bounds__(64) void lr_spx_norms_kernel(const double* __restrict__ S, int c, int d, const double* __restrict__ g2, double* __restrict__ ss) {
    const int lane = threadIdx.x, m = lane & 15, kq = lane >> 4, q = blockIdx.y;
    const int i = blockIdx.x * 16 + m;
    lr_cross_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += 4) {
        const int f = k0 + kq;
        const double s = (i < c && f < d) ? S[size_t(i) * d + f] : 0.0;
        const double a = s * (f < d ? g2[size_t(q) * d + f] : 0.0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, s, acc, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
        if (m == kq + 4 * g && i < c) ss[size_t(q) * c + i] = acc[g];
}

// ph[q][t] = sum_f X[t][f] omega[q][f]: lr_cross_inner with Omega as the landmarks
__global__ __launch_bounds__(LR_CROSS_THREADS) void lr_spx_phase_kernel(const double* __restrict__ X, int64_t n, int d, const double* __restrict__ omega,
                                                                        int Q, double* __restrict__ ph) {
    __shared__ double tiles[LR_CROSS_WAVES][16 * LR_CROSS_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    const int nt = (Q + 15) / 16;
    const int64_t nblk = (n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {                // (the same number of rounds for every wavefront: barriers inside)
        const int64_t row0 = (b * LR_CROSS_WAVES + wave) * 16;
        lr_cross_f64x4 ip[4], xx = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) ip[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
        lr_cross_inner(X, n, d, omega, Q, nt, row0, tiles[wave], ip, xx, lane);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t row = row0 + kq + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = j * 16 + m;
                if (j < nt && row < n && q < Q) ph[size_t(q) * n + row] = ip[j][g];
            }
        }
    }
}

// forward (GRAD = false): K; reverse (GRAD = true): A_q, B_q, their row sums, the alpha rows and the live flags
template <bool GRAD>
__global__ __launch_bounds__(LR_CROSS_THREADS) void lr_spx_kernel(LrSpxArgs A) {
    __shared__ double tiles[LR_CROSS_WAVES][16 * LR_CROSS_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    double* const pt = tiles[wave];
    const int c = A.c, d = A.d, Q = A.Q, nt = (c + 15) / 16;
    const int64_t n = A.n, nblk = (n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {                // (the same number of rounds for every wavefront: barriers inside)
        const int64_t row0 = (b * LR_CROSS_WAVES + wave) * 16;
        if (d <= LR_CROSS_KC) {                                             // the whole rows: loaded once for all components
            __syncthreads();
            lr_spx_load(A.P, n, d, row0, 0, pt, lane);
            __syncthreads();
        }
        double kacc[4][4], gk[4][4], any[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            any[g] = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                kacc[j][g] = 0.0;
                gk[j][g] = 0.0;
                if constexpr (GRAD) {
                    const int64_t row = row0 + kq + 4 * g;
                    const int i = j * 16 + m;
                    if (j < nt && row < n && i < c) gk[j][g] = A.G[row * c + i];
                    if (gk[j][g] != 0.0) any[g] = 1.0;
                }
            }
        }
        for (int q = 0; q < Q; ++q) {
            lr_cross_f64x4 ip[4];
            double xs[4];
            lr_spx_component(A, q, nt, row0, pt, ip, xs, lane);
            double ss[4], phs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = j * 16 + m;
                ss[j] = i < c ? A.ss[size_t(q) * c + i] : 0.0;
                phs[j] = i < c ? A.phS[size_t(q) * c + i] : 0.0;
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t row = row0 + kq + 4 * g;
                const double php = row < n ? A.phP[size_t(q) * n + row] : 0.0;
                double ra = 0.0, rb = 0.0, rl = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = j * 16 + m;
                    if (j < nt && row < n && i < c) {
                        const SpectralTerm t = lr_spx_term(A, q, ip[j][g], xs[g], ss[j], php, phs[j]);
                        if constexpr (GRAD) {
                            const bool on = gk[j][g] != 0.0;
                            const double wa = on ? gk[j][g] * t.d_w1 : 0.0, wb = on ? gk[j][g] * t.d_w2 : 0.0;
                            ra += wa; rb += wb;
                            rl += on ? gk[j][g] * t.d_alpha : 0.0;
                            const size_t at = (size_t(q) * n + row) * c + i;
                            A.WA[at] = wa;
                            A.WB[at] = wb;
                        } else {
                            kacc[j][g] += t.val;
                        }
                    }
                }
                if constexpr (GRAD) {
                    // the row's sums over the 16 lanes that hold its columns, in a fixed order
#pragma unroll
                    for (int o = 8; o > 0; o >>= 1) {
                        ra += __shfl_xor(ra, o, 64);
                        rb += __shfl_xor(rb, o, 64);
                        rl += __shfl_xor(rl, o, 64);
                    }
                    if (m == 0 && row < n) {
                        A.RA[size_t(q) * n + row] = ra;
                        A.RB[size_t(q) * n + row] = rb;
                        A.RL[size_t(q) * n + row] = rl;
                    }
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t row = row0 + kq + 4 * g;
            if constexpr (GRAD) {
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) any[g] = fmax(any[g], __shfl_xor(any[g], o, 64));
                if (m == 0 && row < n) A.live[row] = any[g];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int i = j * 16 + m;
                    if (j < nt && row < n && i < c) A.K[row * c + i] = kacc[j][g];
                }
            }
        }
    }
}

// dP[t][f] = 2 (sum_q g2_qf rowsum(A_q)_t) p_tf - 2 sum_q sum_i A_q[t][i] g2_qf s_if + sum_q omega_qf rowsum(B_q)_t.  A wavefront owns 16 points
// and walks the columns 64 at a time: the A operands of a component's c-deep product stay in registers for its four column tiles.
__global__ __launch_bounds__(LR_CROSS_THREADS) void lr_spx_points_kernel(LrSpxArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    const int c = A.c, d = A.d, Q = A.Q, nt = (c + 15) / 16, nq = (Q + 3) / 4;
    const int64_t n = A.n, nblk = (n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {                // (no barriers in this kernel)
        const int64_t row0 = (b * LR_CROSS_WAVES + wave) * 16;
        if (row0 >= n) break;
        const int64_t arow = row0 + m;                                       // the row of this lane's A operands
        const bool aon = arow < n && A.live[arow] != 0.0;
        for (int f0 = 0; f0 < d; f0 += 64) {
            lr_cross_f64x4 acc[4], cg[4], cw[4];
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
                acc[ft] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
                cg[ft] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
                cw[ft] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
            }
            for (int q = 0; q < Q; ++q) {
                const double* __restrict__ wq = A.WA + (size_t(q) * n + (aon ? arow : 0)) * c;
                const double* __restrict__ g2 = A.g2 + size_t(q) * d;
                double wa[16];
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) wa[kk] = (kk < nt * 4 && aon && kk * 4 + kq < c) ? wq[kk * 4 + kq] : 0.0;
#pragma unroll
                for (int ft = 0; ft < 4; ++ft) {
                    const int f = f0 + ft * 16 + m;
                    if (f0 + ft * 16 < d) {
                        const double gf = f < d ? g2[f] : 0.0;
#pragma unroll
                        for (int kk = 0; kk < 16; ++kk) {
                            if (kk < nt * 4) {
                                const int i = kk * 4 + kq;
                                const double bv = (i < c && f < d) ? gf * A.S[size_t(i) * d + f] : 0.0;
                                acc[ft] = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[kk], bv, acc[ft], 0, 0, 0);
                            }
                        }
                    }
                }
            }
            for (int kk = 0; kk < nq; ++kk) {                               // the Q-deep products of the row sums
                const int q = kk * 4 + kq;
                const bool on = aon && q < Q;
                const double ra = on ? A.RA[size_t(q) * n + arow] : 0.0, rb = on ? A.RB[size_t(q) * n + arow] : 0.0;
#pragma unroll
                for (int ft = 0; ft < 4; ++ft) {
                    const int f = f0 + ft * 16 + m;
                    if (f0 + ft * 16 < d) {
                        const bool in = q < Q && f < d;
                        cg[ft] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra, in ? A.g2[size_t(q) * d + f] : 0.0, cg[ft], 0, 0, 0);
                        cw[ft] = __builtin_amdgcn_mfma_f64_16x16x4f64(rb, in ? A.omega[size_t(q) * d + f] : 0.0, cw[ft], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int ft = 0; ft < 4; ++ft) {
                const int f = f0 + ft * 16 + m;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int64_t row = row0 + kq + 4 * g;
                    if (row < n && f < d) {
                        double v = 0.0;
                        if (A.live[row] != 0.0) v = fma(2.0 * cg[ft][g], A.P[row * d + f], fma(-2.0, acc[ft][g], cw[ft][g]));
                        A.dP[row * d + f] = v;
                    }
                }
            }
        }
    }
}

// part[y][q]: the sums over the points t of share y (see lr_spx_block): wavefront w of workgroup (x, y, q) owns the columns 64 x + 16 w .. of [P | 1]
__global__ __launch_bounds__(LR_CROSS_THREADS) void lr_spx_landmarks_kernel(LrSpxArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    const int c = A.c, d = A.d, nt = (c + 15) / 16, q = blockIdx.z;
    const int f0 = (blockIdx.x * LR_CROSS_WAVES + wave) * 16, f = f0 + m;
    if (f0 > d) return;                                                     // (no barriers in this kernel)
    const bool owner = d < f0 + 16;                                         // this wavefront holds the column of ones
    const int64_t n = A.n, t0 = int64_t(blockIdx.y) * A.share, t1 = t0 + A.share < n ? t0 + A.share : n;
    const double* __restrict__ WA = A.WA + size_t(q) * n * c;
    const double* __restrict__ WB = A.WB + size_t(q) * n * c;
    const double* __restrict__ RA = A.RA + size_t(q) * n;
    const double* __restrict__ RB = A.RB + size_t(q) * n;
    const double* __restrict__ RL = A.RL + size_t(q) * n;
    lr_cross_f64x4 acc[4], accb[4], accu = {0.0, 0.0, 0.0, 0.0}, accv = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
        accb[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
    }
    for (int64_t tb = t0; tb < t1; tb += 4) {
        const int64_t t = tb + kq;
        const bool on = t < t1 && A.live[t] != 0.0;
        double bv = 0.0;
        if (on) bv = f < d ? A.P[t * d + f] : (f == d ? 1.0 : 0.0);
        // one more operand row block: row 0 rowsum(B_q), row 2 the alpha row (against [P | 1]); row 0 rowsum(A_q) (against its squares)
        double au = 0.0, av2 = 0.0;
        if (on && m == 0) { au = RB[t]; av2 = RA[t]; }
        if (on && m == 2) au = RL[t];
        accu = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bv, accu, 0, 0, 0);
        accv = __builtin_amdgcn_mfma_f64_16x16x4f64(av2, bv * bv, accv, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < nt) {
                const int i = j * 16 + m;
                const double av = (on && i < c) ? WA[t * c + i] : 0.0;
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
                if (owner) {
                    const double ab = (on && i < c) ? WB[t * c + i] : 0.0;
                    accb[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ab, bv, accb[j], 0, 0, 0);
                }
            }
        }
    }
    const int ld = d + 1;
    double* out = A.part + (int64_t(blockIdx.y) * A.Q + q) * lr_spx_block(c, d);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = j * 16 + kq + 4 * g;
            if (j < nt && i < c && f <= d) out[size_t(i) * ld + f] = acc[j][g];
            if (j < nt && i < c && f == d) out[size_t(c + 2) * ld + i] = accb[j][g];
        }
    if (kq == 0 && f <= d) {                                                // row 0 of the extra block is register 0 of the lanes l >> 4 == 0
        out[size_t(c) * ld + f] = accu[0];
        out[size_t(c + 1) * ld + f] = accv[0];
    }
    if (kq == 2 && f == d) out[size_t(c + 2) * ld + c] = accu[0];           // row 2, the column of ones
}

// tot[e] = (the earlier chunks' sum) + the shares' partials in order, e over the Q blocks
__global__ __launch_bounds__(256) void lr_spx_reduce_kernel(const double* __restrict__ part, int shares, int64_t width, int first, double* __restrict__ tot) {
    const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (e >= width) return;
    double s = first ? 0.0 : tot[e];
    for (int k = 0; k < shares; ++k) s += part[int64_t(k) * width + e];
    tot[e] = s;
}

// dS, dalpha, domega, dgamma from the summed blocks: thread e < c d is dS[i][f], the next Q d are (q, f) of domega and dgamma, the last Q dalpha
__global__ __launch_bounds__(256) void lr_spx_finish_kernel(LrSpxArgs A, const double* __restrict__ tot, const double* __restrict__ gamma,
                                                            double* __restrict__ dS, double* __restrict__ dalpha, double* __restrict__ domega,
                                                            double* __restrict__ dgamma) {
    const int c = A.c, d = A.d, Q = A.Q, ld = d + 1;
    const int64_t e = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, cd = int64_t(c) * d, qd = int64_t(Q) * d, blk = lr_spx_block(c, d);
    if (e < cd) {
        const int i = int(e / d), f = int(e - int64_t(i) * d);
        const double s = A.S[e];
        double acc = 0.0;
        for (int q = 0; q < Q; ++q) {
            const double* T = tot + q * blk;
            const double ca = T[size_t(i) * ld + d], cb = T[size_t(c + 2) * ld + i];
            acc += 2.0 * A.g2[size_t(q) * d + f] * (ca * s - T[size_t(i) * ld + f]) - A.omega[size_t(q) * d + f] * cb;
        }
        dS[e] = acc;
    } else if (e < cd + qd) {
        const int64_t v = e - cd;
        const int q = int(v / d), f = int(v - int64_t(q) * d);
        const double* T = tot + q * blk;
        double so = 0.0, sg = 0.0, sm = 0.0;
        for (int i = 0; i < c; ++i) {
            const double s = A.S[size_t(i) * d + f];
            so = fma(T[size_t(c + 2) * ld + i], s, so);
            sg = fma(T[size_t(i) * ld + d], s * s, sg);
            sm = fma(s, T[size_t(i) * ld + f], sm);
        }
        domega[v] = T[size_t(c) * ld + f] - so;
        dgamma[v] = 2.0 * gamma[v] * (T[size_t(c + 1) * ld + f] + sg - 2.0 * sm);
    } else if (e < cd + qd + Q) {
        const int q = int(e - cd - qd);
        dalpha[q] = tot[q * blk + size_t(c + 2) * ld + c];
    }
}

#endif  // GPSIG_LR_SPX_KERNELS

}  // namespace gpsig
