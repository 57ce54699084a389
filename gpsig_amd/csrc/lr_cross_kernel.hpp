// lr_cross_kernel.hpp -- the Nystrom cross matrix K[t][i] = kappa(P_t, S_i) of n points (n, d) against c <= 64 landmarks (c, d) for the families of
// base_eval, and its reverse pass, with the d-deep contraction on the float64 matrix cores (v_mfma_f64_16x16x4_f64).  The low-rank feature map
// sees the state-space width d in this product and its adjoint alone (low_rank_calculations.py:59); everything behind it has max(c, r) rows.  With
// the cross matrix as an op of its own the feature kernels take kxs from memory (lr_kx_inst.hip) and d leaves their LDS plan and their tables.
//
// A wavefront owns 16 points against all landmarks: up to four 16-column accumulator tiles.  It walks d in steps of 4:
//   A  lane l holds P[l & 15][k = l >> 4]     (the rows of P are loaded coalesced along d into the wavefront's LDS tile, 64 columns at a time)
//   B  lane l holds S[j 16 + (l & 15)][k]     (from L2: S is at most 2 MB and the same for every wavefront)
//   C  register g of lane l is (row = (l >> 4) + 4 g, column = l & 15) -- the f64 map, not the f32 one
// Beyond n, c and d the operands are zeros; no row is read past its end.
//
// Norms.  |P_t|^2 is the diagonal of the tile's own product P P^T, accumulated by one more MFMA per step on the operand that is already in the
// register (A and B of that product are the same lane value); |S_i|^2 likewise, once per call (lr_cross_norms_kernel), with the same walk over
// k.  Where P_t == S_i bitwise -- landmarks are gathered from the evaluation's own points, so this happens in every training step -- the three
// numbers of base_eval are then the same sums of the same products in the same order, and xs + ss - 2 ip is exactly 0: the Matern families see
// the zero distance they see in the fused kernels.
//
// Reverse pass, G = dL/dK (n, c):
//   lr_cross_grad_points_kernel     ip again by the same pass; (wy, wx, ws, dp0) from base_eval_grad as lr_grad_base_phase takes them;
//                                   dP = (G o wy) S + rowsum(G o wx) o P by a c-deep MFMA per 16 columns, every dP row written once;
//                                   W = G o wy (n, c) and, per point, whether it carries any gradient go to scratch; colsum(G o ws) and
//                                   sum G o dkappa/dp0 leave as one partial per workgroup
//   lr_cross_grad_landmarks_kernel  W^T P by MFMA with the points as the contraction index: workgroup (x, y) owns 64 columns of d and the
//                                   y-th share of the points, one partial (c, d) per share
//   lr_cross_grad_reduce_kernels    the partials added in their order; dS = sum of the shares + colsum(G o ws) o S
// No floating-point atomics: two calls return the same bits.  An element with G == 0 contributes nothing whatever its point holds, and a point
// all of whose G are zero is not multiplied with anything: the padded rows of a ragged batch (NaN in P, zeros in G) get exact zeros in dP and
// leave dS alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grad_core.hpp"
#include "lr_eval_wide.hpp"
#include "lr_fused_args.hpp"
#include "seq_core.hpp"

namespace gpsig {

typedef double lr_cross_f64x4 __attribute__((ext_vector_type(4)));

constexpr int LR_CROSS_THREADS = 256, LR_CROSS_WAVES = LR_CROSS_THREADS / 64;
constexpr int LR_CROSS_KC = 64;                    // columns of d per LDS tile
constexpr int LR_CROSS_LD = LR_CROSS_KC + 1;       // its row stride
constexpr int LR_CROSS_MAX_C = 64;
constexpr int LR_CROSS_MAX_GRID = 1024;            // workgroups of the two kernels that stride over the points

struct LrCrossArgs {
    const double* P; int64_t n; int d;
    const double* S; int c;
    int kind; double p0, p1;
    const double* sn;                              // |S_i|^2 (c), lr_cross_norms_kernel
    double* K;                                     // forward: (n, c)
    // reverse
    const double* G;                               // (n, c)
    double* dP;                                    // (n, d)
    double* W;                                     // scratch (n, c): G o wy
    double* live;                                  // scratch (n): 1 where a point has a non-zero G, else 0
    double* part;                                  // [grid][c + 1]: colsum(G o ws), sum G o dkappa/dp0
    double* dspart;                                // [shares][c][d]
    int64_t share;                                 // points per share (a multiple of 4)
    int shares;
};

// ip[j][g] += sum_f P[row0 + (l >> 4) + 4 g][f] S[16 j + (l & 15)][f] over all f, and xx likewise P P^T of the 16 points (its diagonal: the
// squared norms).  `pt`: the wavefront's [16][LR_CROSS_LD] doubles of LDS.  Every wavefront of the workgroup calls it (two barriers per 64 columns).
__device__ __forceinline__ void lr_cross_inner(const double* __restrict__ P, int64_t n, int d, const double* __restrict__ S, int c, int nt, int64_t row0,
                                               double* pt, lr_cross_f64x4 (&ip)[4], lr_cross_f64x4& xx, int lane) {
    const int m = lane & 15, kq = lane >> 4;
    for (int k0 = 0; k0 < d; k0 += LR_CROSS_KC) {
        __syncthreads();                            // (the previous columns' readers are done)
        const int col = k0 + lane;
        for (int rr = 0; rr < 16; ++rr) {
            const int64_t row = row0 + rr;
            pt[rr * LR_CROSS_LD + lane] = (row < n && col < d) ? P[row * d + col] : 0.0;
        }
        __syncthreads();
        const int steps = (d - k0 < LR_CROSS_KC ? d - k0 + 3 : LR_CROSS_KC) / 4;
        for (int kk = 0; kk < steps; ++kk) {
            const int f = k0 + kk * 4 + kq;
            const double a = pt[m * LR_CROSS_LD + kk * 4 + kq];
            xx = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, xx, 0, 0, 0);
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
}
// The same walk with the tile's loader as a parameter, for the evaluation form (lr_cross_eval_kernel): `load(col)` fills column `lane` of the
// tile's 16 rows with column col of the wavefront's points, zeros beyond their end.  (A text of its own: behind a callable the training kernels
// above compile to other code -- the reverse kernel's register allocation moved.)
template <class Load>
__device__ __forceinline__ void lr_cross_walk(Load&& load, int d, const double* __restrict__ S, int c, int nt, double* pt, lr_cross_f64x4 (&ip)[4],
                                              lr_cross_f64x4& xx, int lane) {
    const int m = lane & 15, kq = lane >> 4;
    for (int k0 = 0; k0 < d; k0 += LR_CROSS_KC) {
        __syncthreads();                            // (the previous columns' readers are done)
        load(k0 + lane);
        __syncthreads();
        const int steps = (d - k0 < LR_CROSS_KC ? d - k0 + 3 : LR_CROSS_KC) / 4;
        for (int kk = 0; kk < steps; ++kk) {
            const int f = k0 + kk * 4 + kq;
            const double a = pt[m * LR_CROSS_LD + kk * 4 + kq];
            xx = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, xx, 0, 0, 0);
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
}

// the diagonal of a wavefront's 16 x 16 tile -> xs[g] = the entry of row (l >> 4) + 4 g, through 16 doubles of the wavefront's LDS tile
// (between two workgroup barriers of the caller's own)
__device__ __forceinline__ void lr_cross_diag_put(const lr_cross_f64x4& xx, double* pt, int lane) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
        if ((lane & 15) == (lane >> 4) + 4 * g) pt[lane & 15] = xx[g];
}

// ---- the evaluation form: kxs of the CALLER'S points, for gpsig_lr_seq_features / _ragged / gpsig_lr_tens_features on state spaces too wide for
// the kernels that hold the points in LDS (lr_eval_wide_inst.hip; the feature kernels that take kxs from memory follow it).  The walk and the
// wavefront layout are lr_cross_kernel's; loader and store differ:
//   loader   the table as the caller gives it, double or float, widened value by value and scaled in float64 as scaled_point<double, In> does
//            (sequences: lengthscales, lags and lag weights on the table's time axis -- with `lengths`, on that of the sequence's own points --, the interpolation bracket found once per (row, lag)
//            into the wavefront's LDS, not once per element) or as lr_tens_cross_kernel does (tensors: Z (lt, T, E, d) in its flat order,
//            lengthscales and lag weights).  The landmarks of a state are float64 values gathered from widened, scaled points: the loader
//            reproduces those bits, so a landmark that is one of the points is at distance exactly 0 in float32 calls too.
//   rows     sequences: point q of the launch is point q % L of sequence q / L; with `lengths` (clamped to [1, L]) the points beyond a
//            sequence's length are never read -- zeros in the operand -- and their kxs rows are not written.  Tensors: the launch takes the
//            tensors [t0, t0 + nt) of T: its point (k nt + tt) E + e is Z's row (k T + t0 + tt) E + e, so that K is kzs of nt tensors.
//   store    in the call's element type: double, or float rounded once.  Arithmetic is float64 for both.
// (LrCrossEvalArgs<In>: lr_eval_wide.hpp)

// the lag interpolation of scaled_point (aux_kernels.hpp; gpsig/lags.py:7-57) in two steps: the bracket of (point t, lag) on an axis of La
// points -- the table's L, or with lengths and lags the sequence's own (scaled_point's seq_len; La == 1: no axis, the point itself) ...
__device__ __forceinline__ int lr_cross_lag_bracket(int La, int t, double lag, double jitter, double* tq_out) {
    if (La == 1) { *tq_out = 0.0; return 0; }                               // (a table of L = 1 too: what the search below gave there, tq = fmax(NaN, 0))
    const double denom = double(La - 1);
    const double tq = fmax(double(t) / denom - lag, 0.0);
    int left = 0;
    for (int i = La - 1; i >= 0; --i)
        if (!(double(i) / denom - tq > jitter)) { left = i; break; }
    *tq_out = tq;
    return left;
}
// ... and the value of column f between its two rows: the same operations on the same values as scaled_point<double, In>.  seq_len as there:
// 0 is the table's axis of L points, 1 returns the sequence's one point.
template <typename In>
__device__ __forceinline__ double lr_cross_lag_value(const In* __restrict__ Xn, int L, int d_in, int f, int left, double tq, int seq_len = 0) {
    if (seq_len == 1) return double(Xn[f]);
    if (seq_len > 0) L = seq_len;
    const double denom = double(L - 1);
    const int right = left + 1 < L ? left + 1 : L - 1;
    const double xl = double(Xn[int64_t(left) * d_in + f]), xr = double(Xn[int64_t(right) * d_in + f]);
    const double tl = double(left) / denom, tr = double(right) / denom;
    return xl + (tq - tl) * (xr - xl) / (tr - tl);
}

template <typename In, bool TENS>
__global__ __launch_bounds__(LR_CROSS_THREADS) void lr_cross_eval_kernel(LrCrossEvalArgs<In> A) {
    __shared__ double tiles[LR_CROSS_WAVES][16 * LR_CROSS_LD];
    __shared__ int64_t roff[LR_CROSS_WAVES][16];                            // a row's sequence (tensors: the row itself) in X, in elements
    __shared__ int rtime[LR_CROSS_WAVES][16];                               // its point in the sequence; -1: the row is not read
    __shared__ int rlen[LR_CROSS_WAVES][16];                                // with lengths: the points of its sequence (the lags' axis); else 0
    __shared__ int bleft[LR_CROSS_WAVES][16 * MAX_LAGS];                    // the lag brackets of the wavefront's rows
    __shared__ double btq[LR_CROSS_WAVES][16 * MAX_LAGS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    double* const pt = tiles[wave];
    const int c = A.c, nt = (c + 15) / 16, d = A.P.d_eff(), d_in = A.P.d_in, L = A.L, nlags = TENS ? 0 : A.P.num_lags;
    const int64_t nblk = (A.n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    double ss[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ss[j] = j * 16 + m < c ? A.sn[j * 16 + m] : 0.0;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {                // (the same number of rounds for every wavefront: barriers inside)
        const int64_t row0 = (b * LR_CROSS_WAVES + wave) * 16;
        __syncthreads();                                                    // (the previous round's readers of the row tables are done)
        if (lane < 16) {
            const int64_t row = row0 + lane;
            int64_t off = 0;
            int t = -1, sl = 0;
            if (row < A.n) {
                if constexpr (TENS) {
                    const int64_t per = A.nt * A.E, k = row / per;
                    off = ((k * A.T + A.t0) * A.E + (row - k * per)) * d;
                    t = 0;
                } else {
                    const int64_t nq = row / L;
                    const int tt = int(row - nq * L);
                    int len = L;
                    if (A.lengths) {
                        len = A.lengths[nq];
                        len = len < 1 ? 1 : (len > L ? L : len);
                        sl = len;
                    }
                    if (tt < len) { off = nq * int64_t(L) * d_in; t = tt; }
                }
            }
            roff[wave][lane] = off;
            rtime[wave][lane] = t;
            rlen[wave][lane] = sl;
        }
        __syncthreads();
        if constexpr (!TENS) {
            for (int q = lane; q < 16 * nlags; q += 64) {                   // once per (row, lag)
                const int rr = q / nlags, lg = q - rr * nlags, t = rtime[wave][rr], sl = rlen[wave][rr];
                double tq = 0.0;
                bleft[wave][q] = t >= 0 ? lr_cross_lag_bracket(sl > 0 ? sl : L, t, A.P.lags[lg], A.P.jitter, &tq) : 0;
                btq[wave][q] = tq;
            }
        }
        lr_cross_f64x4 ip[4], xx = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) ip[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
        lr_cross_walk(
            [&](int col) {                                                  // (its first barrier orders the tables above)
                const bool in = col < d;
                const int lag = in ? col / d_in : 0, f = in ? col - lag * d_in : 0;
                const double ls = A.P.has_ls ? A.P.lsv(f) : 1.0, gm = A.P.num_lags > 0 ? A.P.gamma[lag] : 1.0;
                for (int rr = 0; rr < 16; ++rr) {
                    const int t = rtime[wave][rr];
                    double v = 0.0;
                    if (in && t >= 0) {
                        const In* Xn = A.X + roff[wave][rr];
                        if constexpr (TENS) {
                            v = double(Xn[col]);
                            if (A.P.has_ls) {
                                v = v / ls;
                                if (A.P.num_lags > 0) v = v * gm;
                            }
                        } else {
                            v = lag == 0 ? double(Xn[int64_t(t) * d_in + f])
                                         : lr_cross_lag_value(Xn, L, d_in, f, bleft[wave][rr * nlags + lag - 1], btq[wave][rr * nlags + lag - 1], rlen[wave][rr]);
                            if (A.P.has_ls) v = v / ls;
                            if (A.P.num_lags > 0) v = v * gm;
                        }
                    }
                    pt[rr * LR_CROSS_LD + lane] = v;
                }
            },
            d, A.S, c, nt, pt, ip, xx, lane);
        __syncthreads();
        lr_cross_diag_put(xx, pt, lane);
        __syncthreads();
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t row = row0 + kq + 4 * g;
            const double xs = pt[kq + 4 * g];
            const bool live = rtime[wave][kq + 4 * g] >= 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = j * 16 + m;
                if (j < nt && live && i < c) A.K[row * c + i] = In(base_eval<double>(A.kind, ip[j][g], xs, ss[j], A.p0, A.p1));
            }
        }
    }
}

// (the kernels below are no templates: defined once, in lr_cross_inst.hip; lr_eval_wide_inst.hip takes the templates above alone)
#ifndef GPSIG_LR_CROSS_TEMPLATES_ONLY
// |S_i|^2 by the walk of lr_cross_inner on S itself: one wavefront per 16 landmarks
__global__ __launch_bounds__(64) void lr_cross_norms_kernel(const double* __restrict__ S, int c, int d, double* __restrict__ sn) {
    const int lane = threadIdx.x, m = lane & 15, kq = lane >> 4;
    const int i = blockIdx.x * 16 + m;
    lr_cross_f64x4 ss = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < d; k0 += 4) {
        const int f = k0 + kq;
        const double b = (i < c && f < d) ? S[size_t(i) * d + f] : 0.0;
        ss = __builtin_amdgcn_mfma_f64_16x16x4f64(b, b, ss, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 4; ++g)
        if (m == kq + 4 * g && i < c) sn[i] = ss[g];
}

__global__ __launch_bounds__(LR_CROSS_THREADS) void lr_cross_kernel(LrCrossArgs A) {
    __shared__ double tiles[LR_CROSS_WAVES][16 * LR_CROSS_LD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    double* const pt = tiles[wave];
    const int c = A.c, nt = (c + 15) / 16;
    const int64_t nblk = (A.n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    double ss[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ss[j] = j * 16 + m < c ? A.sn[j * 16 + m] : 0.0;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {                // (the same number of rounds for every wavefront: barriers inside)
        const int64_t row0 = (b * LR_CROSS_WAVES + wave) * 16;
        lr_cross_f64x4 ip[4], xx = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) ip[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
        lr_cross_inner(A.P, A.n, A.d, A.S, c, nt, row0, pt, ip, xx, lane);
        __syncthreads();
        lr_cross_diag_put(xx, pt, lane);
        __syncthreads();
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t row = row0 + kq + 4 * g;
            const double xs = pt[kq + 4 * g];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = j * 16 + m;
                if (j < nt && row < A.n && i < c) A.K[row * c + i] = base_eval<double>(A.kind, ip[j][g], xs, ss[j], A.p0, A.p1);
            }
        }
    }
}

__global__ __launch_bounds__(LR_CROSS_THREADS) void lr_cross_grad_points_kernel(LrCrossArgs A) {
    __shared__ double tiles[LR_CROSS_WAVES][16 * LR_CROSS_LD];
    __shared__ double red[LR_CROSS_WAVES][LR_CROSS_MAX_C + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    double* const pt = tiles[wave];
    const int c = A.c, d = A.d, nt = (c + 15) / 16;
    const int64_t nblk = (A.n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    double ss[4], cs[4] = {0.0, 0.0, 0.0, 0.0}, accP = 0.0;      // cs: this lane's share of colsum(G o ws) of column 16 j + m
#pragma unroll
    for (int j = 0; j < 4; ++j) ss[j] = j * 16 + m < c ? A.sn[j * 16 + m] : 0.0;
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {
        const int64_t row0 = (b * LR_CROSS_WAVES + wave) * 16;
        lr_cross_f64x4 ip[4], xx = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < 4; ++j) ip[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
        lr_cross_inner(A.P, A.n, d, A.S, c, nt, row0, pt, ip, xx, lane);
        __syncthreads();
        lr_cross_diag_put(xx, pt, lane);
        __syncthreads();
        double xs[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) xs[g] = pt[kq + 4 * g];
        __syncthreads();                                                    // (the tile is rewritten: W of the 16 points, [point][landmark], zeros beyond c)
        double ax[4], any[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int64_t row = row0 + kq + 4 * g;
            ax[g] = 0.0; any[g] = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = j * 16 + m;
                double wy = 0.0;
                if (j < nt && row < A.n && i < c) {
                    const double gk = A.G[row * c + i];
                    if (gk != 0.0) {
                        const BaseGrad bg = base_eval_grad(A.kind, ip[j][g], xs[g], ss[j], A.p0, A.p1);
                        wy = gk * (bg.cy - bg.cd);
                        ax[g] = fma(gk, bg.cx + bg.cd, ax[g]);
                        cs[j] = fma(gk, bg.cx2 + bg.cd, cs[j]);
                        accP = fma(gk, bg.dp0, accP);
                        any[g] = 1.0;
                    }
                    A.W[row * c + i] = wy;
                }
                pt[(kq + 4 * g) * LR_CROSS_LD + j * 16 + m] = wy;
            }
            // the row's sums over the 16 lanes that hold its columns, in a fixed order
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                ax[g] += __shfl_xor(ax[g], o, 64);
                any[g] = fmax(any[g], __shfl_xor(any[g], o, 64));
            }
            if (m == 0 && row < A.n) A.live[row] = any[g];
        }
        __syncthreads();
        // dP[row][f] = sum_i W[row][i] S_i[f] + ax[row] P[row][f]: the A operands of the c-deep product stay in registers
        double wa[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) wa[kk] = kk < nt * 4 ? pt[m * LR_CROSS_LD + kk * 4 + kq] : 0.0;
        for (int f0 = 0; f0 < d; f0 += 16) {
            const int f = f0 + m;
            lr_cross_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                if (kk < nt * 4) {
                    const int i = kk * 4 + kq;
                    const double bv = (i < c && f < d) ? A.S[size_t(i) * d + f] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wa[kk], bv, acc, 0, 0, 0);
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int64_t row = row0 + kq + 4 * g;
                if (row < A.n && f < d) A.dP[row * d + f] = ax[g] != 0.0 ? fma(ax[g], A.P[row * d + f], acc[g]) : acc[g];
            }
        }
    }
    // ---- this workgroup's partial sums: the columns over the four row groups of a wavefront, then over the wavefronts, in a fixed order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cs[j] += __shfl_xor(cs[j], 16, 64);
        cs[j] += __shfl_xor(cs[j], 32, 64);
        if (kq == 0) red[wave][j * 16 + m] = cs[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) accP += __shfl_xor(accP, o, 64);
    if (lane == 0) red[wave][LR_CROSS_MAX_C] = accP;
    __syncthreads();
    double* part = A.part + int64_t(blockIdx.x) * (c + 1);
    for (int q = threadIdx.x; q <= c; q += LR_CROSS_THREADS) {
        const int src = q < c ? q : LR_CROSS_MAX_C;
        double s = 0.0;
        for (int w = 0; w < LR_CROSS_WAVES; ++w) s += red[w][src];
        part[q] = s;
    }
}

// dspart[y][i][f] = sum over the points t of share y of W[t][i] P[t][f]: wavefront w of workgroup (x, y) owns the columns 64 x + 16 w ..
__global__ __launch_bounds__(LR_CROSS_THREADS) void lr_cross_grad_landmarks_kernel(LrCrossArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    const int c = A.c, d = A.d, nt = (c + 15) / 16;
    const int f0 = (blockIdx.x * LR_CROSS_WAVES + wave) * 16, f = f0 + m;
    if (f0 >= d) return;                                                    // (no barriers in this kernel)
    const int64_t t0 = int64_t(blockIdx.y) * A.share, t1 = t0 + A.share < A.n ? t0 + A.share : A.n;
    lr_cross_f64x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = lr_cross_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t tb = t0; tb < t1; tb += 4) {
        const int64_t t = tb + kq;
        const bool on = t < t1 && A.live[t] != 0.0;
        const double bv = (on && f < d) ? A.P[t * d + f] : 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < nt) {
                const int i = j * 16 + m;
                const double av = (on && i < c) ? A.W[t * c + i] : 0.0;
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
            }
        }
    }
    double* out = A.dspart + int64_t(blockIdx.y) * c * d;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = j * 16 + kq + 4 * g;
            if (j < nt && i < c && f < d) out[size_t(i) * d + f] = acc[j][g];
        }
}

// colsum[i] = the workgroups' partials in order (i < c), g_base likewise (i == c; may be NULL)
__global__ __launch_bounds__(128) void lr_cross_grad_reduce_cols_kernel(const double* __restrict__ part, int nparts, int c, double* __restrict__ colsum,
                                                                        double* __restrict__ g_base) {
    const int q = threadIdx.x;
    if (q > c) return;
    double s = 0.0;
    for (int k = 0; k < nparts; ++k) s += part[int64_t(k) * (c + 1) + q];
    if (q < c) colsum[q] = s;
    else if (g_base) g_base[0] = s;
}
// dS[i][f] = the shares' partials in order + colsum[i] S[i][f]
__global__ __launch_bounds__(256) void lr_cross_grad_reduce_kernel(const double* __restrict__ dspart, int shares, const double* __restrict__ colsum,
                                                                   const double* __restrict__ S, int c, int d, double* __restrict__ dS) {
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x, width = int64_t(c) * d;
    if (q >= width) return;
    double s = 0.0;
    for (int k = 0; k < shares; ++k) s += dspart[int64_t(k) * width + q];
    const double cs = colsum[q / d];
    dS[q] = cs != 0.0 ? fma(cs, S[q], s) : s;
}

#endif  // GPSIG_LR_CROSS_TEMPLATES_ONLY

}  // namespace gpsig
