// lr_grad_kernel.hpp -- reverse pass of the low-rank feature map of a batch of sequences (lr_fused_kernel.hpp) in ONE kernel (round 4).
//
// The reference trains low-rank mode through TensorFlow's autodiff of Nystrom_map (gpsig/low_rank_calculations.py:26-61), the running
// sums and the sparse projections of signature_kern_first_order_lr_feature (gpsig/signature_algs.py:162-192); there is no gradient code to
// restate.  Round 3 ran that reverse pass as torch ops (gather x gather x value, index_add: gpsig_amd/autodiff.py), which moves every
// (N, L, nnz) product through HBM: 9.1 s for the SVGP covariances of BASELINE configs[2] against 14 ms in exact mode.  Here a workgroup
// owns one sequence at a time and keeps four (width, L) arrays in LDS, like the forward kernel keeps three:
//
//   forward again   x, kxs = kappa(x, S), feat = kxs Wh, U = time difference; E_2 = excumsum_t(U); E_{i+1} = excumsum_t(sketch_i(U, E_i))
//                   -- the E_i go to a per-WORKGROUP scratch (a few tens of KB each: L2-resident), nothing per sequence is stored in HBM
//   levels M .. 2   dP_M[t] = g_M (Phi_M = sum_t P_M);  dU[i1] += sum_e val E_i[i2] dP_i[j]   (the sketch's entries grouped by i1)
//                   dE_i[i2] = sum_e val U[i1] dP_i[j]  (grouped by i2);  dP_{i-1}[t] = g_{i-1} + sum_{t' > t} dE_i[t']
//                   -- both are GATHERS over transposed copies of the sketch (built once per draw on the host), the same loop as the
//                   forward sketch: entries through the scalar unit, operands full-width LDS reads, no atomics, deterministic
//   level 1         dU += dP_1;  dfeat = the time difference's adjoint;  dkxs = dfeat Wh^T;  dWh += kxs^T dfeat
//   base kernel     dx[t] = sum_i dkxs[t][i] d kappa(x_t, S_i) / dx,  dS_i += sum_t dkxs[t][i] d kappa / dS_i  (base_eval_grad, grad_core.hpp)
//
// dWh, dS and the base kernel's own parameter are summed over the sequences a workgroup processes in registers and leave as one partial
// per workgroup (added up by lr_grad_reduce_kernel in a fixed order).  Layout and lane mappings as in lr_fused_kernel.hpp: arrays
// [column][time] with an odd row stride, lane = time for everything elementwise in time, thread = column for the running sums.
//
// SignatureSpectral (lr_seq_features_grad_spectral_kernel, SPEC): kappa(x, S_i) by spectral_pair on the trainable parameters (ld = d,
// read through the scalar unit); kxs is computed once per sequence and kept in the workgroup's scratch next to the E_i for the dWh sums.
// The kernel stops at dkxs: it writes dkxs (N, L, c) to HBM and sums dWh only.  The spectral cross op's reverse kernels
// (spectral_cross_api.hip) turn dkxs into dx, dS, dalpha, domega and dgamma: the parameters' sums over every (point, landmark, component)
// are reduced there per workgroup and combined in a fixed order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"
#include "grad_core.hpp"
#include "lr_fused_args.hpp"
#include "spectral_pair.hpp"

namespace gpsig {

struct LrGradSketch {
    const int32_t* colptr; const LrEntry* ent;        // by output column j: (val, i1, i2)                      P[j]   = sum val U[i1] E[i2]
    const int32_t* ptr1; const LrEntry* ent1;         // by i1: (val, i2, j) in the entry's (i1, i2) fields        dU[i1] += sum val E[i2] dP[j]
    const int32_t* ptr2; const LrEntry* ent2;         // by i2: (val, i1, j)                                        dE[i2]  = sum val U[i1] dP[j]
};

struct LrGradArgs {
    const double* X; int64_t N; int L, d;              // sequences as given (N, L, d): the level primitives take scaled inputs
    const double* S;                                   // landmarks (c, d)
    const double* Wh;                                  // whitening (c, c): feat[j] = sum_i kxs[i] Wh[i][j]
    int c, r, M, difference, kind;
    double p0, p1;
    LrGradSketch sk[LR_FUSED_MAX_SKETCHES];
    const double* dPhi; int F;                         // upstream (N, F)
    double* gX;                                        // (N, L, d)
    double* part;                                      // per-workgroup partial sums [grid][c d + c c + 1]: dS, dWh, d base parameter
    double* escr; int64_t escr_stride;                 // per-workgroup scratch for E_2 .. E_M (doubles per workgroup)
    int lp, rows_b;
};

// the spectral instance's arguments (p0 = Q, p1 = family): the trainable parameters (Q), (Q, d), (Q, d) on the device; dkxs (N, L, c) out;
// kxs of the current sequence at escr + kxs_off; part holds dWh alone ([grid][c c]); gX, dS and the base parameter are not written
struct LrGradSpectralArgs : LrGradArgs {
    const double* alpha; const double* omega; const double* gamma;
    double* dkxs; int64_t kxs_off;
};

// the ragged instance's arguments (lr_fused_args.hpp: lr_ragged): sequence n has lengths[n] of its L points; gX rows beyond them are zeros
struct LrGradRaggedArgs : LrGradArgs { const int32_t* lengths; };
template <> struct lr_ragged<LrGradRaggedArgs> { static constexpr bool value = true; };

constexpr int LR_GRAD_THREADS = 512;                   // (the smaller of the two workgroup sizes built: what the per-thread tables are sized for)
constexpr int LR_GRAD_KW = 8, LR_GRAD_KS = 8;          // (i, j) pairs of dWh and (i, f) pairs of dS per thread: c <= 64, c d <= 4096

// (the LDS footprint, lr_grad_lds_bytes: lr_tile_plan.hpp)

// ---- loops shared with the tiled kernels (lr_tiled_kernel.hpp): `n` time steps / points of arrays with row stride lp, nchunk chunks of 64 lanes
// out[row][t] (+)= sum_e val * a[ia][t] * b[ib][t] over the entries of `row`, t < n: the forward sketch's loop (also the two gathers of the
// reverse pass, over the by-i1 / by-i2 copies of a sketch)
template <int NW, int UNROLL>
__device__ __forceinline__ void lr_sketch_apply(const int32_t* ptr_, const LrEntry* ent_, int nrows, const double* a, const double* b, double* out,
                                                bool accumulate, int lp, int n, int nchunk, int lane, int wave) {
    const lr_const_ptr<int32_t> ptr = lr_as_const(ptr_);
    const lr_const_ptr<LrEntry> ent = lr_as_const(ent_);
    for (int row = wave; row < nrows; row += NW) {
        const int e0 = ptr[row], e1 = ptr[row + 1];
        for (int ch = 0; ch < nchunk; ++ch) {
            const int t = ch * 64 + lane;
            const int tt = t < n ? t : 0;                   // idle lanes read a valid address
            double acc = 0.0;
#pragma unroll UNROLL
            for (int e = e0; e < e1; ++e) {
                const double val = ent[e].val;
                const int ia = ent[e].i1, ib = ent[e].i2;
                acc = fma(val * a[ia * lp + tt], b[ib * lp + tt], acc);
            }
            if (t < n) out[row * lp + t] = accumulate ? out[row * lp + t] + acc : acc;
        }
    }
}
// xb[f][t] = the n points (n, d) at Xn
template <int THREADS>
__device__ __forceinline__ void lr_load_points(const double* Xn, int n, int d, int lp, double* xb) {
    for (int q = threadIdx.x; q < n * d; q += THREADS) {
        const int t = q / d, f = q - t * d;
        xb[f * lp + t] = Xn[q];
    }
}
// kb[i][t] = kappa(x_t, S_i) for the families of base_eval
template <int NW>
__device__ __forceinline__ void lr_cross_base(int kind, double p0, double p1, lr_const_ptr<double> Sg, int c, int d, const double* xb, double* kb,
                                              int lp, int n, int nchunk, int lane, int wave) {
    for (int ch = 0; ch < nchunk; ++ch) {
        const int t = ch * 64 + lane;
        if (t < n) {
            double xs = 0.0;
            for (int f = 0; f < d; ++f) { const double x = xb[f * lp + t]; xs = fma(x, x, xs); }
            for (int i = wave; i < c; i += NW) {
                double ip = 0.0, ss = 0.0;
                for (int f = 0; f < d; ++f) {
                    const double y = Sg[size_t(i) * d + f];
                    ip = fma(xb[f * lp + t], y, ip);
                    ss = fma(y, y, ss);
                }
                kb[i * lp + t] = base_eval<double>(kind, ip, xs, ss, p0, p1);
            }
        }
    }
}

// The tail of a sequence's (a tile's) reverse pass, on the points [q0, np) of the arrays (row stride lp); kxs in B0, dfeat in Xb:
//   dWh[i][j] += sum_t kxs[i][t] dfeat[j][t]  (accW, KW pairs per thread: KW THREADS >= c c);  dkxs[i][t] = sum_j dfeat[j][t] Wh[i][j] -> Y
template <int THREADS, int KW>
__device__ __forceinline__ void lr_grad_whiten_adjoint(int c, int lp, int q0, int np, const double* B0, const double* Xb, lr_const_ptr<double> Whg,
                                                       double* Y, double (&accW)[KW], int lane, int wave) {
    constexpr int NW = THREADS / 64;
    const int nchunk = (np + 63) / 64;
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int q = k * THREADS + threadIdx.x;
        if (q < c * c) {
            const int i = q / c, j = q - i * c;
            double acc = 0.0;
            for (int t = q0; t < np; ++t) acc = fma(B0[i * lp + t], Xb[j * lp + t], acc);
            accW[k] += acc;
        }
    }
    for (int ch = 0; ch < nchunk; ++ch) {
        const int t = ch * 64 + lane;
        if (t >= q0 && t < np) {
            for (int i = wave; i < c; i += NW) {
                double acc = 0.0;
#pragma unroll 4
                for (int j = 0; j < c; ++j) acc = fma(Xb[j * lp + t], Whg[size_t(i) * c + j], acc);
                Y[i * lp + t] = acc;
            }
        }
    }
}
// ... and through the base kernel: d kappa / dx = wy S_i + wx x,  d kappa / dS_i = wy x + ws S_i  (BaseGrad of grad_core.hpp); x in B1, dkxs in Y.
//   Y[i][t] <- dkxs wy,  Xb[i][t] <- dkxs ws,  B0[wave][t] <- this wave's share of sum_i dkxs wx;  the points' gX rows (point t is the
//   sequence's point t0 + t) are written, dS and the base parameter's sums go to accS (KS pairs per thread: KS THREADS >= c d) and accP
template <int THREADS, typename Args, int KS>
__device__ __forceinline__ void lr_grad_base_phase(const Args& A, lr_const_ptr<double> Sg, int64_t n, int t0, int q0, int np, double* B0, const double* B1,
                                                   double* Xb, double* Y, double (&accS)[KS], double& accP, int lane, int wave) {
    constexpr int NW = THREADS / 64;
    const int lp = A.lp, c = A.c, d = A.d, L = A.L;
    const int nchunk = (np + 63) / 64;
    for (int ch = 0; ch < nchunk; ++ch) {
        const int t = ch * 64 + lane;
        const bool mine = t >= q0 && t < np;
        double ax = 0.0;
        if (mine) {
            double xs = 0.0;
            for (int f = 0; f < d; ++f) { const double x = B1[f * lp + t]; xs = fma(x, x, xs); }
            for (int i = wave; i < c; i += NW) {
                double ip = 0.0, ss = 0.0;
                for (int f = 0; f < d; ++f) {
                    const double y = Sg[size_t(i) * d + f];
                    ip = fma(B1[f * lp + t], y, ip);
                    ss = fma(y, y, ss);
                }
                const BaseGrad bg = base_eval_grad(A.kind, ip, xs, ss, A.p0, A.p1);
                const double dk = Y[i * lp + t];
                Y[i * lp + t] = dk * (bg.cy - bg.cd);
                Xb[i * lp + t] = dk * (bg.cx2 + bg.cd);
                ax = fma(dk, bg.cx + bg.cd, ax);
                accP = fma(dk, bg.dp0, accP);
            }
        }
        __syncthreads();                         // (kxs in B0 was last read by the dWh sums, before the caller's barrier)
        if (mine) B0[wave * lp + t] = ax;
        __syncthreads();
        // dx[t][f] = sum_i Y[i][t] S_i[f] + x[f][t] sum_w B0[w][t]
        if (mine) {
            double axs = 0.0;
#pragma unroll
            for (int w2 = 0; w2 < NW; ++w2) axs += B0[w2 * lp + t];
            for (int f = wave; f < d; f += NW) {
                double acc = axs * B1[f * lp + t];
                for (int i = 0; i < c; ++i) acc = fma(Y[i * lp + t], Sg[size_t(i) * d + f], acc);
                A.gX[(n * int64_t(L) + t0 + t) * d + f] = acc;
            }
        }
        __syncthreads();
    }
    // dS[i][f] += sum_t Y[i][t] x[f][t] + S_i[f] sum_t Xb[i][t]
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        const int q = k * THREADS + threadIdx.x;
        if (q < c * d) {
            const int i = q / d, f = q - i * d;
            double a1 = 0.0, a2 = 0.0;
            for (int t = q0; t < np; ++t) {
                a1 = fma(Y[i * lp + t], B1[f * lp + t], a1);
                a2 += Xb[i * lp + t];
            }
            accS[k] += fma(a2, Sg[size_t(i) * d + f], a1);
        }
    }
}
// the gX rows [Ln, L) of a sequence (gXn: its (L, d) block): plain stores, every row written once
template <int THREADS>
__device__ __forceinline__ void lr_zero_padded_rows(double* gXn, int Ln, int L, int d) {
    for (int q = Ln * d + threadIdx.x; q < L * d; q += THREADS) gXn[q] = 0.0;
}
// this workgroup's partial sums [c d + c c + 1]: dS, dWh, d base parameter (`red`: NW doubles of LDS)
template <int THREADS, typename Args, int KW, int KS>
__device__ __forceinline__ void lr_grad_write_partials(const Args& A, const double (&accW)[KW], const double (&accS)[KS], double accP,
                                                       double* red, int lane, int wave) {
    constexpr int NW = THREADS / 64;
    const int c = A.c, d = A.d;
    double* part = A.part + int64_t(blockIdx.x) * (int64_t(c) * d + int64_t(c) * c + 1);
#pragma unroll
    for (int k = 0; k < KS; ++k) {
        const int q = k * THREADS + threadIdx.x;
        if (q < c * d) part[q] = accS[k];
    }
#pragma unroll
    for (int k = 0; k < KW; ++k) {
        const int q = k * THREADS + threadIdx.x;
        if (q < c * c) part[int64_t(c) * d + q] = accW[k];
    }
    __syncthreads();
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) accP += __shfl_xor(accP, o, 64);
    if (lane == 0) red[wave] = accP;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w2 = 0; w2 < NW; ++w2) s += red[w2];
        part[int64_t(c) * d + int64_t(c) * c] = s;
    }
}

template <int THREADS, bool SPEC, typename Args>
__device__ __forceinline__ void lr_seq_features_grad_body(const Args& A) {
    constexpr int NW = THREADS / 64, UNROLL = 8;
    constexpr bool RAGGED = lr_ragged<Args>::value;
    extern __shared__ double lrg_lds[];
    const int lp = A.lp, c = A.c, r = A.r, L = A.L, d = A.d, M = A.M;
    double* const B0 = lrg_lds;                                 // U; later kxs; later per-wave partial sums
    double* const B1 = B0 + size_t(A.rows_b) * lp;              // x; dU; x again
    double* BX = B1 + size_t(A.rows_b) * lp;
    double* BY = BX + size_t(A.rows_b) * lp;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l = A.difference ? L - 1 : L;                     // time steps of U
    const int nchunk = (L + 63) / 64;
    int Ln = L, ln = l, nch = nchunk;                           // the current sequence's points, steps and chunks: the ragged instances set them per sequence
    double* const escr = A.escr + int64_t(blockIdx.x) * A.escr_stride;
    const lr_const_ptr<double> Sg = lr_as_const(A.S);
    const lr_const_ptr<double> Whg = lr_as_const(A.Wh);

    auto apply = [&](const int32_t* ptr_, const LrEntry* ent_, int nrows, const double* a, const double* b, double* out, bool accumulate) {
        lr_sketch_apply<NW, UNROLL>(ptr_, ent_, nrows, a, b, out, accumulate, lp, ln, nch, lane, wave);
    };
    // x[f][t] and kxs[i][t] = kappa(x_t, S_i) of the current sequence
    auto load_x = [&](const double* Xn, double* xb) { lr_load_points<THREADS>(Xn, Ln, d, lp, xb); };
    auto cross = [&](const double* xb, double* kb) {
        if constexpr (SPEC) {
            const lr_const_ptr<double> al = lr_as_const(A.alpha), om = lr_as_const(A.omega), ga = lr_as_const(A.gamma);
            const int Q = int(A.p0), family = int(A.p1);
            for (int ch = 0; ch < nch; ++ch) {
                const int t = ch * 64 + lane;
                if (t < Ln)
                    for (int i = wave; i < c; i += NW)
                        kb[i * lp + t] = spectral_pair(al, om, ga, d, Q, family, d, [&](int f) { return xb[f * lp + t]; },
                                                       [&](int f) { return Sg[size_t(i) * d + f]; });
            }
            return;
        }
        lr_cross_base<NW>(A.kind, A.p0, A.p1, Sg, c, d, xb, kb, lp, Ln, nch, lane, wave);
    };

    double accW[LR_GRAD_KW], accS[LR_GRAD_KS], accP = 0.0;      // this workgroup's sums over its sequences: dWh, dS, d base parameter
#pragma unroll
    for (int k = 0; k < LR_GRAD_KW; ++k) accW[k] = 0.0;
#pragma unroll
    for (int k = 0; k < LR_GRAD_KS; ++k) accS[k] = 0.0;

    for (int64_t n = blockIdx.x; n < A.N; n += gridDim.x) {
        const double* Xn = A.X + n * int64_t(L) * d;
        const double* g = A.dPhi + n * int64_t(A.F);
        if constexpr (RAGGED) {                                 // the sequence's own extent; the gX rows of its padded points are zeros
            Ln = lr_seq_points(A, n, L);
            ln = A.difference ? Ln - 1 : Ln;
            nch = (Ln + 63) / 64;
            if constexpr (SPEC) lr_zero_padded_rows<THREADS>(A.dkxs + n * int64_t(L) * c, Ln, L, c);      // (its output is dkxs, not gX)
            else lr_zero_padded_rows<THREADS>(A.gX + n * int64_t(L) * d, Ln, L, d);
        }
        __syncthreads();
        // ---- forward again: x -> B1, kxs -> BX, feat -> BY, U -> B0
        load_x(Xn, B1);
        __syncthreads();
        cross(B1, BX);
        __syncthreads();
        if constexpr (SPEC)                                     // kxs for the dWh sums below (the spectral kappa is the costly phase)
            for (int q = threadIdx.x; q < c * Ln; q += THREADS) {
                const int i = q / Ln, t = q - i * Ln;
                escr[A.kxs_off + q] = BX[i * lp + t];
            }
        for (int ch = 0; ch < nch; ++ch) {
            const int t = ch * 64 + lane;
            if (t < Ln) {
                for (int j = wave; j < c; j += NW) {
                    double acc = 0.0;
#pragma unroll 4
                    for (int i = 0; i < c; ++i) acc = fma(BX[i * lp + t], Whg[size_t(i) * c + j], acc);
                    BY[j * lp + t] = acc;
                }
            }
        }
        __syncthreads();
        for (int ch = 0; ch < nch; ++ch) {
            const int t = ch * 64 + lane;
            if (t < ln) {
                for (int j = wave; j < c; j += NW) {
                    const double f0 = BY[j * lp + t];
                    B0[j * lp + t] = A.difference ? BY[j * lp + t + 1] - f0 : f0;
                }
            }
        }
        __syncthreads();
        // E_2 = excumsum_t(U) -> BX and the scratch; then E_{i+1} = excumsum_t(sketch_i(U, E_i)), i = 2 .. M-1
        double* cur = BX;
        double* nxt = BY;
        if (M >= 2) {
            for (int j = threadIdx.x; j < c; j += THREADS) {
                double run = 0.0;
                const double* u = B0 + size_t(j) * lp;
                double* e = cur + size_t(j) * lp;
                double* es = escr + size_t(j) * ln;
                for (int t = 0; t < ln; ++t) { const double v = u[t]; e[t] = run; es[t] = run; run += v; }
            }
            __syncthreads();
            int64_t eo = int64_t(c) * ln;
            for (int lev = 2; lev < M; ++lev) {
                apply(A.sk[lev - 2].colptr, A.sk[lev - 2].ent, r, B0, cur, nxt, false);
                __syncthreads();
                for (int j = threadIdx.x; j < r; j += THREADS) {
                    double run = 0.0;
                    double* e = nxt + size_t(j) * lp;
                    double* es = escr + eo + size_t(j) * ln;
                    for (int t = 0; t < ln; ++t) { const double v = e[t]; e[t] = run; es[t] = run; run += v; }
                }
                __syncthreads();
                eo += int64_t(r) * ln;
                double* tmp = cur; cur = nxt; nxt = tmp;
            }
        }
        // ---- backward through the levels.  dU -> B1 (x is read again from memory later)
        for (int q = threadIdx.x; q < c * lp; q += THREADS) B1[q] = 0.0;
        double* Y = nxt;                            // dP of the level being processed
        double* Xb = cur;                           // E of that level, then dE
        if (M >= 2) {
            const double* gM = g + 1 + c + (M - 2) * r;
            for (int ch = 0; ch < nch; ++ch) {
                const int t = ch * 64 + lane;
                if (t < ln)
                    for (int j = wave; j < r; j += NW) Y[j * lp + t] = gM[j];
            }
        }
        __syncthreads();
        for (int lev = M; lev >= 2; --lev) {
            const int w = lev == 2 ? c : r;         // width of E_lev
            // E_lev from the scratch (the forward pass left E_{M} in `cur` already)
            int64_t eo = 0;
            for (int k = 2; k < lev; ++k) eo += int64_t(k == 2 ? c : r) * ln;
            if (lev != M || true) {
                for (int q = threadIdx.x; q < w * ln; q += THREADS) {
                    const int j = q / ln, t = q - j * ln;
                    Xb[j * lp + t] = escr[eo + q];
                }
            }
            __syncthreads();
            const LrGradSketch sk = A.sk[lev - 2];
            apply(sk.ptr1, sk.ent1, c, Xb, Y, B1, true);              // dU[i1] += val E[i2] dP[j]
            __syncthreads();
            apply(sk.ptr2, sk.ent2, w, B0, Y, Xb, false);             // dE[i2]  = val U[i1] dP[j]   (E is no longer needed)
            __syncthreads();
            // dP_{lev-1}[t] = g_{lev-1} + sum_{t' > t} dE[t'], in place
            const double* gl = lev - 1 == 1 ? g + 1 : g + 1 + c + (lev - 3) * r;
            for (int j = threadIdx.x; j < w; j += THREADS) {
                double run = gl[j];
                double* e = Xb + size_t(j) * lp;
                for (int t = ln - 1; t >= 0; --t) { const double v = e[t]; e[t] = run; run += v; }
            }
            __syncthreads();
            double* tmp = Xb; Xb = Y; Y = tmp;      // Y: dP_{lev-1}
        }
        // level 1: Phi_1 = sum_t U (M == 1: that is all there is)
        for (int ch = 0; ch < nch; ++ch) {
            const int t = ch * 64 + lane;
            if (t < ln)
                for (int j = wave; j < c; j += NW) B1[j * lp + t] += M >= 2 ? Y[j * lp + t] : g[1 + j];
        }
        __syncthreads();
        // dfeat[j][t] -> Xb: the adjoint of the time difference (signature_algs.py:180)
        for (int ch = 0; ch < nch; ++ch) {
            const int t = ch * 64 + lane;
            if (t < Ln)
                for (int j = wave; j < c; j += NW)
                    Xb[j * lp + t] = A.difference ? (t >= 1 ? B1[j * lp + t - 1] : 0.0) - (t < ln ? B1[j * lp + t] : 0.0) : B1[j * lp + t];
        }
        __syncthreads();
        // x -> B1 and kxs -> B0 once more (U and dU are done with); the spectral instance reads kxs back from its scratch
        if constexpr (SPEC) {
            for (int q = threadIdx.x; q < c * Ln; q += THREADS) {
                const int i = q / Ln, t = q - i * Ln;
                B0[i * lp + t] = escr[A.kxs_off + q];
            }
        } else {
            load_x(Xn, B1);
            __syncthreads();
            cross(B1, B0);
        }
        __syncthreads();
        lr_grad_whiten_adjoint<THREADS>(c, lp, 0, Ln, B0, Xb, Whg, Y, accW, lane, wave);
        __syncthreads();
        if constexpr (SPEC) {                        // dkxs (L, c) of this sequence out; the spectral cross op's reverse kernels take it from here
            double* dk = A.dkxs + n * int64_t(L) * c;
            for (int q = threadIdx.x; q < Ln * c; q += THREADS) {
                const int t = q / c, i = q - t * c;
                dk[q] = Y[i * lp + t];
            }
            continue;                                // (the loop's first barrier orders these reads before Y is written again)
        }
        lr_grad_base_phase<THREADS>(A, Sg, n, 0, 0, Ln, B0, B1, Xb, Y, accS, accP, lane, wave);
    }
    // ---- this workgroup's partial sums
    if constexpr (SPEC) {
        double* part = A.part + int64_t(blockIdx.x) * (int64_t(c) * c);
#pragma unroll
        for (int k = 0; k < LR_GRAD_KW; ++k) {
            const int q = k * THREADS + threadIdx.x;
            if (q < c * c) part[q] = accW[k];
        }
        return;
    }
    lr_grad_write_partials<THREADS>(A, accW, accS, accP, lrg_lds, lane, wave);
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_grad_kernel(LrGradArgs A) { lr_seq_features_grad_body<THREADS, false>(A); }

// SignatureSpectral: kxs by spectral_pair, dkxs out instead of the base-kernel phase (above)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_grad_spectral_kernel(LrGradSpectralArgs A) { lr_seq_features_grad_body<THREADS, true>(A); }

// out[q] = sum over the workgroups' partials, in order  (no template: defined once, lr_ragged_inst.hip takes the bodies alone)
#ifndef GPSIG_LR_BODIES_ONLY
__global__ void lr_grad_reduce_kernel(const double* __restrict__ part, int nparts, int64_t width, double* __restrict__ gS, int64_t nS,
                                      double* __restrict__ gWh, int64_t nW, double* __restrict__ gp) {
    const int64_t q = int64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (q >= width) return;
    double s = 0.0;
    for (int k = 0; k < nparts; ++k) s += part[int64_t(k) * width + q];
    if (q < nS) gS[q] = s;
    else if (q < nS + nW) gWh[q - nS] = s;
    else if (gp) gp[0] = s;
}
#endif

}  // namespace gpsig
