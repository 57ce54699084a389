// lr_eval_tiled_inst.hip -- the evaluation side's time-tiled, lengths-aware low-rank sequence feature kernels and their launchers (own
// translation unit: the instances of lr_fused_inst.hip, lr_ragged_inst.hip, lr_spectral_tiled_inst.hip and lr_grad_api.hip stay the code they
// were).  Argument blocks and what the kernels compute: lr_eval_tiled.hpp.  The body is a text of its own, not lr_tiled_fwd_body.inc: that one
// is float64 on scaled points and shared by three existing instances; this one is a template on the block's element type, scales the raw
// points itself (phase 0 of lr_seq_features_fused_body, per tile) and runs that body's phases on a tile.
//   layout     as the whole-sequence kernel: arrays [column][time] with the tile's row stride lp = TL + pad (room for the halo point), lane =
//              time in phases 0-2 and the sketches, thread = column in the running sums; behind the arrays one carry row per level.
//   carries    cf[i][j] = sum of P_i[j] (P_1 = U) over the earlier tiles: what E_{i+1} = excumsum_t(P_i) starts from in this tile, and
//              Phi_i after the last tile.  A running sum continues from its carry, so the additions happen in the whole-sequence kernel's order.
//   ragged     Ln = lengths[n] clamped to [1, L] through the scalar unit; ln = Ln - halo steps in lr_tile_count(ln, TL) tiles (one tile of no
//              steps for ln = 0: Phi = [1, 0, ..]).  A tile reads the points [t0, t0 + tl + halo) -- all below Ln.  With lags the interpolation
//              runs on the axis of Ln points (scaled_point's seq_len): its brackets lie below Ln too.
#define GPSIG_LR_BODIES_ONLY         // the headers' kernels that are no templates belong to lr_fused_inst.hip
#include "lr_fused_kernel.hpp"
#include "lr_eval_tiled.hpp"

namespace gpsig {

// One component of SignatureSpectral's kappa, out of line for the reason lr_spectral_tiled_inst.hip gives: inlined, the coefficients of the
// float64 exponential and cosine are hoisted into registers for the whole kernel.
__device__ __attribute__((noinline)) double lr_eval_spectral_term_val(double alpha, double w1, double w2, bool gauss) {
    return spectral_term(alpha, w1, w2, gauss).val;
}
// spectral_pair (spectral_pair.hpp) on that term, on the packed table
template <class FX, class FY>
__device__ __forceinline__ double lr_eval_spectral_pair(lr_const_ptr<double> tab, int Q, int family, int d, FX&& xf, FY&& yf) {
    const lr_const_ptr<double> alpha = tab, omega = tab + Q, gamma = tab + Q + Q * SPECTRAL_STRIDE;
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) {
        double w1 = 0.0, w2 = 0.0;
        for (int f = 0; f < d; ++f) {
            const double diff = xf(f) - yf(f);
            const double gd = gamma[q * SPECTRAL_STRIDE + f] * diff;
            w1 = fma(gd, gd, w1);
            w2 = fma(omega[q * SPECTRAL_STRIDE + f], diff, w2);
        }
        acc += lr_eval_spectral_term_val(alpha[q], w1, w2, spectral_gauss(family, q, Q));
    }
    return acc;
}

// a tile's U from the raw points: `np` points from point t0 of the sequence at Xn, `tl` steps.  xb / ft may be one array.  Ends with a barrier.
// la: scaled_point's seq_len -- the sequence's own points where the call has lengths (its lags then run on the sequence's own axis), else 0.
template <int THREADS, bool SPEC, typename Args, typename T = typename Args::value_type>
__device__ __forceinline__ void lr_tile_u(const Args& A, const T* Xn, int t0, int tl, int np, int la, T* xb, T* kx, T* ft, T* u, int lane, int wave) {
    constexpr int NW = THREADS / 64;
    const int lp = A.lp, c = A.c, L = A.L, d_eff = A.P.d_eff();
    const int pchunk = (np + 63) / 64, nchunk = (tl + 63) / 64;
    if constexpr (lr_eval_kx<Args>::value) {
        // ---- instead of phases 0 and 1: the tile's kxs rows from memory (the wide route: X is kxs (N, L, c), P.d_in = c)
        for (int q = threadIdx.x; q < np * c; q += THREADS) {
            const int t = q / c, i = q - t * c;
            kx[i * lp + t] = Xn[int64_t(t0) * c + q];
        }
    } else {
        // ---- phase 0: scaled observations, xb[fe][t]
        for (int q = threadIdx.x; q < np * d_eff; q += THREADS) {
            const int t = q / d_eff, fe = q - t * d_eff;
            xb[fe * lp + t] = scaled_point<T>(Xn, L, t0 + t, fe, A.P, la);
        }
        __syncthreads();
        // ---- phase 1: kxs, kx[i][t]
        for (int ch = 0; ch < pchunk; ++ch) {
            const int t = ch * 64 + lane;
            if (t < np) {
                T xs = T(0);
                for (int fe = 0; fe < d_eff; ++fe) { const T x = xb[fe * lp + t]; xs = fma(x, x, xs); }
                for (int i = wave; i < c; i += NW) {
                    const lr_const_ptr<T> Si = lr_as_const(A.S) + size_t(i) * d_eff;
                    if constexpr (SPEC) {
                        kx[i * lp + t] = lr_eval_spectral_pair(lr_as_const(A.spec), int(A.p0), int(A.p1), d_eff, [&](int f) { return xb[f * lp + t]; },
                                                               [&](int f) { return Si[f]; });
                    } else if constexpr (sizeof(T) == sizeof(float)) {
                        kx[i * lp + t] = lr_kappa_f32(A.kind, A.p0, A.p1, d_eff, xs, [&](int f) { return xb[f * lp + t]; }, [&](int f) { return Si[f]; });
                    } else {
                        T ip = T(0), ss = T(0);
                        for (int fe = 0; fe < d_eff; ++fe) {
                            const T y = Si[fe];
                            ip = fma(xb[fe * lp + t], y, ip);
                            ss = fma(y, y, ss);
                        }
                        kx[i * lp + t] = base_eval<T>(A.kind, ip, xs, ss, A.p0, A.p1);
                    }
                }
            }
        }
    }
    __syncthreads();
    // ---- phase 2: whitening, ft[j][t] = sum_i kx[i][t] * Wh[i][j]
    for (int ch = 0; ch < pchunk; ++ch) {
        const int t = ch * 64 + lane;
        if (t < np) {
            const lr_const_ptr<T> Wh = lr_as_const(A.Wh);
            for (int j = wave; j < c; j += NW) {
                T acc = T(0);
#pragma unroll 4
                for (int i = 0; i < c; ++i) acc = fma(kx[i * lp + t], Wh[size_t(i) * c + j], acc);
                ft[j * lp + t] = acc;
            }
        }
    }
    __syncthreads();
    // time difference (signature_algs.py:180) or a copy
    for (int ch = 0; ch < nchunk; ++ch) {
        const int t = ch * 64 + lane;
        if (t < tl) {
            for (int j = wave; j < c; j += NW) {
                const T f0 = ft[j * lp + t];
                u[j * lp + t] = A.difference ? ft[j * lp + t + 1] - f0 : f0;
            }
        }
    }
    __syncthreads();
}

// e[t] <- run, run += v[t] over a tile's steps for the columns j < w of `src` (thread = column), starting from and leaving the carry
template <int THREADS, typename T>
__device__ __forceinline__ void lr_eval_excumsum(const T* src, T* dst, int w, int lp, int tl, T* carry, bool store) {
    for (int j = threadIdx.x; j < w; j += THREADS) {
        T run = carry[j];
        const T* u = src + size_t(j) * lp;
        T* e = dst + size_t(j) * lp;
#pragma unroll 8
        for (int t = 0; t < tl; ++t) {
            const T v = u[t];
            if (store) e[t] = run;
            run += v;
        }
        carry[j] = run;
    }
}

template <int THREADS, int UNROLL, bool SPEC, typename Args>
__device__ __forceinline__ void lr_seq_features_eval_tiled_body(const Args& A) {
    using T = typename Args::value_type;
    constexpr int NW = THREADS / 64;
    T* const lds = lr_dyn_lds<T>();
    const int lp = A.lp, c = A.c, r = A.r, L = A.L, M = A.M, rows = A.rows_b, TL = A.TL;
    T* const U = lds;                                       // [c][lp]
    T* const bufA = U + size_t(c) * lp;                     // [rows][lp]
    T* const bufB = bufA + size_t(rows) * lp;               // [rows][lp]
    T* const cf = bufB + size_t(rows) * lp;                 // [LR_TILE_LEVELS][rows]: level i at (i - 1) rows
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int halo = A.difference ? 1 : 0;

    for (int64_t n = blockIdx.x; n < A.N; n += gridDim.x) {
        const T* Xn = A.X + n * int64_t(L) * A.P.d_in;
        T* phi = A.Phi + n * int64_t(A.F);
        const int Ln = lr_seq_points(A, n, L);
        const int ln = Ln - halo;                           // the sequence's own steps (wave-uniform), >= 0
        const int la = A.lengths ? Ln : 0;                  // ragged: lags on the sequence's own axis (dense: the table's, as ever)
        const int ntiles = lr_tile_count(ln, TL);
        __syncthreads();                                    // (the previous sequence's features were read from the carries)
        for (int q = threadIdx.x; q < M * rows; q += THREADS) cf[q] = T(0);
        for (int k = 0; k < ntiles; ++k) {
            const int t0 = lr_tile_first(k, TL), tl = lr_tile_steps(ln, k, TL), np = tl + halo;
            const int nchunk = (tl + 63) / 64;
            lr_tile_u<THREADS, SPEC>(A, Xn, t0, tl, np, la, bufB, bufA, bufB, U, lane, wave);
            lr_eval_excumsum<THREADS>(U, bufA, c, lp, tl, cf, M >= 2);                               // level 1; E_2 of the tile
            __syncthreads();
            T* cur = bufA;
            T* nxt = bufB;
            for (int lev = 2; lev <= M; ++lev) {
                const lr_const_ptr<int32_t> colptr = lr_as_const(A.sk[lev - 2].colptr);
                const auto ent = lr_as_const(A.sk[lev - 2].ent);
                // P_lev[t][j] = sum_e val * U[t][i1] * E[t][i2]                                   low_rank_calculations.py:64-193
                for (int j = wave; j < r; j += NW) {
                    const int e0 = colptr[j], e1 = colptr[j + 1];
                    for (int ch = 0; ch < nchunk; ++ch) {
                        const int t = ch * 64 + lane;
                        const int tt = t < tl ? t : 0;              // idle lanes read a valid address
                        T acc = T(0);
#pragma unroll UNROLL
                        for (int e = e0; e < e1; ++e) {
                            const T val = ent[e].val;         // (member by member: an address-space-4 struct has no copy constructor)
                            const int i1 = ent[e].i1, i2 = ent[e].i2;
                            acc = fma(val * U[i1 * lp + tt], cur[i2 * lp + tt], acc);
                        }
                        if (t < tl) nxt[j * lp + t] = acc;
                    }
                }
                __syncthreads();
                lr_eval_excumsum<THREADS>(nxt, nxt, r, lp, tl, cf + size_t(lev - 1) * rows, lev < M);
                __syncthreads();
                T* tmp = cur; cur = nxt; nxt = tmp;
            }
        }
        if (threadIdx.x == 0) phi[0] = T(1);
        for (int j = threadIdx.x; j < c; j += THREADS) phi[1 + j] = cf[j];
        for (int lev = 2; lev <= M; ++lev)
            for (int j = threadIdx.x; j < r; j += THREADS) phi[1 + c + (lev - 2) * r + j] = cf[size_t(lev - 1) * rows + j];
    }
}

__global__ __launch_bounds__(1024) void lr_seq_features_eval_tiled_kernel(LrEvalTiledArgs A) { lr_seq_features_eval_tiled_body<1024, 8, false>(A); }
__global__ __launch_bounds__(1024) void lr_seq_features_eval_tiled_spectral_kernel(LrEvalTiledArgs A) { lr_seq_features_eval_tiled_body<1024, 8, true>(A); }
__global__ __launch_bounds__(1024) void lr_seq_features_eval_tiled_f32_kernel(LrEvalTiledArgsF32 A) { lr_seq_features_eval_tiled_body<1024, 8, false>(A); }
// ... behind the cross matrix (the wide route): everything after phase 1 is the code above
__global__ __launch_bounds__(1024) void lr_seq_features_eval_tiled_kx_f32_kernel(LrEvalTiledKxArgsF32 A) { lr_seq_features_eval_tiled_body<1024, 8, false>(A); }

namespace {
// F, the work arrays' rows and the tile plan of L points; false where not even one 64-step tile fits
template <typename Args>
bool eval_tiled_fields(Args& A, bool f32, int pad, unsigned* grid, size_t* lds) {
    const int d_eff = A.P.d_eff();
    A.F = 1 + A.c + (A.M - 1) * A.r;
    A.rows_b = lr_fused_rows(A.c, A.r, d_eff);
    const LrTileDir D = lr_eval_tile_dir(f32, A.c, A.r, d_eff, A.L - (A.difference ? 1 : 0), pad);
    A.TL = D.TL; A.ntiles = D.ntiles; A.lp = D.lp;
    *lds = D.lds;
    *grid = unsigned(A.N < (int64_t(1) << 20) ? A.N : (int64_t(1) << 20));
    return D.TL > 0 && A.M <= LR_TILE_LEVELS;
}
}  // namespace

int lr_eval_tiled_launch(hipStream_t stream, LrEvalTiledArgs A, int pad) {
    unsigned grid;
    size_t lds;
    if (!eval_tiled_fields(A, false, pad, &grid, &lds)) return int(hipErrorInvalidValue);
    return A.kind == BASE_SPECTRAL ? lr_launch(lr_seq_features_eval_tiled_spectral_kernel, grid, 1024, lds, stream, A)
                                   : lr_launch(lr_seq_features_eval_tiled_kernel, grid, 1024, lds, stream, A);
}

int lr_eval_tiled_launch(hipStream_t stream, LrEvalTiledArgsF32 A, int pad) {
    unsigned grid;
    size_t lds;
    if (A.kind == BASE_SPECTRAL || !eval_tiled_fields(A, true, pad, &grid, &lds)) return int(hipErrorInvalidValue);
    return lr_launch(lr_seq_features_eval_tiled_f32_kernel, grid, 1024, lds, stream, A);
}

int lr_eval_tiled_kx_launch(hipStream_t stream, LrEvalTiledKxArgsF32 A, int pad) {
    unsigned grid;
    size_t lds;
    A.P = ScaleParams{};
    A.P.d_in = A.c;                                  // rows of kxs: the plan is that of max(c, r) rows
    if (!eval_tiled_fields(A, true, pad, &grid, &lds)) return int(hipErrorInvalidValue);
    return lr_launch(lr_seq_features_eval_tiled_kx_f32_kernel, grid, 1024, lds, stream, A);
}

}  // namespace gpsig
