// wide_kernels.hpp -- gfx950 kernels of the WIDE-STATE-SPACE route (round 6).
//
// Reference shapes: benchmarks/run_gpsig_benchmarks.py:32 runs every data set with num_lags=1 on time-augmented data, a state space of
// 2 (n_features + 1) columns (gpsig/kernels.py:350): 10 .. 1,928 for 9 of the 16 data sets of benchmarks/datasets.json.  The exact-shape kernels
// keep a lane's operands in registers (Kzx: <= 8 columns, the sequence lattices: <= 32); beyond that the base kernel's matrix of
// kernels.py:226 / :329 / :333 is what the reference says it is, a d-deep contraction -- and north_star puts exactly that on the BLAS
// ("MFMA only for the dense matmuls where it is a true contraction").  Here:
//
//   * rows are AUGMENTED so that one dgemm yields the kernel ARGUMENT of the distance kernels, not just the inner product:
//         left form  [v, -|v|^2/2, 1],  right form [v, 1, -|v|^2/2]:   <left(z), right(x)> = <z, x> - |z|^2/2 - |x|^2/2 = -|z - x|^2 / 2 =: a
//     (kernels.py:765-776 forms the same three terms); RBF (:862-864) is exp(a), the Matern families (:955-993) functions of r = sqrt(max(-2a, 1e-40));
//     the reverse pass needs no norm bookkeeping either: the adjoint of a times the augmented rows IS the chain rule through the norms;
//   * ONE kernel then maps arguments to kappa, takes the increments' difference (kernels.py:329-330), the time difference
//     (signature_algs.py:114) and sweeps the chains of signature_algs.py:118-125 -- the argument array (rows = (sequence, time), columns =
//     (component, endpoint, tensor), tensors fastest: a wavefront reads 512 contiguous bytes per component and step) is read once, nothing else
//     of the (lt, T, N, L) tensor ever exists;
//   * the reverse kernel undoes the chains from their totals (as tvs_grad_tile_kernel.hpp does) and writes the adjoint of the argument array, which
//     two more dgemms contract with the augmented rows of the other side.
// Lane = inducing tensor; levels one after the other (level i owns components i(i-1)/2 .. i(i-1)/2 + i - 1, so every column is read by one level).
#pragma once

#include <hip/hip_runtime.h>

#include "seq_core.hpp"
#include "grad_wave_core.hpp"
#include "fast_exp.hpp"

// The kernels that are no templates have ONE definition with external linkage, in wide_api.hip.  A second unit that includes this file for the kernel
// templates (wide_ragged_api.hip: their ragged forms) defines GPSIG_WIDE_GLOBAL as `template <int UNIT = 0> __global__` before it does: there they are
// templates too -- the two it launches (as `name<>`) are instantiated as copies of its own, the others are never emitted.
#ifndef GPSIG_WIDE_GLOBAL
#define GPSIG_WIDE_GLOBAL __global__
#endif

namespace gpsig {

constexpr int WIDE_MAX_LEVELS = 8;
constexpr int WIDE_MAX_ORDER = 4;       // higher-order chains: repeat counts kept per component inside a time step

struct WideTvsArgs {
    const double* arg;      // (Nc * L, CW): row (n - n0) * L + tau, column (k * E + e) * Tpad + t
    int64_t CW, Tpad, Tn;
    int64_t n0, Nc, N;      // this launch: sequences n0 .. n0 + Nc - 1 of N
    int32_t L, M, kind, difference, sum_levels;
    const double* fx;       // (N, M+1) per-sequence factors or NULL
    const double* w;        // (M+1) level weights or NULL
    double* out;            // forward: (T, N) level sum or (M+1, T, N)
    double* aux;            // (N, lt, Tpad) chain totals: written by the forward kernel, read by the reverse kernel; NULL: neither
    const double* G;        // reverse: upstream gradient, (T, N) of the weighted sum (weighted = 1) or (M+1, T, N) of the levels
    double* W;              // reverse: adjoint of arg, same shape
    double* gfac_part;      // reverse, weighted: (TB, N, M+1) partial sums of dL/dfac over the tensors of a block, or NULL
    int32_t weighted;
    int32_t order;          // > 1: the higher-order chains of signature_algs.py:129-160 (at most WIDE_MAX_ORDER)
    double kp0, kp1;        // SignaturePoly: offset and degree (WIDE_KD_POLY)
    double* gb_part;        // reverse, SignaturePoly: (TB, N, M) partial sums of W over the tensors of a block -- the offset's gradient --, or NULL
                            // (SignatureMix: the mixing's gradient, same slots)
    // SignatureMix (WIDE_KD_MIX): kappa = psi(a) + q (hx[row] + hz[column]) with psi(a) = p0 exp(a) + q a, q = 1 - p0 and the half norms h = |v|^2 / 2.  A side's
    // term cancels under a difference taken along the other side (the rows' under increments, the columns' under the time difference): NULL.  The half
    // norms are read NEGATED from the augmented rows' own norm column (stride nrm_ld = d + 2 doubles).
    const double* nrm_row;  // row (n L + tau) of ALL sequences at nrm_row[(n L + tau) * nrm_ld], or NULL
    const double* nrm_col;  // column c at nrm_col[c * nrm_ld], or NULL
    int64_t nrm_ld;
    double* radj_part;      // reverse, rows' term kept: (TB * M, N L) sums of the values' adjoints over the tensors of a block and the components of a level
    double* cadj_part;      // reverse, columns' term kept: (N, CW) sums of the values' adjoints over a sequence's rows
};

// The base kernel as a function of the argument a = -|z - x|^2 / 2, described by wavefront-uniform numbers so that the three Matern families share
// one instruction stream:  kappa = P(r') exp(-r'),  r' = c r,  P = 1 + a1 r' + a2 r'^2  (kernels.py:955-993: (c, a1, a2) = (1, 0, 0), (sqrt 3, 1, 0),
// (sqrt 5, 1, 1/3)); RBF (:862-864) is exp(a) (compile-time: no square root, no polynomial).  exp through the 64-entry table of fast_exp.hpp in LDS
// (13 instructions, <= 1.3 ulp) instead of the library routine (~50 with its special cases -- the first form of these kernels spent 10x the
// instructions of the recursion on them).
// Matern-1/2 is not differentiable at coinciding points, and the squared distance of two EQUAL rows out of a dgemm is rounding noise (~1e-16 |x|^2)
// instead of the exact zero the exact-shape kernels get from coordinate differences: such distances count as zero (the clamp of kernels.py:781 then
// gives kappa = 1 and passes no gradient, as it does there; the reference's own float64 value at such a pair is 1e-8 from one -- DESIGN section 5).
constexpr double WIDE_M12_COINCIDE = 1e-13;

struct WideKap {
    const double* tab;      // 2^(j/64) in LDS
    double c2, a1, a2, thr;
    double p0;              // SignaturePoly: the offset ...
    int pn;                 // ... and the whole degree, 1 .. 8
    double q;               // SignatureMix: 1 - p0 (p0: the mixing)
};

__device__ __forceinline__ WideKap wide_kap(int kind, const double* tab, double p0 = 0.0, double p1 = 0.0) {
    WideKap K;
    K.tab = tab;
    K.p0 = p0;
    K.pn = int(p1);
    K.q = 1.0 - p0;
    K.c2 = kind == BASE_MATERN32 ? 3.0 : (kind == BASE_MATERN52 ? 5.0 : 1.0);
    K.a1 = kind == BASE_MATERN12 ? 0.0 : 1.0;
    K.a2 = kind == BASE_MATERN52 ? 1.0 / 3.0 : 0.0;
    K.thr = kind == BASE_MATERN12 ? WIDE_M12_COINCIDE : 1e-40;
    return K;
}

// The compile-time kind of a kernel instance.  WIDE_KD_ID: kappa(a) = a -- the dot-product families: SignatureLinear (kernels.py:798-808: rows are the
// points or, with differences, their increments -- <.,.> is bilinear, so the differences are taken on the rows before the dgemm and the kernels run in
// their difference = 0 form) and SignatureCosine (:820-828: unit rows, differences of kappa as for the distance kernels).  No exponential: these
// instances neither fill nor read the table in LDS.
// WIDE_KD_POLY: SignaturePoly (kernels.py:844-848), kappa(a) = (a + p0)^p1 on plain rows (a = <z, x>) with a whole degree 1 .. 8; non-linear, so the
// differences are taken on kappa as for the distance kernels.  d kappa / d p0 = d kappa / d a at every entry: the offset's gradient is the plain sum of
// the adjoint array W that the reverse kernels write (their poly instances sum what they store: per lane, per wavefront, one partial per fixed slot, and
// wide_sum_kernel adds the slots in a fixed order -- no atomics, the same bits from every call; across chunkings of the argument array too for Kzx,
// whose host side keeps the dgemms' shapes fixed, not for the lattices).  No table either.
// WIDE_KD_MIX: SignatureMix (kernels.py:881-892), kappa = p0 exp(-|z - x|^2 / 2) + (1 - p0) <z, x> on the distance kernels' augmented rows.  With a the
// dgemm's number and h the half norms, <z, x> = a + hz + hx, so kappa = psi(a) + q (hz + hx), psi(a) = p0 exp(a) + q a: wide_kappa is psi, the one-sided
// terms are added by the kernels where they survive the differences (the args' nrm_* vectors; NULL where they cancel).  d kappa / d p0 = exp(a) - a - hz - hx:
// the reverse kernels sum it times the value's adjoint into poly's gb_part slots.  d kappa / d hz = q: where a side's term survives, the sums of the values'
// adjoints over the other side go back through the un-augmentation (adj vectors there).
constexpr int WIDE_KD_MATERN = 0, WIDE_KD_RBF = 1, WIDE_KD_ID = 2, WIDE_KD_POLY = 3, WIDE_KD_MIX = 4;

// b^n for a wavefront-uniform whole n in 0 .. 8, by repeated squaring (seq_core.hpp: poly_pow without its way out to the library's pow)
__device__ __forceinline__ double wide_pow_n(double b, int n) {
    double r = (n & 1) ? b : 1.0, x = b * b;
    if (n & 2) r *= x;
    x *= x;
    if (n & 4) r *= x;
    if (n & 8) r *= x * x;
    return r;
}

// the exp table of a workgroup of n threads (nothing for the identity and the polynomial kind)
template <int KD>
__device__ __forceinline__ const double* wide_tab(double* etab, int tid, int n) {
    if constexpr (KD == WIDE_KD_ID || KD == WIDE_KD_POLY) {
        return nullptr;
    } else {
        exp_tab_fill(etab, tid, n);
        __syncthreads();
        return etab;
    }
}

template <int KD>
__device__ __forceinline__ double wide_kappa(const WideKap& K, double a) {
    if constexpr (KD == WIDE_KD_ID) {
        return a;
    } else if constexpr (KD == WIDE_KD_POLY) {
        return wide_pow_n(a + K.p0, K.pn);
    } else if constexpr (KD == WIDE_KD_RBF) {
        return kexp_tab(a, K.tab);
    } else if constexpr (KD == WIDE_KD_MIX) {
        return fma(K.p0, kexp_tab(a, K.tab), K.q * a);
    } else {
        double dist = -2.0 * a;
        dist = dist > K.thr ? dist : 0.0;
        const double rp = sqrt(fmax(dist, 1e-40) * K.c2);              // c * sqrt(max(r^2, 1e-40)): kernels.py:779-781
        return fma(fma(K.a2, rp, K.a1), rp, 1.0) * kexp_tab(-rp, K.tab);
    }
}

// kappa and d kappa / d a  (a = -dist / 2: d/da = -2 d/ddist; r' = c sqrt(-2a): dr'/da = -c^2 / r'; the clamp of kernels.py:781 passes no gradient, as
// grad_core.hpp: base_eval_grad)
template <int KD>
__device__ __forceinline__ void wide_kappa_grad(const WideKap& K, double a, double& k, double& dk) {
    if constexpr (KD == WIDE_KD_ID) {
        k = a;
        dk = 1.0;
    } else if constexpr (KD == WIDE_KD_POLY) {
        const double b = a + K.p0, q = wide_pow_n(b, K.pn - 1);
        k = b * q;
        dk = double(K.pn) * q;
    } else if constexpr (KD == WIDE_KD_RBF) {
        k = kexp_tab(a, K.tab);
        dk = k;
    } else if constexpr (KD == WIDE_KD_MIX) {
        const double e = kexp_tab(a, K.tab);
        k = fma(K.p0, e, K.q * a);
        dk = fma(K.p0, e, K.q);
    } else {
        double dist = -2.0 * a;
        dist = dist > K.thr ? dist : 0.0;
        const bool clamped = !(dist > 1e-40);
        const double rp = sqrt(fmax(dist, 1e-40) * K.c2);
        const double e = kexp_tab(-rp, K.tab);
        const double P = fma(fma(K.a2, rp, K.a1), rp, 1.0), dP = fma(2.0 * K.a2, rp, K.a1);
        k = P * e;
        dk = clamped ? 0.0 : (K.c2 / rp) * (P - dP) * e;
    }
}

// SignatureMix: psi, psi' and d psi / d p0 = exp(a) - a
__device__ __forceinline__ void wide_mix_grad(const WideKap& K, double a, double& k, double& dk, double& dp) {
    const double e = kexp_tab(a, K.tab);
    k = fma(K.p0, e, K.q * a);
    dk = fma(K.p0, e, K.q);
    dp = e - a;
}

// SignatureMix in the Kzx chain kernels: where the one-sided terms of a (lane, sequence, level) are read and where its adjoint sums go (all NULL / unused
// for the other kinds: their instances compile to what they were)
struct WideMixCtx {
    const double* nrow;     // the sequence's rows: negated half norm of row tau at nrow[tau * ld] (wavefront-uniform), or NULL
    const double* ncol;     // the lane's columns: component k, endpoint e at ncol[(k * E + e) * cs], or NULL
    int64_t ld, cs;
    double* radj;           // reverse: the slot of (tensor block, level, row tau) at radj[tau], or NULL
    double* cadj;           // reverse: the slot of (sequence, component k, endpoint e, this lane's tensor) at cadj[(k * E + e) * Tpad], or NULL
};

// the raw arguments of I components at one argument row (r points at the lane's column 0 of that row): all loads first, so that they are in flight together
template <int I, int E>
__device__ __forceinline__ void wide_load_row(const double* __restrict__ r, int k0, int64_t Tpad, double (&raw)[I * E]) {
#pragma unroll
    for (int q = 0; q < I * E; ++q) raw[q] = r[(int64_t(k0) * E + q) * Tpad];
}
// the value of component j from them: kappa, or the difference of its two points' (kernels.py:330)
template <int I, int E, int KD>
__device__ __forceinline__ double wide_val(const double (&raw)[I * E], int j, const WideKap& K) {
    if constexpr (E == 2) return wide_kappa<KD>(K, raw[2 * j + 1]) - wide_kappa<KD>(K, raw[2 * j]);
    else return wide_kappa<KD>(K, raw[j]);
}

// the chains of ONE level (I components from k0) of one (tensor, sequence) pair: signature_algs.py:118-125 as one sweep; the arguments of the next
// step are requested before the current step is evaluated
// One time step of the HIGHER-ORDER chains of a level (signature_algs.py:147-158): with U_j the running totals (what first order keeps),
//   r_0 = [m_0],   r_j[0] = m_j U_{j-1},   r_j[l] = m_j r_{j-1}[l-1] / (l+1)  (l < min(j+1, order): the SAME time step),   U_j += sum_l r_j[l].
template <int I>
__device__ __forceinline__ void wide_ho_step(const double (&dk)[I], int order, double (&u)[I]) {
    constexpr int O = WIDE_MAX_ORDER;
    double rp[O], uold = u[0];
    rp[0] = dk[0];
    u[0] += dk[0];
#pragma unroll
    for (int j = 1; j < I; ++j) {
        double rc[O], tot = dk[j] * uold;
        rc[0] = tot;
#pragma unroll
        for (int l = 1; l < O; ++l) {
            rc[l] = (l <= j && l < order) ? (dk[j] * (1.0 / double(l + 1))) * rp[l - 1] : 0.0;
            tot += rc[l];
        }
        uold = u[j];
        u[j] += tot;
#pragma unroll
        for (int l = 0; l < O; ++l) rp[l] = rc[l];
    }
}

template <int I, int E, int KD>
__device__ __forceinline__ void wide_chain_fwd(const double* __restrict__ col, int64_t CW, int64_t Tpad, int k0, int L, int difference, int order, const WideKap& K,
                                               double (&u)[I], const WideMixCtx& X) {
#pragma unroll
    for (int j = 0; j < I; ++j) u[j] = 0.0;
    double prev[I], cur[I * E];
    const double* r = col;
    int steps = L;
    // SignatureMix: the columns' half norms (an increment's: of its two points, subtracted) are lane-constant for the whole sweep, a row's is
    // wavefront-uniform; value = psi + q (columns' + row's)
    double hcm[I];
    auto mixed = [&](int j, int tau, double v) -> double {
        if constexpr (KD == WIDE_KD_MIX) {
            const double hr = X.nrow ? -X.nrow[tau * X.ld] : 0.0;
            return fma(K.q, hcm[j] + hr, v);
        } else {
            return v;
        }
    };
    if constexpr (KD == WIDE_KD_MIX) {
#pragma unroll
        for (int j = 0; j < I; ++j) {
            hcm[j] = 0.0;
            if (X.ncol) hcm[j] = E == 2 ? X.ncol[((k0 + j) * 2) * X.cs] - X.ncol[((k0 + j) * 2 + 1) * X.cs] : -X.ncol[(k0 + j) * X.cs];
        }
    }
    wide_load_row<I, E>(r, k0, Tpad, cur);
    if (difference) {                                                              // signature_algs.py:114
#pragma unroll
        for (int j = 0; j < I; ++j) prev[j] = mixed(j, 0, wide_val<I, E, KD>(cur, j, K));
        r += CW;
        steps = L - 1;
        if (steps > 0) wide_load_row<I, E>(r, k0, Tpad, cur);
    }
    for (int s = 0; s < steps; ++s) {
        double nxt[I * E];
        r += CW;
        if (s + 1 < steps) wide_load_row<I, E>(r, k0, Tpad, nxt);
        double dk[I];
#pragma unroll
        for (int j = 0; j < I; ++j) {
            const double v = mixed(j, difference ? s + 1 : s, wide_val<I, E, KD>(cur, j, K));
            dk[j] = difference ? v - prev[j] : v;
            prev[j] = v;
        }
        if (I > 1 && order > 1) {
            wide_ho_step<I>(dk, order, u);
        } else {
#pragma unroll
            for (int j = I - 1; j >= 1; --j) u[j] = fma(dk[j], u[j - 1], u[j]);      // :120-124 (old values below)
            u[0] += dk[0];
        }
#pragma unroll
        for (int q = 0; q < I * E; ++q) cur[q] = nxt[q];
    }
}

// (L: the rows of this sequence -- A.L, or its own length in a ragged launch)
template <int E, int KD>
__device__ __forceinline__ void wide_level_fwd(int i, const double* col, const WideTvsArgs& A, int L, const WideKap& K, double* u /* [i] */, const WideMixCtx& X) {
    const int k0 = i * (i - 1) / 2;
#define GPSIG_WIDE_CASE(I_)                                                                          \
    case I_: {                                                                                       \
        double v[I_];                                                                                \
        wide_chain_fwd<I_, E, KD>(col, A.CW, A.Tpad, k0, L, A.difference, A.order, K, v, X);                 \
        _Pragma("unroll") for (int j = 0; j < I_; ++j) u[j] = v[j];                                 \
    } break;
    switch (i) {
        GPSIG_WIDE_CASE(1) GPSIG_WIDE_CASE(2) GPSIG_WIDE_CASE(3) GPSIG_WIDE_CASE(4)
        GPSIG_WIDE_CASE(5) GPSIG_WIDE_CASE(6) GPSIG_WIDE_CASE(7) GPSIG_WIDE_CASE(8)
        default: break;
    }
#undef GPSIG_WIDE_CASE
}

// SignatureMix: the one-sided terms of (sequence n, tensor t) (the reverse kernel adds its slots)
template <int KD>
__device__ __forceinline__ WideMixCtx wide_mix_ctx(const WideTvsArgs& A, int64_t n, int64_t t) {
    WideMixCtx X;
    X.nrow = X.ncol = nullptr;
    X.radj = X.cadj = nullptr;
    X.ld = X.cs = 0;
    if constexpr (KD == WIDE_KD_MIX) {
        X.ld = A.nrm_ld;
        X.cs = A.Tpad * A.nrm_ld;
        if (A.nrm_row) X.nrow = A.nrm_row + n * int64_t(A.L) * A.nrm_ld;
        if (A.nrm_col) X.ncol = A.nrm_col + t * A.nrm_ld;
    }
    return X;
}

// grid: (Tpad / 64, sequences of the chunk (grid-stride), levels); block: one wavefront, lane = tensor.  A launch of few sequences is bound by the
// serial sweep of one chain: the levels of a (tensor, sequence) pair go to different workgroups (blockIdx.z + 1 = level), each leaving its chain totals
// in aux (N, lt, Tpad) -- tensors fastest --, and wide_tvs_epilogue_kernel forms the outputs from them.
// RG (ragged batches, wide_ragged_api.hip: wide_tvs_fwd_ragged_kernel): the argument array holds the sequences' own rows back to back -- sequence n has
// len[n] of them from row off[n] - off[n0] of the chunk --, and its chains take len[n] steps.  The totals land in aux as in the dense form: the epilogue is
// the same kernel.  The two kernels are one body; the dense one compiles to what it was.
struct WideTvsRaggedArgs : WideTvsArgs {
    const int32_t* len;     // (N) rows per sequence, >= 1
    const int64_t* off;     // (N + 1) their prefix sums
};

template <int E, int KD>
__global__ void __launch_bounds__(64) wide_tvs_fwd_kernel(const WideTvsArgs A) {
#define GPSIG_WIDE_RG 0
#include "wide_tvs_fwd_body.inc"
#undef GPSIG_WIDE_RG
}
template <int E, int KD>
__global__ void __launch_bounds__(64) wide_tvs_fwd_ragged_kernel(const WideTvsRaggedArgs A) {
#define GPSIG_WIDE_RG 1
#include "wide_tvs_fwd_body.inc"
#undef GPSIG_WIDE_RG
}

// out[t][n] = fac_0 + sum_i fac_i K_i  or  out[i][t][n] = fac_i K_i  (fac = fx[n][i] * w[i]: kernels.py:572-588), K_i = the total of level i's last chain
// (signature_algs.py:125).  One thread per (t, n) of the chunk, tensors fastest.
GPSIG_WIDE_GLOBAL void wide_tvs_epilogue_kernel(const WideTvsArgs A) {
    const int M = A.M, lt = M * (M + 1) / 2;
    const int64_t total = A.Nc * A.Tn;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * blockDim.x) {
        const int64_t t = idx % A.Tn, n = A.n0 + idx / A.Tn;
        double acc = 0.0;
        for (int i = 0; i <= M; ++i) {
            double f = A.fx ? A.fx[n * (M + 1) + i] : 1.0;
            if (A.w) f *= A.w[i];
            const double lev = i == 0 ? 1.0 : A.aux[(n * lt + i * (i - 1) / 2 + i - 1) * A.Tpad + t];       // signature_algs.py:116 / :125
            if (A.sum_levels) acc = fma(lev, f, acc);
            else A.out[(int64_t(i) * A.Tn + t) * A.N + n] = lev * f;
        }
        if (A.sum_levels) A.out[t * A.N + n] = acc;
    }
}

__device__ __forceinline__ double wide_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- reverse pass ------------------------------------------------------------------------------------------------------------------
// With u_j the chain values BEFORE a step and W_j = dL/du_j after it:  dL/dm_j = u_{j-1} W_j,  W_{j-1} += m_j W_j,  and the chain is undone
// by u_j <- u_j - m_j u_{j-1} (tvs_grad_tile_kernel.hpp, grad_ho_kernels.hpp: chain_levels_grad_kernel).  m_j[tau] = v_j[tau + 1] - v_j[tau]
// (signature_algs.py:114), so the adjoint of the VALUE row rho is g[rho - 1] - g[rho]; times d kappa / d a of each endpoint it is the adjoint of the
// argument.  u: the level's totals (destroyed).  c: the level's upstream gradient.  Columns of tensors beyond Tn get zeros (valid = false).
template <int I, int E, int KD>
__device__ __forceinline__ void wide_chain_bwd(const double* __restrict__ col, double* __restrict__ wcol, int64_t CW, int64_t Tpad, int k0, int L,
                                               int difference, int order, const WideKap& K, double (&u)[I], double c, bool valid, double& wsum,
                                               const WideMixCtx& X) {
    double wv[I];
#pragma unroll
    for (int j = 0; j < I; ++j) wv[j] = 0.0;
    // SignatureMix: hc = the half norms of the lane's columns where their term survives (else 0), csum = the lane's sums of the values' adjoints over the
    // rows, per component.  dp (the other kinds leave it alone) = d value / d p0 of an entry, with the entry's sign in the value: exp(a) - a - hz - hx
    double hc[I][E], csum[I];
    if constexpr (KD == WIDE_KD_MIX) {
#pragma unroll
        for (int j = 0; j < I; ++j) {
            csum[j] = 0.0;
#pragma unroll
            for (int e = 0; e < E; ++e) hc[j][e] = X.ncol ? -X.ncol[((k0 + j) * E + e) * X.cs] : 0.0;
        }
    }
    auto eval = [&](const double (&raw)[I * E], int tau, double (&v)[I], double (&d)[I][E], double (&dp)[I][E]) {
        if constexpr (KD == WIDE_KD_MIX) {
            const double hr = X.nrow ? -X.nrow[tau * X.ld] : 0.0;          // (wavefront-uniform; NULL with increments, where it cancels between the endpoints)
#pragma unroll
            for (int j = 0; j < I; ++j) {
                if constexpr (E == 2) {
                    double k1, d1, p1, k0v, d0, p0v;
                    wide_mix_grad(K, raw[2 * j + 1], k1, d1, p1);
                    wide_mix_grad(K, raw[2 * j], k0v, d0, p0v);
                    v[j] = fma(K.q, hc[j][1] - hc[j][0], k1 - k0v); d[j][1] = d1; d[j][0] = -d0;
                    dp[j][1] = p1 - hc[j][1]; dp[j][0] = hc[j][0] - p0v;
                } else {
                    double kk, pp;
                    wide_mix_grad(K, raw[j], kk, d[j][0], pp);
                    v[j] = fma(K.q, hc[j][0] + hr, kk);
                    dp[j][0] = pp - hc[j][0] - hr;
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < I; ++j) {
            if constexpr (E == 2) {
                double k1, d1, k0v, d0;
                wide_kappa_grad<KD>(K, raw[2 * j + 1], k1, d1);
                wide_kappa_grad<KD>(K, raw[2 * j], k0v, d0);
                v[j] = k1 - k0v; d[j][1] = d1; d[j][0] = -d0;
            } else {
                wide_kappa_grad<KD>(K, raw[j], v[j], d[j][0]);
            }
        }
    };
    auto store = [&](double* __restrict__ wr, int tau, const double (&g)[I], const double (&d)[I][E], const double (&dp)[I][E]) {
#pragma unroll
        for (int j = 0; j < I; ++j)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double w = valid ? g[j] * d[j][e] : 0.0;
                wr[((k0 + j) * E + e) * Tpad] = w;
                if constexpr (KD == WIDE_KD_POLY) wsum += w;               // (a padded lane stores and adds exactly zero)
                if constexpr (KD == WIDE_KD_MIX) wsum += valid ? g[j] * dp[j][e] : 0.0;
            }
        if constexpr (KD == WIDE_KD_MIX) {
            // g[j] IS the adjoint of the value of (row tau, component j): its sum over the level's components and the block's tensors to the row's slot,
            // its sum over the rows stays in the lane
            if (X.radj) {
                double sr = 0.0;
#pragma unroll
                for (int j = 0; j < I; ++j) sr += valid ? g[j] : 0.0;
                sr = wide_wave_sum(sr);
                if (threadIdx.x == 0) X.radj[tau] = sr;
            }
            if (X.cadj) {
#pragma unroll
                for (int j = 0; j < I; ++j) csum[j] += valid ? g[j] : 0.0;
            }
        }
    };
    // higher-order chains: the step's repeat-count vectors are rebuilt from the totals BEFORE the step (U_j - sum_l r_j[l], ascending in j), then the
    // adjoints run down: dL/dr_j[l] = W_j + m_{j+1} / (l+2) dL/dr_{j+1}[l+1],  dL/dm_j = dL/dr_j[0] U_{j-1} + sum_{l>=1} dL/dr_j[l] r_{j-1}[l-1] / (l+1),
    // W_{j-1} += m_j dL/dr_j[0]   (W_j = dL/dU_j after the step; first order: one repeat count)
    auto undo_ho = [&](const double (&dk)[I], double (&g)[I]) {
        constexpr int O = WIDE_MAX_ORDER;
        double r[I][O], ub[I];
        ub[0] = u[0] - dk[0];
#pragma unroll
        for (int l = 0; l < O; ++l) r[0][l] = l == 0 ? dk[0] : 0.0;
#pragma unroll
        for (int j = 1; j < I; ++j) {
            double tot = dk[j] * ub[j - 1];
            r[j][0] = tot;
#pragma unroll
            for (int l = 1; l < O; ++l) {
                r[j][l] = (l <= j && l < order) ? (dk[j] * (1.0 / double(l + 1))) * r[j - 1][l - 1] : 0.0;
                tot += r[j][l];
            }
            ub[j] = u[j] - tot;
        }
        double gn[O], add[I];                             // dL/dr_{j+1}[.];  m_j dL/dr_j[0], added to W_{j-1} once the step's adjoints are through
#pragma unroll
        for (int l = 0; l < O; ++l) gn[l] = 0.0;
#pragma unroll
        for (int j = I - 1; j >= 0; --j) {
            const double wj = (j == I - 1) ? c : wv[j + 1 < I ? j + 1 : j];
            double gr[O];
#pragma unroll
            for (int l = 0; l < O; ++l) {
                const bool live = l <= j && l < order;
                const bool up = j + 1 < I && l + 1 < O && l + 1 <= j + 1 && l + 1 < order;
                gr[l] = live ? wj + (up ? (dk[j + 1 < I ? j + 1 : j] * (1.0 / double(l + 2))) * gn[l + 1 < O ? l + 1 : l] : 0.0) : 0.0;
            }
            double gd = gr[0] * (j >= 1 ? ub[j >= 1 ? j - 1 : 0] : 1.0);
#pragma unroll
            for (int l = 1; l < O; ++l)
                if (j >= 1) gd = fma(gr[l] * (1.0 / double(l + 1)), r[j >= 1 ? j - 1 : 0][l - 1], gd);
            g[j] = gd;
            add[j] = dk[j] * gr[0];
#pragma unroll
            for (int l = 0; l < O; ++l) gn[l] = gr[l];
        }
#pragma unroll
        for (int j = 1; j < I; ++j) wv[j] += add[j];
#pragma unroll
        for (int j = 0; j < I; ++j) u[j] = ub[j];
    };
    auto undo1 = [&](const double (&dk)[I], double (&g)[I]) {
        double below = 1.0;
#pragma unroll
        for (int j = 0; j < I; ++j) {
            const double wnext = (j == I - 1) ? c : wv[j + 1 < I ? j + 1 : j];
            g[j] = below * wnext;
            u[j] = fma(-dk[j], below, u[j]);
            below = u[j];
            if (j >= 1) wv[j] = fma(dk[j], wnext, wv[j]);
        }
    };
    auto undo = [&](const double (&dk)[I], double (&g)[I]) {
        if (I > 1 && order > 1) undo_ho(dk, g);
        else undo1(dk, g);
    };
    // (the arguments of the row after next are requested before a row is evaluated: all its loads in flight together)
    const double* r = col + int64_t(L - 1) * CW;
    double* wr = wcol + int64_t(L - 1) * CW;
    double raw[I * E], rnx[I * E];
    wide_load_row<I, E>(r, k0, Tpad, raw);
    if (difference) {
        double nv[I], nd[I][E], ndp[I][E], gprev[I];
        eval(raw, L - 1, nv, nd, ndp);
#pragma unroll
        for (int j = 0; j < I; ++j) gprev[j] = 0.0;
        if (L >= 2) wide_load_row<I, E>(r - CW, k0, Tpad, raw);
        for (int s = L - 2; s >= 0; --s) {
            r -= CW;
            if (s >= 1) wide_load_row<I, E>(r - CW, k0, Tpad, rnx);
            double cv[I], cd[I][E], cdp[I][E], dk[I], g[I], gv[I];
            eval(raw, s, cv, cd, cdp);
#pragma unroll
            for (int j = 0; j < I; ++j) dk[j] = nv[j] - cv[j];
            undo(dk, g);
#pragma unroll
            for (int j = 0; j < I; ++j) gv[j] = g[j] - gprev[j];
            store(wr, s + 1, gv, nd, ndp);                                             // row s + 1 is final
            wr -= CW;
#pragma unroll
            for (int j = 0; j < I; ++j) {
                gprev[j] = g[j]; nv[j] = cv[j];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    nd[j][e] = cd[j][e];
                    if constexpr (KD == WIDE_KD_MIX) ndp[j][e] = cdp[j][e];
                }
            }
#pragma unroll
            for (int q = 0; q < I * E; ++q) raw[q] = rnx[q];
        }
        double gv[I];
#pragma unroll
        for (int j = 0; j < I; ++j) gv[j] = -gprev[j];
        store(wr, 0, gv, nd, ndp);                                                     // row 0
    } else {
        for (int s = L - 1; s >= 0; --s, r -= CW, wr -= CW) {
            if (s >= 1) wide_load_row<I, E>(r - CW, k0, Tpad, rnx);
            double cv[I], cd[I][E], cdp[I][E], g[I];
            eval(raw, s, cv, cd, cdp);
            undo(cv, g);
            store(wr, s, g, cd, cdp);
#pragma unroll
            for (int q = 0; q < I * E; ++q) raw[q] = rnx[q];
        }
    }
    if constexpr (KD == WIDE_KD_MIX) {
        if (X.cadj) {          // (an increment's value is its second point's minus its first's)
#pragma unroll
            for (int j = 0; j < I; ++j)
#pragma unroll
                for (int e = 0; e < E; ++e) X.cadj[((k0 + j) * E + e) * Tpad] = (E == 2 && e == 0) ? -csum[j] : csum[j];
        }
    }
}

template <int E, int KD>
__global__ void __launch_bounds__(64) wide_tvs_bwd_kernel(const WideTvsArgs A) {
    __shared__ double etab[EXP_TAB_N];
    const WideKap K = wide_kap(A.kind, wide_tab<KD>(etab, threadIdx.x, 64), A.kp0, A.kp1);
    const int64_t t = int64_t(blockIdx.x) * 64 + threadIdx.x;
    const bool valid = t < A.Tn;
    const int M = A.M, lt = M * (M + 1) / 2;
    const int i = blockIdx.z + 1, k0 = i * (i - 1) / 2;          // one level per workgroup (as the forward kernel)
    for (int64_t nl = blockIdx.y; nl < A.Nc; nl += gridDim.y) {
        const int64_t n = A.n0 + nl;
        const double* col = A.arg + nl * int64_t(A.L) * A.CW + t;
        double* wcol = A.W + nl * int64_t(A.L) * A.CW + t;
        const double gsum = (A.weighted && valid) ? A.G[t * A.N + n] : 0.0;
        WideMixCtx X = wide_mix_ctx<KD>(A, n, t);
        if constexpr (KD == WIDE_KD_MIX) {          // the slots of (tensor block, level, GLOBAL row) and of (GLOBAL sequence, column): the same partials in every chunking
            if (A.radj_part) X.radj = A.radj_part + (int64_t(blockIdx.x) * M + (i - 1)) * (A.N * int64_t(A.L)) + n * int64_t(A.L);
            if (A.cadj_part) X.cadj = A.cadj_part + n * A.CW + t;
        }
        if (A.gfac_part && i == 1) {                                                   // level 0 == 1: dL/dfac[n][0] = sum_t G[t][n]
            const double s = wide_wave_sum(gsum);
            if (threadIdx.x == 0) A.gfac_part[(int64_t(blockIdx.x) * A.N + n) * (M + 1)] = s;
        }
        double f = A.fx ? A.fx[n * (M + 1) + i] : 1.0;
        if (A.w) f *= A.w[i];
        const double c = A.weighted ? gsum * f : (valid ? A.G[(int64_t(i) * A.Tn + t) * A.N + n] * f : 0.0);
        double u[WIDE_MAX_LEVELS];
        if (A.aux) {
            for (int j = 0; j < i; ++j) u[j] = A.aux[(n * lt + k0 + j) * A.Tpad + t];
        } else {
            wide_level_fwd<E, KD>(i, col, A, A.L, K, u, X);
        }
        if (A.gfac_part) {
            double ui = 0.0;
#pragma unroll
            for (int j = 0; j < WIDE_MAX_LEVELS; ++j)
                if (j == i - 1) ui = u[j];
            const double s = wide_wave_sum(gsum * ui);
            if (threadIdx.x == 0) A.gfac_part[(int64_t(blockIdx.x) * A.N + n) * (M + 1) + i] = s;
        }
        double wsum = 0.0;          // SignaturePoly: this lane's sum of the W entries of (tensor t, sequence n, level i)
#define GPSIG_WIDE_CASE(I_)                                                                                  \
    case I_: {                                                                                               \
        double v[I_];                                                                                        \
        _Pragma("unroll") for (int j = 0; j < I_; ++j) v[j] = u[j];                                         \
        wide_chain_bwd<I_, E, KD>(col, wcol, A.CW, A.Tpad, k0, A.L, A.difference, A.order, K, v, c, valid, wsum, X); \
    } break;
        switch (i) {
            GPSIG_WIDE_CASE(1) GPSIG_WIDE_CASE(2) GPSIG_WIDE_CASE(3) GPSIG_WIDE_CASE(4)
            GPSIG_WIDE_CASE(5) GPSIG_WIDE_CASE(6) GPSIG_WIDE_CASE(7) GPSIG_WIDE_CASE(8)
            default: break;
        }
#undef GPSIG_WIDE_CASE
        if constexpr (KD == WIDE_KD_POLY || KD == WIDE_KD_MIX) {
            if (A.gb_part) {            // the slot of (tensor block, GLOBAL sequence, level): the same partial however the sequences are chunked
                const double s = wide_wave_sum(wsum);
                if (threadIdx.x == 0) A.gb_part[(int64_t(blockIdx.x) * A.N + n) * M + (i - 1)] = s;
            }
        }
    }
}

// out[b] (+)= the sum of part[0 .. n) taken by block b of gridDim.x blocks of 256 threads: a thread adds its entries in ascending order, the block's 256
// sums meet in a fixed tree.  Two launches -- (blocks, part -> tmp), (1, tmp -> g_base[0], add = 1) -- sum the offset's partials in an order that
// depends on n alone (SignaturePoly's reverse passes).
GPSIG_WIDE_GLOBAL void __launch_bounds__(256) wide_sum_kernel(const double* __restrict__ part, int64_t n, int add, double* __restrict__ out) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int64_t idx = blockIdx.x * int64_t(256) + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * 256) s += part[idx];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (int(threadIdx.x) < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = add ? out[blockIdx.x] + sh[0] : sh[0];
}

// gfac[n][m] = sum over the tensor blocks of the partial sums (a fixed order: the result does not depend on the schedule)
GPSIG_WIDE_GLOBAL void wide_gfac_reduce_kernel(const double* __restrict__ part, int TB, int64_t NM, double* __restrict__ gfac) {
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < NM; idx += int64_t(gridDim.x) * blockDim.x) {
        double s = 0.0;
        for (int b = 0; b < TB; ++b) s += part[int64_t(b) * NM + idx];
        gfac[idx] = s;
    }
}

// ---- augmented rows ------------------------------------------------------------------------------------------------------------------
// dst row r (DA = d + 2 columns): the d values of the source row, then (-|v|^2/2, 1) [left form] or (1, -|v|^2/2) [right form].
// Tensor rows are reordered on the way: dst row (k * E + e) * Tpad + t  <-  src row (k * Tn + t) * E + e (the caller's (lt, T, E, d) array), scaled by
// lengthscales / lag weights where P.has_ls (kernels.py:367-398); rows of tensors beyond Tn are zero.  lt == 0: rows as they come (sequences, already scaled).
// The dot-product families (mode; the argument is the inner product itself, the two extra columns stay out of it):
//   WIDE_ROWS_PLAIN  [v, 0, 0] on both sides;
//   WIDE_ROWS_UNIT   [v / |v|, 1 / |v|, 0] (left form), [v / |v|, 0, 1 / |v|] (right form): the norm's reciprocal rides in the column whose partner is
//                    zero on the other side, for the adjoint (wide_unaug_unit_kernel); a row of zero norm is 0 / 0 as in base_eval (seq_core.hpp);
// and with diff != 0 (SignatureLinear) the rows are INCREMENTS, taken before scaling:
//   sequences (lt == 0): dst row n * (diff - 1) + t  <-  src rows n * diff + t + 1 minus n * diff + t   (diff = observations per sequence, rows = N (diff - 1));
//   tensors (lt > 0, E == 1): dst row k * Tpad + t  <-  z^1 - z^0 of the caller's (lt, T, 2, d) array (kernels.py:329-330 collapsed: <z^1, x> - <z^0, x>).
// One wavefront per row.
constexpr int WIDE_ROWS_DIST = 0, WIDE_ROWS_PLAIN = 1, WIDE_ROWS_UNIT = 2;

GPSIG_WIDE_GLOBAL void __launch_bounds__(64) wide_aug_rows_kernel(const double* __restrict__ src, int64_t rows, int d, int right, int lt, int64_t Tn, int64_t Tpad,
                                                           int E, ScaleParams P, int mode, int diff, double* __restrict__ dst) {
    const int DA = d + 2;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const double *s = nullptr, *s0 = nullptr;          // the row, and the row subtracted from it (increments)
        if (lt > 0) {
            const int64_t t = r % Tpad;
            const int ke = int(r / Tpad), k = ke / E, e = ke - k * E;
            if (t < Tn && diff) { s0 = src + (int64_t(k) * Tn + t) * 2 * d; s = s0 + d; }
            else if (t < Tn) s = src + ((int64_t(k) * Tn + t) * E + e) * d;
        } else if (diff) {
            const int64_t n = r / (diff - 1), t = r - n * (diff - 1);
            s0 = src + (n * diff + t) * d; s = s0 + d;
        } else {
            s = src + r * d;
        }
        auto value = [&](int f) -> double {
            if (!s) return 0.0;
            double v = s0 ? s[f] - s0[f] : s[f];
            if (lt > 0 && P.has_ls) {
                const int lag = f / P.d_in, f0 = f - lag * P.d_in;
                v = v / P.lsv(f0);
                if (P.num_lags > 0) v = v * P.gamma[lag];
            }
            return v;
        };
        double ss = 0.0;
        for (int f = threadIdx.x; f < d; f += 64) {
            const double v = value(f);
            if (mode != WIDE_ROWS_UNIT) dst[r * DA + f] = v;
            ss = fma(v, v, ss);
        }
        ss = wide_wave_sum(ss);
        double inv = 0.0;
        if (mode == WIDE_ROWS_UNIT) {
            inv = s ? 1.0 / sqrt(ss) : 0.0;
            for (int f = threadIdx.x; f < d; f += 64) dst[r * DA + f] = s ? value(f) * inv : 0.0;
        }
        if (threadIdx.x == 0) {
            double own = s ? -0.5 * ss : 0.0, other = s ? 1.0 : 0.0;       // own: column d of the left form, d + 1 of the right form
            if (mode == WIDE_ROWS_PLAIN) own = other = 0.0;
            if (mode == WIDE_ROWS_UNIT) { own = inv; other = 0.0; }
            dst[r * DA + d] = right ? other : own;
            dst[r * DA + d + 1] = right ? own : other;
        }
    }
}

// The chain rule through the augmentation: g[f] = ga[f] - ga[norm column] * v[f]   (d(-|v|^2/2)/dv = -v; the constant column carries nothing).
// Tensor rows go back to the caller's (lt, T, E, d) order; sequences as they come.  One thread per output element.
// adj (SignatureMix where this side's term q |v|^2 / 2 survives; else NULL, and the arithmetic is what it was): the sums of the values' adjoints over the
// other side, per augmented row -- the norm column's adjoint becomes ga[norm column] - q adj[row].
GPSIG_WIDE_GLOBAL void wide_unaug_rows_kernel(const double* __restrict__ ga, const double* __restrict__ va, int64_t rows_out, int d, int right, int lt, int64_t Tn,
                                       int64_t Tpad, int E, double* __restrict__ g, const double* __restrict__ adj = nullptr, double q = 0.0) {
    const int DA = d + 2, nc = right ? d + 1 : d;
    const int64_t total = rows_out * d;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * blockDim.x) {
        const int f = int(idx % d);
        const int64_t ro = idx / d;
        int64_t r = ro;
        if (lt > 0) {
            const int e = int(ro % E);
            const int64_t t = (ro / E) % Tn;
            const int k = int(ro / (int64_t(E) * Tn));
            r = (int64_t(k) * E + e) * Tpad + t;
        }
        double gn = ga[r * DA + nc];
        if (adj) gn = fma(-q, adj[r], gn);
        g[idx] = fma(-gn, va[r * DA + f], ga[r * DA + f]);
    }
}

// The adjoints of the dot-product families' rows.  Sources: the adjoint gl of left-form rows vl and / or gr of right-form rows vr (both: one array on both
// sides of the lattices, the two forms of the tensors in Kzz -- the sum of the two); row mapping as wide_aug_rows_kernel.
// WIDE_ROWS_UNIT:  g_v = (g_u - <g_u, u> u) / |v|   (u = v / |v|; 1 / |v| from the form's own column).  One wavefront per output row.
GPSIG_WIDE_GLOBAL void __launch_bounds__(64) wide_unaug_unit_kernel(const double* __restrict__ gl, const double* __restrict__ vl, const double* __restrict__ gr,
                                                             const double* __restrict__ vr, int64_t rows_out, int d, int lt, int64_t Tn, int64_t Tpad, int E,
                                                             double* __restrict__ g) {
    const int DA = d + 2;
    for (int64_t ro = blockIdx.x; ro < rows_out; ro += gridDim.x) {
        int64_t r = ro;
        if (lt > 0) {
            const int e = int(ro % E);
            const int64_t t = (ro / E) % Tn;
            const int k = int(ro / (int64_t(E) * Tn));
            r = (int64_t(k) * E + e) * Tpad + t;
        }
        double pl = 0.0, pr = 0.0;
        for (int f = threadIdx.x; f < d; f += 64) {
            if (gl) pl = fma(gl[r * DA + f], vl[r * DA + f], pl);
            if (gr) pr = fma(gr[r * DA + f], vr[r * DA + f], pr);
        }
        pl = wide_wave_sum(pl);
        pr = wide_wave_sum(pr);
        const double il = gl ? vl[r * DA + d] : 0.0, ir = gr ? vr[r * DA + d + 1] : 0.0;
        for (int f = threadIdx.x; f < d; f += 64) {
            double v = 0.0;
            if (gl) v = fma(-pl, vl[r * DA + f], gl[r * DA + f]) * il;
            if (gr) v += fma(-pr, vr[r * DA + f], gr[r * DA + f]) * ir;
            g[ro * d + f] = v;
        }
    }
}

// WIDE_ROWS_PLAIN rows that are increments (SignatureLinear): an increment's adjoint goes to its two points,
//   sequences (lt == 0, diff = observations per sequence, rows_out = N diff):  gX[t] = gD[t - 1] - gD[t]   (zero outside 0 .. diff - 2),
//   tensors (lt > 0, the caller's (lt, T, 2, d) array, rows_out = lt T 2):     gz^1 = gD,  gz^0 = -gD.
// One thread per output element.
GPSIG_WIDE_GLOBAL void wide_unaug_inc_kernel(const double* __restrict__ gl, const double* __restrict__ gr, int64_t rows_out, int d, int lt, int64_t Tn, int64_t Tpad,
                                      int diff, double* __restrict__ g) {
    const int DA = d + 2;
    const int64_t total = rows_out * d;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * blockDim.x) {
        const int f = int(idx % d);
        const int64_t ro = idx / d;
        auto at = [&](int64_t r) -> double { return (gl ? gl[r * DA + f] : 0.0) + (gr ? gr[r * DA + f] : 0.0); };
        if (lt > 0) {
            const int e = int(ro % 2);
            const int64_t t = (ro / 2) % Tn;
            const int64_t k = ro / (2 * Tn);
            const double v = at(k * Tpad + t);
            g[idx] = e ? v : -v;
        } else {
            const int64_t n = ro / diff, t = ro - n * diff, r0 = n * (diff - 1);
            double v = 0.0;
            if (t >= 1) v = at(r0 + t - 1);
            if (t < diff - 1) v -= at(r0 + t);
            g[idx] = v;
        }
    }
}


// =====================================================================================================================================
// Sequence lattices from kernel-argument lattices in memory (the level diagonals of kernels.py:188-205, the sequence Grams of :208-237
// beyond the exact-shape kernels' columns): the sweeps of grad_wave_core.hpp -- one wavefront per lattice, lane lam owns C consecutive columns
// and works on row t - lam at step t, row prefixes handed to the right neighbour by one DPP shift -- fed by loads of the argument rows instead
// of point rows.  arg lattice of pair p = (i, j): base (p / N2) * si + (p % N2) * sj, row stride ld (a batched product: N2 = 1, si = L1 * L2, ld = L2;
// one product of all points: si = L1 * ld, sj = L2, ld = N2 * L2).
struct WideLatArgs {
    const double* arg;
    int64_t ld, si, sj, N2;
    int64_t P, p0, Ptot;        // this launch: lattices p0 .. p0 + P - 1 of Ptot (the level arrays' pair axis)
    int32_t L1, L2, M, kind, difference;
    double* out;                // forward: (M+1, Ptot) level values
    const double* G;            // reverse: (M+1, Ptot) upstream gradient, lattice pg of this launch at  (pg / N2) * g_i + (pg % N2) * g_j
    int64_t g_i, g_j;
    double* scratch;            // reverse: per group (M-1) * TF * 64 * C doubles (forward Q's, as grad_wave_kernel.hpp)
    double* lam;                // reverse: Lam = dL/ddM, (P, R1, R2) row-major
    int32_t ngroups;
    double kp0, kp1;            // SignaturePoly: offset and degree (WIDE_KD_POLY; p0 above is a lattice index)
    double* gb_part;            // reverse, SignaturePoly: gb_slices partial sums of W per lattice, lattices as G's pair axis (pg at (pg / N2) * g_i + (pg % N2) * g_j), or NULL
    int32_t gb_slices;          // ... (L1 L2 + WIDE_GB_SLICE - 1) / WIDE_GB_SLICE
    // SignatureMix without differences (with them both one-sided terms cancel: NULL): the NEGATED half norms of the launch's left / right sequences' points, from the
    // augmented rows' own norm column (stride nrm_ld doubles); lattice pg = (i, j) reads rows i L1 + r and columns j L2 + c (nrm_same, the diagonal: i L2 + c)
    const double* nrm_row;
    const double* nrm_col;
    int64_t nrm_ld;
    int32_t nrm_same;
};

// SignatureMix: where lattice pg of a launch finds its rows' and its columns' half norms
__device__ __forceinline__ const double* wide_lat_nrow(const WideLatArgs& A, int64_t pg) { return A.nrm_row + (pg / A.N2) * A.L1 * A.nrm_ld; }
__device__ __forceinline__ const double* wide_lat_ncol(const WideLatArgs& A, int64_t pg) {
    return A.nrm_col + (A.nrm_same ? pg / A.N2 : pg % A.N2) * A.L2 * A.nrm_ld;
}
constexpr int WIDE_GB_SLICE = 1024;       // cells of a lattice per wavefront of the polynomial adjoint kernel (16 per lane)

// argument rows (and, in the backward sweep, stored prefix rows) in flight ahead of a step: a step of few columns is shorter than a memory access
constexpr int wide_lat_pf(int C) { return C >= 8 ? 1 : (C == 4 ? 2 : 4); }

template <int C, int KD>
struct WideLatDm {
    double rd[C];
    int nvalid, b0, L2, diff;
    WideKap K;
    int64_t ld;
    const double* lat;
    // SignatureMix without differences (mix_terms sets them; else unused): the row's term q hx[r] rides in raw[C], the slot that only differences use; the
    // lane's columns' terms q hy[c] are kept
    const double* nrow;
    int64_t nld;
    double cn[C];

    __device__ __forceinline__ void mix_terms(const WideLatArgs& A, int64_t pg) {
        nrow = nullptr;
        nld = A.nrm_ld;
        if constexpr (KD == WIDE_KD_MIX) {
            if (!diff && A.nrm_row) {
                nrow = wide_lat_nrow(A, pg);
                const double* nc = wide_lat_ncol(A, pg);
#pragma unroll
                for (int c = 0; c < C; ++c) cn[c] = b0 + c < L2 ? -K.q * nc[(b0 + c) * nld] : 0.0;
            }
        }
    }
    __device__ __forceinline__ void load(int r, bool ok, double (&raw)[C + 1]) const {
        const double* p = lat + int64_t(r) * ld + b0;
#pragma unroll
        for (int c = 0; c <= C; ++c) raw[c] = (ok && b0 + c < L2 && (c < C || diff)) ? p[c] : 0.0;
        if constexpr (KD == WIDE_KD_MIX) {
            if (nrow) raw[C] = ok ? -K.q * nrow[r * nld] : 0.0;
        }
    }
    // kappa differences along the row (diff) or kappa itself (no differences: signature_algs.py:18-19 with difference=False)
    __device__ __forceinline__ void map(const double (&raw)[C + 1], double (&out)[C]) const {
        double k[C + 1];
#pragma unroll
        for (int c = 0; c <= C; ++c) k[c] = (c < C || diff) ? wide_kappa<KD>(K, raw[c]) : 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) out[c] = diff ? k[c + 1] - k[c] : k[c];
        if constexpr (KD == WIDE_KD_MIX) {
            if (nrow) {
#pragma unroll
                for (int c = 0; c < C; ++c) out[c] += raw[C] + cn[c];
            }
        }
    }
    __device__ __forceinline__ void prime(const double (&raw)[C + 1]) { map(raw, rd); }
    // one lattice row from the raw arguments of its new point row (forward: a + 1, backward: a; no differences: a)
    __device__ __forceinline__ void row(const double (&raw)[C + 1], bool forward, double (&dm)[C]) {
        double nd[C];
        map(raw, nd);
#pragma unroll
        for (int c = 0; c < C; ++c) {               // (selects, no branches: the arrays stay in registers)
            const double o = rd[c];
            const double df = forward ? nd[c] - o : o - nd[c];
            const double v = diff ? df : nd[c];
            rd[c] = nd[c];
            dm[c] = c < nvalid ? v : 0.0;
        }
    }
};

__device__ __forceinline__ double wide_from_left(double v) {       // lane l <- lane l-1, 0 into lane 0
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, true);     // wave_shr:1
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wide_from_right(double v) {      // lane l <- lane l+1, 0 into lane 63
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, true);     // wave_shl:1
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// Level values of P lattices: one wavefront per lattice (grid-stride).  K_m (m < M) = Q_m at the last cell, K_M = the sum of the row totals of R_M:
// both arrive at lane 63 (columns beyond the lattice pass the row prefixes on unchanged).
// NW > 1: NW wavefronts per lattice (a workgroup), lane lam = threadIdx.x of 64 NW; the hand-over across a wavefront boundary goes through LDS (two buffers
// alternating by the step's parity, one barrier per step).  For a FEW long lattices (the level diagonals of a minibatch: 50 lattices of 499 x 499 keep
// 50 of 1,024 SIMDs busy with eight columns per lane) -- more steps (R1 + 64 NW - 1), an eighth of the work per step, NW times the wavefronts.
// RG (ragged batches, wide_ragged_api.hip: wide_lattice_fwd_ragged_kernel, the same body -- the dense kernel compiles to what it was): every lattice has its
// own extent, base and row stride.  Pair pg = (i, j) = divmod(pg, N2) is len1[i] x len2[j].
// A full Gram (ld = all packed right rows): first row rbase[i] - rbase[0] of the chunk's argument array, first column cbase[j] -- the sides' packed row
// offsets.  The block diagonal (ld == 0, N2 = 1, len2 = len1, cbase = NULL): the lattice starts rbase[i] - rbase[0] CELLS into the array and its row stride
// is its own len2[j].  C and NW are the launch's, from the longest sequence: a shorter lattice leaves its last lanes without columns, and they pass the
// row prefixes on unchanged.
struct WideLatRaggedArgs : WideLatArgs {
    const int32_t* len1;    // the launch's left sequences
    const int32_t* len2;    // the right sequences (the diagonal: == len1)
    const int64_t* rbase;   // per left sequence of the launch: packed rows (full Gram) or lattice cells (diagonal) before it
    const int64_t* cbase;   // per right sequence: packed rows before it, or NULL
};

template <int C, int LQ, int KD, int NW = 1>
__global__ void __launch_bounds__(64 * NW) wide_lattice_fwd_kernel(const WideLatArgs A) {
#define GPSIG_WIDE_RG 0
#include "wide_lattice_fwd_body.inc"
#undef GPSIG_WIDE_RG
}
template <int C, int LQ, int KD, int NW = 1>
__global__ void __launch_bounds__(64 * NW) wide_lattice_fwd_ragged_kernel(const WideLatRaggedArgs A) {
#define GPSIG_WIDE_RG 1
#include "wide_lattice_fwd_body.inc"
#undef GPSIG_WIDE_RG
}

// Both sweeps (grad_wave_kernel.hpp: seq_grad_wave_kernel with the argument lattice in place of the point rows): Lam[a][b] = dL/ddM[a][b] out.
// grid: ngroups workgroups of one wavefront; a group's pairs one after the other through its scratch slot.
template <int C, int LQ, int KD, int NW = 1>
__global__ void __launch_bounds__(64 * NW) wide_lattice_bwd_kernel(const WideLatArgs A) {
    __shared__ double etab[EXP_TAB_N];
    __shared__ double xw[2][NW][LQ + 2];
    const double* const ktab = wide_tab<KD>(etab, threadIdx.x, 64 * NW);
    constexpr int GL = 64 * NW, PF = wide_lat_pf(C);
    const int lam = threadIdx.x, M = A.M, wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int dr = A.difference ? 1 : 0, R1 = A.L1 - dr, R2 = A.L2 - dr, TF = R1 + GL - 1;
    double* scr = A.scratch + size_t(blockIdx.x) * size_t(M - 1) * TF * GL * C;
    auto slot = [&](int m, int tf, int l, int c) -> double& { return scr[((size_t(m) * TF + tf) * GL + l) * C + c]; };
    auto xw_clear = [&]() {
        if constexpr (NW > 1) {
            __syncthreads();
            if (ln == 63) {
#pragma unroll
                for (int m = 0; m < LQ + 2; ++m) xw[0][wv][m] = xw[1][wv][m] = 0.0;
            }
            __syncthreads();
        }
    };
    for (int64_t pp = blockIdx.x; pp < A.P; pp += gridDim.x) {
        xw_clear();
        const int64_t pg = A.p0 + pp;
        WideLatDm<C, KD> dmg;
        dmg.lat = A.arg + (pg / A.N2) * A.si + (pg % A.N2) * A.sj;
        dmg.ld = A.ld; dmg.b0 = C * lam; dmg.L2 = A.L2; dmg.K = wide_kap(A.kind, ktab, A.kp0, A.kp1); dmg.diff = dr;
        { const int nv = R2 - C * lam; dmg.nvalid = nv < 0 ? 0 : (nv > C ? C : nv); }
        dmg.mix_terms(A, pg);
        double clev[LQ + 2];
#pragma unroll
        for (int p = 0; p < LQ + 2; ++p) clev[p] = (p >= 1 && p <= M) ? A.G[int64_t(p) * A.Ptot + (pg / A.N2) * A.g_i + (pg % A.N2) * A.g_j] : 0.0;
        // ---- forward sweep, Q's of levels < M to the scratch slot
        {
            WaveFwd<C, LQ> fw;
            fw.reset();
            double raw[PF][C + 1];
            if (dr) { dmg.load(0, true, raw[0]); dmg.prime(raw[0]); }
#pragma unroll
            for (int u = 0; u < PF; ++u) { const int r = u - lam + dr; dmg.load(r, r >= 0 && r < A.L1, raw[u]); }
            for (int t0 = 0; t0 < TF; t0 += PF) {
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const int t = t0 + u;
                    if (t >= TF) break;
                    double cin[LQ + 2], cur[C + 1];
                    cin[0] = 0.0;
#pragma unroll
                    for (int m = 1; m < LQ + 2; ++m) {
                        cin[m] = wide_from_left(fw.sout[m]);
                        if constexpr (NW > 1) {
                            const double x = xw[t & 1][wv > 0 ? wv - 1 : 0][m];
                            cin[m] = (ln == 0 && wv > 0) ? x : cin[m];
                        }
                    }
#pragma unroll
                    for (int c = 0; c <= C; ++c) cur[c] = raw[u][c];
                    const int a = t - lam;
                    { const int r = a + PF + dr; dmg.load(r, r >= 0 && r < A.L1, raw[u]); }
                    if (a >= 0 && a < R1) {
                        double dm[C];
                        dmg.row(cur, true, dm);
                        fw.step(dm, cin, M);
#pragma unroll
                        for (int m = 0; m < LQ; ++m)
                            if (m < M - 1) {
#pragma unroll
                                for (int c = 0; c < C; ++c) slot(m, t, lam, c) = fw.q[m][c];
                            }
                    }
                    if constexpr (NW > 1) {
                        if (ln == 63) {
#pragma unroll
                            for (int m = 1; m < LQ + 2; ++m) xw[(t + 1) & 1][wv][m] = fw.sout[m];
                        }
                        __syncthreads();
                    }
                }
            }
        }
        __threadfence();        // the backward sweep reads what other lanes of this wavefront (workgroup) stored
        xw_clear();
        // ---- backward sweep
        {
            WaveBwd<C, LQ> bw;
            bw.reset();
            double rawr[PF][C + 1], qr[PF][LQ][C];
            if (dr) { dmg.load(R1, true, rawr[0]); dmg.prime(rawr[0]); }
            double* lamrow = A.lam + size_t(pp) * R1 * R2;
            auto fetch_q = [&](int a, double (&q)[LQ][C]) {
                const int tf = a - 1 + lam;
#pragma unroll
                for (int m = 0; m < LQ; ++m)
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        double v = 0.0;
                        if (m < M - 1 && a > 0 && a < R1) {
                            if (c > 0) v = slot(m, tf, lam, c - 1);
                            else if (lam > 0) v = slot(m, tf - 1, lam - 1, C - 1);
                        }
                        q[m][c] = v;
                    }
            };
            // the rows of the coming PF steps (arguments and stored prefixes) are in flight while a step computes
#pragma unroll
            for (int v = 0; v < PF; ++v) {
                const int r = R1 - 1 - (v - (GL - 1 - lam));
                dmg.load(r, r >= 0 && r < R1, rawr[v]);
                fetch_q(r, qr[v]);
            }
            for (int u0 = 0; u0 < TF; u0 += PF) {
#pragma unroll
                for (int v = 0; v < PF; ++v) {
                    const int u = u0 + v;
                    if (u >= TF) break;
                    double sin[LQ], raw[C + 1], qcur[LQ][C];
#pragma unroll
                    for (int p = 0; p < LQ; ++p) {
                        sin[p] = wide_from_right(bw.svout[p]);
                        if constexpr (NW > 1) {
                            const double x = xw[u & 1][wv + 1 < NW ? wv + 1 : wv][p];
                            sin[p] = (ln == 63 && wv + 1 < NW) ? x : sin[p];
                        }
                    }
                    const int a = R1 - 1 - (u - (GL - 1 - lam));
#pragma unroll
                    for (int c = 0; c <= C; ++c) raw[c] = rawr[v][c];
#pragma unroll
                    for (int m = 0; m < LQ; ++m)
#pragma unroll
                        for (int c = 0; c < C; ++c) qcur[m][c] = qr[v][m][c];
                    { const int r = a - PF; dmg.load(r, r >= 0 && r < R1, rawr[v]); fetch_q(r, qr[v]); }
                    if (a >= 0 && a < R1) {
                        double dm[C], lv[C];
                        dmg.row(raw, false, dm);
                        bw.step(dm, clev, qcur, sin, M, lv);
#pragma unroll
                        for (int c = 0; c < C; ++c)
                            if (c < dmg.nvalid) lamrow[size_t(a) * R2 + C * lam + c] = lv[c];
                    }
                    if constexpr (NW > 1) {
                        if (ln == 0) {
#pragma unroll
                            for (int p = 0; p < LQ; ++p) xw[(u + 1) & 1][wv][p] = bw.svout[p];
                        }
                        __syncthreads();
                    }
                }
            }
        }
        __threadfence();        // the slot is rewritten by the next pair
    }
}

// W[r][c] = adjoint of the argument at point pair (r, c): the adjoint of the double increment (signature_algs.py:26)
//   Gam[r][c] = Lam[r-1][c-1] - Lam[r-1][c] - Lam[r][c-1] + Lam[r][c]   (zero outside the lattice; no differences: Gam = Lam)
// times d kappa / d a.  One thread per point pair; W in the layout of arg.
template <int KD>
__global__ void wide_lattice_adjoint_kernel(const WideLatArgs A, double* __restrict__ W) {
    __shared__ double etab[EXP_TAB_N];
    const WideKap K = wide_kap(A.kind, wide_tab<KD>(etab, threadIdx.x, blockDim.x), A.kp0, A.kp1);
    const int dr = A.difference ? 1 : 0, R1 = A.L1 - dr, R2 = A.L2 - dr;
    const int64_t cells = int64_t(A.L1) * A.L2, total = A.P * cells;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * blockDim.x) {
        const int64_t pp = idx / cells, pg = A.p0 + pp;
        const int r = int((idx % cells) / A.L2), c = int(idx % A.L2);
        const double* lm = A.lam + pp * int64_t(R1) * R2;
        auto at = [&](int a, int b) -> double { return (a >= 0 && a < R1 && b >= 0 && b < R2) ? lm[int64_t(a) * R2 + b] : 0.0; };
        const double gam = dr ? at(r - 1, c - 1) - at(r - 1, c) - at(r, c - 1) + at(r, c) : at(r, c);
        const int64_t off = (pg / A.N2) * A.si + (pg % A.N2) * A.sj + int64_t(r) * A.ld + c;
        double k, dk;
        wide_kappa_grad<KD>(K, A.arg[off], k, dk);
        W[off] = gam * dk;
    }
}

// The same for SignaturePoly, with the sum of what it stores (the offset's gradient): workgroups of ONE wavefront, each taking a slice of WIDE_GB_SLICE
// cells of one lattice, so that a slice's sum of W is formed in an order that depends on the lattice's shape alone, and lands in the slice's own slot
// (three 64-bit divisions: held to eight wavefronts per SIMD, which its scalar registers would otherwise miss by a few)
GPSIG_WIDE_GLOBAL void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) wide_lattice_adjoint_poly_kernel(const WideLatArgs A, double* __restrict__ W) {
    const WideKap K = wide_kap(A.kind, nullptr, A.kp0, A.kp1);
    const int dr = A.difference ? 1 : 0, R1 = A.L1 - dr, R2 = A.L2 - dr;
    const int64_t cells = int64_t(A.L1) * A.L2;
    const int64_t S = A.gb_slices;
    for (int64_t un = blockIdx.x; un < A.P * S; un += gridDim.x) {
        const int64_t pp = un / S, sl = un - pp * S, pg = A.p0 + pp;
        const double* lm = A.lam + pp * int64_t(R1) * R2;
        auto at = [&](int a, int b) -> double { return (a >= 0 && a < R1 && b >= 0 && b < R2) ? lm[int64_t(a) * R2 + b] : 0.0; };
        const int64_t base = (pg / A.N2) * A.si + (pg % A.N2) * A.sj;
        const int64_t end = (sl + 1) * WIDE_GB_SLICE < cells ? (sl + 1) * WIDE_GB_SLICE : cells;
        double wsum = 0.0;
        for (int64_t cell = sl * WIDE_GB_SLICE + threadIdx.x; cell < end; cell += 64) {
            const int r = int(cell / A.L2), c = int(cell % A.L2);
            const double gam = dr ? at(r - 1, c - 1) - at(r - 1, c) - at(r, c - 1) + at(r, c) : at(r, c);
            const int64_t off = base + int64_t(r) * A.ld + c;
            double k, dk;
            wide_kappa_grad<WIDE_KD_POLY>(K, A.arg[off], k, dk);
            const double w = gam * dk;
            W[off] = w;
            wsum += w;
        }
        wsum = wide_wave_sum(wsum);
        if (threadIdx.x == 0 && A.gb_part) A.gb_part[((pg / A.N2) * A.g_i + (pg % A.N2) * A.g_j) * S + sl] = wsum;
    }
}

// The same for SignatureMix, with the slice's sum of Gam d kappa / d p0 (the mixing's gradient): d kappa / d p0 = exp(a) - a, less the two half norms where
// the one-sided terms survive (no differences).  Slices, slots and order of summation as above.
GPSIG_WIDE_GLOBAL void __launch_bounds__(64) wide_lattice_adjoint_mix_kernel(const WideLatArgs A, double* __restrict__ W) {
    __shared__ double etab[EXP_TAB_N];
    const WideKap K = wide_kap(A.kind, wide_tab<WIDE_KD_MIX>(etab, threadIdx.x, 64), A.kp0, A.kp1);
    const int dr = A.difference ? 1 : 0, R1 = A.L1 - dr, R2 = A.L2 - dr;
    const int64_t cells = int64_t(A.L1) * A.L2;
    const int64_t S = A.gb_slices;
    const bool sided = !dr && A.nrm_row;
    for (int64_t un = blockIdx.x; un < A.P * S; un += gridDim.x) {
        const int64_t pp = un / S, sl = un - pp * S, pg = A.p0 + pp;
        const double* lm = A.lam + pp * int64_t(R1) * R2;
        auto at = [&](int a, int b) -> double { return (a >= 0 && a < R1 && b >= 0 && b < R2) ? lm[int64_t(a) * R2 + b] : 0.0; };
        const int64_t base = (pg / A.N2) * A.si + (pg % A.N2) * A.sj;
        const int64_t end = (sl + 1) * WIDE_GB_SLICE < cells ? (sl + 1) * WIDE_GB_SLICE : cells;
        const double *nr = sided ? wide_lat_nrow(A, pg) : nullptr, *nc = sided ? wide_lat_ncol(A, pg) : nullptr;
        double psum = 0.0;
        for (int64_t cell = sl * WIDE_GB_SLICE + threadIdx.x; cell < end; cell += 64) {
            const int r = int(cell / A.L2), c = int(cell % A.L2);
            const double gam = dr ? at(r - 1, c - 1) - at(r - 1, c) - at(r, c - 1) + at(r, c) : at(r, c);
            const int64_t off = base + int64_t(r) * A.ld + c;
            double k, dk, dp;
            wide_mix_grad(K, A.arg[off], k, dk, dp);
            if (sided) dp += nr[r * A.nrm_ld] + nc[c * A.nrm_ld];
            W[off] = gam * dk;
            psum = fma(gam, dp, psum);
        }
        psum = wide_wave_sum(psum);
        if (threadIdx.x == 0 && A.gb_part) A.gb_part[((pg / A.N2) * A.g_i + (pg % A.N2) * A.g_j) * S + sl] = psum;
    }
}

// SignatureMix without differences: Gam = Lam, and the sums of the values' adjoints over the other side are the row sums and the column sums of the
// launch's Lam lattices.  One wavefront per unit, in an order fixed by the launch's shape: unit u < NI L1 is row r of left sequence il (sums over its lattices'
// columns), the others column c of right sequence jl (over its lattices' rows).  NI x NJ lattices, pair il NJ + jl (the diagonal: NJ = 1 and jl = il).
// radj (NI L1) is written; cadj (NJ L2; the diagonal: NI L2) is written or, acc, added to (the chunks of left sequences one after the other).
GPSIG_WIDE_GLOBAL void __launch_bounds__(64) wide_lattice_sides_kernel(const double* __restrict__ lam, int64_t NI, int64_t NJ, int L1, int L2, int diag, int acc,
                                                                 double* __restrict__ radj, double* __restrict__ cadj) {
    const int64_t rows = NI * L1, cols = (diag ? NI : NJ) * L2, cells = int64_t(L1) * L2;
    for (int64_t un = blockIdx.x; un < rows + cols; un += gridDim.x) {
        double s = 0.0;
        if (un < rows) {
            const int64_t il = un / L1;
            const int r = int(un - il * L1);
            for (int64_t jl = 0; jl < (diag ? 1 : NJ); ++jl) {
                const double* lm = lam + (diag ? il : il * NJ + jl) * cells + int64_t(r) * L2;
                for (int c = threadIdx.x; c < L2; c += 64) s += lm[c];
            }
            s = wide_wave_sum(s);
            if (threadIdx.x == 0) radj[un] = s;
        } else {
            const int64_t uc = un - rows, jl = uc / L2;
            const int c = int(uc - jl * L2);
            for (int64_t il = diag ? jl : 0; il < (diag ? jl + 1 : NI); ++il) {
                const double* lm = lam + (diag ? il : il * NJ + jl) * cells + c;
                for (int r = threadIdx.x; r < L1; r += 64) s += lm[int64_t(r) * L2];
            }
            s = wide_wave_sum(s);
            if (threadIdx.x == 0) cadj[uc] = acc ? cadj[uc] + s : s;
        }
    }
}

// The symmetric Gram's upstream gradient folded onto the pairs i <= j (the levels are symmetric functions of the two sequences):
// Gs[m][i][j] = G[m][i][j] + G[m][j][i] (j > i),  G[m][i][i] (j == i),  0 (j < i).
GPSIG_WIDE_GLOBAL void wide_sym_upstream_kernel(const double* __restrict__ G, int64_t N, int M1, double* __restrict__ Gs) {
    const int64_t total = int64_t(M1) * N * N;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * blockDim.x) {
        const int64_t j = idx % N, i = (idx / N) % N, m = idx / (N * N);
        Gs[idx] = j > i ? G[idx] + G[(m * N + j) * N + i] : (j == i ? G[idx] : 0.0);
    }
}

// dM[pair][a][b] (signature_algs.py:26 / :56) from the argument lattices, for the sweeps that read it from memory (the higher-order reverse pass,
// grad_wave_ho_kernel.hpp).  One thread per lattice cell.
template <int KD>
__global__ void wide_lattice_dm_kernel(const WideLatArgs A, double* __restrict__ dM) {
    __shared__ double etab[EXP_TAB_N];
    const WideKap K = wide_kap(A.kind, wide_tab<KD>(etab, threadIdx.x, blockDim.x), A.kp0, A.kp1);
    const int dr = A.difference ? 1 : 0, R1 = A.L1 - dr, R2 = A.L2 - dr;
    const int64_t cells = int64_t(R1) * R2, total = A.P * cells;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * blockDim.x) {
        const int64_t pp = idx / cells, pg = A.p0 + pp;
        const int a = int((idx % cells) / R2), b = int(idx % R2);
        const double* base = A.arg + (pg / A.N2) * A.si + (pg % A.N2) * A.sj + int64_t(a) * A.ld + b;
        double v = wide_kappa<KD>(K, base[0]);
        if (dr) v = (wide_kappa<KD>(K, base[A.ld + 1]) - wide_kappa<KD>(K, base[A.ld])) - (wide_kappa<KD>(K, base[1]) - v);
        if constexpr (KD == WIDE_KD_MIX) {
            if (!dr && A.nrm_row) v -= K.q * (wide_lat_nrow(A, pg)[a * A.nrm_ld] + wide_lat_ncol(A, pg)[b * A.nrm_ld]);
        }
        dM[idx] = v;
    }
}

// g[r][f] = left-form chain rule of (gl, vl) [+ right-form chain rule of (gr, vr) where given: one array on both sides of the lattices]
// (adjl / adjr, q: as wide_unaug_rows_kernel)
GPSIG_WIDE_GLOBAL void wide_unaug_pair_kernel(const double* __restrict__ gl, const double* __restrict__ vl, const double* __restrict__ gr, const double* __restrict__ vr,
                                       int64_t rows, int d, double* __restrict__ g, const double* __restrict__ adjl = nullptr,
                                       const double* __restrict__ adjr = nullptr, double q = 0.0) {
    const int DA = d + 2;
    const int64_t total = rows * d;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * blockDim.x) {
        const int f = int(idx % d);
        const int64_t r = idx / d;
        double nl = gl[r * DA + d];
        if (adjl) nl = fma(-q, adjl[r], nl);
        double v = fma(-nl, vl[r * DA + f], gl[r * DA + f]);
        if (gr) {
            double nr = gr[r * DA + d + 1];
            if (adjr) nr = fma(-q, adjr[r], nr);
            v += fma(-nr, vr[r * DA + f], gr[r * DA + f]);
        }
        g[idx] = v;
    }
}

// =====================================================================================================================================
// Inducing tensors vs inducing tensors (kernels.py:263-283 + signature_algs.py:76-99) from the argument blocks of every component:
// arg (lt, E * Tpad, E * Tpad), block k = left-form rows of component k times its right-form rows; row / column (e, t) at e * Tpad + t.
// One thread per (t, t'), lanes along t' (contiguous).
struct WideTensArgs {
    const double* arg;
    int64_t Tpad, Tn;
    int32_t M, E, kind, sum_levels;
    const double* w;        // (M+1) weights or NULL
    double* out;            // forward: (T, T) weighted level sum or (M+1, T, T)
    const double* G;        // reverse: (M+1, T, T)
    double* W;              // reverse: adjoint of arg, same layout
    double kp0, kp1;        // SignaturePoly: offset and degree (WIDE_KD_POLY)
    double* gb_part;        // reverse, SignaturePoly: (Tpad / 64, Tpad) partial sums of W, one per (column block, row t), or NULL (SignatureMix: the mixing's gradient)
    // SignatureMix without increments (E == 1; with them the four-term difference cancels both one-sided terms: NULL): the NEGATED half norm of tensor t of
    // component k at nrm[(k * Tpad + t) * nrm_ld] (the left form's own norm column); value = psi(a) + q (hz[t] + hz[t'])
    const double* nrm;
    int64_t nrm_ld;
    double* gval;           // reverse, nrm given: (lt, Tpad, Tpad) the values' adjoints (zeros at padded tensors); wide_lattice_sides_kernel takes their row and column sums
};

// value of component k at (t, t'): kappa, or the four-term difference of its two points on both sides (kernels.py:276-277)
template <int KD>
__device__ __forceinline__ double wide_tens_val(const double* __restrict__ blk, int64_t R, int64_t Tpad, int E, const WideKap& K, int64_t t, int64_t tp) {
    if (E == 2)
        return wide_kappa<KD>(K, blk[(Tpad + t) * R + Tpad + tp]) + wide_kappa<KD>(K, blk[t * R + tp]) - wide_kappa<KD>(K, blk[(Tpad + t) * R + tp]) -
               wide_kappa<KD>(K, blk[t * R + Tpad + tp]);
    return wide_kappa<KD>(K, blk[t * R + tp]);
}

// ... of component k, with SignatureMix's one-sided terms where they survive
template <int KD>
__device__ __forceinline__ double wide_tens_val_k(const WideTensArgs& A, int k, int64_t R, const WideKap& K, int64_t t, int64_t tp) {
    double v = wide_tens_val<KD>(A.arg + int64_t(k) * R * R, R, A.Tpad, A.E, K, t, tp);
    if constexpr (KD == WIDE_KD_MIX) {
        if (A.nrm) v -= K.q * (A.nrm[(k * A.Tpad + t) * A.nrm_ld] + A.nrm[(k * A.Tpad + tp) * A.nrm_ld]);
    }
    return v;
}

template <int KD>
__global__ void __launch_bounds__(64) wide_tens_fwd_kernel(const WideTensArgs A) {
    __shared__ double etab[EXP_TAB_N];
    const WideKap K = wide_kap(A.kind, wide_tab<KD>(etab, threadIdx.x, 64), A.kp0, A.kp1);
    const int64_t tp = int64_t(blockIdx.x) * 64 + threadIdx.x, R = int64_t(A.E) * A.Tpad;
    if (tp >= A.Tn) return;
    for (int64_t t = blockIdx.y; t < A.Tn; t += gridDim.y) {
        double acc = A.w ? A.w[0] : 1.0;                                   // level 0 == 1 (signature_algs.py:88)
        if (!A.sum_levels) A.out[t * A.Tn + tp] = acc;
        int k = 0;
        for (int i = 1; i <= A.M; ++i) {
            double prod = 1.0;
            for (int j = 0; j < i; ++j, ++k) prod *= wide_tens_val_k<KD>(A, k, R, K, t, tp);      // :91-97
            const double f = A.w ? A.w[i] : 1.0;
            if (A.sum_levels) acc = fma(prod, f, acc);
            else A.out[(int64_t(i) * A.Tn + t) * A.Tn + tp] = prod * f;
        }
        if (A.sum_levels) A.out[t * A.Tn + tp] = acc;
    }
}

// grid (Tpad / 64, Tpad rows (grid-stride)): every entry of W is written (zeros at padded tensors)
// (the identity instance has no table and fewer vector registers, and would otherwise spend scalar registers on hoisted addresses to the point of
// losing a wavefront per SIMD to them: it is held to the eight of the RBF instance)
template <int KD>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(KD == WIDE_KD_ID ? 8 : 1))) wide_tens_bwd_kernel(const WideTensArgs A) {
    __shared__ double etab[EXP_TAB_N];
    const WideKap K = wide_kap(A.kind, wide_tab<KD>(etab, threadIdx.x, 64), A.kp0, A.kp1);
    const int64_t tp = int64_t(blockIdx.x) * 64 + threadIdx.x, R = int64_t(A.E) * A.Tpad;
    for (int64_t t = blockIdx.y; t < A.Tpad; t += gridDim.y) {
        const bool valid = t < A.Tn && tp < A.Tn;
        double wsum = 0.0;          // SignaturePoly: this lane's sum of the W entries of (t, t'); a padded row or column adds exactly zero
        int k0 = 0;
        for (int i = 1; i <= A.M; ++i) {
            const double c = valid ? A.G[(int64_t(i) * A.Tn + t) * A.Tn + tp] : 0.0;
            double v[WIDE_MAX_LEVELS];
#pragma unroll
            for (int j = 0; j < WIDE_MAX_LEVELS; ++j) {
                if constexpr (KD == WIDE_KD_MIX) v[j] = j < i ? wide_tens_val_k<KD>(A, k0 + j, R, K, t, tp) : 1.0;
                else v[j] = j < i ? wide_tens_val<KD>(A.arg + int64_t(k0 + j) * R * R, R, A.Tpad, A.E, K, t, tp) : 1.0;
            }
#pragma unroll
            for (int j = 0; j < WIDE_MAX_LEVELS; ++j) {
                if (j >= i) continue;
                double g = c;                                              // dL/dval_j = c * prod of the other components
#pragma unroll
                for (int q = 0; q < WIDE_MAX_LEVELS; ++q)
                    if (q != j && q < i) g *= v[q];
                const double* blk = A.arg + int64_t(k0 + j) * R * R;
                double* wb = A.W + int64_t(k0 + j) * R * R;
                if constexpr (KD == WIDE_KD_MIX) {          // W = g psi', the mixing's partial g d value / d p0, and g itself where the one-sided terms survive
                    double kk, dk, dp;
                    if (A.E == 2) {
                        double ps = 0.0;          // (the four entries: +, +, -, -)
                        wide_mix_grad(K, blk[(A.Tpad + t) * R + A.Tpad + tp], kk, dk, dp); wb[(A.Tpad + t) * R + A.Tpad + tp] = g * dk; ps += dp;
                        wide_mix_grad(K, blk[t * R + tp], kk, dk, dp);                     wb[t * R + tp] = g * dk; ps += dp;
                        wide_mix_grad(K, blk[(A.Tpad + t) * R + tp], kk, dk, dp);          wb[(A.Tpad + t) * R + tp] = -g * dk; ps -= dp;
                        wide_mix_grad(K, blk[t * R + A.Tpad + tp], kk, dk, dp);            wb[t * R + A.Tpad + tp] = -g * dk; ps -= dp;
                        wsum += valid ? g * ps : 0.0;
                    } else {
                        wide_mix_grad(K, blk[t * R + tp], kk, dk, dp);
                        wb[t * R + tp] = g * dk;
                        const double gv = valid ? g : 0.0;
                        if (A.nrm) {
                            dp += A.nrm[((k0 + j) * A.Tpad + t) * A.nrm_ld] + A.nrm[((k0 + j) * A.Tpad + tp) * A.nrm_ld];
                            A.gval[((k0 + j) * A.Tpad + t) * A.Tpad + tp] = gv;
                        }
                        wsum += gv * dp;
                    }
                    continue;
                }
                double kk, dk;
                if (A.E == 2) {
                    double ws = 0.0;          // (the four entries' sum: +, +, -, -)
                    wide_kappa_grad<KD>(K, blk[(A.Tpad + t) * R + A.Tpad + tp], kk, dk); wb[(A.Tpad + t) * R + A.Tpad + tp] = g * dk;
                    if constexpr (KD == WIDE_KD_POLY) ws += g * dk;
                    wide_kappa_grad<KD>(K, blk[t * R + tp], kk, dk);                     wb[t * R + tp] = g * dk;
                    if constexpr (KD == WIDE_KD_POLY) ws += g * dk;
                    wide_kappa_grad<KD>(K, blk[(A.Tpad + t) * R + tp], kk, dk);          wb[(A.Tpad + t) * R + tp] = -g * dk;
                    if constexpr (KD == WIDE_KD_POLY) ws -= g * dk;
                    wide_kappa_grad<KD>(K, blk[t * R + A.Tpad + tp], kk, dk);            wb[t * R + A.Tpad + tp] = -g * dk;
                    if constexpr (KD == WIDE_KD_POLY) ws -= g * dk;
                    if constexpr (KD == WIDE_KD_POLY) wsum += valid ? ws : 0.0;
                } else {
                    wide_kappa_grad<KD>(K, blk[t * R + tp], kk, dk);
                    wb[t * R + tp] = g * dk;
                    if constexpr (KD == WIDE_KD_POLY) wsum += valid ? g * dk : 0.0;
                }
            }
            k0 += i;
        }
        if constexpr (KD == WIDE_KD_POLY || KD == WIDE_KD_MIX) {
            if (A.gb_part) {
                const double s = wide_wave_sum(wsum);
                if (threadIdx.x == 0) A.gb_part[int64_t(blockIdx.x) * A.Tpad + t] = s;
            }
        }
    }
}

// gZ in the caller's (lt, T, E, d) order from the adjoints of the left-form and the right-form augmented rows (rows (k * E + e) * Tpad + t)
GPSIG_WIDE_GLOBAL void wide_unaug_tens_kernel(const double* __restrict__ gl, const double* __restrict__ vl, const double* __restrict__ gr, const double* __restrict__ vr,
                                       int64_t rows_out, int d, int64_t Tn, int64_t Tpad, int E, double* __restrict__ g,
                                       const double* __restrict__ adjl = nullptr, const double* __restrict__ adjr = nullptr, double q = 0.0) {
    const int DA = d + 2;
    const int64_t total = rows_out * d;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * blockDim.x) {
        const int f = int(idx % d);
        const int64_t ro = idx / d;
        const int e = int(ro % E);
        const int64_t t = (ro / E) % Tn;
        const int k = int(ro / (int64_t(E) * Tn));
        const int64_t r = (int64_t(k) * E + e) * Tpad + t;
        double nl = gl[r * DA + d], nr = gr[r * DA + d + 1];
        if (adjl) { nl = fma(-q, adjl[r], nl); nr = fma(-q, adjr[r], nr); }          // (SignatureMix: as wide_unaug_rows_kernel; both or neither)
        g[idx] = fma(-nl, vl[r * DA + f], gl[r * DA + f]) + fma(-nr, vr[r * DA + f], gr[r * DA + f]);
    }
}

// =====================================================================================================================================
// The two contractions of the reverse pass in ONE pass over the adjoint array W (rows = (sequence, time), CW columns), for narrow augmented rows
// (DA <= DAP = 16 / 32):   gZA[c][f] = sum_r W[r][c] XA[r][f]   and   gXA[r][f] = sum_c W[r][c] ZA[c][f].
// rocBLAS runs these as 12 x 10,240-output products over K = 25,000 on 80 macro-tiles (1.1 + 0.7 ms per GB of W at NetFlow's shape: more than every
// hand-written kernel of the step together); here a wavefront owns a strip of 64 rows and walks the columns in tiles of 64: the tile goes to LDS once,
// phase 1 (lane = column) adds its 64 rows into the strip's partial sums of gZA -- XA rows are wavefront-uniform: scalar operands --, phase 2
// (lane = row) adds its 64 columns into gXA, which is complete when the strip ends.  The partial sums (strips, CW, DA) are summed in a fixed order by
// wide_contract_reduce_kernel (deterministic; a quarter of W's bytes at DAP = 16).
struct WideContractArgs {
    const double* W;        // (R, CW)
    const double* XA;       // (R, DA)
    const double* ZA;       // (CW, DA)
    int64_t R, CW;
    int32_t DA, groups;     // column tiles are dealt to `groups` workgroups per strip (grid y): enough wavefronts to fill the chip
    double* gXA_part;       // (groups, R, DAP)
    double* part;           // (strips, CW, DAP)
};

// grid (strips, groups), one wavefront each.  Both products of a tile on the float64 matrix cores (v_mfma_f64_16x16x4; operand layout as
// lowrank_kernels.hpp: A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15], results D[(l >> 4) + 4 r][l & 15]): per 64 x 64 tile and 16 columns of
// the augmented rows 64 + 64 MFMAs against 80 + 80 LDS reads -- the first form (one broadcast LDS read per FMA) ran at rocBLAS's 3.5 ms.
typedef double wide_f64x4 __attribute__((ext_vector_type(4)));

template <int DAP>
__global__ void __launch_bounds__(64) wide_contract_kernel(const WideContractArgs A) {
    constexpr int TS = 65, NB = DAP / 16;
    __shared__ double tile[64 * TS];
    __shared__ double xs[64 * DAP], zs[64 * DAP];            // the strip's rows of XA, the tile's rows of ZA: zero beyond DA
    const int lane = threadIdx.x, DA = A.DA, li = lane & 15, lk = lane >> 4;
    const int64_t ntiles = (A.CW + 63) / 64;
    for (int64_t strip = blockIdx.x; strip * 64 < A.R; strip += gridDim.x) {
        const int64_t r0 = strip * 64;
        const int nr = int(A.R - r0 < 64 ? A.R - r0 : 64);
        __syncthreads();
        for (int e = lane; e < 64 * DAP; e += 64) {
            const int r = e / DAP, f = e % DAP;
            xs[e] = (r < nr && f < DA) ? A.XA[(r0 + r) * DA + f] : 0.0;
        }
        wide_f64x4 acc2[4][NB];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < NB; ++n) acc2[m][n] = wide_f64x4{0.0, 0.0, 0.0, 0.0};
        // a tile's 64 rows of W are requested a whole tile ahead (64 registers): a wavefront has nothing else to hide that latency behind
        double wn[64];
        auto request = [&](int64_t ti) {
            const int64_t c = ti * 64 + lane;
            const double* __restrict__ src = A.W + r0 * A.CW + (c < A.CW ? c : 0);
#pragma unroll
            for (int r = 0; r < 64; ++r) wn[r] = src[int64_t(r < nr ? r : 0) * A.CW];
        };
        if (int64_t(blockIdx.y) < ntiles) request(blockIdx.y);
        for (int64_t ti = blockIdx.y; ti < ntiles; ti += A.groups) {
            const int64_t c0 = ti * 64;
            const bool cok = c0 + lane < A.CW;
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 64; ++r) tile[r * TS + lane] = (r < nr && cok) ? wn[r] : 0.0;
            if (ti + A.groups < ntiles) request(ti + A.groups);
            for (int e = lane; e < 64 * DAP; e += 64) {
                const int cc = e / DAP, f = e % DAP;
                zs[e] = (c0 + cc < A.CW && f < DA) ? A.ZA[(c0 + cc) * DA + f] : 0.0;
            }
            __syncthreads();
            // phase 1: D1[column][f] = sum over the strip's rows of W[row][column] XA[row][f]
            wide_f64x4 acc1[4][NB];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < NB; ++n) acc1[m][n] = wide_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
            for (int k0 = 0; k0 < 64; k0 += 4) {
                double av[4], bv[NB];
#pragma unroll
                for (int m = 0; m < 4; ++m) av[m] = tile[(k0 + lk) * TS + m * 16 + li];
#pragma unroll
                for (int n = 0; n < NB; ++n) bv[n] = xs[(k0 + lk) * DAP + n * 16 + li];
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc1[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bv[n], acc1[m][n], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t col = c0 + m * 16 + lk + 4 * r;
                    if (col < A.CW) {
#pragma unroll
                        for (int n = 0; n < NB; ++n) A.part[(strip * A.CW + col) * DAP + n * 16 + li] = acc1[m][n][r];
                    }
                }
            // phase 2: D2[row][f] += sum over the tile's columns of W[row][column] ZA[column][f]
#pragma unroll 4
            for (int k0 = 0; k0 < 64; k0 += 4) {
                double av[4], bv[NB];
#pragma unroll
                for (int m = 0; m < 4; ++m) av[m] = tile[(m * 16 + li) * TS + k0 + lk];
#pragma unroll
                for (int n = 0; n < NB; ++n) bv[n] = zs[(k0 + lk) * DAP + n * 16 + li];
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < NB; ++n) acc2[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bv[n], acc2[m][n], 0, 0, 0);
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m * 16 + lk + 4 * r;
                if (row < nr) {
#pragma unroll
                    for (int n = 0; n < NB; ++n) A.gXA_part[(int64_t(blockIdx.y) * A.R + r0 + row) * DAP + n * 16 + li] = acc2[m][n][r];
                }
            }
    }
}

// Second form (round 6, DAP = 16): the same tile walk with PART tiles of HR = 32 / 16 rows in LDS (16.6 / 8.3 KB per wavefront instead of 49.6: two wavefronts per SIMD where the
// first form fits three per CU -- its matrix cores idle while its only wavefront loads and stages), and the MFMAs' second operands in REGISTERS: a lane's 16
// entries of the strip's XA rows are loaded once per strip, its 16 entries of the tile's ZA rows once per tile.  MFMA count and partial-sum layout unchanged.
template <int HR>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) wide_contract16_kernel(const WideContractArgs A) {
    constexpr int TS = 65, NH = 64 / HR, Q1 = HR / 4, MB = HR / 16;     // part tiles of HR rows: NH per tile, Q1 reduction steps of phase 1, MB row blocks of phase 2
    __shared__ double tile[HR * TS];
    const int lane = threadIdx.x, DA = A.DA, li = lane & 15, lk = lane >> 4;
    const int64_t ntiles = (A.CW + 63) / 64;
    const bool fok = li < DA;
    for (int64_t strip = blockIdx.x; strip * 64 < A.R; strip += gridDim.x) {
        const int64_t r0 = strip * 64;
        const int nr = int(A.R - r0 < 64 ? A.R - r0 : 64);
        // this lane's entries of the strip's rows of XA as MFMA B operands: step s of half h covers rows 32 h + 4 s + lk
        double bx[NH][Q1];
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int q = 0; q < Q1; ++q) {
                const int row = HR * h + 4 * q + lk;
                bx[h][q] = (row < nr && fok) ? A.XA[(r0 + row) * DA + li] : 0.0;
            }
        wide_f64x4 acc2[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc2[m] = wide_f64x4{0.0, 0.0, 0.0, 0.0};
        double wn[HR];
        auto request = [&](int64_t ti, int h) {
            const int64_t c = ti * 64 + lane;
            const int hb = HR * h < nr ? HR * h : 0;             // (a part tile wholly beyond the strip's rows: any rows inside it, masked at the LDS write)
            const double* __restrict__ src = A.W + (r0 + hb) * A.CW + (c < A.CW ? c : 0);
#pragma unroll
            for (int r = 0; r < HR; ++r) wn[r] = src[int64_t(hb + r < nr ? r : 0) * A.CW];
        };
        if (int64_t(blockIdx.y) < ntiles) request(blockIdx.y, 0);
        for (int64_t ti = blockIdx.y; ti < ntiles; ti += A.groups) {
            const int64_t c0 = ti * 64;
            const bool cok = c0 + lane < A.CW;
            double bz[16];                                   // this lane's entries of the tile's rows of ZA: step s covers columns 4 s + lk
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t col = c0 + 4 * q + lk;
                bz[q] = (col < A.CW && fok) ? A.ZA[col * DA + li] : 0.0;
            }
            wide_f64x4 acc1[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) acc1[m] = wide_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                __syncthreads();
#pragma unroll
                for (int r = 0; r < HR; ++r) tile[r * TS + lane] = (HR * h + r < nr && cok) ? wn[r] : 0.0;
                if (h + 1 < NH) request(ti, h + 1);
                else if (ti + A.groups < ntiles) request(ti + A.groups, 0);
                __syncthreads();
                // phase 1: D1[column][f] += sum over the half's rows of W[row][column] XA[row][f]
#pragma unroll
                for (int q = 0; q < Q1; ++q) {
                    double av[4];
#pragma unroll
                    for (int m = 0; m < 4; ++m) av[m] = tile[(4 * q + lk) * TS + m * 16 + li];
#pragma unroll
                    for (int m = 0; m < 4; ++m) acc1[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bx[h][q], acc1[m], 0, 0, 0);
                }
                // phase 2: D2[row][f] += sum over the tile's columns of W[row][column] ZA[column][f], the half's 32 rows
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    double av[MB];
#pragma unroll
                    for (int m = 0; m < MB; ++m) av[m] = tile[(m * 16 + li) * TS + 4 * q + lk];
#pragma unroll
                    for (int m = 0; m < MB; ++m) acc2[MB * h + m] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bz[q], acc2[MB * h + m], 0, 0, 0);
                }
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t col = c0 + m * 16 + lk + 4 * r;
                    if (col < A.CW) A.part[(strip * A.CW + col) * 16 + li] = acc1[m][r];
                }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m * 16 + lk + 4 * r;
                if (row < nr) A.gXA_part[(int64_t(blockIdx.y) * A.R + r0 + row) * 16 + li] = acc2[m][r];
            }
    }
}

// dst[e][f] = (acc ? dst : 0) + sum over k of part[k][e][f], f < DA of DAP (a fixed order: deterministic)
GPSIG_WIDE_GLOBAL void wide_contract_reduce_kernel(const double* __restrict__ part, int64_t nparts, int64_t rows, int DA, int DAP, int acc, double* __restrict__ dst) {
    const int64_t n = rows * DA;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < n; idx += int64_t(gridDim.x) * blockDim.x) {
        const int64_t e = idx / DA;
        const int f = int(idx % DA);
        double s = acc ? dst[idx] : 0.0;
        for (int64_t k = 0; k < nparts; ++k) s += part[(k * rows + e) * DAP + f];
        dst[idx] = s;
    }
}

}  // namespace gpsig
