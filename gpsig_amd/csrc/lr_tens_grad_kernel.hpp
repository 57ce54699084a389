// lr_tens_grad_kernel.hpp -- reverse pass of the low-rank feature map of inducing tensors (lr_tens_features_fused_kernel, lr_fused_kernel.hpp)
// in ONE kernel.
//
// The reference trains the inducing tensors through TensorFlow's autodiff of Nystrom_map (gpsig/low_rank_calculations.py:26-61) and the chained
// sparse projections of tensor_kern_lr_feature (gpsig/signature_algs.py:194-222); there is no gradient code to restate.  As torch ops
// (gpsig_amd/autodiff.py, _LowRankScope._tens_torch) that is one cross matrix, a product with the whitening and M (M - 1) / 2 chained
// projections of three GEMMs each, replayed in reverse by autograd: about a hundred launches for arrays of a few KB per tensor.  Here a
// workgroup owns one tensor at a time (it strides over the tensors) and keeps everything in LDS:
//
//   forward again   rows (k, e) of the tensor's lt * E components: z, kx = kappa(z, S), ft = kx Wh, U[k] = the difference over e (incremental
//                   tensors) -- as lr_tens_features_fused_body; then level i's chain  R = U[k];  R = sketch_{j-1}(U[k + j], R), j = 1 .. i-1,
//                   this time keeping EVERY projection's output (M (M - 1) / 2 vectors of width r)
//   chains back     level i from its slice of dPhi; for a step R' = sketch(U[k], R):
//                       dU[k][i1] = sum_e val R[i2] dR'[j]   (the sketch's entries grouped by i1)
//                       dR[i2]    = sum_e val U[k][i1] dR'[j]   (grouped by i2)
//                   a thread owns a DESTINATION index and gathers over the transposed copies of the sketch (LrGradSketch: built once per
//                   draw on the host): no atomics.  Every U[k] enters exactly one chain step, so each row of dU is written once
//   whitening       dft = dU with signs -/+ over e;  dkx = dft Wh^T;  dWh += kx^T dft
//   base kernel     dz[row] = sum_i dkx[row][i] d kappa(z_row, S_i) / dz,  dS_i += sum_row dkx[row][i] d kappa / dS_i  (base_eval_grad,
//                   grad_core.hpp: the sequence reverse pass's helper, with its convention at zero distance -- no gradient through the
//                   clamped square root of the Matern families)
//
// dWh, dS and the base kernel's own parameter are summed over the tensors a workgroup processes in registers and leave as one partial per
// workgroup, added up by lr_grad_reduce_kernel in workgroup order: two runs agree bit for bit.  dZ is written per tensor in the caller's
// (lt, T, E, d) layout.
//
// SignatureSpectral (lr_tens_features_grad_spectral_kernel): kappa by spectral_pair on the trainable parameters; the kernel stops at dkx,
// which it writes to HBM in the order of the points of the tensors it was launched for -- row ((k nt + t - t0) E + e) of (lt nt E, c) -- and
// sums dWh only.  For one launch over all tensors that is the flat point order of Z, so the spectral cross op's reverse kernels
// (spectral_cross_api.hip) take Z viewed (lt T E, d) and dkx as they are and return dZ, dS, dalpha, domega, dgamma.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lr_grad_kernel.hpp"

namespace gpsig {

struct LrTensGradArgs {
    const double* Z; int64_t T; int lt, E, d;          // tensors (lt, T, E, d): already scaled, columns as they come
    int64_t t0, nt;                                    // the tensors of this launch: t0 .. t0 + nt - 1
    const double* S;                                   // landmarks (c, d)
    const double* Wh;                                  // whitening (c, c): ft[j] = sum_i kx[i] Wh[i][j]
    int c, r, M, kind;
    double p0, p1;
    LrGradSketch sk[LR_FUSED_MAX_SKETCHES];
    const double* dPhi; int F;                         // upstream (T, F)
    double* gZ;                                        // (lt, T, E, d)
    double* part;                                      // per-workgroup partial sums [grid][c d + c c + 1]: dS, dWh, d base parameter
};

// the spectral instance's arguments (p0 = Q, p1 = family): the trainable parameters (Q), (Q, d), (Q, d) on the device; dkx (lt nt E, c) out;
// part holds dWh alone ([grid][c c]); gZ, dS and the base parameter are not written
struct LrTensGradSpectralArgs : LrTensGradArgs {
    const double* alpha; const double* omega; const double* gamma;
    double* dkx;
};

constexpr int LR_TENS_GRAD_THREADS = 512;
constexpr int LR_TENS_GRAD_KW = 8, LR_TENS_GRAD_KS = 8;     // (i, j) pairs of dWh and (i, f) pairs of dS per thread: c <= 64, c d <= 4096

// doubles of a tensor's arrays: z, kx, ft per row; U and dU; every projection's output; two chain gradients; the per-wave sums
inline size_t lr_tens_grad_lds_bytes(int c, int r, int d, int lt, int E, int M) {
    const size_t rows = size_t(lt) * E, w = size_t(c > r ? c : r), ns = size_t(M) * (M - 1) / 2;
    return sizeof(double) * (rows * (size_t(d) + 2 * size_t(c)) + 2 * size_t(lt) * c + ns * size_t(r) + 2 * w + 16);
}

template <bool SPEC, typename Args>
__device__ __forceinline__ void lr_tens_features_grad_body(const Args& A) {
    constexpr int THREADS = LR_TENS_GRAD_THREADS, NW = THREADS / 64;
    extern __shared__ double lrt_lds[];
    const int c = A.c, r = A.r, lt = A.lt, E = A.E, d = A.d, M = A.M;
    const int rows = lt * E, w = c > r ? c : r, ns = M * (M - 1) / 2;
    double* const zs = lrt_lds;                        // [rows][d]
    double* const kx = zs + rows * d;                  // [rows][c]   kappa; later dkx; later dkx wy
    double* const ft = kx + rows * c;                  // [rows][c]   whitened; later dft; later dkx ws
    double* const U = ft + rows * c;                   // [lt][c]     (U and dU together, rows * c at most: later dkx wx)
    double* const dU = U + lt * c;                     // [lt][c]
    double* const Rs = dU + lt * c;                    // [ns][r]     the projections' outputs, level by level
    double* const dRa = Rs + ns * r;                   // [w]
    double* const dRb = dRa + w;                       // [w]
    double* const red = dRb + w;                       // [NW]
    const lr_const_ptr<double> Sg = lr_as_const(A.S);
    const lr_const_ptr<double> Whg = lr_as_const(A.Wh);

    double accW[LR_TENS_GRAD_KW], accS[LR_TENS_GRAD_KS], accP = 0.0;   // this workgroup's sums over its tensors: dWh, dS, d base parameter
#pragma unroll
    for (int k = 0; k < LR_TENS_GRAD_KW; ++k) accW[k] = 0.0;
#pragma unroll
    for (int k = 0; k < LR_TENS_GRAD_KS; ++k) accS[k] = 0.0;

    for (int64_t t = A.t0 + blockIdx.x; t < A.t0 + A.nt; t += gridDim.x) {
        const double* g = A.dPhi + t * int64_t(A.F);
        __syncthreads();                                 // (the previous tensor's readers are done)
        // ---- forward again
        for (int q = threadIdx.x; q < rows * d; q += THREADS) {
            const int row = q / d, f = q - row * d;
            const int k = row / E, e = row - k * E;
            zs[q] = A.Z[((int64_t(k) * A.T + t) * E + e) * d + f];
        }
        __syncthreads();
        for (int q = threadIdx.x; q < rows * c; q += THREADS) {
            const int row = q / c, i = q - row * c;
            if constexpr (lr_tens_kx<Args>::value) {     // kappa from memory (lr_kx_inst.hip: a SPEC instance, dkx out)
                const int k = row / E, e = row - k * E;
                kx[q] = A.kzs[((int64_t(k) * A.T + t) * E + e) * c + i];
            } else if constexpr (SPEC) {
                kx[q] = spectral_pair(lr_as_const(A.alpha), lr_as_const(A.omega), lr_as_const(A.gamma), d, int(A.p0), int(A.p1), d,
                                      [&](int f) { return zs[row * d + f]; }, [&](int f) { return Sg[size_t(i) * d + f]; });
            } else {
                double ip = 0.0, xs = 0.0, ss = 0.0;
                for (int f = 0; f < d; ++f) {
                    const double x = zs[row * d + f], y = Sg[size_t(i) * d + f];
                    ip = fma(x, y, ip); xs = fma(x, x, xs); ss = fma(y, y, ss);
                }
                kx[q] = base_eval<double>(A.kind, ip, xs, ss, A.p0, A.p1);
            }
        }
        __syncthreads();
        for (int q = threadIdx.x; q < rows * c; q += THREADS) {
            const int row = q / c, j = q - row * c;
            double acc = 0.0;
            for (int i = 0; i < c; ++i) acc = fma(kx[row * c + i], Whg[size_t(i) * c + j], acc);
            ft[q] = acc;
        }
        __syncthreads();
        for (int q = threadIdx.x; q < lt * c; q += THREADS) {
            const int k = q / c, j = q - k * c;
            U[q] = E == 2 ? ft[(k * 2 + 1) * c + j] - ft[(k * 2) * c + j] : ft[k * c + j];
        }
        __syncthreads();
        // the chains of levels 2 .. M, every projection's output kept: level i's are Rs[(i-1)(i-2)/2 ..], its components U[i(i-1)/2 ..]
        for (int i = 2; i <= M; ++i) {
            const int k0 = i * (i - 1) / 2, s0 = (i - 1) * (i - 2) / 2;
            for (int j = 1; j < i; ++j) {
                const lr_const_ptr<int32_t> colptr = lr_as_const(A.sk[j - 1].colptr);
                const lr_const_ptr<LrEntry> ent = lr_as_const(A.sk[j - 1].ent);
                const double* Uk = U + (k0 + j) * c;
                const double* R = j == 1 ? U + k0 * c : Rs + (s0 + j - 2) * r;
                double* out = Rs + (s0 + j - 1) * r;
                for (int jo = threadIdx.x; jo < r; jo += THREADS) {
                    double acc = 0.0;
                    for (int e = colptr[jo]; e < colptr[jo + 1]; ++e) acc = fma(ent[e].val * Uk[ent[e].i1], R[ent[e].i2], acc);
                    out[jo] = acc;
                }
                __syncthreads();
            }
        }
        // ---- the chains backwards: dU
        for (int j = threadIdx.x; j < c; j += THREADS) dU[j] = g[1 + j];                 // level 1: Phi_1 = U[0]
        for (int i = 2; i <= M; ++i) {
            const int k0 = i * (i - 1) / 2, s0 = (i - 1) * (i - 2) / 2;
            const double* gl = g + 1 + c + (i - 2) * r;
            double* dcur = dRa;                          // d of the step's output R'
            double* dnxt = dRb;
            for (int jo = threadIdx.x; jo < r; jo += THREADS) dcur[jo] = gl[jo];
            __syncthreads();
            for (int j = i - 1; j >= 1; --j) {
                const LrGradSketch& sk = A.sk[j - 1];
                const lr_const_ptr<int32_t> ptr1 = lr_as_const(sk.ptr1), ptr2 = lr_as_const(sk.ptr2);
                const lr_const_ptr<LrEntry> ent1 = lr_as_const(sk.ent1), ent2 = lr_as_const(sk.ent2);
                const double* Uk = U + (k0 + j) * c;
                const double* R = j == 1 ? U + k0 * c : Rs + (s0 + j - 2) * r;
                const int wi = j == 1 ? c : r;           // width of the step's input R
                double* dUk = dU + (k0 + j) * c;
                double* dR = j == 1 ? dU + k0 * c : dnxt;   // the chain starts at U[k0]: its gradient is that row of dU
                for (int q = threadIdx.x; q < c + wi; q += THREADS) {
                    double acc = 0.0;
                    if (q < c) {                         // dU[k][i1] = sum val R[i2] dR'[j]: entries (val, i2, j) of row i1
                        for (int e = ptr1[q]; e < ptr1[q + 1]; ++e) acc = fma(ent1[e].val * R[ent1[e].i1], dcur[ent1[e].i2], acc);
                        dUk[q] = acc;
                    } else {                             // dR[i2] = sum val U[k][i1] dR'[j]: entries (val, i1, j) of row i2
                        const int i2 = q - c;
                        for (int e = ptr2[i2]; e < ptr2[i2 + 1]; ++e) acc = fma(ent2[e].val * Uk[ent2[e].i1], dcur[ent2[e].i2], acc);
                        dR[i2] = acc;
                    }
                }
                __syncthreads();
                double* tmp = dcur; dcur = dnxt; dnxt = tmp;
            }
        }
        __syncthreads();                                 // (M == 1: level 1's row of dU)
        // ---- back through the difference over e and the whitening: dft -> ft
        for (int q = threadIdx.x; q < rows * c; q += THREADS) {
            const int row = q / c, j = q - row * c;
            const int k = row / E, e = row - k * E;
            const double v = dU[k * c + j];
            ft[q] = (E == 2 && e == 0) ? -v : v;
        }
        __syncthreads();
        // dWh[i][j] += sum_row kx[row][i] dft[row][j]
#pragma unroll
        for (int k = 0; k < LR_TENS_GRAD_KW; ++k) {
            const int q = k * THREADS + threadIdx.x;
            if (q < c * c) {
                const int i = q / c, j = q - i * c;
                double acc = 0.0;
                for (int row = 0; row < rows; ++row) acc = fma(kx[row * c + i], ft[row * c + j], acc);
                accW[k] += acc;
            }
        }
        __syncthreads();
        // dkx[row][i] = sum_j dft[row][j] Wh[i][j] -> kx
        for (int q = threadIdx.x; q < rows * c; q += THREADS) {
            const int row = q / c, i = q - row * c;
            double acc = 0.0;
            for (int j = 0; j < c; ++j) acc = fma(ft[row * c + j], Whg[size_t(i) * c + j], acc);
            kx[q] = acc;
        }
        __syncthreads();
        if constexpr (SPEC) {                            // dkx of this tensor's points out; the spectral cross op's reverse kernels take it from here
            const int64_t tl = t - A.t0;
            for (int q = threadIdx.x; q < rows * c; q += THREADS) {
                const int row = q / c, i = q - row * c;
                const int k = row / E, e = row - k * E;
                A.dkx[((int64_t(k) * A.nt + tl) * E + e) * c + i] = kx[q];
            }
            continue;                                    // (the loop's first barrier orders these reads before kx is written again)
        } else {
            // through the base kernel: d kappa / dz = wy S_i + wx z,  d kappa / dS_i = wy z + ws S_i  (BaseGrad of grad_core.hpp)
            //   kx <- dkx wy,  ft <- dkx ws,  U.. <- dkx wx
            double* const wxb = U;
            for (int q = threadIdx.x; q < rows * c; q += THREADS) {
                const int row = q / c, i = q - row * c;
                double ip = 0.0, xs = 0.0, ss = 0.0;
                for (int f = 0; f < d; ++f) {
                    const double x = zs[row * d + f], y = Sg[size_t(i) * d + f];
                    ip = fma(x, y, ip); xs = fma(x, x, xs); ss = fma(y, y, ss);
                }
                const BaseGrad bg = base_eval_grad(A.kind, ip, xs, ss, A.p0, A.p1);
                const double dk = kx[q];
                kx[q] = dk * (bg.cy - bg.cd);
                ft[q] = dk * (bg.cx2 + bg.cd);
                wxb[q] = dk * (bg.cx + bg.cd);
                accP = fma(dk, bg.dp0, accP);
            }
            __syncthreads();
            // dz[row][f] = sum_i kx[row][i] S_i[f] + z[row][f] sum_i wx[row][i]
            for (int q = threadIdx.x; q < rows * d; q += THREADS) {
                const int row = q / d, f = q - row * d;
                const int k = row / E, e = row - k * E;
                double ax = 0.0, acc = 0.0;
                for (int i = 0; i < c; ++i) {
                    ax += wxb[row * c + i];
                    acc = fma(kx[row * c + i], Sg[size_t(i) * d + f], acc);
                }
                A.gZ[((int64_t(k) * A.T + t) * E + e) * d + f] = fma(ax, zs[q], acc);
            }
            // dS[i][f] += sum_row kx[row][i] z[row][f] + S_i[f] sum_row ft[row][i]
#pragma unroll
            for (int k = 0; k < LR_TENS_GRAD_KS; ++k) {
                const int q = k * THREADS + threadIdx.x;
                if (q < c * d) {
                    const int i = q / d, f = q - i * d;
                    double a1 = 0.0, a2 = 0.0;
                    for (int row = 0; row < rows; ++row) {
                        a1 = fma(kx[row * c + i], zs[row * d + f], a1);
                        a2 += ft[row * c + i];
                    }
                    accS[k] += fma(a2, Sg[size_t(i) * d + f], a1);
                }
            }
        }
    }
    // ---- this workgroup's partial sums
    if constexpr (SPEC) {
        double* part = A.part + int64_t(blockIdx.x) * (int64_t(c) * c);
#pragma unroll
        for (int k = 0; k < LR_TENS_GRAD_KW; ++k) {
            const int q = k * THREADS + threadIdx.x;
            if (q < c * c) part[q] = accW[k];
        }
    } else {
        double* part = A.part + int64_t(blockIdx.x) * (int64_t(c) * d + int64_t(c) * c + 1);
#pragma unroll
        for (int k = 0; k < LR_TENS_GRAD_KS; ++k) {
            const int q = k * THREADS + threadIdx.x;
            if (q < c * d) part[q] = accS[k];
        }
#pragma unroll
        for (int k = 0; k < LR_TENS_GRAD_KW; ++k) {
            const int q = k * THREADS + threadIdx.x;
            if (q < c * c) part[int64_t(c) * d + q] = accW[k];
        }
        __syncthreads();
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) accP += __shfl_xor(accP, o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = accP;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int w2 = 0; w2 < NW; ++w2) s += red[w2];
            part[int64_t(c) * d + int64_t(c) * c] = s;
        }
    }
}

// (no templates: defined once, in lr_grad_api.hip; lr_kx_inst.hip takes the body alone)
#ifndef GPSIG_LR_BODIES_ONLY
__global__ __launch_bounds__(LR_TENS_GRAD_THREADS) void lr_tens_features_grad_kernel(LrTensGradArgs A) { lr_tens_features_grad_body<false>(A); }

// SignatureSpectral: kappa by spectral_pair, dkx out instead of the base-kernel phase (above)
__global__ __launch_bounds__(LR_TENS_GRAD_THREADS) void lr_tens_features_grad_spectral_kernel(LrTensGradSpectralArgs A) { lr_tens_features_grad_body<true>(A); }
#endif

}  // namespace gpsig
