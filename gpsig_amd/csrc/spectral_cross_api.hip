// spectral_cross_api.hip -- SignatureSpectral's Nystrom cross matrix kappa(points, landmarks) (low_rank_calculations.py:59, kernels.py:921-942):
//
//   * the multi-pass low-rank feature route's cross kernels for this family (lowrank_kernels.hpp has the run-time family ones), and
//   * the training path's op with its reverse pass, the parameters read from DEVICE memory (they change at every optimiser step):
//         gpsig_spectral_cross        K (n, c) = kappa(P, S)
//         gpsig_spectral_cross_grad   G = dL/dK (n, c) -> dP (n, d), dS (c, d), dalpha (Q), domega (Q, d), dgamma (Q, d)
//     The reverse pass: dP by one thread per point (landmarks wave-uniform); dS and the parameters -- sums over every pair -- by
//     workgroups of (landmark, slice of the points) that reduce in LDS into per-workgroup partial sums, combined by a second pass in a
//     fixed order: no atomics, two runs agree bit for bit.  Per-pair arithmetic: spectral_pair.hpp.
//   * spectral_cross_grad_launch: the same reverse pass for the low-rank training path's spectral entry points (lr_grad_api.hip), which
//     hand over dkxs as G, partial sums in a buffer of their own and, for the second and later chunks of sequences, add to the outputs.
#include "ctx.hpp"
#include "lr_fused_args.hpp"
#include "spectral_pair.hpp"

using namespace gpsig;

namespace gpsig {

namespace {

// Nystrom cross matrix of sequences: out[(n*L + t)][i] = kappa(x~[n][t], S[i])   (the spectral kernel takes no scaling: x~ = x)
__global__ void lr_seq_cross_spectral_kernel(const double* __restrict__ X, int64_t N, int L, ScaleParams P, const double* __restrict__ S, int c,
                                             int Q, int family, const double* __restrict__ spec, double* __restrict__ out) {
    const int d_eff = P.d_eff();
    const int64_t total = N * L * c;
    for (int64_t q = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; q < total; q += int64_t(gridDim.x) * blockDim.x) {
        const int i = int(q % c);
        const int64_t pt = q / c;
        const int64_t n = pt / L;
        const int t = int(pt % L);
        const double* Xn = X + n * int64_t(L) * P.d_in;
        out[q] = spectral_pair(spec, spec + Q, spec + Q + Q * SPECTRAL_STRIDE, SPECTRAL_STRIDE, Q, family, d_eff,
                               [&](int f) { return scaled_point<double>(Xn, L, t, f, P); }, [&](int f) { return S[i * d_eff + f]; });
    }
}

// the same for tensor components Z (rows, d') as the caller gives them
__global__ void lr_tens_cross_spectral_kernel(const double* __restrict__ Z, int64_t rows, ScaleParams P, const double* __restrict__ S, int c,
                                              int Q, int family, const double* __restrict__ spec, double* __restrict__ out) {
    const int d_eff = P.d_eff();
    const int64_t total = rows * c;
    for (int64_t q = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; q < total; q += int64_t(gridDim.x) * blockDim.x) {
        const int i = int(q % c);
        const int64_t r = q / c;
        out[q] = spectral_pair(spec, spec + Q, spec + Q + Q * SPECTRAL_STRIDE, SPECTRAL_STRIDE, Q, family, d_eff,
                               [&](int f) { return Z[r * d_eff + f]; }, [&](int f) { return S[i * d_eff + f]; });
    }
}

struct SpecCrossArgs {
    const double* P; int64_t n;
    const double* S; int c;
    int d, Q, family;
    const double* alpha; const double* omega; const double* gamma;      // (Q), (Q, d), (Q, d)
    const double* G;                                                    // (n, c)
    double* dP;
    double* part; int nchunk, nv;                                       // partial sums: (c * nchunk, nv), nv = d + Q (1 + 2d)
    int accumulate;                                                     // the combine pass adds dS and the parameters' sums to its outputs
};

constexpr int SC_THREADS = 256;

__global__ __launch_bounds__(SC_THREADS) void spectral_cross_kernel(SpecCrossArgs A, double* __restrict__ K) {
    const int d = A.d;
    const int64_t total = A.n * A.c;
    for (int64_t q = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; q < total; q += int64_t(gridDim.x) * blockDim.x) {
        const int i = int(q % A.c);
        const int64_t pt = q / A.c;
        K[q] = spectral_pair(A.alpha, A.omega, A.gamma, d, A.Q, A.family, d, [&](int f) { return A.P[pt * d + f]; },
                             [&](int f) { return A.S[int64_t(i) * d + f]; });
    }
}

// dP: thread = point, the landmarks and the parameters wave-uniform (scalar loads); DMAX >= d columns in registers
template <int DMAX>
__global__ __launch_bounds__(SC_THREADS) void spectral_cross_grad_points_kernel(SpecCrossArgs A) {
    const int d = A.d, Q = A.Q;
    const lr_const_ptr<double> al = lr_as_const(A.alpha), om = lr_as_const(A.omega), ga = lr_as_const(A.gamma);
    for (int64_t pt = blockIdx.x * int64_t(SC_THREADS) + threadIdx.x; pt < A.n; pt += int64_t(gridDim.x) * SC_THREADS) {
        double x[DMAX], gx[DMAX];
#pragma unroll
        for (int f = 0; f < DMAX; ++f) {
            x[f] = f < d ? A.P[pt * d + f] : 0.0;
            gx[f] = 0.0;
        }
        for (int i = 0; i < A.c; ++i) {
            const lr_const_ptr<double> y = lr_as_const(A.S) + size_t(i) * d;
            const double g = A.G[pt * A.c + i];
            for (int q = 0; q < Q; ++q) {
                double w1 = 0.0, w2 = 0.0;
#pragma unroll
                for (int f = 0; f < DMAX; ++f)
                    if (f < d) {
                        const double diff = x[f] - y[f];
                        const double gd = ga[q * d + f] * diff;
                        w1 = fma(gd, gd, w1);
                        w2 = fma(om[q * d + f], diff, w2);
                    }
                const SpectralTerm t = spectral_term(al[q], w1, w2, spectral_gauss(A.family, q, Q));
                const double c1 = 2 * g * t.d_w1, c2 = g * t.d_w2;
#pragma unroll
                for (int f = 0; f < DMAX; ++f)
                    if (f < d) {
                        const double diff = x[f] - y[f], gq = ga[q * d + f];
                        gx[f] += c1 * gq * gq * diff + c2 * om[q * d + f];
                    }
            }
        }
#pragma unroll
        for (int f = 0; f < DMAX; ++f)
            if (f < d) A.dP[pt * d + f] = gx[f];
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// dS and the parameters: workgroup (slice, landmark i); a thread takes the points slice * 256 + lane + k * nchunk * 256.  Per component q
// the 1 + 2d sums are reduced over the wavefront (butterfly), then over the four wavefronts in order; dS[i] at the end the same way.
template <int DMAX>
__global__ __launch_bounds__(SC_THREADS) void spectral_cross_grad_landmarks_kernel(SpecCrossArgs A) {
    constexpr int NW = SC_THREADS / 64;
    constexpr int W = 1 + 2 * DMAX;
    __shared__ double red[NW][W];
    const int d = A.d, Q = A.Q, i = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const lr_const_ptr<double> al = lr_as_const(A.alpha), om = lr_as_const(A.omega), ga = lr_as_const(A.gamma);
    const lr_const_ptr<double> y = lr_as_const(A.S) + size_t(i) * d;
    double* part = A.part + (size_t(i) * A.nchunk + blockIdx.x) * A.nv;
    const int64_t step = int64_t(A.nchunk) * SC_THREADS;
    double gs[DMAX];
#pragma unroll
    for (int f = 0; f < DMAX; ++f) gs[f] = 0.0;
    for (int q = 0; q < Q; ++q) {
        const bool gauss = spectral_gauss(A.family, q, Q);
        double va = 0.0, vo[DMAX], vg[DMAX];
#pragma unroll
        for (int f = 0; f < DMAX; ++f) vo[f] = vg[f] = 0.0;
        for (int64_t pt = int64_t(blockIdx.x) * SC_THREADS + threadIdx.x; pt < A.n; pt += step) {
            const double g = A.G[pt * A.c + i];
            double x[DMAX];
            double w1 = 0.0, w2 = 0.0;
#pragma unroll
            for (int f = 0; f < DMAX; ++f)
                if (f < d) {
                    x[f] = A.P[pt * d + f];
                    const double diff = x[f] - y[f];
                    const double gd = ga[q * d + f] * diff;
                    w1 = fma(gd, gd, w1);
                    w2 = fma(om[q * d + f], diff, w2);
                }
            const SpectralTerm t = spectral_term(al[q], w1, w2, gauss);
            const double c1 = 2 * g * t.d_w1, c2 = g * t.d_w2;
            va = fma(g, t.d_alpha, va);
#pragma unroll
            for (int f = 0; f < DMAX; ++f)
                if (f < d) {
                    const double diff = x[f] - y[f], gq = ga[q * d + f];
                    vo[f] = fma(c2, diff, vo[f]);
                    vg[f] = fma(c1 * gq, diff * diff, vg[f]);
                    gs[f] -= c1 * gq * gq * diff + c2 * om[q * d + f];
                }
        }
        va = wave_sum(va);
        if (lane == 0) red[wave][0] = va;
#pragma unroll
        for (int f = 0; f < DMAX; ++f)
            if (f < d) {
                const double so = wave_sum(vo[f]), sg = wave_sum(vg[f]);
                if (lane == 0) { red[wave][1 + f] = so; red[wave][1 + d + f] = sg; }
            }
        __syncthreads();
        if (threadIdx.x < 1 + 2 * d) {
            double s = 0.0;
            for (int w = 0; w < NW; ++w) s += red[w][threadIdx.x];
            part[d + q * (1 + 2 * d) + threadIdx.x] = s;
        }
        __syncthreads();
    }
#pragma unroll
    for (int f = 0; f < DMAX; ++f)
        if (f < d) {
            const double s = wave_sum(gs[f]);
            if (lane == 0) red[wave][f] = s;
        }
    __syncthreads();
    if (threadIdx.x < d) {
        double s = 0.0;
        for (int w = 0; w < NW; ++w) s += red[w][threadIdx.x];
        part[threadIdx.x] = s;
    }
}

// output o < c d: dS[o] = sum of the nchunk partials of landmark o / d; otherwise parameter v = o - c d: sum over every partial row
__global__ __launch_bounds__(SC_THREADS) void spectral_cross_grad_combine_kernel(SpecCrossArgs A, double* __restrict__ dS, double* __restrict__ dalpha,
                                                                               double* __restrict__ domega, double* __restrict__ dgamma) {
    __shared__ double red[SC_THREADS];
    const int d = A.d, o = blockIdx.x;
    const int64_t cd = int64_t(A.c) * d;
    int64_t b0, b1;
    int col;
    if (o < cd) {
        b0 = int64_t(o / d) * A.nchunk; b1 = b0 + A.nchunk; col = o % d;
    } else {
        b0 = 0; b1 = int64_t(A.c) * A.nchunk; col = d + int(o - cd);
    }
    double s = 0.0;
    for (int64_t b = b0 + threadIdx.x; b < b1; b += SC_THREADS) s += A.part[b * A.nv + col];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = SC_THREADS / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double* out;
    if (o < cd) {
        out = dS + o;
    } else {
        const int v = int(o - cd), w = 1 + 2 * d, q = v / w, k = v % w;
        out = k == 0 ? dalpha + q : (k <= d ? domega + q * d + k - 1 : dgamma + q * d + k - 1 - d);
    }
    *out = A.accumulate ? *out + red[0] : red[0];
}

int cross_check(gpsig_ctx* c, int Q, int family, int d, int64_t n, int cc) {
    if (!c) return GPSIG_ERR_INVALID;
    if (Q < 1 || Q > 64 || family < 0 || family > 2) return fail(c, GPSIG_ERR_INVALID, "spectral kernel: bad number of components / family");
    if (d < 1 || d > SPECTRAL_STRIDE) return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral base kernel is built for at most %d features", int(SPECTRAL_STRIDE));
    if (n < 0 || cc < 1) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    if (c->ptr_mode != GPSIG_PTR_DEVICE) return fail(c, GPSIG_ERR_INVALID, "the spectral cross op takes device pointers");
    HIPCHK(c, hipSetDevice(c->device));
    return GPSIG_OK;
}

}  // namespace

int lr_seq_cross_spectral_launch(hipStream_t stream, const double* X, int64_t N, int L, ScaleParams P, const double* S, int c, int Q, int family,
                                 const double* spec, double* out) {
    hipLaunchKernelGGL(lr_seq_cross_spectral_kernel, dim3(grid_for(N * L * c)), dim3(256), 0, stream, X, N, L, P, S, c, Q, family, spec, out);
    return int(hipGetLastError());
}

int lr_tens_cross_spectral_launch(hipStream_t stream, const double* Z, int64_t rows, ScaleParams P, const double* S, int c, int Q, int family,
                                  const double* spec, double* out) {
    hipLaunchKernelGGL(lr_tens_cross_spectral_kernel, dim3(grid_for(rows * c)), dim3(256), 0, stream, Z, rows, P, S, c, Q, family, spec, out);
    return int(hipGetLastError());
}


// at most 32 slices of the points per landmark: the partial sums stay small (c * 32 rows) and a workgroup a few hundred pairs deep
static int cross_grad_slices(int64_t n) {
    const int64_t slices = (n + SC_THREADS - 1) / SC_THREADS;
    return int(slices < 32 ? slices : 32);
}

size_t spectral_cross_grad_part_doubles(int64_t n, int cc, int d, int Q) {
    return size_t(cc) * size_t(cross_grad_slices(n)) * size_t(d + Q * (1 + 2 * d));
}

int spectral_cross_grad_launch(hipStream_t stream, int Q, int family, int d, const double* P, int64_t n, const double* S, int cc,
                               const double* alpha, const double* omega, const double* gamma, const double* G, double* dP, double* part,
                               double* dS, double* dalpha, double* domega, double* dgamma, bool accumulate) {
    SpecCrossArgs A{};
    A.P = P; A.n = n; A.S = S; A.c = cc; A.d = d; A.Q = Q; A.family = family; A.alpha = alpha; A.omega = omega; A.gamma = gamma;
    A.G = G; A.dP = dP;
    A.nchunk = cross_grad_slices(n);
    A.nv = d + Q * (1 + 2 * d);
    A.part = part;
    A.accumulate = accumulate ? 1 : 0;
    const unsigned gp = unsigned(grid_for(n, SC_THREADS));
    const dim3 gl(unsigned(A.nchunk), unsigned(cc));
    if (d <= 8) {
        hipLaunchKernelGGL(spectral_cross_grad_points_kernel<8>, dim3(gp), dim3(SC_THREADS), 0, stream, A);
        hipLaunchKernelGGL(spectral_cross_grad_landmarks_kernel<8>, gl, dim3(SC_THREADS), 0, stream, A);
    } else if (d <= 16) {
        hipLaunchKernelGGL(spectral_cross_grad_points_kernel<16>, dim3(gp), dim3(SC_THREADS), 0, stream, A);
        hipLaunchKernelGGL(spectral_cross_grad_landmarks_kernel<16>, gl, dim3(SC_THREADS), 0, stream, A);
    } else {
        hipLaunchKernelGGL(spectral_cross_grad_points_kernel<32>, dim3(gp), dim3(SC_THREADS), 0, stream, A);
        hipLaunchKernelGGL(spectral_cross_grad_landmarks_kernel<32>, gl, dim3(SC_THREADS), 0, stream, A);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return int(e);
    const unsigned outs = unsigned(int64_t(cc) * d + int64_t(Q) * (1 + 2 * d));
    hipLaunchKernelGGL(spectral_cross_grad_combine_kernel, dim3(outs), dim3(SC_THREADS), 0, stream, A, dS, dalpha, domega, dgamma);
    return int(hipGetLastError());
}

}  // namespace gpsig

extern "C" {

int gpsig_spectral_cross(gpsig_ctx* c, int32_t Q, int32_t family, int32_t d, const double* P, int64_t n, const double* S, int32_t cc,
                         const double* alpha, const double* omega, const double* gamma, double* K) {
    CHK(cross_check(c, Q, family, d, n, cc));
    if (n == 0) return GPSIG_OK;
    if (!P || !S || !alpha || !omega || !gamma || !K) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    SpecCrossArgs A{};
    A.P = P; A.n = n; A.S = S; A.c = cc; A.d = d; A.Q = Q; A.family = family; A.alpha = alpha; A.omega = omega; A.gamma = gamma;
    hipLaunchKernelGGL(spectral_cross_kernel, dim3(grid_for(n * cc)), dim3(SC_THREADS), 0, c->stream, A, K);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

int gpsig_spectral_cross_grad(gpsig_ctx* c, int32_t Q, int32_t family, int32_t d, const double* P, int64_t n, const double* S, int32_t cc,
                              const double* alpha, const double* omega, const double* gamma, const double* G, double* dP, double* dS,
                              double* dalpha, double* domega, double* dgamma) {
    CHK(cross_check(c, Q, family, d, n, cc));
    if (!dS || !dalpha || !domega || !dgamma) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    if (n == 0) {
        CHK(zero_async(c, dS, sizeof(double) * size_t(cc) * d));
        CHK(zero_async(c, dalpha, sizeof(double) * size_t(Q)));
        CHK(zero_async(c, domega, sizeof(double) * size_t(Q) * d));
        CHK(zero_async(c, dgamma, sizeof(double) * size_t(Q) * d));
        return GPSIG_OK;
    }
    if (!P || !S || !alpha || !omega || !gamma || !G || !dP) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    void* part;
    CHK(ensure(c, B_GR0, sizeof(double) * spectral_cross_grad_part_doubles(n, cc, d, Q) + 64, &part));
    const int rc = spectral_cross_grad_launch(c->stream, Q, family, d, P, n, S, cc, alpha, omega, gamma, G, dP, static_cast<double*>(part), dS,
                                              dalpha, domega, dgamma, false);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral cross reverse pass: %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

}  // extern "C"
