// spectral_cross_api.hip -- SignatureSpectral's Nystrom cross matrix kappa(points, landmarks) (low_rank_calculations.py:59, kernels.py:921-942):
//
//   * the multi-pass low-rank feature route's cross kernels for this family (lowrank_kernels.hpp has the run-time family ones), and
//   * the training path's op with its reverse pass, the parameters read from DEVICE memory (they change at every optimiser step):
//         gpsig_spectral_cross        K (n, c) = kappa(P, S)
//         gpsig_spectral_cross_grad   G = dL/dK (n, c) -> dP (n, d), dS (c, d), dalpha (Q), domega (Q, d), dgamma (Q, d)
//     The reverse pass: dP by one thread per point (landmarks wave-uniform); dS and the parameters -- sums over every pair -- by
//     workgroups of (landmark, slice of the points) that reduce in LDS into per-workgroup partial sums, combined by a second pass in a
//     fixed order: no atomics, two runs agree bit for bit.  Per-pair arithmetic: spectral_pair.hpp.
//     These kernels serve d <= 32.  Beyond, up to 4096 columns and 64 landmarks, the two entry points hand over -- before anything else -- to the
//     kernels on the float64 matrix cores (lr_cross_spectral_inst.hip, lr_cross_spectral_kernel.hpp).
//   * spectral_cross_grad_launch: the same reverse pass for the low-rank training path's spectral entry points (lr_grad_api.hip), which
//     hand over dkxs as G, partial sums in a buffer of their own and, for the second and later chunks of sequences, add to the outputs.
//     spectral_cross_grad_len_launch: the same for sequences with per-sequence lengths, whose padded points take no part.
#include "ctx.hpp"
#include "launchers.hpp"
#include "lr_fused_args.hpp"

#include <type_traits>
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

// ... of N sequences in rows of L points (n = N L), of which sequence n has lengths[n]: the points beyond take no part
struct SpecCrossLenArgs : SpecCrossArgs { int L; const int32_t* lengths; };
template <typename Args>
__device__ __forceinline__ bool spec_cross_live(const Args& A, int64_t pt) {
    if constexpr (std::is_same<Args, SpecCrossLenArgs>::value) {
        const int64_t n = pt / A.L;
        const int v = A.lengths[n];
        return int(pt - n * A.L) < (v < 1 ? 1 : v);             // (t < L always: the upper clamp of the length changes nothing)
    } else {
        return true;
    }
}

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
#include "spectral_cross_points_body.inc"
}
template <int DMAX>
__global__ __launch_bounds__(SC_THREADS) void spectral_cross_grad_points_len_kernel(SpecCrossLenArgs A) {
#include "spectral_cross_points_body.inc"
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
#include "spectral_cross_landmarks_body.inc"
}
template <int DMAX>
__global__ __launch_bounds__(SC_THREADS) void spectral_cross_grad_landmarks_len_kernel(SpecCrossLenArgs A) {
#include "spectral_cross_landmarks_body.inc"
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

// the three launches of the reverse pass on a filled argument block (SpecCrossArgs, or SpecCrossLenArgs: the lengths-aware kernels)
template <typename Args>
static int cross_grad_run(hipStream_t stream, Args A, double* dS, double* dalpha, double* domega, double* dgamma) {
    constexpr bool LEN = std::is_same<Args, SpecCrossLenArgs>::value;
    const int d = A.d;
    A.nchunk = cross_grad_slices(A.n);
    A.nv = d + A.Q * (1 + 2 * d);
    const unsigned gp = unsigned(grid_for(A.n, SC_THREADS));
    const dim3 gl(unsigned(A.nchunk), unsigned(A.c));
    auto run = [&](auto dmax) {
        constexpr int DMAX = decltype(dmax)::value;
        if constexpr (LEN) {
            hipLaunchKernelGGL(spectral_cross_grad_points_len_kernel<DMAX>, dim3(gp), dim3(SC_THREADS), 0, stream, A);
            hipLaunchKernelGGL(spectral_cross_grad_landmarks_len_kernel<DMAX>, gl, dim3(SC_THREADS), 0, stream, A);
        } else {
            hipLaunchKernelGGL(spectral_cross_grad_points_kernel<DMAX>, dim3(gp), dim3(SC_THREADS), 0, stream, A);
            hipLaunchKernelGGL(spectral_cross_grad_landmarks_kernel<DMAX>, gl, dim3(SC_THREADS), 0, stream, A);
        }
    };
    if (d <= 8) run(std::integral_constant<int, 8>());
    else if (d <= 16) run(std::integral_constant<int, 16>());
    else run(std::integral_constant<int, 32>());
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return int(e);
    const unsigned outs = unsigned(int64_t(A.c) * d + int64_t(A.Q) * (1 + 2 * d));
    hipLaunchKernelGGL(spectral_cross_grad_combine_kernel, dim3(outs), dim3(SC_THREADS), 0, stream, static_cast<const SpecCrossArgs&>(A), dS, dalpha,
                       domega, dgamma);
    return int(hipGetLastError());
}

int spectral_cross_grad_launch(hipStream_t stream, int Q, int family, int d, const double* P, int64_t n, const double* S, int cc,
                               const double* alpha, const double* omega, const double* gamma, const double* G, double* dP, double* part,
                               double* dS, double* dalpha, double* domega, double* dgamma, bool accumulate) {
    SpecCrossArgs A{};
    A.P = P; A.n = n; A.S = S; A.c = cc; A.d = d; A.Q = Q; A.family = family; A.alpha = alpha; A.omega = omega; A.gamma = gamma;
    A.G = G; A.dP = dP;
    A.part = part;
    A.accumulate = accumulate ? 1 : 0;
    return cross_grad_run(stream, A, dS, dalpha, domega, dgamma);
}

int spectral_cross_grad_len_launch(hipStream_t stream, int Q, int family, int d, const double* P, int64_t N, int L, const int32_t* lengths,
                                   const double* S, int cc, const double* alpha, const double* omega, const double* gamma, const double* G, double* dP,
                                   double* part, double* dS, double* dalpha, double* domega, double* dgamma, bool accumulate) {
    SpecCrossLenArgs A{};
    A.P = P; A.n = N * L; A.S = S; A.c = cc; A.d = d; A.Q = Q; A.family = family; A.alpha = alpha; A.omega = omega; A.gamma = gamma;
    A.G = G; A.dP = dP;
    A.part = part;
    A.accumulate = accumulate ? 1 : 0;
    A.L = L; A.lengths = lengths;
    return cross_grad_run(stream, A, dS, dalpha, domega, dgamma);
}

}  // namespace gpsig

extern "C" {

int gpsig_spectral_cross(gpsig_ctx* c, int32_t Q, int32_t family, int32_t d, const double* P, int64_t n, const double* S, int32_t cc,
                         const double* alpha, const double* omega, const double* gamma, double* K) {
    if (c && d > SPECTRAL_STRIDE) return spectral_cross_wide(c, Q, family, d, P, n, S, cc, alpha, omega, gamma, K);       // lr_cross_spectral_inst.hip
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
    if (c && d > SPECTRAL_STRIDE) return spectral_cross_wide_grad(c, Q, family, d, P, n, S, cc, alpha, omega, gamma, G, dP, dS, dalpha, domega, dgamma);
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
