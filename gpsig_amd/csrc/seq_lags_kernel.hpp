// seq_lags_kernel.hpp -- add_lags_to_sequences (gpsig/lags.py:41-63) for a ragged batch, each sequence on ITS OWN time axis, forward and
// reverse: the training path's lag op behind gpsig_seq_lags_ragged_dev / gpsig_seq_lags_ragged_grad (seq_lags_inst.hip).  float64, device
// pointers.
//
//   X (N, L, d), lengths (N) int32 clamped to [1, L] here, lags (p) on the device  ->  out (N, L, p + 1, d)
//   sequence n is X[n, :len]: its axis is i / (len - 1), the query of lag j at observation t is tq = max(t / (len - 1) - lag_j, 0)  (lags.py:56-57),
//   the bracket is left = the last i with not (i / (len - 1) - tq > jitter), right = min(left + 1, len - 1)                      (lags.py:20-23),
//   the value is x_l + (tq - t_l) (x_r - x_l) / (t_r - t_l)                                                                     (lags.py:32)
//   -- the operations of scaled_point (aux_kernels.hpp) on an axis of len points, so that the evaluation side's kernels and this op agree.
//   t >= len: every copy repeats output row len - 1 (the pool the landmarks are gathered from holds real points only); the input rows at or beyond
//   len are never read.  len == 1: no axis (0 / 0 in the reference); the lagged copies are the point itself and the lags receive no gradient.
//
// The bracket is found arithmetically: floor((tq + jitter) (len - 1)) and one step up or down by the reference's own predicate -- the product's
// rounding moves the floor by one at most.  (scaled_point searches the axis from its end: O(L) per element.)
//
// Reverse: one workgroup per sequence, one thread per column f, which owns dX[n, :, f]: it writes copy 0's gradient (rows >= len folded into row
// len - 1, exact zeros behind), then walks each lag's queries in time order and adds (1 - w) g and w g to the bracket's rows, w = (tq - t_l) /
// (t_r - t_l).  No atomics: the same bits at every call.  dlags[j] = - sum g (x_r - x_l) / (t_r - t_l) over the queries the clamp at 0 did not
// catch: per thread in time order, across the workgroup's threads in thread order through the LDS (`part`, one value per (sequence, lag)), across
// sequences in order by seq_lags_reduce_kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gpsig {

constexpr int SEQ_LAGS_THREADS = 256;      // most threads of a reverse workgroup (64 for d <= 64, 128 for d <= 128)
constexpr int SEQ_LAGS_MAX_GRID = 1 << 16;

struct SeqLagsArgs {
    const double* X;            // (N, L, d)
    const int32_t* lengths;     // (N)
    const double* lags;         // (p)
    int64_t N;
    int L, d, p;
    double jitter;
    double* out;                // forward: (N, L, p + 1, d)
    const double* G;            // reverse: d out
    double* dX;                 //          (N, L, d), every element written
    double* part;               //          (N, p) partial sums of dlags
};

__device__ __forceinline__ int seq_lags_len(const SeqLagsArgs& A, int64_t n) {
    const int len = A.lengths[n];
    return len < 1 ? 1 : (len > A.L ? A.L : len);
}

// the bracket of (observation t, lag) on an axis of len >= 2 points; *free_q: the clamp at 0 did not catch the query
__device__ __forceinline__ int seq_lags_bracket(int len, int t, double lag, double jitter, double* tq_out, bool* free_q) {
    const double denom = double(len - 1);
    const double a = double(t) / denom - lag;
    const double tq = fmax(a, 0.0);                                          // lags.py:57
    int i = int(floor((tq + jitter) * denom));
    i = i < 0 ? 0 : (i > len - 1 ? len - 1 : i);
    if (double(i) / denom - tq > jitter) --i;                                // lags.py:20-22 (never true at i = 0: tq >= 0)
    else if (i + 1 < len && !(double(i + 1) / denom - tq > jitter)) ++i;
    *tq_out = tq;
    *free_q = a > 0.0;
    return i;
}

__global__ __launch_bounds__(256) void seq_lags_fwd_kernel(SeqLagsArgs A) {
    const int d = A.d, p1 = A.p + 1, L = A.L;
    const int64_t total = A.N * L * p1 * d;
    for (int64_t idx = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; idx < total; idx += int64_t(gridDim.x) * blockDim.x) {
        int64_t q = idx / d;
        const int f = int(idx - q * d);
        const int j = int(q % p1);
        q /= p1;
        const int t = int(q % L);
        const int64_t n = q / L;
        const int len = seq_lags_len(A, n);
        const int te = t < len ? t : len - 1;
        const double* Xn = A.X + n * int64_t(L) * d;
        double v;
        if (j == 0 || len == 1) {
            v = Xn[int64_t(te) * d + f];
        } else {
            double tq;
            bool free_q;
            const int left = seq_lags_bracket(len, te, A.lags[j - 1], A.jitter, &tq, &free_q);
            const int right = left + 1 < len ? left + 1 : len - 1;                                       // lags.py:23
            const double denom = double(len - 1);
            const double xl = Xn[int64_t(left) * d + f], xr = Xn[int64_t(right) * d + f];
            const double tl = double(left) / denom, tr = double(right) / denom;
            v = xl + (tq - tl) * (xr - xl) / (tr - tl);                                                  // lags.py:32
        }
        A.out[idx] = v;
    }
}

__global__ __launch_bounds__(SEQ_LAGS_THREADS) void seq_lags_grad_kernel(SeqLagsArgs A) {
    __shared__ double sh[SEQ_LAGS_THREADS];
    const int d = A.d, p = A.p, p1 = p + 1, L = A.L;
    for (int64_t n = blockIdx.x; n < A.N; n += gridDim.x) {
        const int len = seq_lags_len(A, n);
        const double denom = double(len - 1);
        const double* Xn = A.X + n * int64_t(L) * d;
        const double* Gn = A.G + n * int64_t(L) * p1 * d;
        double* dXn = A.dX + n * int64_t(L) * d;
        for (int j = 0; j <= p; ++j) {
            const double lag = j ? A.lags[j - 1] : 0.0;
            double dl = 0.0;
            for (int f = threadIdx.x; f < d; f += blockDim.x) {
                double gt = 0.0;                                                                         // output rows >= len - 1 are one value
                for (int t = len - 1; t < L; ++t) gt += Gn[(int64_t(t) * p1 + j) * d + f];
                if (j == 0) {
                    for (int s = 0; s < len - 1; ++s) dXn[int64_t(s) * d + f] = Gn[int64_t(s) * p1 * d + f];
                    dXn[int64_t(len - 1) * d + f] = gt;
                    for (int s = len; s < L; ++s) dXn[int64_t(s) * d + f] = 0.0;
                } else if (len == 1) {
                    dXn[f] += gt;
                } else {
                    for (int t = 0; t < len; ++t) {
                        const double g = t < len - 1 ? Gn[(int64_t(t) * p1 + j) * d + f] : gt;
                        double tq;
                        bool free_q;
                        const int left = seq_lags_bracket(len, t, lag, A.jitter, &tq, &free_q);
                        const int right = left + 1 < len ? left + 1 : len - 1;
                        const double tl = double(left) / denom, tr = double(right) / denom;
                        const double w = (tq - tl) / (tr - tl);
                        dXn[int64_t(left) * d + f] += (1.0 - w) * g;
                        dXn[int64_t(right) * d + f] += w * g;
                        if (free_q) dl -= g * (Xn[int64_t(right) * d + f] - Xn[int64_t(left) * d + f]) / (tr - tl);
                    }
                }
            }
            if (j > 0) {
                sh[threadIdx.x] = dl;
                __syncthreads();
                if (threadIdx.x == 0) {
                    double s = 0.0;
                    for (int k = 0; k < int(blockDim.x); ++k) s += sh[k];
                    A.part[n * p + (j - 1)] = s;
                }
                __syncthreads();
            }
        }
    }
}

// dlags[j] = sum_n part[n][j], in order
__global__ void seq_lags_reduce_kernel(const double* __restrict__ part, int64_t N, int p, double* __restrict__ dlags) {
    const int j = threadIdx.x;
    if (j < p) {
        double s = 0.0;
        for (int64_t n = 0; n < N; ++n) s += part[n * p + j];
        dlags[j] = s;
    }
}

}  // namespace gpsig
