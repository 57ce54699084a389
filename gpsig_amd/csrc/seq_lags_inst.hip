// seq_lags_inst.hip -- gpsig_seq_lags_ragged_dev / gpsig_seq_lags_ragged_grad: the lagged copies of a ragged batch on per-sequence time axes and
// their reverse pass (kernels and what they compute: seq_lags_kernel.hpp).  The training path's scale_sequences goes through this pair where an
// evaluation gives lengths and the kernel has lags (lag_axis = "sequence"); lengthscales and lag weights stay torch ops behind it.
// Scratch of the reverse pass, in B_GR2: one partial sum of dlags per (sequence, lag).
#include "ctx.hpp"
#include "aux_kernels.hpp"
#include "seq_lags_kernel.hpp"

#include <algorithm>

using namespace gpsig;

namespace {

int lags_check(gpsig_ctx* c, int64_t N, int L, int d, int p) {
    if (!c) return GPSIG_ERR_INVALID;
    if (c->ptr_mode != GPSIG_PTR_DEVICE) return fail(c, GPSIG_ERR_INVALID, "the ragged lag op takes device pointers");
    if (N < 0 || L < 1 || d < 1 || p < 1) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    if (p > MAX_LAGS) return fail(c, GPSIG_ERR_UNSUPPORTED, "the ragged lag op is built for num_lags <= %d", MAX_LAGS);
    if (d > MAX_FEATURES_WIDE) return fail(c, GPSIG_ERR_UNSUPPORTED, "the ragged lag op is built for at most %d columns", MAX_FEATURES_WIDE);
    if (N > (int64_t(1) << 40) / L) return fail(c, GPSIG_ERR_UNSUPPORTED, "too many points");
    HIPCHK(c, hipSetDevice(c->device));
    return GPSIG_OK;
}

void lags_fields(const double* X, const int32_t* lengths, const double* lags, int64_t N, int L, int d, int p, SeqLagsArgs* A) {
    A->X = X; A->lengths = lengths; A->lags = lags;
    A->N = N; A->L = L; A->d = d; A->p = p;
    A->jitter = 1e-6;                                  // settings.jitter inside lin_interp (gpsig/lags.py:22), as scale_params
}

}  // namespace

extern "C" {

int gpsig_seq_lags_ragged_dev(gpsig_ctx* c, const double* X, const int32_t* lengths, const double* lags, int64_t N, int32_t L, int32_t d, int32_t p,
                              double* out) {
    CHK(lags_check(c, N, L, d, p));
    if (N == 0) return GPSIG_OK;
    if (!X || !lengths || !lags || !out) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    SeqLagsArgs A{};
    lags_fields(X, lengths, lags, N, L, d, p, &A);
    A.out = out;
    const int64_t total = N * L * (p + 1) * d;
    const unsigned grid = unsigned(std::min<int64_t>((total + 255) / 256, SEQ_LAGS_MAX_GRID));
    hipLaunchKernelGGL(seq_lags_fwd_kernel, dim3(grid), dim3(256), 0, c->stream, A);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

int gpsig_seq_lags_ragged_grad(gpsig_ctx* c, const double* X, const int32_t* lengths, const double* lags, const double* G, int64_t N, int32_t L,
                               int32_t d, int32_t p, double* dX, double* dlags) {
    CHK(lags_check(c, N, L, d, p));
    if (!dlags) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    if (N == 0) return zero_async(c, dlags, sizeof(double) * size_t(p));
    if (!X || !lengths || !lags || !G || !dX) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    void* scr;
    CHK(ensure(c, B_GR2, sizeof(double) * size_t(N) * p + 64, &scr));
    SeqLagsArgs A{};
    lags_fields(X, lengths, lags, N, L, d, p, &A);
    A.G = G; A.dX = dX; A.part = static_cast<double*>(scr);
    const unsigned threads = unsigned(std::min((d + 63) / 64 * 64, SEQ_LAGS_THREADS));
    hipLaunchKernelGGL(seq_lags_grad_kernel, dim3(unsigned(std::min<int64_t>(N, SEQ_LAGS_MAX_GRID))), dim3(threads), 0, c->stream, A);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(seq_lags_reduce_kernel, dim3(1), dim3(64), 0, c->stream, A.part, N, p, dlags);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

}  // extern "C"
