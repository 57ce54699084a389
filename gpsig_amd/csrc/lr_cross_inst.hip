// lr_cross_inst.hip -- gpsig_lr_cross / gpsig_lr_cross_grad: the Nystrom cross matrix of the families of base_eval on the float64 matrix cores and
// its reverse pass (kernels and what they compute: lr_cross_kernel.hpp).  The training path's wide state spaces go through this pair: the feature
// kernels that take kxs from memory (lr_kx_inst.hip, gpsig_lr_seq_features_kx_dev / gpsig_lr_tens_features_kx_dev) follow it, their reverse
// passes hand dkxs back to it.
// Scratch of the reverse pass, in B_GR2: |S_i|^2 and the column sums (2 c), W = G o wy (n c) and a flag per point (n), the points kernel's
// partials (grid (c + 1)) and the landmark kernel's (shares c d).  The shares are capped so that their partials stay inside the context's chunk
// budget (wide_chunk_mb, as the wide route's chunks); with one share the sum over the points is a single chain.
#include "ctx.hpp"
#include "lr_cross_kernel.hpp"

#include <algorithm>

using namespace gpsig;

namespace {

// the wide route's chunk budget (wide_api.hip: wide_chunk_bytes)
size_t chunk_budget(const gpsig_ctx* c) {
    if (c->wide_chunk_mb > 0) return size_t(c->wide_chunk_mb) << 20;
    return size_t(c->grad_scratch_mb > 0 ? c->grad_scratch_mb : 4096) << 20;
}

int cross_check(gpsig_ctx* c, const gpsig_params* p, int64_t n, int cc) {
    if (!c) return GPSIG_ERR_INVALID;
    if (!p) return fail(c, GPSIG_ERR_INVALID, "params is NULL");
    if (p->dtype != GPSIG_F64) return fail(c, GPSIG_ERR_UNSUPPORTED, "the low-rank cross op is built for float64 only");
    if (p->base_kernel == GPSIG_BASE_SPECTRAL) return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral base kernel has a cross op of its own (gpsig_spectral_cross)");
    if (p->base_kernel < GPSIG_BASE_LINEAR || p->base_kernel > GPSIG_BASE_MATERN52) return fail(c, GPSIG_ERR_INVALID, "unknown base kernel %d", p->base_kernel);
    if (c->ptr_mode != GPSIG_PTR_DEVICE) return fail(c, GPSIG_ERR_INVALID, "the low-rank cross op takes device pointers");
    if (n < 0 || cc < 1 || p->num_features < 1) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    if (cc > LR_CROSS_MAX_C) return fail(c, GPSIG_ERR_UNSUPPORTED, "the low-rank cross op is built for num_components <= %d", LR_CROSS_MAX_C);
    if (p->num_features > MAX_FEATURES_WIDE) return fail(c, GPSIG_ERR_UNSUPPORTED, "the low-rank cross op is built for at most %d columns", MAX_FEATURES_WIDE);
    if (n > (int64_t(1) << 40)) return fail(c, GPSIG_ERR_UNSUPPORTED, "too many points");
    HIPCHK(c, hipSetDevice(c->device));
    return GPSIG_OK;
}

void cross_fields(const gpsig_params* p, const double* P, int64_t n, const double* S, int cc, LrCrossArgs* A) {
    A->P = P; A->n = n; A->d = p->num_features;
    A->S = S; A->c = cc;
    A->kind = int(p->base_kernel); A->p0 = p->base_params[0]; A->p1 = p->base_params[1];
}

unsigned points_grid(int64_t n) {
    const int64_t nblk = (n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    return unsigned(std::min<int64_t>(nblk, LR_CROSS_MAX_GRID));
}

int norms(gpsig_ctx* c, const LrCrossArgs& A, double* sn) {
    hipLaunchKernelGGL(lr_cross_norms_kernel, dim3(unsigned((A.c + 15) / 16)), dim3(64), 0, c->stream, A.S, A.c, A.d, sn);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

}  // namespace

namespace gpsig {
int lr_cross_norms_launch(hipStream_t stream, const double* S, int c, int d, double* sn) {
    hipLaunchKernelGGL(lr_cross_norms_kernel, dim3(unsigned((c + 15) / 16)), dim3(64), 0, stream, S, c, d, sn);
    return int(hipGetLastError());
}
}  // namespace gpsig

extern "C" {

int gpsig_lr_cross(gpsig_ctx* c, const gpsig_params* p, const double* P, int64_t n, const double* S, int32_t cc, double* K) {
    CHK(cross_check(c, p, n, cc));
    if (n == 0) return GPSIG_OK;
    if (!P || !S || !K) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    void* scr;
    CHK(ensure(c, B_GR2, sizeof(double) * 2 * LR_CROSS_MAX_C + 64, &scr));
    LrCrossArgs A{};
    cross_fields(p, P, n, S, cc, &A);
    A.sn = static_cast<double*>(scr);
    A.K = K;
    CHK(norms(c, A, static_cast<double*>(scr)));
    hipLaunchKernelGGL(lr_cross_kernel, dim3(points_grid(n)), dim3(LR_CROSS_THREADS), 0, c->stream, A);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

int gpsig_lr_cross_grad(gpsig_ctx* c, const gpsig_params* p, const double* P, int64_t n, const double* S, int32_t cc, const double* G, double* dP,
                        double* dS, double* g_base) {
    CHK(cross_check(c, p, n, cc));
    if (!dS) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    const int d = p->num_features;
    if (n == 0) {
        CHK(zero_async(c, dS, sizeof(double) * size_t(cc) * d));
        if (g_base) CHK(zero_async(c, g_base, sizeof(double)));
        return GPSIG_OK;
    }
    if (!P || !S || !G || !dP) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    // the points' shares of the landmark sums: 1024 points each, at most 256 of them and no more than the budget has room for partials
    const size_t each = sizeof(double) * size_t(cc) * d;
    const int64_t fit = std::max<int64_t>(1, int64_t(chunk_budget(c) / each));
    const int64_t shares = std::min<int64_t>(std::min<int64_t>((n + 1023) / 1024, 256), fit);
    const int64_t share = ((n + shares - 1) / shares + 3) / 4 * 4;
    const unsigned grid = points_grid(n);
    const size_t head = 2 * LR_CROSS_MAX_C, nW = size_t(n) * cc, nL = size_t(n), nP = size_t(grid) * (cc + 1), nD = size_t(shares) * cc * d;
    void* scr;
    CHK(ensure(c, B_GR2, sizeof(double) * (head + nW + nL + nP + nD) + 64, &scr));
    double* const sn = static_cast<double*>(scr);
    double* const colsum = sn + LR_CROSS_MAX_C;
    LrCrossArgs A{};
    cross_fields(p, P, n, S, cc, &A);
    A.sn = sn;
    A.G = G; A.dP = dP;
    A.W = sn + head; A.live = A.W + nW; A.part = A.live + nL; A.dspart = A.part + nP;
    A.share = share; A.shares = int(shares);
    CHK(norms(c, A, sn));
    hipLaunchKernelGGL(lr_cross_grad_points_kernel, dim3(grid), dim3(LR_CROSS_THREADS), 0, c->stream, A);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(lr_cross_grad_landmarks_kernel, dim3(unsigned((d + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES)), unsigned(shares)),
                       dim3(LR_CROSS_THREADS), 0, c->stream, A);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(lr_cross_grad_reduce_cols_kernel, dim3(1), dim3(128), 0, c->stream, A.part, int(grid), cc, colsum, g_base);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(lr_cross_grad_reduce_kernel, dim3(unsigned((int64_t(cc) * d + 255) / 256)), dim3(256), 0, c->stream, A.dspart, int(shares),
                       colsum, S, cc, d, dS);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

}  // extern "C"
