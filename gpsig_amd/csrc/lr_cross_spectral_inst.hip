// lr_cross_spectral_inst.hip -- gpsig_spectral_cross / gpsig_spectral_cross_grad on state spaces of 33 .. 4096 columns: SignatureSpectral's Nystrom
// cross matrix on the float64 matrix cores and its reverse pass (kernels and what they compute: lr_cross_spectral_kernel.hpp).  The two entry
// points (spectral_cross_api.hip) hand over here before anything else where d > 32; up to 32 columns they run the kernels they ran.  The training
// path's wide spectral maps go through this pair: the feature kernels that take kxs from memory (lr_kx_inst.hip) follow it, their reverse passes
// hand dkxs back to it.
// Scratch, in B_GR2: gamma^2 (Q d), the landmarks' norms and phases (2 Q c) and the summed blocks (Q block); per chunk of points their phases,
// A_q, B_q, three row sums and a flag (Q (2 c + 4) + 1 doubles a point) and the shares' partial blocks.  Chunk and shares are sized so that all of it
// stays inside the context's chunk budget (wide_chunk_mb, else grad_scratch_mb) -- half of it for the points, a quarter for the partials, never
// fewer than 64 points or one share --; the chunks' sums are added in chunk order.  dP does not go through the partials: its bits do not depend
// on the budget.
#include "ctx.hpp"
#include "launchers.hpp"
#define GPSIG_LR_SPX_KERNELS
#include "lr_cross_spectral_kernel.hpp"

#include <algorithm>

using namespace gpsig;

namespace {

// the wide route's chunk budget (wide_api.hip: wide_chunk_bytes)
size_t chunk_budget(const gpsig_ctx* c) {
    if (c->wide_chunk_mb > 0) return size_t(c->wide_chunk_mb) << 20;
    return size_t(c->grad_scratch_mb > 0 ? c->grad_scratch_mb : 4096) << 20;
}

int wide_check(gpsig_ctx* c, int Q, int family, int d, int64_t n, int cc) {
    if (!c) return GPSIG_ERR_INVALID;
    if (Q < 1 || Q > LR_SPX_MAX_Q || family < 0 || family > 2) return fail(c, GPSIG_ERR_INVALID, "spectral kernel: bad number of components / family");
    if (n < 0 || cc < 1) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    if (d > MAX_FEATURES_WIDE) return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral cross op is built for at most %d columns", MAX_FEATURES_WIDE);
    if (cc > LR_CROSS_MAX_C)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral cross op beyond %d columns is built for num_components <= %d", int(SPECTRAL_STRIDE), LR_CROSS_MAX_C);
    if (n > (int64_t(1) << 40)) return fail(c, GPSIG_ERR_UNSUPPORTED, "too many points");
    if (c->ptr_mode != GPSIG_PTR_DEVICE) return fail(c, GPSIG_ERR_INVALID, "the spectral cross op takes device pointers");
    HIPCHK(c, hipSetDevice(c->device));
    return GPSIG_OK;
}

unsigned points_grid(int64_t n) {
    const int64_t nblk = (n + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES);
    return unsigned(std::min<int64_t>(nblk, LR_CROSS_MAX_GRID));
}

// what a call computes once: gamma^2, the landmarks' norms and phases, at `head` (Q d + 2 Q c doubles)
int prepare(gpsig_ctx* c, LrSpxArgs* A, const double* gamma, double* head) {
    const int Q = A->Q, d = A->d, cc = A->c;
    const int rc = spectral_cross_prepare_launch(c->stream, A->S, cc, d, Q, A->omega, gamma, head);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "%s", hipGetErrorString(hipError_t(rc)));
    A->g2 = head; A->ss = head + size_t(Q) * d; A->phS = A->ss + size_t(Q) * cc;
    return GPSIG_OK;
}

}  // namespace

namespace gpsig {

int spectral_cross_prepare_launch(hipStream_t stream, const double* S, int cc, int d, int Q, const double* omega, const double* gamma, double* head) {
    double* const g2 = head;
    double* const ss = g2 + size_t(Q) * d;
    double* const phS = ss + size_t(Q) * cc;
    hipLaunchKernelGGL(lr_spx_prep_kernel, dim3(unsigned((int64_t(Q) * d + 255) / 256)), dim3(256), 0, stream, gamma, int64_t(Q) * d, g2);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return int(e);
    hipLaunchKernelGGL(lr_spx_norms_kernel, dim3(unsigned((cc + 15) / 16), unsigned(Q)), dim3(64), 0, stream, S, cc, d, static_cast<const double*>(g2), ss);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return int(e);
    hipLaunchKernelGGL(lr_spx_phase_kernel, dim3(points_grid(cc)), dim3(LR_CROSS_THREADS), 0, stream, S, int64_t(cc), d, omega, Q, phS);
    return int(hipGetLastError());
}

int spectral_cross_wide(gpsig_ctx* c, int Q, int family, int d, const double* P, int64_t n, const double* S, int cc, const double* alpha,
                        const double* omega, const double* gamma, double* K) {
    CHK(wide_check(c, Q, family, d, n, cc));
    if (n == 0) return GPSIG_OK;
    if (!P || !S || !alpha || !omega || !gamma || !K) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    const size_t head = size_t(Q) * d + 2 * size_t(Q) * cc;
    const int64_t nck = std::min<int64_t>(n, std::max<int64_t>(64, int64_t(chunk_budget(c) / 2 / (sizeof(double) * Q))));
    void* scr;
    CHK(ensure(c, B_GR2, sizeof(double) * (head + size_t(Q) * nck) + 64, &scr));
    LrSpxArgs A{};
    A.d = d; A.S = S; A.c = cc; A.Q = Q; A.family = family; A.alpha = alpha; A.omega = omega;
    CHK(prepare(c, &A, gamma, static_cast<double*>(scr)));
    double* const phP = static_cast<double*>(scr) + head;
    A.phP = phP;
    for (int64_t t0 = 0; t0 < n; t0 += nck) {
        const int64_t nn = std::min<int64_t>(nck, n - t0);
        A.P = P + t0 * d; A.n = nn; A.K = K + t0 * cc;
        hipLaunchKernelGGL(lr_spx_phase_kernel, dim3(points_grid(nn)), dim3(LR_CROSS_THREADS), 0, c->stream, A.P, nn, d, omega, Q, phP);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(lr_spx_kernel<false>, dim3(points_grid(nn)), dim3(LR_CROSS_THREADS), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    return GPSIG_OK;
}

int spectral_cross_wide_grad(gpsig_ctx* c, int Q, int family, int d, const double* P, int64_t n, const double* S, int cc, const double* alpha,
                             const double* omega, const double* gamma, const double* G, double* dP, double* dS, double* dalpha, double* domega,
                             double* dgamma) {
    CHK(wide_check(c, Q, family, d, n, cc));
    if (!dS || !dalpha || !domega || !dgamma) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    if (n == 0) {
        CHK(zero_async(c, dS, sizeof(double) * size_t(cc) * d));
        CHK(zero_async(c, dalpha, sizeof(double) * size_t(Q)));
        CHK(zero_async(c, domega, sizeof(double) * size_t(Q) * d));
        CHK(zero_async(c, dgamma, sizeof(double) * size_t(Q) * d));
        return GPSIG_OK;
    }
    if (!P || !S || !alpha || !omega || !gamma || !G || !dP) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    const size_t budget = chunk_budget(c);
    const int64_t blk = lr_spx_block(cc, d), width = int64_t(Q) * blk;
    const size_t per_point = size_t(Q) * (2 * size_t(cc) + 4) + 1;
    const int64_t nck = std::min<int64_t>(n, std::max<int64_t>(64, int64_t(budget / 2 / (sizeof(double) * per_point))));
    const int64_t fit = std::max<int64_t>(1, int64_t(budget / 4 / (sizeof(double) * size_t(width))));
    const int64_t max_shares = std::min<int64_t>(std::min<int64_t>((nck + 1023) / 1024, 256), fit);
    const size_t head = size_t(Q) * d + 2 * size_t(Q) * cc;
    void* scr;
    CHK(ensure(c, B_GR2, sizeof(double) * (head + size_t(width) + per_point * size_t(nck) + size_t(max_shares) * size_t(width)) + 64, &scr));
    LrSpxArgs A{};
    A.d = d; A.S = S; A.c = cc; A.Q = Q; A.family = family; A.alpha = alpha; A.omega = omega;
    CHK(prepare(c, &A, gamma, static_cast<double*>(scr)));
    double* const tot = static_cast<double*>(scr) + head;
    double* const phP = tot + width;
    const size_t qn = size_t(Q) * nck;
    A.phP = phP;
    A.WA = phP + qn; A.WB = A.WA + qn * cc;
    A.RA = A.WB + qn * cc; A.RB = A.RA + qn; A.RL = A.RB + qn;
    A.live = A.RL + qn;
    A.part = A.live + nck;
    for (int64_t t0 = 0; t0 < n; t0 += nck) {
        // the arrays of a chunk of nn points are (Q, nn, .): the kernels index them by A.n
        const int64_t nn = std::min<int64_t>(nck, n - t0);
        const int64_t shares = std::min<int64_t>(std::min<int64_t>((nn + 1023) / 1024, 256), fit);
        A.P = P + t0 * d; A.n = nn; A.G = G + t0 * cc; A.dP = dP + t0 * d;
        A.share = ((nn + shares - 1) / shares + 3) / 4 * 4; A.shares = int(shares);
        const unsigned grid = points_grid(nn);
        hipLaunchKernelGGL(lr_spx_phase_kernel, dim3(grid), dim3(LR_CROSS_THREADS), 0, c->stream, A.P, nn, d, omega, Q, phP);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(lr_spx_kernel<true>, dim3(grid), dim3(LR_CROSS_THREADS), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(lr_spx_points_kernel, dim3(grid), dim3(LR_CROSS_THREADS), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(lr_spx_landmarks_kernel, dim3(unsigned((d + 1 + 16 * LR_CROSS_WAVES - 1) / (16 * LR_CROSS_WAVES)), unsigned(shares), unsigned(Q)),
                           dim3(LR_CROSS_THREADS), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(lr_spx_reduce_kernel, dim3(unsigned((width + 255) / 256)), dim3(256), 0, c->stream, A.part, int(shares), width,
                           t0 == 0 ? 1 : 0, tot);
        HIPCHK(c, hipGetLastError());
    }
    const int64_t outs = int64_t(cc) * d + int64_t(Q) * d + Q;
    hipLaunchKernelGGL(lr_spx_finish_kernel, dim3(unsigned((outs + 255) / 256)), dim3(256), 0, c->stream, A, tot, gamma, dS, dalpha, domega, dgamma);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

}  // namespace gpsig
