// spectral_kappa_api.hip -- SignatureSpectral's kappa as a batched op with its reverse pass, for exact-mode training (autodiff._SpectralKappa):
//     gpsig_spectral_kappa        K (batch, m, n) = kappa(A (batch, m, d), B (batch, n, d))
//     gpsig_spectral_kappa_grad   G = dL/dK -> dA, dB, dalpha (Q), domega (Q, d), dgamma (Q, d)
// the parameters read from DEVICE memory.  What base_kernel_matrix("spectral", ...) computes without the (batch, m, n, d) difference tensor.
// Forward: the kernels of wide_spectral_kernel.hpp through their launchers -- gamma^2 once per call, the norms and phases once per side (once in all where A
// and B are the same array), then wide_spx_kernel on the batch strides.  Reverse: spectral_kappa_kernel.hpp, with the two skinny products U B and
// sum_q U_q^T (g2_q o A) left to rocBLAS (solver_dgemm_batched): both are plain GEMMs once the components are stacked -- (Q nr x n)(n x d) and
// (n x Q nr)(Q nr x d) per batch member --, which is the shape a library GEMM tiles well; the hand-written contraction of wide_api.hip (contract_both)
// serves rows of at most 32 columns and would need the stacking besides.
// Chunks: whole batch members while one fits the context's chunk budget (wide_chunk_bytes), else blocks of rows (multiples of 64) of one member, every
// array of a chunk in ONE scratch block laid out for the planned chunk; a single 64-row block beyond the budget is still served.  Every entry of K and
// every row of dA depends on its own chunk alone; the column-side sums (cu, cv, the product into dB) and the parameters' sums are added in chunk order,
// the slots inside a chunk in slot order: no floating-point atomics, two calls return the same bits.
#include "ctx.hpp"
#include "launchers.hpp"
#include "wide_spectral_kernel.hpp"
#include "spectral_kappa_kernel.hpp"

#include <algorithm>
#include <string>

using namespace gpsig;

namespace {

int kappa_check(gpsig_ctx* c, int Q, int family, int d, int64_t batch, int64_t m, int64_t n) {
    if (!c) return GPSIG_ERR_INVALID;
    if (family < 0 || family > 2) return fail(c, GPSIG_ERR_INVALID, "spectral kappa op: bad family");
    if (Q < 1 || Q > SPK_MAX_Q) return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral kappa op is built for 1 <= Q <= %d components (got %d)", SPK_MAX_Q, Q);
    if (d < 1 || d > SPK_MAX_D) return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral kappa op is built for 1 <= d <= %d columns (got %d)", SPK_MAX_D, d);
    if (batch < 0 || m < 0 || n < 0) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    if (m > 0x7fffffff || n > 0x7fffffff) return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral kappa op is built for m, n < 2^31");
    if (c->ptr_mode != GPSIG_PTR_DEVICE) return fail(c, GPSIG_ERR_INVALID, "the spectral kappa op takes device pointers");
    if (c->capturing) return fail(c, GPSIG_ERR_UNSUPPORTED, "graph capture: the spectral kappa op does not record (its scratch follows the shapes, rocBLAS may allocate)");
    HIPCHK(c, hipSetDevice(c->device));
    return GPSIG_OK;
}

size_t up8(size_t v) { return (v + 7) & ~size_t(7); }

// doubles of the forward pass's chunk (gamma^2 and the two sides' norms and phases)
size_t fwd_doubles(int Q, int d, int64_t n, int64_t nb, int64_t nr) {
    return up8(size_t(Q) * d) + up8(2 * size_t(Q) * nb * nr) + up8(2 * size_t(Q) * nb * n);
}

// the scratch block of a reverse chunk of nb members x nr rows: the fields of K (where given) on `base`; returns its doubles
size_t bwd_layout(SpecKappaArgs* K, double* base, int Q, int d, int64_t n, int64_t nb, int64_t nr, double** sideA, double** sideB, double** g2, double** da1) {
    const size_t ncb = size_t((n + SPK_TILE - 1) / SPK_TILE), nrb = size_t((nr + SPK_TILE - 1) / SPK_TILE);
    const size_t nbr = size_t(nb) * nr, nbn = size_t(nb) * n, q = size_t(Q);
    const size_t slices = (std::max(nbr, nbn) + SPK_SLICE - 1) / SPK_SLICE;
    size_t at = 0;
    auto take = [&](size_t count) { const size_t o = at; at += up8(count); return base ? base + o : nullptr; };
    double* const p_g2 = take(q * d);
    double* const p_tot = take(q + 2 * q * d);
    double* const p_sa = take(2 * q * nbr);
    double* const p_sb = take(2 * q * nbn);
    double* const p_U = take(q * nbr * n);
    double* const p_UB = take(q * nbr * d);
    double* const p_AS = take(q * nbr * d);
    double* const p_rus = take(ncb * q * nbr);
    double* const p_rvs = take(ncb * q * nbr);
    double* const p_ru = take(q * nbr);
    double* const p_rv = take(q * nbr);
    double* const p_cus = take(nrb * q * nbn);
    double* const p_cvs = take(nrb * q * nbn);
    double* const p_cu = take(q * nbn);
    double* const p_cv = take(q * nbn);
    double* const p_das = take(ncb * size_t(nb) * nrb * q);
    double* const p_da1 = take(size_t(nb) * nrb * q);
    double* const p_pp = take(slices * 2 * q * d);
    if (K) {
        K->tot = p_tot; K->U = p_U; K->UB = p_UB; K->AS = p_AS; K->rus = p_rus; K->rvs = p_rvs; K->ru = p_ru; K->rv = p_rv;
        K->cus = p_cus; K->cvs = p_cvs; K->cu = p_cu; K->cv = p_cv; K->das = p_das; K->ppart = p_pp;
        *sideA = p_sa; *sideB = p_sb; *g2 = p_g2; *da1 = p_da1;
    }
    return at;
}

// nb whole members, or (nb = 1) nr rows of one -- a multiple of 64, or all m --: the largest chunk whose doubles(nb, nr) fit the budget, never
// less than one member's first 64 rows
template <class F>
void plan_chunk(int64_t batch, int64_t m, size_t budget, F doubles, int64_t* nb, int64_t* nr) {
    const size_t lim = budget / sizeof(double), one = doubles(1, m);
    if (one <= lim) {
        int64_t k = std::min<int64_t>(batch, int64_t(lim / one));
        while (k > 1 && doubles(k, m) > lim) --k;
        *nb = std::max<int64_t>(k, 1); *nr = m;
        return;
    }
    int64_t lo = 1, hi = (m + SPK_TILE - 1) / SPK_TILE;          // blocks of 64 rows: lo fits (or is the minimum), hi + 1 does not
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) / 2;
        if (doubles(1, std::min<int64_t>(mid * SPK_TILE, m)) <= lim) lo = mid; else hi = mid - 1;
    }
    *nb = 1; *nr = std::min<int64_t>(lo * SPK_TILE, m);
}

int hipfail(gpsig_ctx* c, int rc) { return rc == 0 ? GPSIG_OK : fail(c, GPSIG_ERR_HIP, "spectral kappa op: %s", hipGetErrorString(hipError_t(rc))); }

// the norms (Q, rows) and, Q * rows doubles on, the phases of `rows` rows X (rows, d) at `side`
int side(gpsig_ctx* c, const double* X, int64_t rows, int d, int Q, const double* omega, const double* g2, double* out) {
    return hipfail(c, wide_spx_side_launch(c->stream, X, rows, d, d, Q, omega, g2, out, out + int64_t(Q) * rows));
}

int gemm_batched(gpsig_ctx* c, bool tb, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, int64_t sa, const double* B, int64_t ldb, int64_t sb,
                 double beta, double* C, int64_t ldc, int64_t sc, int64_t batch) {
    if (m > 0x7fffffff || n > 0x7fffffff || k > 0x7fffffff || batch > 0x7fffffff)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "spectral kappa op: a product's dimension beyond 2^31 (lower the chunk budget)");
    std::string err;
    if (!solver_dgemm_batched(&c->blas_handle, c->stream, false, tb, int(m), int(n), int(k), 1.0, A, int(lda), sa, B, int(ldb), sb, beta, C, int(ldc), sc,
                              int(batch), &err))
        return fail(c, GPSIG_ERR_HIP, "%s", err.c_str());
    return GPSIG_OK;
}

}  // namespace

extern "C" {

int gpsig_spectral_kappa(gpsig_ctx* c, int32_t Q, int32_t family, int32_t d, const double* A, const double* B, int64_t batch, int64_t m, int64_t n,
                         const double* alpha, const double* omega, const double* gamma, double* K) {
    CHK(kappa_check(c, Q, family, d, batch, m, n));
    if (batch == 0 || m == 0 || n == 0) return GPSIG_OK;
    if (!A || !B || !alpha || !omega || !gamma || !K) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    int64_t nb, nr;
    plan_chunk(batch, m, wide_chunk_bytes(c), [&](int64_t b, int64_t r) { return fwd_doubles(Q, d, n, b, r); }, &nb, &nr);
    void* scr;
    CHK(ensure(c, B_WD2, sizeof(double) * fwd_doubles(Q, d, n, nb, nr) + 64, &scr));
    double* const g2 = static_cast<double*>(scr);
    double* const sa = g2 + up8(size_t(Q) * d);
    double* const sb = sa + up8(2 * size_t(Q) * nb * nr);
    CHK(hipfail(c, wide_spx_prep_launch(c->stream, gamma, int64_t(Q) * d, g2)));
    const bool same = A == B && m == n;
    for (int64_t b0 = 0; b0 < batch; b0 += nb) {
        const int64_t nbc = std::min(nb, batch - b0);
        for (int64_t r0 = 0; r0 < m; r0 += nr) {
            const int64_t nrc = std::min(nr, m - r0);
            const bool alias = same && nrc == m;             // the chunk's rows of A are the rows of B
            CHK(side(c, A + (b0 * m + r0) * d, nbc * nrc, d, Q, omega, g2, sa));
            if (r0 == 0 && !alias) CHK(side(c, B + b0 * n * d, nbc * n, d, Q, omega, g2, sb));
            const double* const sB = alias ? sa : sb;
            WideSpxArgs W;
            memset(&W, 0, sizeof(W));
            W.A = A + (b0 * m + r0) * d; W.B = B + b0 * n * d; W.C = K + (b0 * m + r0) * n;
            W.m = nrc; W.n = n; W.lda = d; W.ldb = d; W.ldc = n; W.sa = m * d; W.sb = n * d; W.sc = m * n; W.batch = nbc;
            W.d = d; W.Q = Q; W.family = family; W.alpha = alpha; W.g2 = g2;
            W.nrmA = sa; W.phA = sa + int64_t(Q) * nbc * nrc; W.planeA = nbc * nrc; W.rowsA = nrc;
            W.nrmB = sB; W.phB = sB + int64_t(Q) * nbc * n; W.planeB = nbc * n; W.rowsB = n;
            CHK(hipfail(c, wide_spx_launch(c->stream, W)));
        }
    }
    return GPSIG_OK;
}

int gpsig_spectral_kappa_grad(gpsig_ctx* c, int32_t Q, int32_t family, int32_t d, const double* A, const double* B, int64_t batch, int64_t m, int64_t n,
                              const double* alpha, const double* omega, const double* gamma, const double* G, double* dA, double* dB, double* dalpha,
                              double* domega, double* dgamma) {
    CHK(kappa_check(c, Q, family, d, batch, m, n));
    if (!dalpha || !domega || !dgamma) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    if (batch == 0 || m == 0 || n == 0) {                        // K is empty: no gradient reaches anything
        CHK(zero_async(c, dalpha, sizeof(double) * size_t(Q)));
        CHK(zero_async(c, domega, sizeof(double) * size_t(Q) * d));
        CHK(zero_async(c, dgamma, sizeof(double) * size_t(Q) * d));
        if (dA) CHK(zero_async(c, dA, sizeof(double) * size_t(batch) * m * d));
        if (dB) CHK(zero_async(c, dB, sizeof(double) * size_t(batch) * n * d));
        return GPSIG_OK;
    }
    if (!A || !B || !alpha || !omega || !gamma || !G || !dA || !dB) return fail(c, GPSIG_ERR_INVALID, "NULL pointer");
    int64_t nb, nr;
    plan_chunk(batch, m, wide_chunk_bytes(c),
               [&](int64_t b, int64_t r) { return bwd_layout(nullptr, nullptr, Q, d, n, b, r, nullptr, nullptr, nullptr, nullptr); }, &nb, &nr);
    void* scr;
    CHK(ensure(c, B_WD2, sizeof(double) * bwd_layout(nullptr, nullptr, Q, d, n, nb, nr, nullptr, nullptr, nullptr, nullptr) + 64, &scr));
    SpecKappaArgs S;
    memset(&S, 0, sizeof(S));
    double *sa, *sb, *g2, *da1;
    bwd_layout(&S, static_cast<double*>(scr), Q, d, n, nb, nr, &sa, &sb, &g2, &da1);
    S.m = m; S.n = n; S.d = d; S.Q = Q; S.family = family; S.alpha = alpha; S.omega = omega; S.gamma = gamma; S.g2 = g2;
    S.ncb = (n + SPK_TILE - 1) / SPK_TILE;
    const int64_t qd = int64_t(Q) * d;
    CHK(zero_async(c, S.tot, sizeof(double) * size_t(Q + 2 * qd)));
    CHK(hipfail(c, wide_spx_prep_launch(c->stream, gamma, qd, g2)));
    const bool same = A == B && m == n;
    hipStream_t st = c->stream;
    for (int64_t b0 = 0; b0 < batch; b0 += nb) {
        const int64_t nbc = std::min(nb, batch - b0);
        S.A = A + b0 * m * d; S.B = B + b0 * n * d; S.G = G + b0 * m * n; S.dA = dA + b0 * m * d; S.dB = dB + b0 * n * d;
        S.nb = nbc;
        for (int64_t r0 = 0; r0 < m; r0 += nr) {
            const int64_t nrc = std::min(nr, m - r0);
            S.nr = nrc; S.r0 = r0; S.nrb = (nrc + SPK_TILE - 1) / SPK_TILE;
            const bool alias = same && nrc == m;
            CHK(side(c, S.A + r0 * d, nbc * nrc, d, Q, omega, g2, sa));
            if (r0 == 0 && !alias) CHK(side(c, S.B, nbc * n, d, Q, omega, g2, sb));
            const double* const sB = alias ? sa : sb;
            S.nrmA = sa; S.phA = sa + int64_t(Q) * nbc * nrc;
            S.nrmB = sB; S.phB = sB + int64_t(Q) * nbc * n;
            CHK(hipfail(c, spk_weights_launch(st, S)));
            const int64_t wr = nbc * Q * nrc, wc = nbc * Q * n;
            CHK(hipfail(c, spk_reduce_launch(st, S.rus, S.ncb, wr, 1, S.ru)));
            CHK(hipfail(c, spk_reduce_launch(st, S.rvs, S.ncb, wr, 1, S.rv)));
            CHK(hipfail(c, spk_reduce_launch(st, S.cus, S.nrb, wc, r0 == 0 ? 1 : 0, S.cu)));
            CHK(hipfail(c, spk_reduce_launch(st, S.cvs, S.nrb, wc, r0 == 0 ? 1 : 0, S.cv)));
            CHK(hipfail(c, spk_reduce_launch(st, S.das, S.ncb, nbc * S.nrb * Q, 1, da1)));
            CHK(hipfail(c, spk_reduce_launch(st, da1, nbc * S.nrb, Q, 0, S.tot)));
            CHK(hipfail(c, spk_scale_launch(st, S)));
            // row-major UB (Q nr, d) = U (Q nr, n) B (n, d) per member; dB (n, d) (+)= U^T (n, Q nr) AS (Q nr, d)
            CHK(gemm_batched(c, false, d, Q * nrc, n, S.B, d, n * d, S.U, n, Q * nrc * n, 0.0, S.UB, d, Q * nrc * d, nbc));
            CHK(gemm_batched(c, true, d, n, Q * nrc, S.AS, d, Q * nrc * d, S.U, n, Q * nrc * n, r0 == 0 ? 0.0 : 1.0, S.dB, d, n * d, nbc));
            CHK(hipfail(c, spk_rows_launch(st, S)));
            CHK(hipfail(c, spk_param_launch(st, S, 0)));
            CHK(hipfail(c, spk_reduce_launch(st, S.ppart, (nbc * nrc + SPK_SLICE - 1) / SPK_SLICE, 2 * qd, 0, S.tot + Q)));
            if (r0 + nrc == m) {                                 // the members' column sums are complete
                CHK(hipfail(c, spk_param_launch(st, S, 1)));
                CHK(hipfail(c, spk_reduce_launch(st, S.ppart, (nbc * n + SPK_SLICE - 1) / SPK_SLICE, 2 * qd, 0, S.tot + Q)));
                CHK(hipfail(c, spk_cols_launch(st, S)));
            }
        }
    }
    CHK(hipfail(c, spk_finish_launch(st, S, dalpha, domega, dgamma)));
    return GPSIG_OK;
}

}  // extern "C"
