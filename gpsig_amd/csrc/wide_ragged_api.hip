// wide_ragged_api.hip -- ragged batches in EXACT (non-low-rank) mode on the wide-state-space route: the entry points gpsig_kernel_Kdiag_ragged,
// gpsig_kernel_K_tens_vs_seq_ragged, gpsig_kernel_K_tens_n_seq_covs_ragged and gpsig_kernel_K_ragged (include/gpsig_hip.h).  Forward evaluation only.
//
// Sequence n of a table (N, L, d) with lengths len[n] in [1, L] is X[n, :len[n]], evaluated as that truncated sequence would be on its own: no row at or
// beyond len[n] is read.  The plan (ragged_plan.hpp) needs the lengths on the host -- in device-pointer mode one copy of N int32 and a stream
// synchronisation --, so graph capture is refused.  Then, as in wide_api.hip, "arguments by a contraction, then chain / lattice kernels":
//   * the lengths-aware prep_seq_scaled_kernel writes the scaled (and, with lags, interpolated on each sequence's own axis) rows PACKED, (sum len, d);
//     wide_aug_rows_kernel augments the packed table as it does any table of rows;
//   * Kzx: one dgemm per chunk of whole sequences gives the argument array (sum_chunk len, CW); wide_tvs_fwd_kernel's ragged form takes a sequence's
//     column base from its packed offset and its step count from its length; the chain totals land in the dense layout and wide_tvs_epilogue_kernel is
//     the dense one;
//   * level diagonals (Kdiag, the normalisation factors, Kxx of the covariances): wide_ragged_diag_args_kernel (wide_ragged_kernel.hpp) fills the
//     block-diagonal argument lattices on the float64 matrix cores, wide_lattice_fwd_kernel's ragged form sweeps them;
//   * full Grams: one dgemm per chunk of left sequences against all packed right rows; lattice (i, j) sits at (off1[i] - off1[i0], off2[j]).
// Columns per lane and wavefronts per lattice come from the batch's longest sequence; nothing is sorted or queued by length.  Chunks follow option
// wide_chunk_mb.  Served: SignatureRBF and the Matern families, float64, num_levels <= 8, first order, lattices of at most 512 columns; the route is
// taken at any width (the automatic width rules of the dense entry points do not apply).  Everything else is refused by name (rg_check).
#include "ctx.hpp"
#include "api_common.hpp"
#include "launchers.hpp"
#include "aux_kernels.hpp"
#define GPSIG_WIDE_GLOBAL template <int UNIT = 0> __global__          // (wide_kernels.hpp: the kernels that are no templates are defined in wide_api.hip)
#include "wide_kernels.hpp"
#include "wide_ragged_kernel.hpp"
#include "ragged_plan.hpp"

#include <string>
#include <vector>

using namespace gpsig;

namespace {

const char* const WHO = "ragged exact evaluation (exact_ragged)";
constexpr int RG_LAT_MAX_COLS = 512;            // 64 lanes x 8 columns (wide_api.hip: WIDE_LAT_MAX_COLS)

bool rg_family(int base_kernel) {
    return base_kernel == GPSIG_BASE_RBF || base_kernel == GPSIG_BASE_MATERN12 || base_kernel == GPSIG_BASE_MATERN32 || base_kernel == GPSIG_BASE_MATERN52;
}

// what is not built, each by the bound that refuses it
int rg_check(gpsig_ctx* c, const gpsig_params* p) {
    if (p->dtype != GPSIG_F64) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s is built for float64 only (a float32 caller computes in float64 and rounds)", WHO);
    if (!rg_family(p->base_kernel))
        return fail(c, GPSIG_ERR_UNSUPPORTED, "%s serves SignatureRBF and the Matern families only (base kernel %d: the rows or norm terms of the linear, cosine, "
                    "poly, mix and spectral families need offsets of their own)", WHO, p->base_kernel);
    if (p->num_levels > WIDE_MAX_LEVELS) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s is built for num_levels <= %d (got %d)", WHO, WIDE_MAX_LEVELS, p->num_levels);
    if (p->order > 1 && p->num_levels > 1) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s serves first order only (order = %d)", WHO, p->order);
    if (c->wide == 0) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s runs on the wide route only: context option wide = 0 refuses it", WHO);
    if (routes_as_captured(c))          // (under option capture_routes too: the warm-up of a recording is told, not the recording)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "graph recording: %s is not served during library graph capture: the plan needs the lengths on the host", WHO);
    return GPSIG_OK;
}

int rg_dgemm(gpsig_ctx* c, int64_t m, int64_t n, int64_t k, const double* A, const double* B, double* C) {          // column-major C (m x n) = A_cm^T (m x k) B_cm (k x n)
    if (m > 0x7fffffff || n > 0x7fffffff) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s: a matrix dimension beyond 2^31", WHO);
    if (m == 0 || n == 0) return GPSIG_OK;
    std::string err;
    if (!solver_dgemm(&c->blas_handle, c->stream, true, false, int(m), int(n), int(k), 1.0, A, int(k), B, int(k), 0.0, C, int(m), &err))
        return fail(c, GPSIG_ERR_HIP, "%s", err.c_str());
    return GPSIG_OK;
}

// One side of a call: the plan on the host, its arrays on the device, the packed scaled rows.
struct RgSide {
    RaggedPlan pl;
    int64_t N = 0;
    const int32_t* len = nullptr;       // device (N)
    const int64_t* off = nullptr;       // device (N + 1)
    const int64_t* doff = nullptr;      // device (N + 1)
    const double* rows = nullptr;       // device (pl.rows(), d_eff)
};

// lengths: N int32 in the call's pointer mode, or NULL where the side may be dense (every sequence has its L rows).  X: the caller's table.
int rg_side(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& sp, const void* X, int id_in, int64_t N, int L, const int32_t* lengths, bool dense_ok,
            int id_meta, int id_rows, RgSide* s) {
    if (L < 1) return fail(c, GPSIG_ERR_INVALID, "sequence length must be >= 1");
    if (N < 0) return fail(c, GPSIG_ERR_INVALID, "negative number of sequences");
    if (!lengths && !dense_ok && N > 0) return fail(c, GPSIG_ERR_INVALID, "null lengths pointer");
    std::vector<int32_t> host;
    host.assign(size_t(N), L);
    if (lengths && N > 0) {
        if (c->ptr_mode == GPSIG_PTR_DEVICE) {
            HIPCHK(c, hipMemcpyAsync(host.data(), lengths, sizeof(int32_t) * size_t(N), hipMemcpyDeviceToHost, c->stream));
            CHK(host_sync(c));
        } else {
            memcpy(host.data(), lengths, sizeof(int32_t) * size_t(N));
        }
    }
    int64_t bad = 0;
    if (!ragged_offsets(host.data(), N, L, &s->pl, &bad))
        return fail(c, GPSIG_ERR_INVALID, "lengths[%lld] = %d outside [1, %d]", (long long)bad, int(host[size_t(bad)]), L);
    s->N = N;
    // off, doff (int64), len (int32), in one block
    const size_t n1 = size_t(N) + 1, bytes = sizeof(int64_t) * 2 * n1 + sizeof(int32_t) * size_t(N);
    std::vector<unsigned char> img(bytes);
    memcpy(img.data(), s->pl.off.data(), sizeof(int64_t) * n1);
    memcpy(img.data() + sizeof(int64_t) * n1, s->pl.doff.data(), sizeof(int64_t) * n1);
    if (N > 0) memcpy(img.data() + sizeof(int64_t) * 2 * n1, host.data(), sizeof(int32_t) * size_t(N));
    void* meta;
    CHK(ensure(c, id_meta, bytes + 64, &meta));
    HIPCHK(c, hipMemcpyAsync(meta, img.data(), bytes, hipMemcpyHostToDevice, c->stream));
    CHK(host_sync(c));                  // the image goes out of scope
    s->off = static_cast<const int64_t*>(meta);
    s->doff = s->off + n1;
    s->len = reinterpret_cast<const int32_t*>(s->doff + n1);
    const void* dX;
    CHK(in_dev(c, id_in, X, sizeof(double) * size_t(N) * L * p->num_features, &dX));
    const int d_eff = sp.d_eff();
    void* rows;
    CHK(ensure(c, id_rows, sizeof(double) * size_t(s->pl.rows()) * d_eff + 64, &rows));
    if (N > 0) {
        hipLaunchKernelGGL(prep_seq_scaled_kernel<double>, dim3(unsigned(N < 65535 ? N : 65535)), dim3(256), 0, c->stream, static_cast<const double*>(dX), N, L, sp,
                           s->len, s->off, static_cast<double*>(rows));
        HIPCHK(c, hipGetLastError());
    }
    s->rows = static_cast<const double*>(rows);
    return GPSIG_OK;
}

// the packed rows of a side in the left (right = 0) or the right form of the distance kernels' augmentation (wide_kernels.hpp), into buffer `id`
int rg_aug(gpsig_ctx* c, const RgSide& s, int d, int right, int id, const double** out) {
    const int64_t rows = s.pl.rows();
    void* a;
    CHK(ensure(c, id, sizeof(double) * size_t(rows) * (d + 2) + 64, &a));
    if (rows > 0) {
        ScaleParams none;
        memset(&none, 0, sizeof(none));
        none.d_in = d;
        hipLaunchKernelGGL(wide_aug_rows_kernel<>, dim3(unsigned(rows < 65535 ? rows : 65535)), dim3(64), 0, c->stream, s.rows, rows, d, right, 0, int64_t(0), int64_t(0),
                           1, none, int(WIDE_ROWS_DIST), 0, static_cast<double*>(a));
        HIPCHK(c, hipGetLastError());
    }
    *out = static_cast<const double*>(a);
    return GPSIG_OK;
}

int rg_lat_cols_check(gpsig_ctx* c, const gpsig_params* p, const RgSide& s) {
    const int cols = s.pl.max_len - (p->difference ? 1 : 0);
    if (cols > RG_LAT_MAX_COLS) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s serves sequence lattices of at most %d columns (got %d)", WHO, RG_LAT_MAX_COLS, cols);
    return GPSIG_OK;
}

// the ragged forms of the lattice kernel: the kinds served only (the RBF kernel at compile time, the Matern families at run time)
typedef void (*RgLatKernel)(const WideLatRaggedArgs);
template <int LQ, int KD>
RgLatKernel rg_lat_kernel_of(int C, int NW) {
    if (NW == 2) return wide_lattice_fwd_ragged_kernel<1, LQ, KD, 2>;
    if (NW == 4) return wide_lattice_fwd_ragged_kernel<1, LQ, KD, 4>;
    if (NW == 8) return wide_lattice_fwd_ragged_kernel<1, LQ, KD, 8>;
    switch (C) {
        case 1: return wide_lattice_fwd_ragged_kernel<1, LQ, KD, 1>;
        case 2: return wide_lattice_fwd_ragged_kernel<2, LQ, KD, 1>;
        case 4: return wide_lattice_fwd_ragged_kernel<4, LQ, KD, 1>;
        default: return wide_lattice_fwd_ragged_kernel<8, LQ, KD, 1>;
    }
}
RgLatKernel rg_lat_kernel(int M, int C, int base_kernel, int NW) {
    if (base_kernel == GPSIG_BASE_RBF) return M <= 4 ? rg_lat_kernel_of<3, WIDE_KD_RBF>(C, NW) : rg_lat_kernel_of<7, WIDE_KD_RBF>(C, NW);
    return M <= 4 ? rg_lat_kernel_of<3, WIDE_KD_MATERN>(C, NW) : rg_lat_kernel_of<7, WIDE_KD_MATERN>(C, NW);
}

void rg_lat_common(const gpsig_params* p, WideLatRaggedArgs* A) {
    memset(A, 0, sizeof(*A));
    A->M = p->num_levels; A->kind = p->base_kernel; A->kp0 = p->base_params[0]; A->kp1 = p->base_params[1]; A->difference = p->difference ? 1 : 0;
}

// raw level diagonals (M+1, N) of a side: block-diagonal argument lattices in chunks of whole sequences, then the lattice sweeps
int rg_diag_levels(gpsig_ctx* c, const gpsig_params* p, int d, const RgSide& s, double* out) {
    if (s.N == 0) return GPSIG_OK;
    CHK(rg_lat_cols_check(c, p, s));
    const int DA = d + 2, dr = p->difference ? 1 : 0;
    const double *XL, *XR;
    CHK(rg_aug(c, s, d, 0, B_WD0, &XL));
    CHK(rg_aug(c, s, d, 1, B_WD1, &XR));
    std::vector<int64_t> bounds;
    ragged_chunks(s.pl.doff, sizeof(double), wide_chunk_bytes(c), &bounds);
    void* arg;
    CHK(ensure(c, B_WD2, sizeof(double) * size_t(ragged_chunk_max(s.pl.doff, bounds)) + 64, &arg));
    const int C = wide_lat_columns(s.pl.max_len - dr);
    const unsigned tb = unsigned((s.pl.max_len + WIDE_RG_TILE - 1) / WIDE_RG_TILE);
    for (size_t k = 0; k + 1 < bounds.size(); ++k) {
        const int64_t n0 = bounds[k], nc = bounds[k + 1] - n0;
        WideRaggedDiagArgs D;
        memset(&D, 0, sizeof(D));
        D.XL = XL; D.XR = XR; D.arg = static_cast<double*>(arg); D.len = s.len; D.off = s.off; D.doff = s.doff; D.n0 = n0; D.Nc = nc; D.DA = DA;
        hipLaunchKernelGGL(wide_ragged_diag_args_kernel, dim3(tb, tb, unsigned(nc < 65535 ? nc : 65535)), dim3(WIDE_RG_THREADS), 0, c->stream, D);
        HIPCHK(c, hipGetLastError());
        const int NW = wide_lat_waves(c, C, nc);
        WideLatRaggedArgs A;
        rg_lat_common(p, &A);
        A.arg = static_cast<const double*>(arg); A.ld = 0; A.N2 = 1; A.P = nc; A.p0 = 0; A.Ptot = s.N;
        A.L1 = A.L2 = s.pl.max_len;
        A.out = out + n0;                       // (the kernel's pair index starts at 0 in this chunk's lattices)
        A.len1 = A.len2 = s.len + n0; A.rbase = s.doff + n0; A.cbase = nullptr;
        hipLaunchKernelGGL(rg_lat_kernel(p->num_levels, C, p->base_kernel, NW), dim3(unsigned(nc < 65535 ? nc : 65535)), dim3(64 * NW), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    return GPSIG_OK;
}

// raw levels (M+1, N1 N2) of every pair of the two sides (s2 may be s1)
int rg_gram_levels(gpsig_ctx* c, const gpsig_params* p, int d, const RgSide& s1, const RgSide& s2, double* out) {
    if (s1.N == 0 || s2.N == 0) return GPSIG_OK;
    CHK(rg_lat_cols_check(c, p, s2));
    const int DA = d + 2, dr = p->difference ? 1 : 0;
    const double *XL, *XR;
    CHK(rg_aug(c, s1, d, 0, B_WD0, &XL));
    CHK(rg_aug(c, s2, d, 1, B_WD1, &XR));
    const int64_t R2 = s2.pl.rows();
    std::vector<int64_t> bounds;
    ragged_chunks(s1.pl.off, sizeof(double) * size_t(R2), wide_chunk_bytes(c), &bounds);
    void* arg;
    CHK(ensure(c, B_WD2, sizeof(double) * size_t(ragged_chunk_max(s1.pl.off, bounds)) * size_t(R2) + 64, &arg));
    const int C = wide_lat_columns(s2.pl.max_len - dr);
    for (size_t k = 0; k + 1 < bounds.size(); ++k) {
        const int64_t i0 = bounds[k], ni = bounds[k + 1] - i0, r0 = s1.pl.off[size_t(i0)], rows = s1.pl.off[size_t(i0 + ni)] - r0;
        // row-major arg (rows, R2) = XL_chunk XR^T  ==  column-major (R2 x rows) = XR_cm^T XL_chunk,cm
        CHK(rg_dgemm(c, R2, rows, DA, XR, XL + r0 * DA, static_cast<double*>(arg)));
        const int64_t P = ni * s2.N;
        const int NW = wide_lat_waves(c, C, P);
        WideLatRaggedArgs A;
        rg_lat_common(p, &A);
        A.arg = static_cast<const double*>(arg); A.ld = R2; A.N2 = s2.N; A.P = P; A.p0 = 0; A.Ptot = s1.N * s2.N;
        A.L1 = s1.pl.max_len; A.L2 = s2.pl.max_len;
        A.out = out + i0 * s2.N;
        A.len1 = s1.len + i0; A.len2 = s2.len; A.rbase = s1.off + i0; A.cbase = s2.off;
        hipLaunchKernelGGL(rg_lat_kernel(p->num_levels, C, p->base_kernel, NW), dim3(unsigned(P < 65535 ? P : 65535)), dim3(64 * NW), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    return GPSIG_OK;
}

// per-sequence factors (N, M+1) of a side into buffer id_fac: w[m] / sqrt(diag_m + jitter) (w == NULL: 1 / sqrt), from its own level diagonals (left in
// id_dlev, sequence-major, for a second set of factors)
int rg_side_factors(gpsig_ctx* c, const gpsig_params* p, int d, const RgSide& s, const double* w, int id_dlev, int id_fac, const double** fac) {
    const int M1 = p->num_levels + 1;
    void *lev, *dl, *f;
    CHK(ensure(c, B_RG4, sizeof(double) * size_t(s.N) * M1 + 64, &lev));
    CHK(ensure(c, id_dlev, sizeof(double) * size_t(s.N) * M1 + 64, &dl));
    CHK(ensure(c, id_fac, sizeof(double) * size_t(s.N) * M1 + 64, &f));
    if (s.N > 0) {
        CHK(rg_diag_levels(c, p, d, s, static_cast<double*>(lev)));
        hipLaunchKernelGGL(levels_relayout_kernel, dim3(grid_for(s.N * int64_t(M1))), dim3(256), 0, c->stream, static_cast<const double*>(lev), s.N, M1, int64_t(1),
                           int64_t(M1), static_cast<double*>(dl));
        hipLaunchKernelGGL(factors_kernel<double>, dim3(grid_for(s.N * int64_t(M1))), dim3(256), 0, c->stream, static_cast<const double*>(dl), s.N, M1, w, p->jitter, 0,
                           static_cast<double*>(f));
        HIPCHK(c, hipGetLastError());
    }
    *fac = static_cast<const double*>(f);
    return GPSIG_OK;
}

int rg_factors_again(gpsig_ctx* c, const gpsig_params* p, int64_t N, const double* dlev, const double* w, double jitter, int id_fac, const double** fac) {
    const int M1 = p->num_levels + 1;
    void* f;
    CHK(ensure(c, id_fac, sizeof(double) * size_t(N) * M1 + 64, &f));
    if (N > 0) {
        hipLaunchKernelGGL(factors_kernel<double>, dim3(grid_for(N * int64_t(M1))), dim3(256), 0, c->stream, dlev, N, M1, w, jitter, 0, static_cast<double*>(f));
        HIPCHK(c, hipGetLastError());
    }
    *fac = static_cast<const double*>(f);
    return GPSIG_OK;
}

// Kzx.  Z: the caller's (lt, T, E, d) array on the device, scaled here; fx (N, M+1) or NULL; w (M+1); out (T, N) or (M+1, T, N)
int rg_tvs(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& sz, int d, const double* Z, const RgSide& s, int64_t Tn, int increments, const double* fx,
           const double* w, int sum_levels, double* out) {
    if (s.N == 0 || Tn == 0) return GPSIG_OK;
    const int M = p->num_levels, lt = M * (M + 1) / 2, E = increments ? 2 : 1, DA = d + 2;
    const int64_t Tpad = (Tn + 63) / 64 * 64, CW = int64_t(lt) * E * Tpad, TB = Tpad / 64, zr = CW;
    void *za, *ax;
    CHK(ensure(c, B_WD0, sizeof(double) * size_t(zr) * DA + 64, &za));
    hipLaunchKernelGGL(wide_aug_rows_kernel<>, dim3(unsigned(zr < 65535 ? zr : 65535)), dim3(64), 0, c->stream, Z, zr, d, 0, lt, Tn, Tpad, E, sz, int(WIDE_ROWS_DIST), 0,
                       static_cast<double*>(za));
    HIPCHK(c, hipGetLastError());
    const double* XA;
    CHK(rg_aug(c, s, d, 1, B_WD1, &XA));
    std::vector<int64_t> bounds;
    ragged_chunks(s.pl.off, sizeof(double) * size_t(CW), wide_chunk_bytes(c), &bounds);
    void* arg;
    CHK(ensure(c, B_WD2, sizeof(double) * size_t(ragged_chunk_max(s.pl.off, bounds)) * size_t(CW) + 64, &arg));
    CHK(ensure(c, B_WD8, sizeof(double) * size_t(s.N) * lt * Tpad + 64, &ax));
    for (size_t k = 0; k + 1 < bounds.size(); ++k) {
        const int64_t n0 = bounds[k], nc = bounds[k + 1] - n0, r0 = s.pl.off[size_t(n0)], rows = s.pl.off[size_t(n0 + nc)] - r0;
        // row-major arg (rows, CW) = XA_chunk ZA^T  ==  column-major (CW x rows) = ZA_cm^T XA_chunk,cm
        CHK(rg_dgemm(c, CW, rows, DA, static_cast<const double*>(za), XA + r0 * DA, static_cast<double*>(arg)));
        WideTvsRaggedArgs A;
        memset(&A, 0, sizeof(A));
        A.arg = static_cast<const double*>(arg); A.CW = CW; A.Tpad = Tpad; A.Tn = Tn; A.n0 = n0; A.Nc = nc; A.N = s.N;
        A.L = s.pl.max_len; A.M = M; A.kind = p->base_kernel; A.kp0 = p->base_params[0]; A.kp1 = p->base_params[1]; A.difference = p->difference ? 1 : 0;
        A.sum_levels = sum_levels; A.fx = fx; A.w = w; A.out = out; A.aux = static_cast<double*>(ax); A.order = 1;
        A.len = s.len; A.off = s.off;
        const dim3 grid(unsigned(TB), unsigned(nc < 65535 ? nc : 65535), unsigned(M));
        if (p->base_kernel == GPSIG_BASE_RBF) {
            if (E == 2) hipLaunchKernelGGL((wide_tvs_fwd_ragged_kernel<2, WIDE_KD_RBF>), grid, dim3(64), 0, c->stream, A);
            else hipLaunchKernelGGL((wide_tvs_fwd_ragged_kernel<1, WIDE_KD_RBF>), grid, dim3(64), 0, c->stream, A);
        } else {
            if (E == 2) hipLaunchKernelGGL((wide_tvs_fwd_ragged_kernel<2, WIDE_KD_MATERN>), grid, dim3(64), 0, c->stream, A);
            else hipLaunchKernelGGL((wide_tvs_fwd_ragged_kernel<1, WIDE_KD_MATERN>), grid, dim3(64), 0, c->stream, A);
        }
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(wide_tvs_epilogue_kernel<>, dim3(grid_for(nc * Tn)), dim3(256), 0, c->stream, static_cast<const WideTvsArgs&>(A));
        HIPCHK(c, hipGetLastError());
    }
    return GPSIG_OK;
}

// K / the Gram of the covariances on prepared sides (s2 == NULL: symmetric), as api.hip's seq_K_generic composes the dense one: factors, raw levels, epilogue
int rg_K(gpsig_ctx* c, const gpsig_params* p, int d, const RgSide& s1, const RgSide* s2, int return_levels, double* out) {
    const bool sym = s2 == nullptr;
    const RgSide& sr = sym ? s1 : *s2;
    const int M1 = p->num_levels + 1;
    const double* w;
    CHK(upload_weights(c, p, &w));
    const double *fa = nullptr, *fb = nullptr;
    double jitter_diag = 0.0;
    if (p->normalization) {
        CHK(rg_side_factors(c, p, d, s1, w, B_DLEV0, B_FAC0, &fa));
        if (sym) CHK(rg_factors_again(c, p, s1.N, static_cast<const double*>(c->buf[B_DLEV0].p), nullptr, p->jitter, B_FAC1, &fb));
        else CHK(rg_side_factors(c, p, d, *s2, nullptr, B_DLEV1, B_FAC1, &fb));
        if (sym) jitter_diag = p->jitter;           // kernels.py:431 (symmetric) vs :463-464 (cross: diagonals only)
    } else {
        CHK(rg_factors_again(c, p, s1.N, nullptr, w, 0.0, B_FAC0, &fa));
    }
    void* lev;
    CHK(ensure(c, B_GR5, sizeof(double) * size_t(M1) * size_t(s1.N) * size_t(sr.N) + 64, &lev));
    CHK(rg_gram_levels(c, p, d, s1, sr, static_cast<double*>(lev)));
    if (s1.N > 0 && sr.N > 0) {
        hipLaunchKernelGGL(levels_epilogue_kernel, dim3(grid_for(s1.N * sr.N)), dim3(256), 0, c->stream, static_cast<const double*>(lev), s1.N, sr.N, M1, fa, fb,
                           jitter_diag, return_levels ? 0 : 1, out);
        HIPCHK(c, hipGetLastError());
    }
    return GPSIG_OK;
}

// Kdiag on a prepared side (NULL where the kernel normalises: sigma * variances, no data touched -- kernels.py:486-490)
int rg_Kdiag(gpsig_ctx* c, const gpsig_params* p, int d, const RgSide* s, int64_t N, int return_levels, double* out) {
    const int M1 = p->num_levels + 1;
    const double* w;
    CHK(upload_weights(c, p, &w));
    void* tmp;
    CHK(ensure(c, B_TMP0, sizeof(double) * size_t(N) * M1 + 8, &tmp));
    if (N == 0) return GPSIG_OK;
    if (p->normalization) hipLaunchKernelGGL(fill_kernel<double>, dim3(grid_for(N * M1)), dim3(256), 0, c->stream, static_cast<double*>(tmp), N * M1, 1.0);
    else CHK(rg_diag_levels(c, p, d, *s, static_cast<double*>(tmp)));
    hipLaunchKernelGGL(weight_levels_kernel<double>, dim3(grid_for(N)), dim3(256), 0, c->stream, static_cast<const double*>(tmp), N, M1, w, return_levels ? 0 : 1, out);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

#define ENTER_RG(c, p)     \
    ENTER(c, p);           \
    CHK(rg_check((c), (p)));

}  // namespace

extern "C" {

int gpsig_kernel_Kdiag_ragged(gpsig_ctx* c, const gpsig_params* p, const void* X, int64_t N, int32_t L, const int32_t* lengths, int32_t return_levels,
                              void* out) {
    ENTER_RG(c, p);
    ScaleParams sp;
    CHK(scale_params(c, p, true, &sp));
    const size_t ob = sizeof(double) * size_t(N) * (return_levels ? p->num_levels + 1 : 1);
    void* dout;
    CHK(out_dev(c, B_OUT0, out, ob, &dout));
    RgSide s;
    CHK(rg_side(c, p, sp, X, B_IN0, N, L, lengths, false, B_RG0, B_RG2, &s));          // (normalised too: the lengths are checked)
    CHK(rg_Kdiag(c, p, sp.d_eff(), &s, N, return_levels, static_cast<double*>(dout)));
    CHK(out_done(c, out, dout, ob));
    return finish(c);
}

int gpsig_kernel_K_tens_vs_seq_ragged(gpsig_ctx* c, const gpsig_params* p, const void* Z, const void* X, int64_t T, int64_t N, int32_t L,
                                      const int32_t* lengths, int32_t increments, int32_t return_levels, void* out) {
    ENTER_RG(c, p);
    ScaleParams sp;
    CHK(scale_params(c, p, true, &sp));
    const int d = sp.d_eff(), lt = p->num_levels * (p->num_levels + 1) / 2, E = increments ? 2 : 1;
    const void* dZ;
    CHK(in_dev(c, B_IN0, Z, sizeof(double) * size_t(lt) * T * E * d, &dZ));
    const size_t ob = sizeof(double) * size_t(T) * N * (return_levels ? p->num_levels + 1 : 1);
    void* dout;
    CHK(out_dev(c, B_OUT0, out, ob, &dout));
    RgSide s;
    CHK(rg_side(c, p, sp, X, B_IN1, N, L, lengths, false, B_RG0, B_RG2, &s));
    const double *fx = nullptr, *w;
    CHK(upload_weights(c, p, &w));
    if (p->normalization) CHK(rg_side_factors(c, p, d, s, nullptr, B_DLEV0, B_FAC1, &fx));          // kernels.py:572-581
    CHK(rg_tvs(c, p, sp, d, static_cast<const double*>(dZ), s, T, increments, fx, w, return_levels ? 0 : 1, static_cast<double*>(dout)));
    CHK(out_done(c, out, dout, ob));
    return finish(c);
}

int gpsig_kernel_K_tens_n_seq_covs_ragged(gpsig_ctx* c, const gpsig_params* p, const void* Z, const void* X, int64_t T, int64_t N, int32_t L,
                                          const int32_t* lengths, int32_t increments, int32_t full_X_cov, int32_t return_levels, void* Kzz, void* Kzx,
                                          void* Kxx) {
    ENTER_RG(c, p);
    ScaleParams sp;
    CHK(scale_params(c, p, true, &sp));
    const int M1 = p->num_levels + 1, d = sp.d_eff(), lt = p->num_levels * (p->num_levels + 1) / 2, E = increments ? 2 : 1;
    const size_t lv = return_levels ? size_t(M1) : 1;
    const void* dZ;
    CHK(in_dev(c, B_IN0, Z, sizeof(double) * size_t(lt) * T * E * d, &dZ));
    const size_t bzz = sizeof(double) * size_t(T) * T * lv, bzx = sizeof(double) * size_t(T) * N * lv;
    const size_t bxx = sizeof(double) * (full_X_cov ? size_t(N) * N : size_t(N)) * lv;
    void *dzz, *dzx, *dxx;
    CHK(out_dev(c, B_OUT0, Kzz, bzz, &dzz));
    CHK(out_dev(c, B_OUT1, Kzx, bzx, &dzx));
    CHK(out_dev(c, B_OUT2, Kxx, bxx, &dxx));
    RgSide s;
    CHK(rg_side(c, p, sp, X, B_IN1, N, L, lengths, false, B_RG0, B_RG2, &s));
    // Kzz: never normalised (kernels.py:623, :641/:665), and no sequence in it: the dense call's
    CHK(tens_gram_f64(c, p, dZ, T, increments, return_levels, dzz));
    const double *fx = nullptr, *w;
    CHK(upload_weights(c, p, &w));
    if (p->normalization) CHK(rg_side_factors(c, p, d, s, nullptr, B_DLEV0, B_FAC1, &fx));          // kernels.py:638 / :660
    CHK(rg_tvs(c, p, sp, d, static_cast<const double*>(dZ), s, T, increments, fx, w, return_levels ? 0 : 1, static_cast<double*>(dzx)));
    if (full_X_cov) CHK(rg_K(c, p, d, s, nullptr, return_levels, static_cast<double*>(dxx)));          // kernels.py:630-640
    else CHK(rg_Kdiag(c, p, d, &s, N, return_levels, static_cast<double*>(dxx)));                      // kernels.py:653-663
    CHK(out_done(c, Kzz, dzz, bzz));
    CHK(out_done(c, Kzx, dzx, bzx));
    CHK(out_done(c, Kxx, dxx, bxx));
    return finish(c);
}

int gpsig_kernel_K_ragged(gpsig_ctx* c, const gpsig_params* p, const void* X, const void* X2, int64_t N1, int64_t N2, int32_t L1, const int32_t* lengths,
                          int32_t L2, const int32_t* lengths2, int32_t return_levels, void* out) {
    ENTER_RG(c, p);
    ScaleParams sp;
    CHK(scale_params(c, p, true, &sp));
    const bool sym = X2 == nullptr;
    const int64_t Nc = sym ? N1 : N2;
    const size_t ob = sizeof(double) * size_t(N1) * size_t(Nc) * (return_levels ? p->num_levels + 1 : 1);
    void* dout;
    CHK(out_dev(c, B_OUT0, out, ob, &dout));
    RgSide s1, s2;
    CHK(rg_side(c, p, sp, X, B_IN0, N1, L1, lengths, true, B_RG0, B_RG2, &s1));
    if (!sym) CHK(rg_side(c, p, sp, X2, B_IN1, N2, L2, lengths2, true, B_RG1, B_RG3, &s2));
    CHK(rg_K(c, p, sp.d_eff(), s1, sym ? nullptr : &s2, return_levels, static_cast<double*>(dout)));
    CHK(out_done(c, out, dout, ob));
    return finish(c);
}

}  // extern "C"
