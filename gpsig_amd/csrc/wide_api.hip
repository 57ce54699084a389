// wide_api.hip -- host side of the wide-state-space route (wide_kernels.hpp): augmented rows, the kernel-argument array by rocBLAS dgemm in chunks
// of whole sequences, the fused map / difference / chain kernels, and for the reverse pass the adjoint array contracted back by two more dgemms.
// Called from api.hip (evaluations, level primitives) and grad_api.hip (their gradients) with device pointers; *done = false leaves the call to the
// exact-shape kernels.  float64; RBF and the Matern families (the distance kernels: kappa is a function of the ONE number the dgemm yields) and the two
// dot-product families, whose kappa IS that number: SignatureLinear on plain rows -- increments where the kernel takes differences, so that the kernels run in
// their difference = 0 form on one row less and half the tensor columns --, SignatureCosine on unit rows.
// SignaturePoly (whole degrees) on plain rows; SignatureMix on the distance kernels' rows, psi of the dgemm's number plus the one-sided norm terms (mix_sides).
// SignatureSpectral in exact mode beyond 32 columns, forward only (wide_spectral): kappa is no function of one inner product, so the argument array is
// filled by wide_spectral_kernel.hpp's kernel on plain rows instead of the dgemm, and holds kappa itself -- the kernels run in their identity kind with
// SignatureCosine's difference handling.  Every entry depends on its row and column alone: the same bits under any chunking.
#include "ctx.hpp"
#include "api_common.hpp"
#include "launchers.hpp"
#include "aux_kernels.hpp"
#include "wide_kernels.hpp"
#include "wide_spectral_kernel.hpp"

#include <string>

namespace gpsig {

// (shared with the ragged form of the route, wide_ragged_api.hip: launchers.hpp)
size_t wide_chunk_bytes(const gpsig_ctx* c) {
    if (c->wide_chunk_mb > 0) return size_t(c->wide_chunk_mb) << 20;
    // 4 GB by default (the forward pass holds one such array, the reverse pass two and the partial sums of the narrow contraction: a launch of a
    // minibatch is bound by the serial sweep of one chain, so halving it doubles that time -- NetFlow's shape is 2 GB); grad_scratch_mb scales it
    return size_t(c->grad_scratch_mb > 0 ? c->grad_scratch_mb : 4096) << 20;
}
// wavefronts per lattice: a launch of few lattices of more than 256 columns spreads each lattice's columns over eight wavefronts of one column per
// lane instead of eight columns per lane of one (NetFlow's / CMUsubject16's level diagonals, 50 / 23 lattices of 499 x 499: reverse pass 3.5 -> 3.2 / 2.9 ms;
// at four and two columns per lane the barrier per step costs more than the shorter steps save: AUSLAN 0.74 -> 0.79).  Option wide_lat_waves: 0 never,
// 1 wherever there are two or more columns per lane (the tests), -1 this rule
int wide_lat_waves(const gpsig_ctx* c, int C, int64_t lattices) {
    if (C < 2 || c->wide_lat_waves == 0) return 1;
    if (c->wide_lat_waves > 0) return C;
    return (C == 8 && lattices <= 128) ? C : 1;
}
int wide_lat_columns(int R2) { return R2 <= 64 ? 1 : (R2 <= 128 ? 2 : (R2 <= 256 ? 4 : 8)); }

namespace {

// (SignaturePoly: the whole degrees 1 .. 8 of the kernels' repeated squaring -- any other degree is left to the routes that call the library's pow)
bool wide_kind(const gpsig_params* p) {
    const int base_kernel = p->base_kernel;
    if (base_kernel == GPSIG_BASE_POLY) return wide_poly_degree(p) > 0;
    if (base_kernel == GPSIG_BASE_MIX) return true;
    return base_kernel == GPSIG_BASE_RBF || base_kernel == GPSIG_BASE_MATERN12 || base_kernel == GPSIG_BASE_MATERN32 || base_kernel == GPSIG_BASE_MATERN52 ||
           wide_dot_kind(base_kernel);
}
// the kernels' compile-time kind, and the form of the rows that go into the dgemm
// (SignaturePoly: the points themselves as plain rows, a = <z, x>; it is non-linear, so its differences are taken on kappa inside the kernels)
int kind_of(int base_kernel) {
    if (base_kernel == GPSIG_BASE_POLY) return WIDE_KD_POLY;
    if (base_kernel == GPSIG_BASE_MIX) return WIDE_KD_MIX;          // (the distance kernels' augmented rows: rows_mode falls through to WIDE_ROWS_DIST)
    if (base_kernel == GPSIG_BASE_SPECTRAL) return WIDE_KD_ID;      // (the argument array holds kappa: wide_spectral_kernel.hpp)
    return base_kernel == GPSIG_BASE_RBF ? WIDE_KD_RBF : (wide_dot_kind(base_kernel) ? WIDE_KD_ID : WIDE_KD_MATERN);
}
int rows_mode(int base_kernel) {
    if (base_kernel == GPSIG_BASE_POLY || base_kernel == GPSIG_BASE_SPECTRAL) return WIDE_ROWS_PLAIN;
    return base_kernel == GPSIG_BASE_LINEAR ? WIDE_ROWS_PLAIN : (base_kernel == GPSIG_BASE_COSINE ? WIDE_ROWS_UNIT : WIDE_ROWS_DIST);
}
// SignatureLinear: <.,.> is bilinear, so the differences along the sequences (signature_algs.py:26 / :114) and between a tensor's two points
// (kernels.py:329-330) are taken on the ROWS -- exact to rounding under translation, like the exact-shape kernels' MODE_INC, where a four-term difference of
// inner products of shifted paths is not -- and the kernels see difference = 0, one row less per sequence and one column per component
bool rows_are_increments(const gpsig_params* p) { return p->base_kernel == GPSIG_BASE_LINEAR && p->difference; }
bool tensors_collapse(const gpsig_params* p, int increments) { return p->base_kernel == GPSIG_BASE_LINEAR && increments; }

// body with KD = the compile-time kind of base kernel `base`
#define GPSIG_WIDE_KIND(base, ...)                                                            \
    switch (kind_of(base)) {                                                                  \
        case WIDE_KD_RBF: { constexpr int KD = WIDE_KD_RBF; __VA_ARGS__; } break;             \
        case WIDE_KD_ID: { constexpr int KD = WIDE_KD_ID; __VA_ARGS__; } break;               \
        case WIDE_KD_POLY: { constexpr int KD = WIDE_KD_POLY; __VA_ARGS__; } break;           \
        case WIDE_KD_MIX: { constexpr int KD = WIDE_KD_MIX; __VA_ARGS__; } break;             \
        default: { constexpr int KD = WIDE_KD_MATERN; __VA_ARGS__; } break;                   \
    }

// SignatureMix: kappa = psi(a) + q (h_row + h_column) (wide_kernels.hpp: WIDE_KD_MIX).  Which of the two one-sided terms a primitive's kernels must add,
// and its reverse pass must carry back -- the ONE place that decides it, for the forward and the reverse entry points alike.  A side's term is the same
// number at both ends of any difference taken along the OTHER side, and cancels there:
//   Kzx (rows = sequence points, columns = tensor points): the time difference runs along the rows and cancels the COLUMNS' term; increments subtract a
//   tensor's two points and cancel the ROWS' term;
//   sequence lattices: the double difference cancels both, without it both stay;   Kzz: the four-term difference of increments cancels both, without both stay.
struct MixSides { bool rows, cols; };
enum MixPrim { MIX_TVS, MIX_LAT, MIX_TENS };
MixSides mix_sides(const gpsig_params* p, MixPrim prim, int increments) {
    MixSides s = {false, false};
    if (p->base_kernel != GPSIG_BASE_MIX) return s;
    if (prim == MIX_TVS) { s.rows = !increments; s.cols = !p->difference; }
    else if (prim == MIX_LAT) s.rows = s.cols = !p->difference;
    else s.rows = s.cols = !increments;
    return s;
}

int dgemm(gpsig_ctx* c, bool ta, bool tb, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, const double* B, int64_t ldb, double beta,
          double* C, int64_t ldc) {
    if (m > 0x7fffffff || n > 0x7fffffff || k > 0x7fffffff || lda > 0x7fffffff || ldb > 0x7fffffff || ldc > 0x7fffffff)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "wide route: a matrix dimension beyond 2^31");
    if (m == 0 || n == 0) return GPSIG_OK;
    std::string err;
    if (!solver_dgemm(&c->blas_handle, c->stream, ta, tb, int(m), int(n), int(k), 1.0, A, int(lda), B, int(ldb), beta, C, int(ldc), &err))
        return fail(c, GPSIG_ERR_HIP, "%s", err.c_str());
    return GPSIG_OK;
}

int dgemm_batched(gpsig_ctx* c, bool ta, bool tb, int64_t m, int64_t n, int64_t k, const double* A, int64_t lda, int64_t sa, const double* B, int64_t ldb,
                  int64_t sb, double* C, int64_t ldc, int64_t sc, int64_t batch) {
    if (m > 0x7fffffff || n > 0x7fffffff || k > 0x7fffffff || batch > 0x7fffffff)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "wide route: a matrix dimension beyond 2^31");
    if (m == 0 || n == 0 || batch == 0) return GPSIG_OK;
    std::string err;
    if (!solver_dgemm_batched(&c->blas_handle, c->stream, ta, tb, int(m), int(n), int(k), 1.0, A, int(lda), sa, B, int(ldb), sb, 0.0, C, int(ldc), sc, int(batch), &err))
        return fail(c, GPSIG_ERR_HIP, "%s", err.c_str());
    return GPSIG_OK;
}

// ---- SignatureSpectral (exact mode beyond 32 columns): what a call computes once -- the table on the device, gamma^2 -- and per side
struct SpxSetup {
    const double *alpha, *omega, *g2;
    int Q, family, d;
};
int spx_setup(gpsig_ctx* c, const gpsig_params* p, int d, SpxSetup* s) {
    const double* tab;
    CHK(spectral_table_wide(c, p, &tab));
    s->Q = int(p->base_params[0]); s->family = int(p->base_params[1]); s->d = d;
    s->alpha = tab; s->omega = tab + s->Q;
    void* g2;
    CHK(ensure(c, B_WS0, sizeof(double) * size_t(s->Q) * d + 64, &g2));
    const int rc = wide_spx_prep_launch(c->stream, s->omega + size_t(s->Q) * d, int64_t(s->Q) * d, static_cast<double*>(g2));
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral wide route: %s", hipGetErrorString(hipError_t(rc)));
    s->g2 = static_cast<const double*>(g2);
    return GPSIG_OK;
}
// the norms and phases (Q, rows) each of the plain rows X (rows, d + 2), in buffer `id`: *nrm, then the phases `Q * rows` doubles on
int spx_side(gpsig_ctx* c, const SpxSetup& s, const double* X, int64_t rows, int id, const double** nrm) {
    void* b;
    CHK(ensure(c, id, sizeof(double) * 2 * size_t(s.Q) * size_t(rows) + 64, &b));
    double* n = static_cast<double*>(b);
    const int rc = wide_spx_side_launch(c->stream, X, rows, s.d + 2, s.d, s.Q, s.omega, s.g2, n, n + int64_t(s.Q) * rows);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral wide route: %s", hipGetErrorString(hipError_t(rc)));
    *nrm = n;
    return GPSIG_OK;
}
// C_b (m, ldc) = kappa(A_b (m, d + 2), B_b (n, d + 2)) for `batch` matrices `sa`, `sb`, `sc` doubles apart; nA / nB: spx_side's arrays of ALL `planeA` /
// `planeB` rows of the two sides, the first row of A_0 / B_0 at row a0 / b0 of them
int spx_arguments(gpsig_ctx* c, const SpxSetup& s, const double* A, const double* B, double* C, int64_t m, int64_t n, int64_t ldc, int64_t sa, int64_t sb,
                  int64_t sc, int64_t batch, const double* nA, int64_t planeA, int64_t a0, const double* nB, int64_t planeB, int64_t b0) {
    if (m > 0x7fffffff || n > 0x7fffffff || ldc > 0x7fffffff) return fail(c, GPSIG_ERR_UNSUPPORTED, "wide route: a matrix dimension beyond 2^31");
    const int DA = s.d + 2;
    WideSpxArgs K;
    memset(&K, 0, sizeof(K));
    K.A = A; K.B = B; K.C = C; K.m = m; K.n = n; K.lda = DA; K.ldb = DA; K.ldc = ldc; K.sa = sa; K.sb = sb; K.sc = sc; K.batch = batch;
    K.d = s.d; K.Q = s.Q; K.family = s.family; K.alpha = s.alpha; K.g2 = s.g2;
    K.nrmA = nA + a0; K.phA = nA + int64_t(s.Q) * planeA + a0; K.planeA = planeA; K.rowsA = sa / DA;
    K.nrmB = nB + b0; K.phB = nB + int64_t(s.Q) * planeB + b0; K.planeB = planeB; K.rowsB = sb / DA;
    const int rc = wide_spx_launch(c->stream, K);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral wide route: %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}
bool spx_context_ok(const gpsig_ctx* c, const gpsig_params* p) {
    return c->wide != 0 && !routes_as_captured(c) && p->num_levels >= 1 && p->num_levels <= WIDE_MAX_LEVELS;
}

int aug_rows(gpsig_ctx* c, const double* src, int64_t rows, int d, int right, int mode, int diff, double* dst) {
    if (rows == 0) return GPSIG_OK;
    ScaleParams none;
    memset(&none, 0, sizeof(none));
    none.d_in = d;
    hipLaunchKernelGGL(wide_aug_rows_kernel, dim3(unsigned(rows < 65535 ? rows : 65535)), dim3(64), 0, c->stream, src, rows, d, right, 0, int64_t(0), int64_t(0), 1,
                       none, mode, diff, dst);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

typedef void (*WideLatKernel)(const WideLatArgs);
template <int LQ, int KD>
WideLatKernel lat_kernel_of(int C, bool bwd, int NW) {
    if (NW == 2) return bwd ? wide_lattice_bwd_kernel<1, LQ, KD, 2> : wide_lattice_fwd_kernel<1, LQ, KD, 2>;
    if (NW == 4) return bwd ? wide_lattice_bwd_kernel<1, LQ, KD, 4> : wide_lattice_fwd_kernel<1, LQ, KD, 4>;
    if (NW == 8) return bwd ? wide_lattice_bwd_kernel<1, LQ, KD, 8> : wide_lattice_fwd_kernel<1, LQ, KD, 8>;
    switch (C) {
        case 1: return bwd ? wide_lattice_bwd_kernel<1, LQ, KD> : wide_lattice_fwd_kernel<1, LQ, KD>;
        case 2: return bwd ? wide_lattice_bwd_kernel<2, LQ, KD> : wide_lattice_fwd_kernel<2, LQ, KD>;
        case 4: return bwd ? wide_lattice_bwd_kernel<4, LQ, KD> : wide_lattice_fwd_kernel<4, LQ, KD>;
        default: return bwd ? wide_lattice_bwd_kernel<8, LQ, KD> : wide_lattice_fwd_kernel<8, LQ, KD>;
    }
}
// levels kept by a lane: 3 (num_levels <= 4) or 7; the RBF kernel and the identity (dot-product families) at compile time, the Matern families at run time.  NW > 1: NW wavefronts per
// lattice with one column per lane (C is ignored)
WideLatKernel lat_kernel(int M, int C, bool bwd, int base_kernel, int NW = 1) {
    GPSIG_WIDE_KIND(base_kernel, return M <= 4 ? lat_kernel_of<3, KD>(C, bwd, NW) : lat_kernel_of<7, KD>(C, bwd, NW))
    return nullptr;
}

// the augmented rows of both sides: ZA (lt * E * Tpad, DA) left form, XA (NL, DA) right form.  E, NL: as the KERNELS see them -- SignatureLinear: E = 1 from
// the caller's two points per tensor (zdiff), NL = N (L - 1) increment rows of sequences of xdiff = L observations
int wide_tvs_rows(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& sz, const double* Z, const double* Xs, int lt, int E, int64_t Tn, int64_t Tpad, int64_t NL,
                  int d, int zdiff, int xdiff, double** ZA, double** XA) {
    const int mode = rows_mode(p->base_kernel);
    const int DA = d + 2;
    const int64_t zr = int64_t(lt) * E * Tpad;
    void *za, *xa;
    CHK(ensure(c, B_WD0, sizeof(double) * size_t(zr) * DA + 64, &za));
    CHK(ensure(c, B_WD1, sizeof(double) * size_t(NL) * DA + 64, &xa));
    ScaleParams none;
    memset(&none, 0, sizeof(none));
    none.d_in = d;
    hipLaunchKernelGGL(wide_aug_rows_kernel, dim3(unsigned(zr < 65535 ? zr : 65535)), dim3(64), 0, c->stream, Z, zr, d, 0, lt, Tn, Tpad, E, sz,
                       mode, zdiff, static_cast<double*>(za));
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(wide_aug_rows_kernel, dim3(unsigned(NL < 65535 ? NL : 65535)), dim3(64), 0, c->stream, Xs, NL, d, 1, 0, int64_t(0), int64_t(0), 1,
                       none, mode, xdiff, static_cast<double*>(xa));
    HIPCHK(c, hipGetLastError());
    *ZA = static_cast<double*>(za); *XA = static_cast<double*>(xa);
    return GPSIG_OK;
}

// The two contractions of a reverse pass with the adjoint array W (R, CW) of an argument array  arg = XA (R, DA) ZA^T (CW, DA):
//     gXA (R, DA) = W ZA   (overwritten),      gZA (CW, DA) (+)= W^T XA   (accumulated over the chunks of R).
int contract_both(gpsig_ctx* c, const double* W, const double* XA, const double* ZA, int64_t R, int64_t CW, int DA, bool accumulate, double* gXA, double* gZA) {
    if (DA <= 32 && c->wide_contract != 0) {
        // narrow rows: both contractions in one hand-written pass over W (wide_contract_kernel); rocBLAS spreads such skinny products over too few tiles
        const int64_t strips = (R + 63) / 64, ntiles = (CW + 63) / 64;
        const int DAP = DA <= 16 ? 16 : 32;
        int64_t groups = ((DAP == 16 && c->wide_contract != 2 ? 8192 : 4096) + strips - 1) / strips;            // several wavefronts per SIMD
        if (groups > ntiles) groups = ntiles;
        if (groups < 1) groups = 1;
        void *part, *gxp;
        CHK(ensure(c, B_WD9, sizeof(double) * size_t(strips) * CW * DAP + 64, &part));
        CHK(ensure(c, B_WD8, sizeof(double) * size_t(groups) * R * DAP + 64, &gxp));
        WideContractArgs K;
        memset(&K, 0, sizeof(K));
        K.W = W; K.XA = XA; K.ZA = ZA; K.R = R; K.CW = CW; K.DA = DA; K.groups = int(groups);
        K.gXA_part = static_cast<double*>(gxp); K.part = static_cast<double*>(part);
        const dim3 gridc(unsigned(strips < 65535 ? strips : 65535), unsigned(groups));
        // 1 (default): part tiles of 16 rows (8.3 KB of LDS per wavefront; 1.18 ms per 4 GB of W at 12 columns where the first form takes 3.14), 3: of 32 rows (1.53), 2: the first form
        if (DAP == 16 && c->wide_contract == 3) hipLaunchKernelGGL(wide_contract16_kernel<32>, gridc, dim3(64), 0, c->stream, K);
        else if (DAP == 16 && c->wide_contract != 2) hipLaunchKernelGGL(wide_contract16_kernel<16>, gridc, dim3(64), 0, c->stream, K);
        else if (DAP == 16) hipLaunchKernelGGL(wide_contract_kernel<16>, gridc, dim3(64), 0, c->stream, K);
        else hipLaunchKernelGGL(wide_contract_kernel<32>, gridc, dim3(64), 0, c->stream, K);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(wide_contract_reduce_kernel, dim3(grid_for(CW * DA)), dim3(256), 0, c->stream, static_cast<const double*>(part), strips, CW, DA, DAP,
                           accumulate ? 1 : 0, gZA);
        hipLaunchKernelGGL(wide_contract_reduce_kernel, dim3(grid_for(R * DA)), dim3(256), 0, c->stream, static_cast<const double*>(gxp), groups, R, DA, DAP, 0, gXA);
        HIPCHK(c, hipGetLastError());
        return GPSIG_OK;
    }
    // gZA (CW, DA) += W^T XA:  column-major gZA^T (DA x CW) = XA_cm (DA x R) W_cm^T (R x CW)
    CHK(dgemm(c, false, true, DA, CW, R, XA, DA, W, CW, accumulate ? 1.0 : 0.0, gZA, DA));
    // gXA (R, DA) = W ZA:   column-major gXA^T (DA x R) = ZA_cm (DA x CW) W_cm (CW x R)
    return dgemm(c, false, false, DA, R, CW, ZA, DA, W, CW, 0.0, gXA, DA);
}

// SignaturePoly's offset: g_base[0] += the sum of the n partial sums that a reverse pass left in part (room for WIDE_GB_BLOCKS more doubles behind them), in
// an order that depends on n alone (wide_sum_kernel)
constexpr int WIDE_GB_BLOCKS = 1024;
int gbase_reduce(gpsig_ctx* c, double* part, int64_t n, double* g_base) {
    const int64_t nb = (n + 255) / 256;
    const int blocks = int(nb < 1 ? 1 : (nb > WIDE_GB_BLOCKS ? WIDE_GB_BLOCKS : nb));
    hipLaunchKernelGGL(wide_sum_kernel, dim3(blocks), dim3(256), 0, c->stream, static_cast<const double*>(part), n, 0, part + n);
    hipLaunchKernelGGL(wide_sum_kernel, dim3(1), dim3(256), 0, c->stream, static_cast<const double*>(part + n), int64_t(blocks), 1, g_base);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

}  // namespace

// Is the route built for this call?  (float64 is the caller's business.)
bool wide_tvs_available(const gpsig_ctx* c, const gpsig_params* p, int d, int64_t Tn, int64_t N, int L) {
    if (c->wide == 0 || routes_as_captured(c)) return false;
    if (!wide_kind(p) || (p->order > WIDE_MAX_ORDER && p->num_levels > WIDE_MAX_ORDER) || p->num_levels > WIDE_MAX_LEVELS || p->num_levels < 1) return false;
    if (Tn < 1 || N < 1 || L < 1 || d < 1) return false;
    if (rows_are_increments(p) && L < 2) return false;        // (no increment rows)
    return true;
}

// ---- the forward side's own predicates: exact-mode SignatureSpectral beyond 32 columns is served by the forward functions only
bool wide_spectral(const gpsig_params* p) { return p->base_kernel == GPSIG_BASE_SPECTRAL && p->num_features * (p->num_lags + 1) > SPECTRAL_STRIDE; }

bool wide_tvs_fwd_available(const gpsig_ctx* c, const gpsig_params* p, int d, int64_t Tn, int64_t N, int L) {
    if (!wide_spectral(p)) return wide_tvs_available(c, p, d, Tn, N, L);
    return spx_context_ok(c, p) && !(p->order > WIDE_MAX_ORDER && p->num_levels > WIDE_MAX_ORDER) && Tn >= 1 && N >= 1 && L >= 1;
}
static bool tens_fits(const gpsig_params* p, int64_t Tn) {
    const int64_t Tpad = (Tn + 63) / 64 * 64;
    return Tn >= 1 && size_t(p->num_levels * (p->num_levels + 1) / 2) * size_t(4 * Tpad * Tpad) * sizeof(double) <= (size_t(2) << 30);
}
bool wide_tens_fwd_available(const gpsig_ctx* c, const gpsig_params* p, int64_t Tn) {
    if (!wide_spectral(p)) return wide_tens_available(c, p, Tn);
    return spx_context_ok(c, p) && tens_fits(p, Tn);
}
bool wide_lat_fwd_available(const gpsig_ctx* c, const gpsig_params* p, int L1, int L2) {
    if (!wide_spectral(p)) return wide_lat_available(c, p, L1, L2);
    return spx_context_ok(c, p) && !(p->order > 1 && p->num_levels > 1) && L1 >= 1 && L2 >= 1 && L2 - (p->difference ? 1 : 0) <= 512;
}
// why a call of exact-mode SignatureSpectral beyond 32 columns is not served (lattice: a sequence lattice of L2 columns; else Kzx / Kzz)
int wide_spectral_refusal(gpsig_ctx* c, const gpsig_params* p, bool lattice, int L2) {
    const char* const who = "exact-mode SignatureSpectral beyond 32 columns (spectral_wide)";
    if (c->wide == 0) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s runs on the wide route only: context option wide = 0 refuses it", who);
    if (routes_as_captured(c))
        return fail(c, GPSIG_ERR_UNSUPPORTED, "graph recording: %s is served by the wide route only, which does not record (the exact-shape kernels that record reach %d columns)", who,
                    int(SPECTRAL_STRIDE));
    if (p->num_levels > WIDE_MAX_LEVELS) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s is built for num_levels <= %d (got %d)", who, WIDE_MAX_LEVELS, p->num_levels);
    if (lattice && p->order > 1 && p->num_levels > 1)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "%s serves first-order sequence lattices only (order = %d; Kzx: orders <= %d)", who, p->order, WIDE_MAX_ORDER);
    if (lattice) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s serves sequence lattices of at most 512 columns (got %d)", who, L2 - (p->difference ? 1 : 0));
    if (p->order > WIDE_MAX_ORDER && p->num_levels > WIDE_MAX_ORDER) return fail(c, GPSIG_ERR_UNSUPPORTED, "%s serves Kzx at orders <= %d (got %d)", who, WIDE_MAX_ORDER, p->order);
    return fail(c, GPSIG_ERR_UNSUPPORTED, "%s: the argument blocks of the inducing tensors must fit 2 GB, and every size must be positive", who);
}

// Kzx (kernels.py:313-340 + signature_algs.py:101-127 + the epilogue of kernels.py:572-588).  Z: the caller's (lt, T, E, d) array, scaled here when
// sz.has_ls; Xs: (N, L, d) scaled sequences.  fx (N, M+1), w (M+1): factors or NULL.  out: (T, N) level sum or (M+1, T, N).  aux: chain totals or NULL.
int wide_tvs_forward(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& sz, int d, const double* Z, const double* Xs, int64_t Tn, int64_t N, int L,
                     int increments, const double* fx, const double* w, int sum_levels, double* out, double* aux) {
    const bool xinc = rows_are_increments(p), zinc = tensors_collapse(p, increments);
    const int xdiff = xinc ? L : 0;
    if (xinc) L -= 1;                                            // the kernels' rows per sequence
    const int M = p->num_levels, lt = M * (M + 1) / 2, E = (increments && !zinc) ? 2 : 1, DA = d + 2;
    const int64_t Tpad = (Tn + 63) / 64 * 64, CW = int64_t(lt) * E * Tpad, TB = Tpad / 64;
    double *ZA, *XA;
    CHK(wide_tvs_rows(c, p, sz, Z, Xs, lt, E, Tn, Tpad, N * int64_t(L), d, zinc ? 1 : 0, xdiff, &ZA, &XA));
    const size_t per_seq = sizeof(double) * size_t(L) * CW;
    int64_t chunk = int64_t(wide_chunk_bytes(c) / per_seq);
    if (chunk < 1) chunk = 1;
    if (chunk > N) chunk = N;
    void* arg;
    CHK(ensure(c, B_WD2, per_seq * size_t(chunk) + 64, &arg));
    if (!aux) {          // the chain totals the epilogue reads: the caller's array (kept for the reverse pass) or scratch
        void* ax;
        CHK(ensure(c, B_WD8, sizeof(double) * size_t(N) * lt * Tpad + 64, &ax));
        aux = static_cast<double*>(ax);
    }
    hipEvent_t e0, e1;
    bool timed;
    CHK(timing_begin(c, &e0, &e1, &timed));
    const bool spx = wide_spectral(p);
    SpxSetup ss;
    const double *nz = nullptr, *nx = nullptr;
    if (spx) {
        CHK(spx_setup(c, p, d, &ss));
        CHK(spx_side(c, ss, ZA, CW, B_WS1, &nz));
        CHK(spx_side(c, ss, XA, N * int64_t(L), B_WS2, &nx));
    }
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int64_t nc = N - n0 < chunk ? N - n0 : chunk;
        // row-major arg (nc L, CW) = XA_chunk (nc L, DA) ZA^T  ==  column-major arg^T (CW x nc L) = ZA_cm^T (CW x DA) XA_cm (DA x nc L)
        if (spx) CHK(spx_arguments(c, ss, XA + n0 * L * DA, ZA, static_cast<double*>(arg), nc * L, CW, CW, 0, 0, 0, 1, nx, N * int64_t(L), n0 * L, nz, CW, 0));
        else CHK(dgemm(c, true, false, CW, nc * L, DA, ZA, DA, XA + n0 * L * DA, DA, 0.0, static_cast<double*>(arg), CW));
        WideTvsArgs A;
        memset(&A, 0, sizeof(A));
        A.arg = static_cast<const double*>(arg); A.CW = CW; A.Tpad = Tpad; A.Tn = Tn; A.n0 = n0; A.Nc = nc; A.N = N;
        A.L = L; A.M = M; A.kind = p->base_kernel; A.kp0 = p->base_params[0]; A.kp1 = p->base_params[1]; A.difference = (p->difference && !xinc) ? 1 : 0; A.sum_levels = sum_levels;
        A.fx = fx; A.w = w; A.out = out; A.aux = aux; A.order = p->order < p->num_levels ? p->order : p->num_levels;
        const MixSides ms = mix_sides(p, MIX_TVS, increments);          // (the rows' own norm column: d + 1 of the right form, d of the left form)
        A.nrm_ld = DA; A.nrm_row = ms.rows ? XA + d + 1 : nullptr; A.nrm_col = ms.cols ? ZA + d : nullptr;
        const dim3 grid(unsigned(TB), unsigned(nc < 65535 ? nc : 65535), unsigned(M));
        GPSIG_WIDE_KIND(p->base_kernel,
                        if (E == 2) hipLaunchKernelGGL((wide_tvs_fwd_kernel<2, KD>), grid, dim3(64), 0, c->stream, A);
                        else hipLaunchKernelGGL((wide_tvs_fwd_kernel<1, KD>), grid, dim3(64), 0, c->stream, A))
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(wide_tvs_epilogue_kernel, dim3(grid_for(nc * Tn)), dim3(256), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    if (timed) {
        HIPCHK(c, hipEventRecord(e1, c->stream));
        c->t_launches += 1;
        c->t_pairs += Tn * N;
        c->t_kernel = spx ? "wide_tvs (wide_spx_kernel + wide_tvs_fwd_kernel)" : "wide_tvs (dgemm + wide_tvs_fwd_kernel)";
        c->t_flops += 2.0 * double(CW) * double(N) * L * DA;
    }
    return GPSIG_OK;
}

// The reverse pass.  Z (lt, T, E, d), X (N, L, d): scaled operands as the gradient entry points take them.  fac == NULL: G (M+1, T, N), gradient of the
// level array; fac (N, M+1): G (T, N), gradient of the weighted level sum, and gfac (N, M+1) receives the factors' gradient.
int wide_tvs_backward(gpsig_ctx* c, const gpsig_params* p, int d, const double* Z, const double* X, const double* G, int64_t Tn, int64_t N, int L,
                      int increments, const double* fac, const double* aux, double* gZ, double* gX, double* gfac, double* g_base) {
    const bool xinc = rows_are_increments(p), zinc = tensors_collapse(p, increments);
    const int xdiff = xinc ? L : 0, mode = rows_mode(p->base_kernel);
    const int64_t NLx = N * int64_t(L);                          // the caller's rows
    if (xinc) L -= 1;                                            // the kernels' rows per sequence
    const int M = p->num_levels, lt = M * (M + 1) / 2, Ez = increments ? 2 : 1, E = zinc ? 1 : Ez, DA = d + 2;
    const int64_t Tpad = (Tn + 63) / 64 * 64, CW = int64_t(lt) * E * Tpad, TB = Tpad / 64, NL = N * int64_t(L);
    ScaleParams none;
    memset(&none, 0, sizeof(none));
    none.d_in = d;
    double *ZA, *XA;
    CHK(wide_tvs_rows(c, p, none, Z, X, lt, E, Tn, Tpad, NL, d, zinc ? 1 : 0, xdiff, &ZA, &XA));
    const size_t per_seq = sizeof(double) * size_t(L) * CW;
    int64_t chunk = int64_t(wide_chunk_bytes(c) / per_seq);
    if (chunk < 1) chunk = 1;
    if (chunk > N) chunk = N;
    // SignaturePoly's offset (g_base: device, or NULL) is to come out with the same bits however the argument array is chunked.  Its partial sums are
    // indexed by the global sequence (below), but the arguments themselves must not depend on the chunking either, and a dgemm's last bits depend on its
    // shape (seen at 302 augmented columns).  So with the offset asked for, the arguments come from one dgemm per block of `blk` sequences -- a number
    // that depends on L alone, at least 256 rows --, and chunks hold whole blocks (at least one: the budget yields to that), so that every dgemm has
    // the same shape in every chunking.  (This rests on rocBLAS returning the same bits for dgemms of one shape whose outputs start at different
    // offsets of the argument buffer.  Nothing in its interface promises that; tests/test_gpu_wide_poly.py holds it at the shapes it runs.)
    // (SignatureMix's mixing: the same slots, the same dgemm blocks)
    const bool gb = g_base && wide_base_param_kind(p->base_kernel);
    const MixSides ms = mix_sides(p, MIX_TVS, increments);
    int64_t blk = chunk;                                         // sequences per dgemm
    if (gb) {
        blk = 1;
        while (blk * L < 256) blk *= 2;
        chunk = chunk / blk * blk;
        if (chunk < blk) chunk = blk;
        if (chunk > N) chunk = N;
    }
    void *arg, *Wb, *gza, *gxa, *gfp = nullptr;
    CHK(ensure(c, B_WD2, per_seq * size_t(chunk) + 64, &arg));
    CHK(ensure(c, B_WD3, per_seq * size_t(chunk) + 64, &Wb));
    CHK(ensure(c, B_WD4, sizeof(double) * size_t(CW) * DA + 64, &gza));
    CHK(ensure(c, B_WD5, sizeof(double) * size_t(NL) * DA + 64, &gxa));
    if (fac) CHK(ensure(c, B_WD6, sizeof(double) * size_t(TB) * N * (M + 1) + 64, &gfp));
    // ... every (tensor block, sequence, level) leaves the sum of its W entries in a slot of its own
    void* gbp = nullptr;
    const int64_t gbn = int64_t(TB) * N * M;
    if (gb) CHK(ensure(c, B_WD11, sizeof(double) * size_t(gbn + WIDE_GB_BLOCKS) + 64, &gbp));
    // SignatureMix, a side's term kept: the sums of the values' adjoints over the other side -- slots per (tensor block, level, row) / (sequence, column),
    // added in a fixed order below (wide_gfac_reduce_kernel), and handed to the un-augmentation of that side
    void *rap = nullptr, *cap = nullptr, *radj = nullptr, *cadj = nullptr;
    if (ms.rows) {
        CHK(ensure(c, B_WD12, sizeof(double) * size_t(TB) * M * size_t(NL) + 64, &rap));
        CHK(ensure(c, B_WD14, sizeof(double) * size_t(NL) + 64, &radj));
    }
    if (ms.cols) {
        CHK(ensure(c, B_WD13, sizeof(double) * size_t(N) * size_t(CW) + 64, &cap));
        CHK(ensure(c, B_WD15, sizeof(double) * size_t(CW) + 64, &cadj));
    }
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int64_t nc = N - n0 < chunk ? N - n0 : chunk;
        for (int64_t b0 = 0; b0 < nc; b0 += blk) {
            const int64_t nb = nc - b0 < blk ? nc - b0 : blk;
            CHK(dgemm(c, true, false, CW, nb * L, DA, ZA, DA, XA + (n0 + b0) * L * DA, DA, 0.0, static_cast<double*>(arg) + b0 * L * CW, CW));
        }
        WideTvsArgs A;
        memset(&A, 0, sizeof(A));
        A.arg = static_cast<const double*>(arg); A.CW = CW; A.Tpad = Tpad; A.Tn = Tn; A.n0 = n0; A.Nc = nc; A.N = N;
        A.L = L; A.M = M; A.kind = p->base_kernel; A.kp0 = p->base_params[0]; A.kp1 = p->base_params[1]; A.difference = (p->difference && !xinc) ? 1 : 0;
        A.fx = fac; A.w = nullptr; A.aux = const_cast<double*>(aux);
        A.G = G; A.W = static_cast<double*>(Wb); A.gfac_part = static_cast<double*>(gfp); A.weighted = fac ? 1 : 0;
        A.gb_part = static_cast<double*>(gbp);
        A.nrm_ld = DA; A.nrm_row = ms.rows ? XA + d + 1 : nullptr; A.nrm_col = ms.cols ? ZA + d : nullptr;
        A.radj_part = static_cast<double*>(rap); A.cadj_part = static_cast<double*>(cap);
        A.order = p->order < p->num_levels ? p->order : p->num_levels;
        const dim3 grid(unsigned(TB), unsigned(nc < 65535 ? nc : 65535), unsigned(M));
        GPSIG_WIDE_KIND(p->base_kernel,
                        if (E == 2) hipLaunchKernelGGL((wide_tvs_bwd_kernel<2, KD>), grid, dim3(64), 0, c->stream, A);
                        else hipLaunchKernelGGL((wide_tvs_bwd_kernel<1, KD>), grid, dim3(64), 0, c->stream, A))
        HIPCHK(c, hipGetLastError());
        CHK(contract_both(c, static_cast<const double*>(Wb), XA + n0 * L * DA, ZA, nc * int64_t(L), CW, DA, n0 > 0, static_cast<double*>(gxa) + n0 * L * DA,
                          static_cast<double*>(gza)));
    }
    const int64_t zrows = int64_t(lt) * Tn * Ez;                // the caller's rows
    const double qmix = 1.0 - p->base_params[0];
    if (ms.rows) hipLaunchKernelGGL(wide_gfac_reduce_kernel, dim3(grid_for(NL)), dim3(256), 0, c->stream, static_cast<const double*>(rap), int(TB * M), NL,
                                    static_cast<double*>(radj));
    if (ms.cols) hipLaunchKernelGGL(wide_gfac_reduce_kernel, dim3(grid_for(CW)), dim3(256), 0, c->stream, static_cast<const double*>(cap), int(N), CW,
                                    static_cast<double*>(cadj));
    HIPCHK(c, hipGetLastError());
    // (plain rows -- SignatureLinear without increments / differences -- take the distance kernels' un-augmentation as it is: both extra columns of
    // such rows are zero on BOTH sides, so the adjoint of the norm column, a product with the other side's zero column, is exactly 0 and g = ga)
    if (mode == WIDE_ROWS_UNIT)
        hipLaunchKernelGGL(wide_unaug_unit_kernel, dim3(unsigned(zrows < 65535 ? zrows : 65535)), dim3(64), 0, c->stream, static_cast<const double*>(gza), ZA,
                           static_cast<const double*>(nullptr), static_cast<const double*>(nullptr), zrows, d, lt, Tn, Tpad, E, gZ);
    else if (zinc)
        hipLaunchKernelGGL(wide_unaug_inc_kernel, dim3(grid_for(zrows * d)), dim3(256), 0, c->stream, static_cast<const double*>(gza),
                           static_cast<const double*>(nullptr), zrows, d, lt, Tn, Tpad, 0, gZ);
    else
        hipLaunchKernelGGL(wide_unaug_rows_kernel, dim3(grid_for(zrows * d)), dim3(256), 0, c->stream, static_cast<const double*>(gza), ZA, zrows, d, 0, lt, Tn,
                           Tpad, E, gZ, static_cast<const double*>(cadj), qmix);
    HIPCHK(c, hipGetLastError());
    if (mode == WIDE_ROWS_UNIT)
        hipLaunchKernelGGL(wide_unaug_unit_kernel, dim3(unsigned(NLx < 65535 ? NLx : 65535)), dim3(64), 0, c->stream, static_cast<const double*>(nullptr),
                           static_cast<const double*>(nullptr), static_cast<const double*>(gxa), XA, NLx, d, 0, int64_t(1), int64_t(0), 1, gX);
    else if (xinc)
        hipLaunchKernelGGL(wide_unaug_inc_kernel, dim3(grid_for(NLx * d)), dim3(256), 0, c->stream, static_cast<const double*>(nullptr),
                           static_cast<const double*>(gxa), NLx, d, 0, int64_t(1), int64_t(0), xdiff, gX);
    else
        hipLaunchKernelGGL(wide_unaug_rows_kernel, dim3(grid_for(NL * d)), dim3(256), 0, c->stream, static_cast<const double*>(gxa), XA, NL, d, 1, 0, int64_t(1),
                           int64_t(0), 1, gX, static_cast<const double*>(radj), qmix);
    HIPCHK(c, hipGetLastError());
    if (fac) {
        hipLaunchKernelGGL(wide_gfac_reduce_kernel, dim3(grid_for(N * (M + 1))), dim3(256), 0, c->stream, static_cast<const double*>(gfp), int(TB),
                           N * int64_t(M + 1), gfac);
        HIPCHK(c, hipGetLastError());
    }
    if (gb) CHK(gbase_reduce(c, static_cast<double*>(gbp), gbn, g_base));
    return GPSIG_OK;
}


// ---- sequence lattices ----------------------------------------------------------------------------------------------------------------------
constexpr int WIDE_LAT_MAX_COLS = 512;            // 64 lanes x 8 columns

bool wide_lat_available(const gpsig_ctx* c, const gpsig_params* p, int L1, int L2) {
    if (c->wide == 0 || routes_as_captured(c)) return false;
    if (!wide_kind(p) || p->num_levels > WIDE_MAX_LEVELS || p->num_levels < 1) return false;
    const int dr = p->difference ? 1 : 0;
    if (p->order > 1 && p->num_levels > 1) {      // higher orders: the forward and the reverse sweeps of grad_wave_ho_kernel.hpp (<= 5 levels, orders <= 4)
        if (wide_dot_kind(p->base_kernel) || wide_base_param_kind(p->base_kernel)) return false;      // (these families' higher orders: the feature contraction / the exact-shape kernels, the any-shape kernel beyond)
        HoSweeps hf, hb;
        return L1 - dr >= 1 && L2 - dr >= 1 && ho_levels_plan(c, p, L1 - dr, L2 - dr, &hf) && ho_sweeps_plan(c, p, L1 - dr, L2 - dr, &hb);
    }
    if (rows_are_increments(p) && (L1 < 2 || L2 < 2)) return false;      // (no increment rows)
    return L1 >= 1 && L2 >= 1 && L2 - dr <= WIDE_LAT_MAX_COLS;
}

// the reverse pass of the HIGHER-ORDER recursion on this route: argument lattices by dgemm -> dM lattices (wide_lattice_dm_kernel) -> both sweeps of a
// pair in one wavefront (grad_wave_ho_kernel.hpp) -> the adjoint contracted back by dgemms; any number of columns
bool wide_lat_ho_available(const gpsig_ctx* c, const gpsig_params* p, int L1, int L2) {
    if (c->wide == 0 || routes_as_captured(c) || !wide_kind(p) || wide_dot_kind(p->base_kernel) || wide_base_param_kind(p->base_kernel) || !(p->order > 1 && p->num_levels > 1)) return false;
    const int dr = p->difference ? 1 : 0;
    HoSweeps hs;
    return L1 >= 1 && L2 >= 1 && ho_sweeps_plan(c, p, L1 - dr, L2 - dr, &hs);
}

namespace {

// SignatureLinear with differences: the lattices of the INCREMENT rows, without differences (rows_are_increments)
struct LatInc {
    gpsig_params q;
    int xd1 = 0, xd2 = 0;       // observations per sequence where the rows are increments, else 0
    LatInc(const gpsig_params*& p, int& L1, int& L2) : q(*p) {
        if (!rows_are_increments(p)) return;
        xd1 = L1; xd2 = L2; L1 -= 1; L2 -= 1;
        q.difference = 0;
        p = &q;
    }
};

struct LatPlan {
    int DA, dr, R1, R2, C;
    int64_t P, Ptot, chunk_i, ld, si, sj, N2;      // chunk_i: left sequences per chunk (diag: sequences per chunk)
    double *XL, *XR;
};

// augmented rows (left form of the left sequences, right form of the right ones) and the chunking of the argument lattices
// (xd1, xd2 > 0: the rows are the increments of sequences of xd1 / xd2 observations, L1 / L2 of them per sequence -- LatInc)
int lat_plan(gpsig_ctx* c, const gpsig_params* p, int d, const double* Xs, const double* Ys, int64_t N1, int64_t N2, int L1, int L2, bool diag, int bufs,
             int xd1, int xd2, LatPlan* pl) {
    pl->DA = d + 2; pl->dr = p->difference ? 1 : 0; pl->R1 = L1 - pl->dr; pl->R2 = L2 - pl->dr; pl->C = wide_lat_columns(pl->R2);
    void *xl, *xr;
    CHK(ensure(c, B_WD0, sizeof(double) * size_t(N1) * L1 * pl->DA + 64, &xl));
    CHK(ensure(c, B_WD1, sizeof(double) * size_t(N2) * L2 * pl->DA + 64, &xr));
    CHK(aug_rows(c, Xs, N1 * int64_t(L1), d, 0, rows_mode(p->base_kernel), xd1, static_cast<double*>(xl)));
    CHK(aug_rows(c, Ys ? Ys : Xs, N2 * int64_t(L2), d, 1, rows_mode(p->base_kernel), xd2, static_cast<double*>(xr)));
    pl->XL = static_cast<double*>(xl); pl->XR = static_cast<double*>(xr);
    const size_t per_i = sizeof(double) * size_t(L1) * L2 * size_t(diag ? 1 : N2) * size_t(bufs);
    int64_t chunk = int64_t(wide_chunk_bytes(c) / (per_i ? per_i : 1));
    if (chunk < 1) chunk = 1;
    if (chunk > N1) chunk = N1;
    pl->chunk_i = chunk;
    pl->Ptot = diag ? N1 : N1 * N2;
    if (diag) { pl->ld = L2; pl->si = int64_t(L1) * L2; pl->sj = 0; pl->N2 = 1; }
    else { pl->ld = N2 * int64_t(L2); pl->si = int64_t(L1) * pl->ld; pl->sj = L2; pl->N2 = N2; }
    return GPSIG_OK;
}

// the argument lattices of the left sequences i0 .. i0 + ni - 1 into `arg`
// (j0 > 0: the right sequences j0 .. N2 - 1 only -- the symmetric Gram's reverse pass, pairs i <= j)
// (spx: SignatureSpectral -- the entries are kappa, from wide_spectral_kernel.hpp's kernel with the sides' norms and phases nl, nr of all N1 L1 / N2 L2 rows)
struct LatSpx { SpxSetup s; const double *nl = nullptr, *nr = nullptr; int64_t N1 = 0; };
int lat_arguments(gpsig_ctx* c, const LatPlan& pl, int64_t i0, int64_t ni, int64_t N2, int L1, int L2, bool diag, double* arg, int64_t j0 = 0,
                  const LatSpx* spx = nullptr) {
    const int DA = pl.DA;
    if (spx && diag)
        return spx_arguments(c, spx->s, pl.XL + i0 * L1 * DA, pl.XR + i0 * L2 * DA, arg, L1, L2, L2, int64_t(L1) * DA, int64_t(L2) * DA, int64_t(L1) * L2, ni,
                             spx->nl, spx->N1 * L1, i0 * L1, spx->nr, N2 * L2, i0 * L2);
    if (spx)
        return spx_arguments(c, spx->s, pl.XL + i0 * L1 * DA, pl.XR + j0 * L2 * DA, arg, ni * L1, (N2 - j0) * L2, (N2 - j0) * L2, 0, 0, 0, 1, spx->nl,
                             spx->N1 * L1, i0 * L1, spx->nr, N2 * L2, j0 * L2);
    if (diag)      // per sequence: row-major arg (L1, L2) = XL_n XR_n^T  ==  column-major (L2 x L1) = XR_n,cm^T (L2 x DA) XL_n,cm (DA x L1)
        return dgemm_batched(c, true, false, L2, L1, DA, pl.XR + i0 * L2 * DA, DA, int64_t(L2) * DA, pl.XL + i0 * L1 * DA, DA, int64_t(L1) * DA, arg, L2,
                             int64_t(L1) * L2, ni);
    // row-major arg (ni L1, N2 L2) = XL_chunk XR^T  ==  column-major (N2 L2 x ni L1) = XR_cm^T XL_chunk,cm
    return dgemm(c, true, false, (N2 - j0) * L2, ni * L1, DA, pl.XR + j0 * L2 * DA, DA, pl.XL + i0 * L1 * DA, DA, 0.0, arg, (N2 - j0) * L2);
}

}  // namespace

// Raw levels (M+1, P) of the lattices of pairs (i, j) -- P = N1 N2, pair index i N2 + j -- or (i, i) -- diag, P = N1.  Xs, Ys: scaled sequences
// (Ys == NULL: Xs on both sides).  signature_algs.py:8-35 on kernels.py:188-237's tensors.
int wide_lat_forward(gpsig_ctx* c, const gpsig_params* p, int d, const double* Xs, const double* Ys, int64_t N1, int64_t N2, int L1, int L2, bool diag,
                     double* out) {
    const LatInc inc(p, L1, L2);
    LatPlan pl;
    const bool ho = p->order > 1 && p->num_levels > 1;
    HoSweeps hs;
    if (ho && !ho_levels_plan(c, p, L1 - (p->difference ? 1 : 0), L2 - (p->difference ? 1 : 0), &hs))
        return fail(c, GPSIG_ERR_UNSUPPORTED, "no higher-order forward sweep for this shape");
    CHK(lat_plan(c, p, d, Xs, Ys, N1, N2, L1, L2, diag, ho ? 2 : 1, inc.xd1, inc.xd2, &pl));
    const int M = p->num_levels;
    void *arg, *dmat = nullptr;
    CHK(ensure(c, B_WD2, sizeof(double) * size_t(pl.chunk_i) * L1 * L2 * size_t(diag ? 1 : N2) + 64, &arg));
    if (ho) CHK(ensure(c, B_WD6, sizeof(double) * size_t(pl.chunk_i) * L1 * L2 * size_t(diag ? 1 : N2) + 64, &dmat));
    const int NW = ho ? 1 : wide_lat_waves(c, pl.C, diag ? (N1 < pl.chunk_i ? N1 : pl.chunk_i) : (N1 < pl.chunk_i ? N1 : pl.chunk_i) * N2);
    WideLatKernel fn = ho ? nullptr : lat_kernel(M, pl.C, false, p->base_kernel, NW);
    hipEvent_t e0, e1;
    bool timed;
    CHK(timing_begin(c, &e0, &e1, &timed));
    LatSpx spx;
    const bool is_spx = wide_spectral(p);
    if (is_spx) {
        if (ho) return wide_spectral_refusal(c, p, true, L2);
        spx.N1 = N1;
        CHK(spx_setup(c, p, d, &spx.s));
        CHK(spx_side(c, spx.s, pl.XL, N1 * int64_t(L1), B_WS1, &spx.nl));
        CHK(spx_side(c, spx.s, pl.XR, N2 * int64_t(L2), B_WS2, &spx.nr));
    }
    for (int64_t i0 = 0; i0 < N1; i0 += pl.chunk_i) {
        const int64_t ni = N1 - i0 < pl.chunk_i ? N1 - i0 : pl.chunk_i;
        CHK(lat_arguments(c, pl, i0, ni, N2, L1, L2, diag, static_cast<double*>(arg), 0, is_spx ? &spx : nullptr));
        WideLatArgs A;
        memset(&A, 0, sizeof(A));
        A.arg = static_cast<const double*>(arg); A.ld = pl.ld; A.si = pl.si; A.sj = pl.sj; A.N2 = pl.N2;
        A.P = diag ? ni : ni * N2; A.p0 = 0; A.Ptot = pl.Ptot;
        A.L1 = L1; A.L2 = L2; A.M = M; A.kind = p->base_kernel; A.kp0 = p->base_params[0]; A.kp1 = p->base_params[1]; A.difference = pl.dr;
        A.out = out + (diag ? i0 : i0 * N2);              // (the kernel's pair index starts at 0 in this chunk's lattices)
        if (mix_sides(p, MIX_LAT, 0).rows) {              // (both sides or neither; the chunk's left sequences, every right sequence -- the diagonal: the chunk's)
            A.nrm_ld = pl.DA; A.nrm_same = diag ? 1 : 0;
            A.nrm_row = pl.XL + i0 * L1 * pl.DA + d; A.nrm_col = pl.XR + (diag ? i0 : 0) * L2 * pl.DA + d + 1;
        }
        if (ho) {
            if (pl.R1 < 1 || pl.R2 < 1) return fail(c, GPSIG_ERR_UNSUPPORTED, "empty lattices");
            GPSIG_WIDE_KIND(p->base_kernel, hipLaunchKernelGGL(wide_lattice_dm_kernel<KD>, dim3(grid_for(A.P * int64_t(pl.R1) * pl.R2)), dim3(256), 0, c->stream, A,
                                                               static_cast<double*>(dmat)))
            HIPCHK(c, hipGetLastError());
            CHK(ho_levels_launch(c, hs, M, pl.R1, pl.R2, static_cast<const double*>(dmat), out, pl.Ptot, diag ? 1 : N2, diag ? 0 : 1, diag ? 1 : N2, diag,
                                 diag ? i0 : i0 * N2, A.P));
            continue;
        }
        hipLaunchKernelGGL(fn, dim3(unsigned(A.P < 65535 ? A.P : 65535)), dim3(64 * NW), 0, c->stream, A);
        HIPCHK(c, hipGetLastError());
    }
    if (timed) {
        HIPCHK(c, hipEventRecord(e1, c->stream));
        c->t_launches += 1;
        c->t_pairs += pl.Ptot;
        c->t_kernel = is_spx ? "wide_lattice (wide_spx_kernel + wide_lattice_fwd_kernel)" : "wide_lattice (dgemm + wide_lattice_fwd_kernel)";
    }
    return GPSIG_OK;
}

// Gradients of sum_m G[m][pair] level_m[pair] with respect to the scaled sequences.  G: (M+1, P).  Ys == NULL: Xs on both sides and both sides'
// gradients land in gX (the symmetric Gram as the cross Gram of X with itself; the diagonal); else gX, gY.
int wide_lat_backward(gpsig_ctx* c, const gpsig_params* p, int d, const double* Xs, const double* Ys, int64_t N1, int64_t N2, int L1, int L2, bool diag,
                      const double* G, double* gX, double* gY, double* g_base) {
    const LatInc inc(p, L1, L2);
    LatPlan pl;
    const bool ho = p->order > 1 && p->num_levels > 1;
    HoSweeps hs;
    if (ho && !ho_sweeps_plan(c, p, L1 - (p->difference ? 1 : 0), L2 - (p->difference ? 1 : 0), &hs))
        return fail(c, GPSIG_ERR_UNSUPPORTED, "no higher-order sweeps for this shape");
    // first order, MANY SHORT lattices (a Gram of sequences of at most 65 observations): four lattices per wavefront from a dM lattice (seq_grad_wave_o1_kernel) instead of
    // one per 64-lane wavefront; few lattices (a minibatch's level diagonals) stay with the lattice kernels below.  Option wide_o1_sweeps: 0 never, 1 (default) from 1,024 lattices, 2 wherever the shape fits (tests)
    bool short_lat = false;
    if (!ho && c->wide_o1_sweeps != 0 && ((diag ? N1 : N1 * N2) >= 1024 || c->wide_o1_sweeps == 2))
        short_lat = o1_sweeps_plan(c, p, L1 - (p->difference ? 1 : 0), L2 - (p->difference ? 1 : 0), &hs);
    CHK(lat_plan(c, p, d, Xs, Ys, N1, N2, L1, L2, diag, (ho || short_lat) ? 3 : 2, inc.xd1, inc.xd2, &pl));
    // the symmetric Gram (one array on both sides): the pairs i <= j with the upstream gradient folded onto them -- half the lattices
    const bool fold = !diag && Ys == nullptr && N1 == N2 && L1 == L2 && c->wide_sym_fold != 0;
    if (fold) {
        // (a chunk of ni left sequences still sweeps its ni x ni square whole -- zeros below the diagonal: chunks of at most N / 16 keep that under 4 %)
        const int64_t cap = N1 / 16 > 8 ? N1 / 16 : 8;
        if (pl.chunk_i > cap) pl.chunk_i = cap;
        void* gs;
        CHK(ensure(c, B_WD10, sizeof(double) * size_t(p->num_levels + 1) * N1 * N1 + 64, &gs));
        hipLaunchKernelGGL(wide_sym_upstream_kernel, dim3(grid_for(int64_t(p->num_levels + 1) * N1 * N1)), dim3(256), 0, c->stream, G, N1, p->num_levels + 1,
                           static_cast<double*>(gs));
        HIPCHK(c, hipGetLastError());
        G = static_cast<const double*>(gs);
    }
    const int M = p->num_levels, DA = pl.DA;
    const int64_t per_i = int64_t(L1) * L2 * (diag ? 1 : N2);
    void *arg, *lam, *gxl, *gxr, *scr, *dmat = nullptr;
    if (ho || short_lat) CHK(ensure(c, B_WD6, sizeof(double) * size_t(pl.chunk_i) * per_i + 64, &dmat));
    CHK(ensure(c, B_WD2, sizeof(double) * size_t(pl.chunk_i) * per_i + 64, &arg));
    CHK(ensure(c, B_WD3, sizeof(double) * size_t(pl.chunk_i) * per_i + 64, &lam));
    CHK(ensure(c, B_WD4, sizeof(double) * size_t(N1) * L1 * DA + 64, &gxl));
    CHK(ensure(c, B_WD5, sizeof(double) * size_t(N2) * L2 * DA + 64, &gxr));
    const int64_t Pmax = diag ? pl.chunk_i : pl.chunk_i * N2;
    const int NW = (ho || short_lat) ? 1 : wide_lat_waves(c, pl.C, Pmax);
    const int TF = pl.R1 + 64 * NW - 1;
    const size_t per_group = sizeof(double) * size_t(M > 1 ? M - 1 : 1) * TF * 64 * (NW > 1 ? NW : pl.C);
    int64_t groups = int64_t(wide_chunk_bytes(c) / per_group);
    if (groups < 1) groups = 1;
    if (groups > Pmax) groups = Pmax;
    if (groups > 4096) groups = 4096;
    if (ho || short_lat) groups = 1;      // (these sweeps bring their own slots, if any)
    CHK(ensure(c, B_WD7, per_group * size_t(groups) + 64, &scr));
    WideLatKernel fn = (ho || short_lat) ? nullptr : lat_kernel(M, pl.C, true, p->base_kernel, NW);
    // SignaturePoly's offset (g_base: device, or NULL): every slice of every lattice leaves the sum of its W entries in a slot of its own, lattices in the
    // order of G's pair axis (zero where the folded symmetric Gram visits no lattice)
    void* gbp = nullptr;
    const bool poly = p->base_kernel == GPSIG_BASE_POLY, mix = p->base_kernel == GPSIG_BASE_MIX, gb = g_base && (poly || mix);
    // SignatureMix without differences: the row and the column sums of the Lam lattices, per point of the left / the right sequences
    const bool sided = mix_sides(p, MIX_LAT, 0).rows;
    void *radj = nullptr, *cadj = nullptr;
    if (sided) {
        CHK(ensure(c, B_WD14, sizeof(double) * size_t(N1) * L1 + 64, &radj));
        CHK(ensure(c, B_WD15, sizeof(double) * size_t(N2) * L2 + 64, &cadj));
    }
    const int gbs = int((int64_t(L1) * L2 + WIDE_GB_SLICE - 1) / WIDE_GB_SLICE);
    const int64_t gbn = (diag ? N1 : N1 * N2) * gbs;
    if (gb) {
        CHK(ensure(c, B_WD11, sizeof(double) * size_t(gbn + WIDE_GB_BLOCKS) + 64, &gbp));
        CHK(zero_async(c, gbp, sizeof(double) * size_t(gbn)));
    }
    for (int64_t i0 = 0; i0 < N1; i0 += pl.chunk_i) {
        const int64_t ni = N1 - i0 < pl.chunk_i ? N1 - i0 : pl.chunk_i;
        const int64_t j0 = fold ? i0 : 0, N2e = N2 - j0;              // right sequences of this chunk
        CHK(lat_arguments(c, pl, i0, ni, N2, L1, L2, diag, static_cast<double*>(arg), j0));
        WideLatArgs A;
        memset(&A, 0, sizeof(A));
        A.arg = static_cast<const double*>(arg); A.ld = pl.ld; A.si = pl.si; A.sj = pl.sj; A.N2 = pl.N2;
        if (!diag) { A.ld = N2e * int64_t(L2); A.si = int64_t(L1) * A.ld; A.N2 = N2e; }
        A.P = diag ? ni : ni * N2e; A.p0 = 0; A.Ptot = pl.Ptot;
        A.L1 = L1; A.L2 = L2; A.M = M; A.kind = p->base_kernel; A.kp0 = p->base_params[0]; A.kp1 = p->base_params[1]; A.difference = pl.dr;
        A.G = G + (diag ? i0 : i0 * N2 + j0);
        A.g_i = diag ? 1 : N2; A.g_j = diag ? 0 : 1;
        A.scratch = static_cast<double*>(scr); A.lam = static_cast<double*>(lam);
        A.gb_slices = gbs;
        if (sided) {              // (this chunk's left sequences and its right sequences j0 .. N2 - 1; the diagonal: the chunk's on both sides)
            A.nrm_ld = DA; A.nrm_same = diag ? 1 : 0;
            A.nrm_row = pl.XL + i0 * L1 * DA + d; A.nrm_col = pl.XR + (diag ? i0 : j0) * L2 * DA + d + 1;
        }
        if (gb) A.gb_part = static_cast<double*>(gbp) + (diag ? i0 : i0 * N2 + j0) * gbs;
        const int64_t ng = A.P < groups ? A.P : groups;
        A.ngroups = int(ng);
        if ((ho || short_lat) && pl.R1 > 0 && pl.R2 > 0) {
            GPSIG_WIDE_KIND(p->base_kernel, hipLaunchKernelGGL(wide_lattice_dm_kernel<KD>, dim3(grid_for(A.P * int64_t(pl.R1) * pl.R2)), dim3(256), 0, c->stream, A,
                                                               static_cast<double*>(dmat)))
            HIPCHK(c, hipGetLastError());
            // (the sweeps address G by (i, j') = divmod(pair0 + pair, N2e): i absolute with pair0 = i0 N2e, j' relative to the chunk's first right sequence)
            CHK(ho_sweeps_launch(c, hs, M, pl.R1, pl.R2, static_cast<const double*>(dmat), static_cast<double*>(lam), G + j0, pl.Ptot, diag ? 1 : N2, diag ? 0 : 1,
                                 diag ? 1 : N2e, diag, diag ? i0 : i0 * N2e, A.P));
        } else if (pl.R1 > 0 && pl.R2 > 0) {
            hipLaunchKernelGGL(fn, dim3(unsigned(ng)), dim3(64 * NW), 0, c->stream, A);
            HIPCHK(c, hipGetLastError());
        }
        // the adjoint of the arguments, in place of the arguments
        if (sided) {
            const int64_t units = ni * int64_t(L1) + (diag ? ni : N2e) * int64_t(L2);
            hipLaunchKernelGGL(wide_lattice_sides_kernel, dim3(grid_for(units, 1)), dim3(64), 0, c->stream, static_cast<const double*>(lam), ni, diag ? int64_t(1) : N2e,
                               L1, L2, diag ? 1 : 0, (!diag && i0 > 0) ? 1 : 0, static_cast<double*>(radj) + i0 * L1, static_cast<double*>(cadj) + (diag ? i0 : j0) * L2);
            HIPCHK(c, hipGetLastError());
        }
        if (poly)          // (a kernel of its own: one wavefront per slice of a lattice, with the slice's sum of W)
            hipLaunchKernelGGL(wide_lattice_adjoint_poly_kernel, dim3(grid_for(A.P * gbs, 1)), dim3(64), 0, c->stream, A, static_cast<double*>(arg));
        else if (mix)
            hipLaunchKernelGGL(wide_lattice_adjoint_mix_kernel, dim3(grid_for(A.P * gbs, 1)), dim3(64), 0, c->stream, A, static_cast<double*>(arg));
        else
            GPSIG_WIDE_KIND(p->base_kernel, hipLaunchKernelGGL(wide_lattice_adjoint_kernel<KD>, dim3(grid_for(A.P * int64_t(L1) * L2)), dim3(256), 0, c->stream, A,
                                                               static_cast<double*>(arg)))
        HIPCHK(c, hipGetLastError());
        const double* W = static_cast<const double*>(arg);
        double* gl = static_cast<double*>(gxl) + i0 * L1 * DA;
        if (diag) {
            // gXL_n (L1, DA) = W_n XR_n: column-major (DA x L1) = XR_n,cm (DA x L2) W_n,cm (L2 x L1);  gXR_n (L2, DA) = W_n^T XL_n: (DA x L2) = XL_n,cm (DA x L1) W_n,cm^T
            CHK(dgemm_batched(c, false, false, DA, L1, L2, pl.XR + i0 * L2 * DA, DA, int64_t(L2) * DA, W, L2, int64_t(L1) * L2, gl, DA, int64_t(L1) * DA, ni));
            CHK(dgemm_batched(c, false, true, DA, L2, L1, pl.XL + i0 * L1 * DA, DA, int64_t(L1) * DA, W, L2, int64_t(L1) * L2,
                              static_cast<double*>(gxr) + i0 * L2 * DA, DA, int64_t(L2) * DA, ni));
        } else {
            CHK(contract_both(c, W, pl.XL + i0 * L1 * DA, pl.XR + j0 * L2 * DA, ni * int64_t(L1), N2e * int64_t(L2), DA, i0 > 0, gl,
                              static_cast<double*>(gxr) + j0 * L2 * DA));
        }
    }
    if (gb) CHK(gbase_reduce(c, static_cast<double*>(gbp), gbn, g_base));
    // through the augmentation: left form into gX; right form into gX as well (one array on both sides) or into gY
    const int64_t xr_rows = N1 * int64_t(L1), yr_rows = N2 * int64_t(L2);
    const bool same = Ys == nullptr;
    const double *gl = static_cast<const double*>(gxl), *gr = static_cast<const double*>(gxr), *none = nullptr;
    if (rows_mode(p->base_kernel) == WIDE_ROWS_UNIT) {
        hipLaunchKernelGGL(wide_unaug_unit_kernel, dim3(unsigned(xr_rows < 65535 ? xr_rows : 65535)), dim3(64), 0, c->stream, gl, pl.XL, same ? gr : none,
                           same ? pl.XR : none, xr_rows, d, 0, int64_t(1), int64_t(0), 1, gX);
        if (!same)
            hipLaunchKernelGGL(wide_unaug_unit_kernel, dim3(unsigned(yr_rows < 65535 ? yr_rows : 65535)), dim3(64), 0, c->stream, none, none, gr, pl.XR, yr_rows, d,
                               0, int64_t(1), int64_t(0), 1, gY);
        HIPCHK(c, hipGetLastError());
        return GPSIG_OK;
    }
    if (inc.xd1) {          // increment rows: N (L + 1) output rows from N L rows of adjoints
        hipLaunchKernelGGL(wide_unaug_inc_kernel, dim3(grid_for(N1 * int64_t(inc.xd1) * d)), dim3(256), 0, c->stream, gl, same ? gr : none,
                           N1 * int64_t(inc.xd1), d, 0, int64_t(1), int64_t(0), inc.xd1, gX);
        if (!same)
            hipLaunchKernelGGL(wide_unaug_inc_kernel, dim3(grid_for(N2 * int64_t(inc.xd2) * d)), dim3(256), 0, c->stream, none, gr, N2 * int64_t(inc.xd2), d, 0,
                               int64_t(1), int64_t(0), inc.xd2, gY);
        HIPCHK(c, hipGetLastError());
        return GPSIG_OK;
    }
    // (plain rows of SignatureLinear too: their norm column's adjoint is exactly 0 -- see wide_tvs_backward)
    const double qmix = 1.0 - p->base_params[0];
    hipLaunchKernelGGL(wide_unaug_pair_kernel, dim3(grid_for(xr_rows * d)), dim3(256), 0, c->stream, gl, pl.XL, same ? gr : none, same ? pl.XR : none, xr_rows, d,
                       gX, static_cast<const double*>(radj), same ? static_cast<const double*>(cadj) : none, qmix);
    HIPCHK(c, hipGetLastError());
    if (!same) {
        hipLaunchKernelGGL(wide_unaug_rows_kernel, dim3(grid_for(yr_rows * d)), dim3(256), 0, c->stream, gr, pl.XR, yr_rows, d, 1, 0, int64_t(1), int64_t(0), 1,
                           gY, static_cast<const double*>(cadj), qmix);
        HIPCHK(c, hipGetLastError());
    }
    return GPSIG_OK;
}

// ---- inducing tensors vs inducing tensors ----------------------------------------------------------------------------------------------------
bool wide_tens_available(const gpsig_ctx* c, const gpsig_params* p, int64_t Tn) {
    if (c->wide == 0 || routes_as_captured(c)) return false;
    if (!wide_kind(p) || p->num_levels > WIDE_MAX_LEVELS || p->num_levels < 1) return false;
    const int64_t Tpad = (Tn + 63) / 64 * 64;
    // the argument blocks of every component at once (10 components x 1,024^2 x 8 bytes = 84 MB at 500 tensors with increments)
    return Tn >= 1 && size_t(p->num_levels * (p->num_levels + 1) / 2) * size_t(4 * Tpad * Tpad) * sizeof(double) <= (size_t(2) << 30);
}

namespace {
// left- and right-form augmented rows of the tensors (B_WD0, B_WD6) and the argument blocks (B_WD2)
// (E as the kernels see it: SignatureLinear with increments has E = 1, rows z^1 - z^0 -- zdiff)
int tens_arguments(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& sz, int d, const double* Z, int lt, int E, int zdiff, int64_t Tn, int64_t Tpad, double** ZL,
                   double** ZR, double** arg) {
    const int DA = d + 2;
    const int64_t zr = int64_t(lt) * E * Tpad, R = int64_t(E) * Tpad;
    void *zl, *zrr, *ar;
    CHK(ensure(c, B_WD0, sizeof(double) * size_t(zr) * DA + 64, &zl));
    CHK(ensure(c, B_WD6, sizeof(double) * size_t(zr) * DA + 64, &zrr));
    CHK(ensure(c, B_WD2, sizeof(double) * size_t(lt) * R * R + 64, &ar));
    for (int right = 0; right < 2; ++right) {
        hipLaunchKernelGGL(wide_aug_rows_kernel, dim3(unsigned(zr < 65535 ? zr : 65535)), dim3(64), 0, c->stream, Z, zr, d, right, lt, Tn, Tpad, E, sz,
                           rows_mode(p->base_kernel), zdiff, static_cast<double*>(right ? zrr : zl));
        HIPCHK(c, hipGetLastError());
    }
    // block k, row-major (R, R) = ZL_k ZR_k^T  ==  column-major (R x R) = ZR_k,cm^T (R x DA) ZL_k,cm (DA x R)
    if (wide_spectral(p)) {          // (forward only; plain rows: both forms hold the same rows, one pre-pass serves both sides)
        SpxSetup ss;
        const double* nz;
        CHK(spx_setup(c, p, d, &ss));
        CHK(spx_side(c, ss, static_cast<const double*>(zl), zr, B_WS1, &nz));
        CHK(spx_arguments(c, ss, static_cast<const double*>(zl), static_cast<const double*>(zrr), static_cast<double*>(ar), R, R, R, R * DA, R * DA, R * R, lt, nz,
                          zr, 0, nz, zr, 0));
    } else {
        CHK(dgemm_batched(c, true, false, R, R, DA, static_cast<const double*>(zrr), DA, R * DA, static_cast<const double*>(zl), DA, R * DA,
                          static_cast<double*>(ar), R, R * R, lt));
    }
    *ZL = static_cast<double*>(zl); *ZR = static_cast<double*>(zrr); *arg = static_cast<double*>(ar);
    return GPSIG_OK;
}
}  // namespace

// Kzz: Z the caller's (lt, T, E, d) array (scaled here when sz.has_ls); w (M+1) or NULL; out (T, T) weighted sum or (M+1, T, T)
int wide_tens_forward(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& sz, int d, const double* Z, int64_t Tn, int increments, const double* w,
                      int sum_levels, double* out) {
    const bool zinc = tensors_collapse(p, increments);
    const int M = p->num_levels, lt = M * (M + 1) / 2, E = (increments && !zinc) ? 2 : 1;
    const int64_t Tpad = (Tn + 63) / 64 * 64;
    double *ZL, *ZR, *arg;
    hipEvent_t e0, e1;
    bool timed;
    CHK(timing_begin(c, &e0, &e1, &timed));          // (around the rows, the batched dgemm and the kernel: what the record's name says)
    CHK(tens_arguments(c, p, sz, d, Z, lt, E, zinc ? 1 : 0, Tn, Tpad, &ZL, &ZR, &arg));
    WideTensArgs A;
    memset(&A, 0, sizeof(A));
    A.arg = arg; A.Tpad = Tpad; A.Tn = Tn; A.M = M; A.E = E; A.kind = p->base_kernel; A.kp0 = p->base_params[0]; A.kp1 = p->base_params[1]; A.sum_levels = sum_levels; A.w = w; A.out = out;
    if (mix_sides(p, MIX_TENS, increments).rows) { A.nrm = ZL + d; A.nrm_ld = d + 2; }          // (both sides are the tensors: one vector)
    GPSIG_WIDE_KIND(p->base_kernel, hipLaunchKernelGGL(wide_tens_fwd_kernel<KD>, dim3(unsigned(Tpad / 64), unsigned(Tn < 65535 ? Tn : 65535)), dim3(64), 0, c->stream, A))
    HIPCHK(c, hipGetLastError());
    if (timed) {
        HIPCHK(c, hipEventRecord(e1, c->stream));
        c->t_launches += 1;
        c->t_pairs += Tn * Tn;
        c->t_kernel = wide_spectral(p) ? "wide_tens (wide_spx_kernel + wide_tens_fwd_kernel)" : "wide_tens (dgemm + wide_tens_fwd_kernel)";
    }
    return GPSIG_OK;
}

// gradient of sum_m G[m][t][t'] level_m[t][t'] with respect to the scaled tensors Z (lt, T, E, d)
int wide_tens_backward(gpsig_ctx* c, const gpsig_params* p, int d, const double* Z, int64_t Tn, int increments, const double* G, double* gZ, double* g_base) {
    const bool zinc = tensors_collapse(p, increments);
    const int M = p->num_levels, lt = M * (M + 1) / 2, Ez = increments ? 2 : 1, E = zinc ? 1 : Ez, DA = d + 2;
    const int64_t Tpad = (Tn + 63) / 64 * 64, R = int64_t(E) * Tpad, zr = int64_t(lt) * R;
    ScaleParams none;
    memset(&none, 0, sizeof(none));
    none.d_in = d;
    double *ZL, *ZR, *arg;
    CHK(tens_arguments(c, p, none, d, Z, lt, E, zinc ? 1 : 0, Tn, Tpad, &ZL, &ZR, &arg));
    void *Wb, *gzl, *gzr;
    CHK(ensure(c, B_WD3, sizeof(double) * size_t(lt) * R * R + 64, &Wb));
    CHK(ensure(c, B_WD4, sizeof(double) * size_t(zr) * DA + 64, &gzl));
    CHK(ensure(c, B_WD5, sizeof(double) * size_t(zr) * DA + 64, &gzr));
    WideTensArgs A;
    memset(&A, 0, sizeof(A));
    A.arg = arg; A.Tpad = Tpad; A.Tn = Tn; A.M = M; A.E = E; A.kind = p->base_kernel; A.kp0 = p->base_params[0]; A.kp1 = p->base_params[1]; A.G = G; A.W = static_cast<double*>(Wb);
    // SignaturePoly's offset (g_base: device, or NULL): every (column block, row) leaves the sum of its W entries in a slot of its own
    void* gbp = nullptr;
    const bool gb = g_base && wide_base_param_kind(p->base_kernel);
    const int64_t gbn = (Tpad / 64) * Tpad;
    if (gb) CHK(ensure(c, B_WD11, sizeof(double) * size_t(gbn + WIDE_GB_BLOCKS) + 64, &gbp));
    A.gb_part = static_cast<double*>(gbp);
    // SignatureMix without increments: the values' adjoints (lt, Tpad, Tpad) next to W; their row sums go back with the left form's adjoint, their column
    // sums with the right form's
    const bool sided = mix_sides(p, MIX_TENS, increments).rows;
    void *gval = nullptr, *radj = nullptr, *cadj = nullptr;
    if (sided) {
        CHK(ensure(c, B_WD12, sizeof(double) * size_t(lt) * Tpad * Tpad + 64, &gval));
        CHK(ensure(c, B_WD14, sizeof(double) * size_t(zr) + 64, &radj));
        CHK(ensure(c, B_WD15, sizeof(double) * size_t(zr) + 64, &cadj));
        A.nrm = ZL + d; A.nrm_ld = DA; A.gval = static_cast<double*>(gval);
    }
    GPSIG_WIDE_KIND(p->base_kernel, hipLaunchKernelGGL(wide_tens_bwd_kernel<KD>, dim3(unsigned(Tpad / 64), unsigned(Tpad < 65535 ? Tpad : 65535)), dim3(64), 0, c->stream, A))
    HIPCHK(c, hipGetLastError());
    // gZL_k (R, DA) = W_k ZR_k: column-major (DA x R) = ZR_k,cm (DA x R) W_k,cm (R x R);   gZR_k = W_k^T ZL_k: (DA x R) = ZL_k,cm W_k,cm^T
    CHK(dgemm_batched(c, false, false, DA, R, R, ZR, DA, R * DA, static_cast<const double*>(Wb), R, R * R, static_cast<double*>(gzl), DA, R * DA, lt));
    CHK(dgemm_batched(c, false, true, DA, R, R, ZL, DA, R * DA, static_cast<const double*>(Wb), R, R * R, static_cast<double*>(gzr), DA, R * DA, lt));
    if (gb) CHK(gbase_reduce(c, static_cast<double*>(gbp), gbn, g_base));
    if (sided) {          // (lt "diagonal lattices" of Tpad x Tpad: one wavefront per row and per column)
        hipLaunchKernelGGL(wide_lattice_sides_kernel, dim3(grid_for(2 * zr, 1)), dim3(64), 0, c->stream, static_cast<const double*>(gval), int64_t(lt), int64_t(1),
                           int(Tpad), int(Tpad), 1, 0, static_cast<double*>(radj), static_cast<double*>(cadj));
        HIPCHK(c, hipGetLastError());
    }
    const int64_t rows_out = int64_t(lt) * Tn * Ez;             // the caller's rows
    if (rows_mode(p->base_kernel) == WIDE_ROWS_UNIT)
        hipLaunchKernelGGL(wide_unaug_unit_kernel, dim3(unsigned(rows_out < 65535 ? rows_out : 65535)), dim3(64), 0, c->stream, static_cast<const double*>(gzl), ZL,
                           static_cast<const double*>(gzr), ZR, rows_out, d, lt, Tn, Tpad, E, gZ);
    else if (zinc)
        hipLaunchKernelGGL(wide_unaug_inc_kernel, dim3(grid_for(rows_out * d)), dim3(256), 0, c->stream, static_cast<const double*>(gzl),
                           static_cast<const double*>(gzr), rows_out, d, lt, Tn, Tpad, 0, gZ);
    else
        hipLaunchKernelGGL(wide_unaug_tens_kernel, dim3(grid_for(rows_out * d)), dim3(256), 0, c->stream, static_cast<const double*>(gzl), ZL,
                           static_cast<const double*>(gzr), ZR, rows_out, d, Tn, Tpad, E, gZ, static_cast<const double*>(radj), static_cast<const double*>(cadj),
                           1.0 - p->base_params[0]);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

}  // namespace gpsig
