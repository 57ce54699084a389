// grad_api.hip -- C-ABI entry points of the gradient path (include/gpsig_hip.h, "gradients").
//
// Reverse-mode derivatives of the four level primitives (_K_seq, _K_seq_diag, _K_tens, _K_tens_vs_seq of
// gpsig/kernels.py:188-340) with respect to their (already scaled) inputs; first-order algorithm, float64.  The
// reference differentiates these through TensorFlow (training.py:149-164); there is no reference gradient code
// to cite, the formulas are in grad_core.hpp.  Host side only: staging, chunking by the scratch budget, launches.
#include "ctx.hpp"
#include "launchers.hpp"
#include "grad_kernels.hpp"
#include "grad_ho_kernels.hpp"
#include "grad_wave_ho_kernel.hpp"
#include "grad_wave_kernel.hpp"
#include "grad_fused_kernel.hpp"

namespace gpsig {
// G: lanes per pair group -- 16 (four pairs per wavefront), 32 (two) or 64 (one); diff: the lattice of double increments (difference=True, the
// reference's default) or the kernel matrix of the points itself
static FusedGradLaunchFn fused_grad_lookup(int kind, int DP, int LQ, int G, bool diff) {
    if (G == 16) return diff ? fused_grad_lookup_diff_g16(kind, DP, LQ) : fused_grad_lookup_nodiff_g16(kind, DP, LQ);
    if (G == 32) return diff ? fused_grad_lookup_diff_g32(kind, DP, LQ) : fused_grad_lookup_nodiff_g32(kind, DP, LQ);
    if (G == 64) return diff ? fused_grad_lookup_diff_g64(kind, DP, LQ) : fused_grad_lookup_nodiff_g64(kind, DP, LQ);
    return nullptr;
}
}  // namespace gpsig

using namespace gpsig;

// ---- the sweeps of the higher-order reverse pass (grad_wave_ho_kernel.hpp), shared by the point route below and the wide route (wide_api.hip) ----
namespace gpsig {
bool ho_sweeps_plan(const gpsig_ctx* c, const gpsig_params* p, int R1, int R2, HoSweeps* hs) {
    const int M = p->num_levels, order = p->order < M ? p->order : M;
    // the decision (lane shape, the ho_g32 rule, scratch-free or HBM slots): ho_sweeps_plan_shape of grad_plan.hpp
    const GradInstance g = ho_sweeps_plan_shape(c->grad_impl, c->ho_g32, M, p->order, R1, R2, &hs->lds);
    hs->fn = nullptr;
    hs->G = g.G; hs->C = g.C;
    if (g.family == GRAD_HO_UNDO)
        hs->fn = g.G == 16 ? wave_ho_undo_lookup_g16(g.C, order, M) : (g.G == 32 ? wave_ho_undo_lookup_g32(g.C, order, M) : wave_ho_undo_lookup_g64(g.C, order, M));
    else if (g.family == GRAD_HO_SLOT)
        hs->fn = wave_ho_lookup(g.G, g.C, order, M);
    if (!hs->fn) return false;
    hs->slot = hs->lds == 0 ? sizeof(double) * size_t(ho_stash_words(order, M)) * size_t(R1 + hs->G - 1) * hs->G * hs->C : 0;
    return true;
}

// first order, short lattices (<= 64 columns) from a dM lattice in memory: seq_grad_wave_o1_kernel, launched through ho_sweeps_launch
bool o1_sweeps_plan(const gpsig_ctx* c, const gpsig_params* p, int R1, int R2, HoSweeps* hs) {
    const int M = p->num_levels;
    if (c->grad_impl != 0 || (p->order > 1 && M > 1) || R1 < 1 || R2 < 1 || R2 > 64 || M > 8) return false;
    hs->G = 16; hs->C = R2 <= 32 ? 2 : 4;
    hs->fn = wave_o1_lookup(hs->G, hs->C, M);
    hs->lds = sizeof(double) * size_t(64 / hs->G) * size_t(R1) * size_t(M <= 4 ? 3 : 7);
    hs->slot = 0;
    return hs->fn != nullptr && hs->lds <= 64 * 1024;
}

// the forward pass by one sweep per pair (seq_levels_wave_ho_kernel): the same lane shapes
bool ho_levels_plan(const gpsig_ctx* c, const gpsig_params* p, int R1, int R2, HoSweeps* hs) {
    const int M = p->num_levels, order = p->order < M ? p->order : M;
    if (c->grad_impl != 0 || order < 2 || R1 < 1 || R2 < 1) return false;
    static const int shapes[][2] = {{16, 2}, {16, 4}, {64, 2}, {64, 4}, {64, 8}};
    hs->fn = nullptr; hs->lds = 0; hs->slot = 0;
    for (auto& sh : shapes) {
        if (sh[0] * sh[1] < R2) continue;
        hs->G = sh[0]; hs->C = sh[1];
        if (hs->G == 16 && hs->C == 4 && (c->ho_g32 > 0 || (c->ho_g32 < 0 && order >= 3))) { hs->G = 32; hs->C = 2; }
        hs->fn = hs->G == 16 ? wave_ho_levels_lookup_g16(hs->C, order, M) : (hs->G == 32 ? wave_ho_levels_lookup_g32(hs->C, order, M) : wave_ho_levels_lookup_g64(hs->C, order, M));
        break;
    }
    return hs->fn != nullptr;
}

// dM (npairs, R1, R2) -> levels: level m of pair (i, j) at out[m * gm + i * gi + j * gj], (i, j) as in ho_sweeps_launch
int ho_levels_launch(gpsig_ctx* c, const HoSweeps& hs, int M, int R1, int R2, const double* dM, double* out, int64_t gm, int64_t gi, int64_t gj, int64_t N2,
                     bool diag, int64_t pair0, int64_t npairs) {
    const int PW = 64 / hs.G;
    int64_t ngroups = npairs < 16384 ? npairs : 16384;
    if (ngroups < PW) ngroups = PW;
    ngroups = (ngroups + PW - 1) / PW * PW;
    WaveHoArgs A;
    memset(&A, 0, sizeof(A));
    A.gm = gm; A.gi = gi; A.gj = gj; A.N2 = int(N2); A.diag = diag ? 1 : 0;
    A.R1 = R1; A.R2 = R2; A.M = M;
    A.dM = dM; A.lam = out; A.pair0 = pair0; A.npairs = npairs; A.ngroups = int(ngroups);
    const hipError_t e = hs.fn(A, int(ngroups / PW), 0, c->stream);
    if (e != hipSuccess) return fail(c, GPSIG_ERR_HIP, "higher-order levels: launch failed: %s", hipGetErrorString(e));
    return GPSIG_OK;
}

// dM (npairs, R1, R2) -> lam (npairs, R1, R2); G[level * gm + i * gi + j * gj] with (i, j) = divmod(pair0 + pair, N2) (diag: i = j = pair0 + pair)
int ho_sweeps_launch(gpsig_ctx* c, const HoSweeps& hs, int M, int R1, int R2, const double* dM, double* lam, const double* G, int64_t gm, int64_t gi,
                     int64_t gj, int64_t N2, bool diag, int64_t pair0, int64_t npairs) {
    const int PW = 64 / hs.G;
    int64_t ngroups = hs.slot ? int64_t((size_t(c->grad_scratch_mb > 0 ? c->grad_scratch_mb : 4096) << 20) / 2 / hs.slot) : 16384;
    if (ngroups > (hs.slot ? 8192 : 16384)) ngroups = hs.slot ? 8192 : 16384;
    if (ngroups > npairs) ngroups = npairs;
    if (ngroups < PW) ngroups = PW;
    ngroups = (ngroups + PW - 1) / PW * PW;
    void* scr;
    CHK(ensure(c, B_GR6, hs.slot * size_t(ngroups) + 64, &scr));
    WaveHoArgs A;
    memset(&A, 0, sizeof(A));
    A.G = G; A.gm = gm; A.gi = gi; A.gj = gj; A.N2 = int(N2); A.diag = diag ? 1 : 0;
    A.R1 = R1; A.R2 = R2; A.M = M; A.scratch = static_cast<double*>(scr);
    A.dM = dM; A.lam = lam; A.pair0 = pair0; A.npairs = npairs; A.ngroups = int(ngroups);
    const hipError_t e = hs.fn(A, int(ngroups / PW), hs.lds, c->stream);
    if (e != hipSuccess) return fail(c, GPSIG_ERR_HIP, "higher-order sweeps: launch failed: %s", hipGetErrorString(e));
    return GPSIG_OK;
}
}  // namespace gpsig

namespace {

int grad_check(gpsig_ctx* c, const gpsig_params* p, int* d, int* DP, int max_d = 64) {
    if (!c) return GPSIG_ERR_INVALID;
    if (!p) return fail(c, GPSIG_ERR_INVALID, "params is NULL");
    if (p->dtype != GPSIG_F64) return fail(c, GPSIG_ERR_UNSUPPORTED, "gradients are built for float64 only");
    if (p->num_levels < 1) return fail(c, GPSIG_ERR_INVALID, "num_levels must be >= 1");
    if (p->num_levels > GRAD_MAX_LEVELS) return fail(c, GPSIG_ERR_UNSUPPORTED, "gradients are built for num_levels <= %d", GRAD_MAX_LEVELS);
    if (p->order < 1 || p->order > p->num_levels) return fail(c, GPSIG_ERR_INVALID, "order=%d outside [1, num_levels]", p->order);
    if (p->base_kernel < GPSIG_BASE_LINEAR || p->base_kernel > GPSIG_BASE_MATERN52) return fail(c, GPSIG_ERR_INVALID, "unknown base kernel %d", p->base_kernel);
    if (p->num_features < 1 || p->num_lags < 0) return fail(c, GPSIG_ERR_INVALID, "bad num_features / num_lags");
    *d = p->num_features * (p->num_lags + 1);      // raw entry points: columns are taken as they come
    // (max_d > 64: entry points with a wide route -- wide_api.hip --, which is then the only one that takes such a call: *DP = 0)
    if (*d > max_d) return fail(c, GPSIG_ERR_UNSUPPORTED, "gradients are built for at most %d feature columns (got %d)", max_d, *d);
    *DP = *d <= 4 ? 4 : (*d <= 8 ? 8 : (*d <= 16 ? 16 : (*d <= 32 ? 32 : (*d <= 64 ? 64 : 0))));
    HIPCHK(c, hipSetDevice(c->device));
    return GPSIG_OK;
}

int lattice_mode(const gpsig_params* p) {
    if (!p->difference) return MODE_PT_NODIFF;
    return p->base_kernel == GPSIG_BASE_LINEAR ? MODE_INC : MODE_PT_DIFF;
}

size_t scratch_budget(const gpsig_ctx* c) { return size_t(c->grad_scratch_mb > 0 ? c->grad_scratch_mb : 4096) << 20; }

int to_timemajor(gpsig_ctx* c, const double* X, double* XT, int64_t N, int L, int d, int DP, int64_t stride) {
    hipLaunchKernelGGL(grad_to_timemajor_kernel, dim3(grid_for(int64_t(L) * DP * stride)), dim3(256), 0, c->stream, X, XT, int(N), L, d, DP, stride);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}
int from_timemajor(gpsig_ctx* c, const double* gXT, double* gX, int64_t N, int L, int d, int DP, int64_t stride) {
    if (N * L * d == 0) return GPSIG_OK;
    hipLaunchKernelGGL(grad_from_timemajor_kernel, dim3(grid_for(N * L * d)), dim3(256), 0, c->stream, gXT, gX, int(N), L, d, DP, stride, 0);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

template <typename A>
int launch_seq(gpsig_ctx* c, int DP, dim3 grid, const A& a) {
    switch (DP) {
        case 4: hipLaunchKernelGGL(seq_pair_grad_kernel<4>, grid, dim3(64), 0, c->stream, a); break;
        case 8: hipLaunchKernelGGL(seq_pair_grad_kernel<8>, grid, dim3(64), 0, c->stream, a); break;
        case 16: hipLaunchKernelGGL(seq_pair_grad_kernel<16>, grid, dim3(64), 0, c->stream, a); break;
        case 32: hipLaunchKernelGGL(seq_pair_grad_kernel<32>, grid, dim3(64), 0, c->stream, a); break;
        default: hipLaunchKernelGGL(seq_pair_grad_kernel<64>, grid, dim3(64), 0, c->stream, a); break;
    }
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}
int launch_tvs(gpsig_ctx* c, int DP, dim3 grid, const TvsGradArgs& a) {
    switch (DP) {
        case 4: hipLaunchKernelGGL(tvs_pair_grad_kernel<4>, grid, dim3(64), 0, c->stream, a); break;
        case 8: hipLaunchKernelGGL(tvs_pair_grad_kernel<8>, grid, dim3(64), 0, c->stream, a); break;
        case 16: hipLaunchKernelGGL(tvs_pair_grad_kernel<16>, grid, dim3(64), 0, c->stream, a); break;
        case 32: hipLaunchKernelGGL(tvs_pair_grad_kernel<32>, grid, dim3(64), 0, c->stream, a); break;
        default: hipLaunchKernelGGL(tvs_pair_grad_kernel<64>, grid, dim3(64), 0, c->stream, a); break;
    }
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}
// scratch-free tensor-vs-sequence gradient; built where the per-lane accumulators (M * E * DP doubles) fit the register file
bool tvs_fused_available(int DP, int M, int E) { return M <= 4 && DP <= 8; }
int launch_tvs_fused(gpsig_ctx* c, int DP, int E, dim3 grid, const TvsGradArgs& a) {
    if (DP == 4 && E == 1) hipLaunchKernelGGL((tvs_pair_grad_fused_kernel<4, 4, 1>), grid, dim3(64), 0, c->stream, a);
    else if (DP == 4) hipLaunchKernelGGL((tvs_pair_grad_fused_kernel<4, 4, 2>), grid, dim3(64), 0, c->stream, a);
    else if (E == 1) hipLaunchKernelGGL((tvs_pair_grad_fused_kernel<8, 4, 1>), grid, dim3(64), 0, c->stream, a);
    else hipLaunchKernelGGL((tvs_pair_grad_fused_kernel<8, 4, 2>), grid, dim3(64), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}
// tensor-lane variant (operands in LDS, wavefront reduction of the observations' gradient)
// E here is what a LANE holds: incremental tensors are split over lane pairs (one point each), so every launch is E == 1
size_t tvs_lanet_lds(int DP, int L, bool zreg) {
    return sizeof(double) * ((zreg ? 0 : size_t(4) * 64 * (DP + 2)) + size_t(L) * DP + size_t(L) + 2 * 64 * (DP + 2));
}
bool tvs_lanet_zreg(const gpsig_ctx* c) { return c->tvs_zreg < 0 ? true : c->tvs_zreg != 0; }
bool tvs_lanet_available(const gpsig_ctx* c, int DP, int M, int L) { return M <= 4 && DP <= 8 && tvs_lanet_lds(DP, L, tvs_lanet_zreg(c)) <= 64 * 1024; }
int launch_tvs_lanet(gpsig_ctx* c, int DP, bool paired, dim3 grid, const TvsLaneTGradArgs& a) {
    const bool zreg = tvs_lanet_zreg(c);
    const size_t lds = tvs_lanet_lds(DP, a.L, zreg);
#define LANET(DP_, Z_, P_)                                                                                                                           \
    do {                                                                                                                                            \
        if (a.kind == BASE_LINEAR) hipLaunchKernelGGL((tvs_grad_lanet_kernel<DP_, 4, 1, BASE_LINEAR, Z_, P_>), grid, dim3(64), lds, c->stream, a); \
        else if (a.kind == BASE_RBF) hipLaunchKernelGGL((tvs_grad_lanet_kernel<DP_, 4, 1, BASE_RBF, Z_, P_>), grid, dim3(64), lds, c->stream, a);  \
        else hipLaunchKernelGGL((tvs_grad_lanet_kernel<DP_, 4, 1, -1, Z_, P_>), grid, dim3(64), lds, c->stream, a);                                \
    } while (0)
#define LANET2(DP_)                                              \
    do {                                                         \
        if (zreg) { if (paired) LANET(DP_, true, true); else LANET(DP_, true, false); }   \
        else { if (paired) LANET(DP_, false, true); else LANET(DP_, false, false); }      \
    } while (0)
    if (DP == 4) LANET2(4); else LANET2(8);
#undef LANET2
#undef LANET
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}
// row-owned variant: every shape
int launch_tens_row(gpsig_ctx* c, int DP, int E, dim3 grid, const TensGradArgs& a) {
#define TROW(DP_)                                                                                                     \
    do {                                                                                                             \
        if (E == 1) hipLaunchKernelGGL((tens_row_grad_kernel<DP_, 1>), grid, dim3(64), 0, c->stream, a);             \
        else hipLaunchKernelGGL((tens_row_grad_kernel<DP_, 2>), grid, dim3(64), 0, c->stream, a);                    \
    } while (0)
    if (DP == 4) TROW(4); else if (DP == 8) TROW(8); else if (DP == 16) TROW(16); else if (DP == 32) TROW(32); else TROW(64);
#undef TROW
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}
int launch_tens(gpsig_ctx* c, int DP, dim3 grid, const TensGradArgs& a) {
    switch (DP) {
        case 4: hipLaunchKernelGGL(tens_pair_grad_kernel<4>, grid, dim3(64), 0, c->stream, a); break;
        case 8: hipLaunchKernelGGL(tens_pair_grad_kernel<8>, grid, dim3(64), 0, c->stream, a); break;
        case 16: hipLaunchKernelGGL(tens_pair_grad_kernel<16>, grid, dim3(64), 0, c->stream, a); break;
        case 32: hipLaunchKernelGGL(tens_pair_grad_kernel<32>, grid, dim3(64), 0, c->stream, a); break;
        default: hipLaunchKernelGGL(tens_pair_grad_kernel<64>, grid, dim3(64), 0, c->stream, a); break;
    }
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

// gbase: 2 doubles on the device, zeroed
int gbase_begin(gpsig_ctx* c, double** dev) {
    void* p;
    CHK(ensure(c, B_GR7, 2 * sizeof(double), &p));
    CHK(zero_async(c, p, 2 * sizeof(double)));
    *dev = static_cast<double*>(p);
    return GPSIG_OK;
}
int gbase_end(gpsig_ctx* c, const double* dev, double* user) {
    if (!user) return GPSIG_OK;
    HIPCHK(c, hipMemcpyAsync(user, dev, 2 * sizeof(double), c->ptr_mode == GPSIG_PTR_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    return GPSIG_OK;
}


// ---- wavefront-parallel path (grad_wave_kernel.hpp) ------------------------------------------------------------------------
WaveLaunchFn wave_plan(int mode, int R2, int DP, int M, int* G, int* C) {
    const GradInstance g = wave_plan_shape(mode, R2, DP, M);           // grad_plan.hpp
    if (g.family != GRAD_WAVE) return nullptr;
    *G = g.G; *C = g.C;
    return mode == MODE_INC ? wave_lookup_inc(g.G, g.C, DP, M - 1) : (mode == MODE_PT_DIFF ? wave_lookup_ptd(g.G, g.C, DP, M - 1) : wave_lookup_ptn(g.G, g.C, DP, M - 1));
}
static_assert(int(MODE_INC) == int(GRAD_MODE_INC) && int(MODE_PT_DIFF) == int(GRAD_MODE_PT_DIFF) && int(MODE_PT_NODIFF) == int(GRAD_MODE_PT_NODIFF),
              "grad_plan.hpp restates the lattice modes of seq_core.hpp");

// workgroups of lam_contract_kernel: the partner loop waits on its Lam loads, so the launch is sized for several wavefronts per SIMD
constexpr int64_t CONTRACT_BLOCKS = 16384;

template <int SIDE>
int launch_contract(gpsig_ctx* c, int DP, dim3 grid, int block, size_t lds, const LamContractArgs& a) {
    const bool nodiff = a.mode == MODE_PT_NODIFF, rbf = a.kind == BASE_RBF;
#define LC(DP_)                                                                                                                         \
    do {                                                                                                                                \
        if (rbf) {                                                                                                                      \
            if (nodiff) hipLaunchKernelGGL((lam_contract_kernel<DP_, SIDE, BASE_RBF, true>), grid, dim3(block), lds, c->stream, a);     \
            else hipLaunchKernelGGL((lam_contract_kernel<DP_, SIDE, BASE_RBF, false>), grid, dim3(block), lds, c->stream, a);           \
        } else {                                                                                                                        \
            if (nodiff) hipLaunchKernelGGL((lam_contract_kernel<DP_, SIDE, -1, true>), grid, dim3(block), lds, c->stream, a);           \
            else hipLaunchKernelGGL((lam_contract_kernel<DP_, SIDE, -1, false>), grid, dim3(block), lds, c->stream, a);                 \
        }                                                                                                                               \
    } while (0)
    // (round 4: DP = 32 / 64 used to fall into the 16-column instance, which silently dropped the columns beyond 16 -- reached by the
    // higher-order route only, whose callers pad 17 .. 64 columns to 32 / 64; found by the feature route's parity test at d = 32)
    if (DP == 4) LC(4); else if (DP == 8) LC(8); else if (DP == 16) LC(16); else if (DP == 32) LC(32); else if (DP == 64) LC(64);
    else return fail(c, GPSIG_ERR_UNSUPPORTED, "no contraction kernel for %d padded columns", DP);
#undef LC
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

int seq_grad_wave(gpsig_ctx* c, const gpsig_params* p, WaveLaunchFn fn, int G, int C, int DP, int mode, const double* X, const double* Y, int64_t N1,
                  int64_t N2, int L1, int L2, int d, bool diag, bool sym, const double* Gup, double* gX, double* gY, double* gbase) {
    const int M = p->num_levels, dr = mode == MODE_PT_NODIFF ? 0 : 1;
    const int R1 = L1 - dr, R2 = L2 - dr, TF = R1 + G - 1, PW = 64 / G;
    CHK(zero_async(c, gX, sizeof(double) * size_t(N1) * L1 * d));
    if (!diag && !sym) CHK(zero_async(c, gY, sizeof(double) * size_t(N2) * L2 * d));
    if (R1 <= 0 || R2 <= 0) return GPSIG_OK;                 // empty lattice: the levels do not depend on the data
    const size_t per_pair = sizeof(double) * size_t(R1) * R2;
    const int64_t row_pairs = diag ? 1 : N2;
    int64_t ni_max = int64_t(scratch_budget(c) / (per_pair * size_t(row_pairs)));
    if (ni_max < 1) ni_max = 1;
    if (ni_max > N1) ni_max = N1;
    if (ni_max > 65535) ni_max = 65535;
    void *lam, *scr;
    CHK(ensure(c, B_GR5, per_pair * size_t(row_pairs) * size_t(ni_max) + 64, &lam));
    const int64_t max_pairs = ni_max * row_pairs;
    int64_t ngroups = max_pairs < 8192 ? max_pairs : 8192;
    ngroups = (ngroups + PW - 1) / PW * PW;
    const size_t slot = sizeof(double) * size_t(M > 1 ? M - 1 : 1) * TF * G * C;
    CHK(ensure(c, B_GR6, slot * size_t(ngroups) + 64, &scr));
    WaveGradArgs A;
    memset(&A, 0, sizeof(A));
    A.X = X; A.Y = Y; A.N1 = int(N1); A.N2 = int(N2); A.L1 = L1; A.L2 = L2; A.d = d;
    A.M = M; A.kind = p->base_kernel; A.mode = mode; A.p0 = p->base_params[0]; A.p1 = p->base_params[1];
    A.diag = diag ? 1 : 0;
    A.G = Gup; A.gm = diag ? N1 : N1 * N2; A.gi = diag ? 1 : N2; A.gj = diag ? 0 : 1;
    A.scratch = static_cast<double*>(scr); A.lam = static_cast<double*>(lam);
    LamContractArgs K;
    memset(&K, 0, sizeof(K));
    K.X = X; K.Y = Y; K.L1 = L1; K.L2 = L2; K.d = d; K.kind = p->base_kernel; K.mode = mode; K.p0 = A.p0; K.p1 = A.p1;
    K.lam = A.lam; K.diag = A.diag; K.j0 = 0; K.nj = diag ? 1 : N2;
    for (int64_t i0 = 0; i0 < N1; i0 += ni_max) {
        const int64_t ni = (N1 - i0 < ni_max) ? N1 - i0 : ni_max;
        A.pair0 = i0 * row_pairs; A.npairs = ni * row_pairs;
        int64_t ng = A.npairs < ngroups ? A.npairs : ngroups;
        ng = (ng + PW - 1) / PW * PW;
        A.ngroups = int(ng);
        hipError_t e = fn(A, int(ng / PW), c->stream);
        if (e != hipSuccess) return fail(c, GPSIG_ERR_HIP, "seq_grad_wave_kernel launch failed: %s", hipGetErrorString(e));
        K.i0 = i0; K.ni = ni;
        auto slices = [](int64_t targets, int64_t partners) {
            int64_t s = (CONTRACT_BLOCKS + targets - 1) / targets;
            if (s > partners) s = partners;
            if (s > 1024) s = 1024;
            return s < 1 ? int64_t(1) : s;
        };
        // x side: targets i0..i0+ni, partners = all j
        K.gT = gX; K.gbase = gbase;
        K.nslices = int(diag ? 1 : slices(ni, N2));
        int blk = L1 >= 256 ? 256 : int((L1 + 63) / 64 * 64);
        CHK(launch_contract<0>(c, DP, dim3(unsigned(ni), unsigned(K.nslices)), blk, sizeof(double) * size_t(L2) * (DP + 1), K));
        // y side: targets = all j (diag: the same i's), partners = i0..i0+ni
        K.gT = gY; K.gbase = nullptr;
        K.nslices = int(diag ? 1 : slices(N2, ni));
        blk = L2 >= 256 ? 256 : int((L2 + 63) / 64 * 64);
        CHK(launch_contract<1>(c, DP, dim3(unsigned(diag ? ni : N2), unsigned(K.nslices)), blk, sizeof(double) * size_t(L1) * (DP + 1), K));
    }
    return GPSIG_OK;
}


// ---- scratch-free wavefront path (seq_grad_wave2_kernel): one launch per register-resident side ------------------------------
// The linear kernel on increments only; both sides of a call, or neither: wave2_plan_call of grad_plan.hpp (with wave2_lds, the dynamic LDS
// of the scratch-free kernels, and WAVE2_LDS_MAX)
bool wave2_plan(int mode, int R1, int R2, int DP, int M, bool one_side, Wave2LaunchFn* fx, int* Gx, Wave2LaunchFn* fy, int* Gy) {
    GradInstance gx, gy;
    *fx = *fy = nullptr;
    if (!wave2_plan_call(mode, R1, R2, DP, M, one_side, &gx, &gy)) return false;
    *Gx = gx.G; *Gy = gy.G;
    *fx = wave2_lookup_inc(gx.G, gx.C, DP, M - 1);
    *fy = one_side ? *fx : wave2_lookup_inc(gy.G, gy.C, DP, M - 1);
    if (!*fx || !*fy) *fx = *fy = nullptr;
    return *fx != nullptr;
}

// tasks of the scratch-free kernels: one register-side sequence (0 .. NR) x a run of streamed sequences (0 .. NS); diag: (r, r).
int wave2_tasks(gpsig_ctx* c, int64_t NS, int64_t NR, bool diag, const SeqTask** tasks, size_t* ntasks_out) {
    int64_t run = diag ? 1 : (NS * NR + 16383) / 16384;
    if (run < 1) run = 1;
    if (run > NS) run = NS;
    const int64_t key[10] = {NS, NR, run, diag ? 1 : 0, 0, 0, 0, 0, 0, 2};
    int n = 0;
    CHK(task_list(c, key, [&](std::vector<SeqTask>& T) {
        T.clear();
        for (int64_t r = 0; r < NR; ++r) {
            if (diag) { T.push_back(SeqTask{int32_t(r), int32_t(r), 1}); continue; }
            for (int64_t x0 = 0; x0 < NS; x0 += run) T.push_back(SeqTask{int32_t(r), int32_t(x0), int32_t(NS - x0 < run ? NS - x0 : run)});
        }
        return int64_t(0);
    }, tasks, &n));
    *ntasks_out = size_t(n);
    return GPSIG_OK;
}

// gradient of the register-resident side R (NR sequences) against the streamed side S; pairs (s, r) for all s (diag: s == r)
int wave2_side(gpsig_ctx* c, const gpsig_params* p, Wave2LaunchFn fn, int G, int mode, const double* S, const double* R, double* gR, int64_t NS, int64_t NR,
               int LS, int LR, int d, bool diag, const double* Gup, int64_t gm, int64_t gs, int64_t gr, bool gsym, double gscale, double* gbase,
               double gbase_scale) {
    const int M = p->num_levels, dr = mode == MODE_PT_NODIFF ? 0 : 1, PW = 64 / G;
    const int R1 = LS - dr;
    const SeqTask* dt;
    size_t ntasks;
    CHK(wave2_tasks(c, NS, NR, diag, &dt, &ntasks));
    Wave2Args A;
    memset(&A, 0, sizeof(A));
    A.S = S; A.R = R; A.gR = gR; A.NS = int(NS); A.NR = int(NR); A.LS = LS; A.LR = LR; A.d = d;
    A.M = M; A.kind = p->base_kernel; A.mode = mode; A.p0 = p->base_params[0]; A.p1 = p->base_params[1];
    A.tasks = dt; A.ntasks = int(ntasks);
    A.G = Gup; A.gm = gm; A.gs = gs; A.gr = gr; A.gsym = gsym ? 1 : 0; A.gscale = gscale;
    A.gbase = gbase; A.gbase_scale = gbase_scale;
    const int nblocks = int((ntasks + PW - 1) / PW);
    hipError_t e = fn(A, nblocks, wave2_lds(G, R1, M), c->stream);
    if (e != hipSuccess) return fail(c, GPSIG_ERR_HIP, "seq_grad_wave2_kernel launch failed: %s", hipGetErrorString(e));
    return GPSIG_OK;
}

// ---- point kernels: scratch-free sweeps that store Lam (seq_lam_undo_kernel) + lam_contract_kernel for both sides -------------
Wave2LaunchFn lam_undo_plan(int mode, int kind, int R1, int R2, int DP, int M, int* G, int* C) {
    const bool rbf = kind == BASE_RBF;
    const GradInstance g = lam_undo_plan_shape(mode, rbf, R1, R2, DP, M);           // grad_plan.hpp
    if (g.family != GRAD_LAM_UNDO) return nullptr;
    *G = g.G; *C = g.C;
    return mode == MODE_PT_DIFF ? (rbf ? lam_undo_lookup_ptd_rbf : lam_undo_lookup_ptd_gen)(g.G, g.C, DP, M - 1)
                                : (rbf ? lam_undo_lookup_ptn_rbf : lam_undo_lookup_ptn_gen)(g.G, g.C, DP, M - 1);
}

// Blocks of pairs (i0 .. i0+ni) x (j0 .. j0+nj) sized to the scratch budget for Lam.  Symmetric Gram: block rows i0 .. i0+ni
// take the columns j >= i0 only; a pair beyond the block's own square appears once and carries G[i][j] + G[j][i].
int seq_grad_undo(gpsig_ctx* c, const gpsig_params* p, Wave2LaunchFn fn, int G, int DP, int mode, const double* X, const double* Y, int64_t N1,
                  int64_t N2, int L1, int L2, int d, bool diag, bool sym, const double* Gup, double* gX, double* gY, double* gbase) {
    const int M = p->num_levels, dr = mode == MODE_PT_NODIFF ? 0 : 1, PW = 64 / G;
    const int R1 = L1 - dr, R2 = L2 - dr;
    CHK(zero_async(c, gX, sizeof(double) * size_t(N1) * L1 * d));
    if (!diag && !sym) CHK(zero_async(c, gY, sizeof(double) * size_t(N2) * L2 * d));
    if (R1 <= 0 || R2 <= 0) return GPSIG_OK;                 // empty lattice: the levels do not depend on the data
    const size_t per_pair = sizeof(double) * size_t(R1) * R2;
    Wave2Args A;
    memset(&A, 0, sizeof(A));
    A.S = X; A.R = Y; A.NS = int(N1); A.NR = int(N2); A.LS = L1; A.LR = L2; A.d = d;
    A.M = M; A.kind = p->base_kernel; A.mode = mode; A.p0 = p->base_params[0]; A.p1 = p->base_params[1];
    A.G = Gup; A.gm = diag ? N1 : N1 * N2; A.gs = diag ? 1 : N2; A.gr = diag ? 0 : 1; A.gscale = 1.0;
    A.diag = diag ? 1 : 0;
    LamContractArgs K;
    memset(&K, 0, sizeof(K));
    K.X = X; K.Y = Y; K.L1 = L1; K.L2 = L2; K.d = d; K.kind = p->base_kernel; K.mode = mode; K.p0 = A.p0; K.p1 = A.p1;
    K.diag = A.diag;
    {
        // the largest block: never more than the budget unless a single row of pairs exceeds it
        const size_t row = per_pair * size_t(diag ? 1 : N2), all = row * size_t(N1), cap = scratch_budget(c) > row ? scratch_budget(c) : row;
        void* lam;
        CHK(ensure(c, B_GR5, (all < cap ? all : cap) + 64, &lam));
    }
    for (int64_t i0 = 0; i0 < N1;) {
        const int64_t j0 = (diag || sym) ? i0 : 0;
        const int64_t nj = diag ? 1 : N2 - j0;
        int64_t ni = int64_t(scratch_budget(c) / (per_pair * size_t(nj)));
        if (ni < 1) ni = 1;
        if (ni > N1 - i0) ni = N1 - i0;
        if (ni > 65535) ni = 65535;
        void* lam;
        CHK(ensure(c, B_GR5, per_pair * size_t(nj) * size_t(ni) + 64, &lam));
        const SeqTask* dt;
        size_t ntasks;
        CHK(wave2_tasks(c, ni, diag ? ni : nj, diag, &dt, &ntasks));
        A.tasks = dt; A.ntasks = int(ntasks);
        A.lam = static_cast<double*>(lam); A.i0 = i0; A.j0 = j0; A.nj = nj;
        A.gsym = sym ? 1 : 0; A.gsym_from = i0 + ni;
        hipError_t e = fn(A, int((ntasks + PW - 1) / PW), wave2_lds(G, R1, M), c->stream);
        if (e != hipSuccess) return fail(c, GPSIG_ERR_HIP, "seq_lam_undo_kernel launch failed: %s", hipGetErrorString(e));
        K.lam = A.lam; K.i0 = i0; K.ni = ni; K.j0 = j0; K.nj = nj;
        auto slices = [](int64_t targets, int64_t partners) {
            int64_t s = (CONTRACT_BLOCKS + targets - 1) / targets;
            if (s > partners) s = partners;
            if (s > 1024) s = 1024;
            return s < 1 ? int64_t(1) : s;
        };
        K.gT = gX; K.gbase = gbase;
        K.nslices = int(diag ? 1 : slices(ni, nj));
        int blk = L1 >= 256 ? 256 : int((L1 + 63) / 64 * 64);
        CHK(launch_contract<0>(c, DP, dim3(unsigned(ni), unsigned(K.nslices)), blk, sizeof(double) * size_t(L2) * (DP + 1), K));
        K.gT = (diag || sym) ? gX : gY; K.gbase = nullptr;
        K.nslices = int(diag ? 1 : slices(nj, ni));
        blk = L2 >= 256 ? 256 : int((L2 + 63) / 64 * 64);
        CHK(launch_contract<1>(c, DP, dim3(unsigned(diag ? ni : nj), unsigned(K.nslices)), blk, sizeof(double) * size_t(L1) * (DP + 1), K));
        i0 += ni;
    }
    return GPSIG_OK;
}

// ---- RBF on points with differences, order 1: both sweeps and both sides' contractions in one launch (grad_fused_kernel.hpp) ----------
constexpr size_t FUSED_LDS_MAX = 96 * 1024;

// The register-resident side (the lattice's columns) holds at most 64 points with 16 lanes per pair (four pairs per wavefront), at most 256 with
// 64 (one pair per wavefront; half of either with the two columns per lane of 9 .. 16 state-space columns): Y, or -- for a cross Gram whose Y is longer than its X -- X with the roles exchanged (*swap; the lattice of (y, x)
// is the transpose of that of (x, y) and the levels are the same).  nullptr where the kernel is not built.
FusedGradLaunchFn fused_grad_plan(const gpsig_ctx* c, const gpsig_params* p, int mode, int L1, int L2, int DP, bool diag, bool sym, bool* swap, int* G) {
    *swap = false;
    if (c->grad_impl != 0 || diag || mode == MODE_INC || p->order > 1) return nullptr;
    const bool diff = mode == MODE_PT_DIFF;
    const int M = p->num_levels;
    if (M < 2 || M > 6 || DP > (diff ? 16 : 8) || L1 < 2 || L2 < 2) return nullptr;
    const int C = fused_grad_columns(DP);                            // 4 columns per lane; 2 for state spaces of 9 .. 16 columns
    if (!sym && L1 < L2 && L2 > 16 * C) *swap = true;                 // the shorter side on the columns once the longer one needs 64 lanes
    const int cols = *swap ? L1 : L2, rows = *swap ? L2 : L1;
    if (cols > 64 * C) return nullptr;
    *G = cols > 32 * C ? 64 : (cols > 16 * C ? 32 : 16);
    if (sizeof(double) * size_t(fused_lds(rows, rows - (diff ? 1 : 0), DP, M - 1, *G, C).total) > FUSED_LDS_MAX) return nullptr;
    return fused_grad_lookup(p->base_kernel, DP, M - 1, *G, diff);  // RBF and the Matern families
}

// Tasks: 64 / G consecutive register-side sequences (a "quad") against a run of streamed ones.  Symmetric Gram: the runs start at the quad's
// first sequence -- every unordered pair once (the kernel skips s < r inside the quad's own square), carrying G[s][r] + G[r][s].
// S / R: the streamed / register-resident side (X / Y unless the plan exchanged them); gs / gr: the upstream's strides along them.
int seq_grad_fused(gpsig_ctx* c, const gpsig_params* p, FusedGradLaunchFn fn, int G, int DP, bool diff, const double* S, const double* R, int64_t NS, int64_t NR, int LS,
                   int LR, int d, bool sym, const double* Gup, int64_t gs, int64_t gr, double* gS, double* gR) {
    const int PW = 64 / G;
    CHK(zero_async(c, gS, sizeof(double) * size_t(NS) * LS * d));
    if (!sym) CHK(zero_async(c, gR, sizeof(double) * size_t(NR) * LR * d));
    const int64_t quads = (NR + PW - 1) / PW;
    const int64_t work = sym ? quads * (NS + 1) / 2 : quads * NS;          // (quad, streamed sequence) units
    int64_t run = work / 8192;
    run = run < 1 ? 1 : (run > 32 ? 32 : run);
    const int64_t key[10] = {NS, NR, run, sym ? 1 : 0, PW, 0, 0, 0, 0, 3};
    const SeqTask* dt;
    int n = 0;
    CHK(task_list(c, key, [&](std::vector<SeqTask>& T) {
        T.clear();
        for (int64_t r0 = 0; r0 < NR; r0 += PW)
            for (int64_t x0 = sym ? r0 : 0; x0 < NS; x0 += run) T.push_back(SeqTask{int32_t(r0), int32_t(x0), int32_t(NS - x0 < run ? NS - x0 : run)});
        return int64_t(0);
    }, &dt, &n));
    if (n == 0) return GPSIG_OK;
    FusedGradArgs A;
    memset(&A, 0, sizeof(A));
    A.S = S; A.R = R; A.gS = gS; A.gR = sym ? gS : gR;
    A.NS = int(NS); A.NR = int(NR); A.LS = LS; A.LR = LR; A.d = d;
    A.tasks = dt;
    A.G = Gup; A.gm = NS * NR; A.gs = gs; A.gr = gr;
    A.sym = sym ? 1 : 0;
    const hipError_t e = fn(A, n, sizeof(double) * size_t(fused_lds(LS, LS - (diff ? 1 : 0), DP, p->num_levels - 1, G, fused_grad_columns(DP)).total), c->stream);
    if (e != hipSuccess) return fail(c, GPSIG_ERR_HIP, "seq_grad_fused_kernel launch failed: %s", hipGetErrorString(e));
    return GPSIG_OK;
}

// The backward sweep alone, continuing from the stash gpsig_seq_gram_levels_stash left in the context (desc: its descriptor).  The tasks are
// pieces of the evaluation kernel's own tasks -- same quads of register-side sequences, same runs (circulant for the symmetric Gram: streamed
// indices wrap and a pair belongs to whichever orientation seq_emit owns) -- so that a pair's slot in the stash is where that kernel wrote it.
int seq_grad_fused_stash(gpsig_ctx* c, const gpsig_params* p, int DP, const double* X, const double* Y, int64_t N1, int64_t N2, int L1, int L2, int d,
                         bool sym, const double* Gup, double* gX, double* gY, const int64_t* desc, bool* done) {
    *done = false;
    const int M = p->num_levels, LQ = M - 1;
    if (desc[0] == 0 || desc[0] != c->stash_gen || desc[0] != c->stash_desc[0]) return GPSIG_OK;             // nothing kept, or overwritten since
    const int pred = int(desc[1]), ypb = int(desc[3]);
    const int64_t max_run = desc[2];
    if (ypb != 4 || desc[7] != L1 - 1 || desc[6] != fused_stash_stride(L1 - 1, LQ, 16, 4) || (pred != PRED_ALL && pred != PRED_CIRCULANT)) return GPSIG_OK;
    if ((pred == PRED_CIRCULANT) != sym && !(sym && pred == PRED_ALL)) return GPSIG_OK;
    FusedGradLaunchFn fn = fused_grad_stash_lookup(p->base_kernel, DP, LQ);
    void* st = c->buf[B_STASH].p;
    if (!fn || !st || L2 > 64 || L1 < 2 || L2 < 2) return GPSIG_OK;
    const size_t lds = sizeof(double) * size_t(fused_lds(L1, L1 - 1, DP, LQ, 16, 4).total);
    if (lds > FUSED_LDS_MAX) return GPSIG_OK;
    CHK(zero_async(c, gX, sizeof(double) * size_t(N1) * L1 * d));
    if (!sym) CHK(zero_async(c, gY, sizeof(double) * size_t(N2) * L2 * d));
    const int64_t PIECE = c->grad_fused_piece > 0 ? c->grad_fused_piece : 16;       // streamed sequences per workgroup
    const int64_t key[10] = {N1, N2, max_run, pred, PIECE, 0, 0, 0, 0, 5}, key2[10] = {N1, N2, max_run, pred, PIECE, 0, 0, 0, 0, 6};
    auto pieces = [&](std::vector<SeqTask>& T, bool bases) {
        std::vector<SeqTask> F = seq_build_tasks(N1, N2, ypb, pred, int(max_run), 0, 1);
        T.clear();
        int64_t at = 0;
        for (const SeqTask& t : F) {
            for (int64_t o = 0; o < t.nx; o += PIECE) {
                const int64_t n = t.nx - o < PIECE ? t.nx - o : PIECE, a0 = at + o;
                int64_t x0 = int64_t(t.x0) + o;
                if (pred == PRED_CIRCULANT) x0 %= N1;
                if (bases) T.push_back(SeqTask{int32_t(uint32_t(a0 & 0xffffffff)), int32_t(a0 >> 32), 0});
                else T.push_back(SeqTask{t.y0, int32_t(x0), int32_t(n)});
            }
            at += t.nx;
        }
        return at;
    };
    const SeqTask *dt, *dp;
    int n = 0, n2 = 0;
    int64_t slots = 0;
    CHK(task_list(c, key, [&](std::vector<SeqTask>& T) { return pieces(T, false); }, &dt, &n, &slots));
    CHK(task_list(c, key2, [&](std::vector<SeqTask>& T) { return pieces(T, true); }, &dp, &n2));
    if (n == 0 || n != n2 || slots * ypb != desc[5]) return GPSIG_OK;
    FusedGradArgs A;
    memset(&A, 0, sizeof(A));
    const bool circ = pred == PRED_CIRCULANT;
    A.S = X; A.R = Y; A.gS = gX; A.gR = sym ? gX : gY;
    A.NS = int(N1); A.NR = int(N2); A.LS = L1; A.LR = L2; A.d = d;
    A.tasks = dt; A.pair0_list = dp;
    A.G = Gup; A.gm = N1 * N2; A.gs = N2; A.gr = 1;
    A.sym = circ ? 1 : 0;                               // (a symmetric Gram evaluated pair by pair, PRED_ALL: every ordered pair with its own G[s][r])
    A.circ = circ ? 1 : 0;
    A.stash = static_cast<const double*>(st); A.stash_stride = desc[6];
    const hipError_t e = fn(A, n, lds, c->stream);
    if (e != hipSuccess) return fail(c, GPSIG_ERR_HIP, "seq_grad_fused_kernel (backward sweep from the stash) launch failed: %s", hipGetErrorString(e));
    *done = true;
    return GPSIG_OK;
}

// ---- higher-order algorithm (order > 1), fused: ho_dm_kernel -> both sweeps of a pair in one wavefront (grad_wave_ho_kernel.hpp) ->
// lam_contract_kernel.  num_levels <= 5, min(order, num_levels) <= 4, lattices of at most 512 columns.  The scratch-free sweeps where their
// row totals fit LDS (option grad_impl = 0), otherwise -- or with grad_impl = 3 -- the sweeps with the prefixes in an HBM slot per pair group;
// any other grad_impl keeps the lattice operations below (the A/B reference of the tests).
int seq_grad_ho_wave(gpsig_ctx* c, const gpsig_params* p, int DP, int mode, const double* X, const double* Y, int64_t N1, int64_t N2, int L1, int L2,
                     int d, bool diag, bool sym, const double* Gup, double* gX, double* gY, double* gbase, bool* done) {
    *done = false;
    const int M = p->num_levels, dr = mode == MODE_PT_NODIFF ? 0 : 1;
    const int R1 = L1 - dr, R2 = L2 - dr;
    HoSweeps hs;
    if (!ho_sweeps_plan(c, p, R1, R2, &hs)) return GPSIG_OK;
    const size_t cells = size_t(R1) * R2, per_pair = sizeof(double) * cells * 2;           // dM and Lam
    const int64_t gm = diag ? N1 : N1 * N2, gi = diag ? 1 : N2, gj = diag ? 0 : 1;
    const int64_t nj = diag ? 1 : N2;
    // slot kernel: half of the budget for the lattices of a pair block, half for the slots of the groups in flight
    int64_t ni_max = int64_t(scratch_budget(c) / (hs.slot ? 2 : 1) / (per_pair * size_t(nj)));
    if (ni_max < 1) ni_max = 1;
    if (ni_max > N1) ni_max = N1;
    if (ni_max > 65535) ni_max = 65535;
    void* lat;
    CHK(ensure(c, B_GR5, per_pair * size_t(nj) * size_t(ni_max) + 64, &lat));
    // the symmetric Gram (one array on both sides): the pairs i <= j with the upstream gradient folded onto them, as the wide route's reverse pass
    const bool fold = sym && !diag && N1 == N2 && L1 == L2 && c->wide_sym_fold != 0;
    if (fold) {
        const int64_t cap = N1 / 16 > 8 ? N1 / 16 : 8;          // (the chunk's square below the diagonal is swept with zero upstream gradients: keep it small)
        if (ni_max > cap) ni_max = cap;
        void* gs;
        CHK(ensure(c, B_WD10, sizeof(double) * size_t(M + 1) * N1 * N1 + 64, &gs));
        hipLaunchKernelGGL(ho_sym_upstream_kernel, dim3(grid_for(int64_t(M + 1) * N1 * N1)), dim3(256), 0, c->stream, Gup, N1, M + 1, static_cast<double*>(gs));
        HIPCHK(c, hipGetLastError());
        Gup = static_cast<const double*>(gs);
    }
    LamContractArgs K;
    memset(&K, 0, sizeof(K));
    K.X = X; K.Y = Y; K.L1 = L1; K.L2 = L2; K.d = d; K.kind = p->base_kernel; K.mode = mode == MODE_INC ? MODE_PT_DIFF : mode;
    K.p0 = p->base_params[0]; K.p1 = p->base_params[1]; K.diag = diag ? 1 : 0;
    for (int64_t i0 = 0; i0 < N1; i0 += ni_max) {
        const int64_t ni = (N1 - i0 < ni_max) ? N1 - i0 : ni_max;
        const int64_t j0 = fold ? i0 : 0, nje = nj - j0;             // the chunk's right sequences
        const int64_t npairs = ni * nje, P = npairs * int64_t(cells);
        double* const dmat = static_cast<double*>(lat);
        double* const lam = dmat + P;
        const HoBlock B{i0, ni, diag ? i0 : j0, nje, diag ? 1 : 0};
        hipLaunchKernelGGL(ho_dm_kernel, dim3(grid_for(P)), dim3(256), 0, c->stream, X, Y, L1, L2, d, int(p->base_kernel), mode == MODE_PT_NODIFF ? 1 : 0,
                           K.p0, K.p1, B, R1, R2, dmat);
        HIPCHK(c, hipGetLastError());
        CHK(ho_sweeps_launch(c, hs, M, R1, R2, dmat, lam, Gup + j0, gm, gi, gj, diag ? N2 : nje, diag, i0 * nje, npairs));
        K.lam = lam; K.i0 = i0; K.ni = ni; K.j0 = B.j0; K.nj = nje;
        auto slices = [](int64_t targets, int64_t partners) {
            int64_t s = (CONTRACT_BLOCKS + targets - 1) / targets;
            if (s > partners) s = partners;
            if (s > 1024) s = 1024;
            return s < 1 ? int64_t(1) : s;
        };
        K.gT = gX; K.gbase = gbase;
        K.nslices = int(diag ? 1 : slices(ni, nje));
        int blk = L1 >= 256 ? 256 : int((L1 + 63) / 64 * 64);
        CHK(launch_contract<0>(c, DP, dim3(unsigned(ni), unsigned(K.nslices)), blk, sizeof(double) * size_t(L2) * (DP + 1), K));
        K.gT = (diag || sym) ? gX : gY; K.gbase = nullptr;
        K.nslices = int(diag ? 1 : slices(nje, ni));
        blk = L2 >= 256 ? 256 : int((L2 + 63) / 64 * 64);
        CHK(launch_contract<1>(c, DP, dim3(unsigned(diag ? ni : nje), unsigned(K.nslices)), blk, sizeof(double) * size_t(L1) * (DP + 1), K));
    }
    *done = true;
    return GPSIG_OK;
}

// ---- higher-order algorithm (order > 1): lattice operations over blocks of pairs (grad_ho_kernels.hpp) + lam_contract_kernel ----
int seq_grad_ho(gpsig_ctx* c, const gpsig_params* p, int DP, int mode, const double* X, const double* Y, int64_t N1, int64_t N2, int L1, int L2,
                int d, bool diag, bool sym, const double* Gup, double* gX, double* gY, double* gbase) {
    const int M = p->num_levels, D = p->order, dr = mode == MODE_PT_NODIFF ? 0 : 1;
    const int R1 = L1 - dr, R2 = L2 - dr;
    CHK(zero_async(c, gX, sizeof(double) * size_t(N1) * L1 * d));
    if (!diag && !sym) CHK(zero_async(c, gY, sizeof(double) * size_t(N2) * L2 * d));
    if (R1 <= 0 || R2 <= 0) return GPSIG_OK;
    {
        bool fused = false;
        CHK(seq_grad_ho_wave(c, p, DP, mode, X, Y, N1, N2, L1, L2, d, diag, sym, Gup, gX, gY, gbase, &fused));
        if (fused) return GPSIG_OK;
    }
    auto dm_of = [&](int m) { return m < D ? m : D; };
    // slots: dM | R_m[r][s] for m = 2 .. M-1 | two grids of adjoints | two temporaries | Lam
    std::vector<int> roff(M + 1, 0);
    int nslots = 1;
    for (int m = 2; m <= M - 1; ++m) { roff[m] = nslots; nslots += dm_of(m) * dm_of(m); }
    const int u0 = nslots, u1 = u0 + D * D, t0 = u1 + D * D, t1 = t0 + 1, lamslot = t1 + 1;
    nslots = lamslot + 1;
    const size_t cells = size_t(R1) * R2, per_pair = sizeof(double) * cells * size_t(nslots);
    const int64_t gm = diag ? N1 : N1 * N2, gi = diag ? 1 : N2, gj = diag ? 0 : 1;
    LamContractArgs K;
    memset(&K, 0, sizeof(K));
    // the double increment of <x, y> is the lattice of the linear kernel on increments: the contraction takes it as a point kernel
    K.X = X; K.Y = Y; K.L1 = L1; K.L2 = L2; K.d = d; K.kind = p->base_kernel; K.mode = mode == MODE_INC ? MODE_PT_DIFF : mode;
    K.p0 = p->base_params[0]; K.p1 = p->base_params[1]; K.diag = diag ? 1 : 0;
    for (int64_t i0 = 0; i0 < N1;) {
        const int64_t nj = diag ? 1 : N2;
        int64_t ni = int64_t(scratch_budget(c) / (per_pair * size_t(nj)));
        if (ni < 1) ni = 1;
        if (ni > N1 - i0) ni = N1 - i0;
        if (ni > 65535) ni = 65535;
        void* scr;
        CHK(ensure(c, B_GR5, per_pair * size_t(nj) * size_t(ni) + 64, &scr));
        const int64_t npairs = ni * nj, P = npairs * int64_t(cells);
        double* const base = static_cast<double*>(scr);
        auto slot = [&](int k) { return base + int64_t(k) * P; };
        auto Rm = [&](int m, int r, int s) { return m == 1 ? slot(0) : slot(roff[m] + r * dm_of(m) + s); };
        const HoBlock B{i0, ni, diag ? i0 : 0, nj, diag ? 1 : 0};
        auto mul = [&](const double* A_, const double* B_, double* dst, double scale, int acc) {
            hipLaunchKernelGGL(ho_mul_kernel, dim3(grid_for(P)), dim3(256), 0, c->stream, A_, B_, dst, P, scale, acc);
        };
        auto cum = [&](const double* src, double* dst, int axis, int reverse) {
            hipLaunchKernelGGL(ho_cumsum_kernel, dim3(grid_for(npairs * (axis == 0 ? R2 : R1), 64)), dim3(64), 0, c->stream, src, dst, npairs, R1,
                               R2, axis, reverse, 1.0, 0);
        };
        auto bcast = [&](int m, double* dst, int acc) {
            hipLaunchKernelGGL(ho_bcast_kernel, dim3(grid_for(P)), dim3(256), 0, c->stream, Gup, int64_t(m) * gm, gi, gj, B, int64_t(cells), dst, acc);
        };
        // sums of the previous level's grid into t0: all of it, column j2 (over r), row j2 (over s)
        auto sum_all = [&](int m) { const int dp = dm_of(m); for (int r = 0; r < dp; ++r) for (int s = 0; s < dp; ++s) mul(Rm(m, r, s), nullptr, slot(t0), 1.0, r + s > 0); };
        auto sum_col = [&](int m, int j2) { const int dp = dm_of(m); for (int r = 0; r < dp; ++r) mul(Rm(m, r, j2), nullptr, slot(t0), 1.0, r > 0); };
        auto sum_row = [&](int m, int j2) { const int dp = dm_of(m); for (int s = 0; s < dp; ++s) mul(Rm(m, j2, s), nullptr, slot(t0), 1.0, s > 0); };
        hipLaunchKernelGGL(ho_dm_kernel, dim3(grid_for(P)), dim3(256), 0, c->stream, X, Y, L1, L2, d, int(p->base_kernel), mode == MODE_PT_NODIFF ? 1 : 0,
                           K.p0, K.p1, B, R1, R2, slot(0));
        // forward: the grids of levels 2 .. M-1 (signature_algs.py:61-69); level M's own grid is never needed
        for (int m = 2; m <= M - 1; ++m) {
            const int dc = dm_of(m);
            sum_all(m - 1); cum(slot(t0), slot(t1), 0, 0); cum(slot(t1), slot(t0), 1, 0);
            mul(slot(0), slot(t0), Rm(m, 0, 0), 1.0, 0);                                                   // :64
            for (int j = 2; j <= dc; ++j) {
                sum_col(m - 1, j - 2); cum(slot(t0), slot(t1), 0, 0);
                mul(slot(0), slot(t1), Rm(m, 0, j - 1), 1.0 / j, 0);                                       // :66
                sum_row(m - 1, j - 2); cum(slot(t0), slot(t1), 1, 0);
                mul(slot(0), slot(t1), Rm(m, j - 1, 0), 1.0 / j, 0);                                       // :67
                for (int k = 2; k <= dc; ++k) mul(slot(0), Rm(m - 1, j - 2, k - 2), Rm(m, j - 1, k - 1), 1.0 / (double(j) * k), 0);   // :69
            }
        }
        // backward
        int ucur = u0, unext = u1;
        auto U = [&](int set, int r, int s) { return slot(set + r * D + s); };
        for (int r = 0; r < dm_of(M); ++r) for (int s = 0; s < dm_of(M); ++s) bcast(M, U(ucur, r, s), 0);
        CHK(zero_async(c, slot(lamslot), sizeof(double) * size_t(P)));
        for (int m = M; m >= 2; --m) {
            const int dc = dm_of(m), dp = dm_of(m - 1);
            // Lam += U_m[r][s] * (multiplier of dM in R_m[r][s])
            sum_all(m - 1); cum(slot(t0), slot(t1), 0, 0); cum(slot(t1), slot(t0), 1, 0);
            mul(U(ucur, 0, 0), slot(t0), slot(lamslot), 1.0, 1);
            for (int j = 2; j <= dc; ++j) {
                sum_col(m - 1, j - 2); cum(slot(t0), slot(t1), 0, 0);
                mul(U(ucur, 0, j - 1), slot(t1), slot(lamslot), 1.0 / j, 1);
                sum_row(m - 1, j - 2); cum(slot(t0), slot(t1), 1, 0);
                mul(U(ucur, j - 1, 0), slot(t1), slot(lamslot), 1.0 / j, 1);
                for (int k = 2; k <= dc; ++k) mul(U(ucur, j - 1, k - 1), Rm(m - 1, j - 2, k - 2), slot(lamslot), 1.0 / (double(j) * k), 1);
            }
            // U_{m-1}: upstream of K_{m-1} + the transposed operations of level m
            mul(slot(0), U(ucur, 0, 0), slot(t0), 1.0, 0); cum(slot(t0), slot(t1), 0, 1); cum(slot(t1), slot(t0), 1, 1);
            for (int r = 0; r < dp; ++r)
                for (int s = 0; s < dp; ++s) { bcast(m - 1, U(unext, r, s), 0); mul(slot(t0), nullptr, U(unext, r, s), 1.0, 1); }
            for (int j = 2; j <= dc; ++j) {
                mul(slot(0), U(ucur, 0, j - 1), slot(t0), 1.0 / j, 0); cum(slot(t0), slot(t1), 0, 1);
                for (int r = 0; r < dp; ++r) mul(slot(t1), nullptr, U(unext, r, j - 2), 1.0, 1);
                mul(slot(0), U(ucur, j - 1, 0), slot(t0), 1.0 / j, 0); cum(slot(t0), slot(t1), 1, 1);
                for (int s = 0; s < dp; ++s) mul(slot(t1), nullptr, U(unext, j - 2, s), 1.0, 1);
                for (int k = 2; k <= dc; ++k) mul(slot(0), U(ucur, j - 1, k - 1), U(unext, j - 2, k - 2), 1.0 / (double(j) * k), 1);
            }
            std::swap(ucur, unext);
        }
        mul(U(ucur, 0, 0), nullptr, slot(lamslot), 1.0, 1);                                              // level 1: R_1 = dM
        HIPCHK(c, hipGetLastError());
        // Lam -> gradients of both sides
        K.lam = slot(lamslot); K.i0 = i0; K.ni = ni; K.j0 = B.j0; K.nj = nj;
        auto slices = [](int64_t targets, int64_t partners) {
            int64_t s = (CONTRACT_BLOCKS + targets - 1) / targets;
            if (s > partners) s = partners;
            if (s > 1024) s = 1024;
            return s < 1 ? int64_t(1) : s;
        };
        K.gT = gX; K.gbase = gbase;
        K.nslices = int(diag ? 1 : slices(ni, nj));
        int blk = L1 >= 256 ? 256 : int((L1 + 63) / 64 * 64);
        CHK(launch_contract<0>(c, DP, dim3(unsigned(ni), unsigned(K.nslices)), blk, sizeof(double) * size_t(L2) * (DP + 1), K));
        K.gT = (diag || sym) ? gX : gY; K.gbase = nullptr;
        K.nslices = int(diag ? 1 : slices(nj, ni));
        blk = L2 >= 256 ? 256 : int((L2 + 63) / 64 * 64);
        CHK(launch_contract<1>(c, DP, dim3(unsigned(diag ? ni : nj), unsigned(K.nslices)), blk, sizeof(double) * size_t(L1) * (DP + 1), K));
        i0 += ni;
    }
    return GPSIG_OK;
}

// shared body of the Gram and the diagonal gradient
int seq_grad(gpsig_ctx* c, const gpsig_params* p, const void* X, const void* Y, int64_t N1, int64_t N2, int L1, int L2, bool diag,
             const void* G, void* gX, void* gY, double* g_base) {
    int d, DP;
    CHK(grad_check(c, p, &d, &DP, 4096));
    if (N1 < 0 || N2 < 0 || L1 < 1 || L2 < 1) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    // wide route (wide_api.hip): argument lattices by dgemm, both sweeps by one wavefront per lattice, the adjoint contracted back by dgemms
    const bool wide_ho = N1 > 0 && N2 > 0 && wide_lat_ho_available(c, p, L1, (diag || Y == nullptr) ? L1 : L2);      // order > 1: the reverse pass only
    const bool wide_ok = wide_ho || (N1 > 0 && N2 > 0 && wide_lat_available(c, p, L1, (diag || Y == nullptr) ? L1 : L2));
    if (DP == 0 && !wide_ok) return fail(c, GPSIG_ERR_UNSUPPORTED, "gradients are built for at most 64 feature columns here (got %d)", d);
    // SignaturePoly's sequence GRAM gradient beyond 64 columns stays refused although the wide lattices would take it (its level diagonals are served):
    // tests/test_gpu_grad.py (the block at "beyond 64 columns ... an error for the others", poly at 65 columns) pins this answer
    if (DP == 0 && !diag && p->base_kernel == GPSIG_BASE_POLY)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "gradients are built for at most 64 feature columns here (got %d)", d);
    if (N1 > 0x7fffffff || N2 > 0x7fffffff) return fail(c, GPSIG_ERR_UNSUPPORTED, "more than 2^31 sequences");
    const bool sym = !diag && Y == nullptr;
    if (sym) { N2 = N1; L2 = L1; }
    const int M = p->num_levels, M1 = M + 1;
    const int mode = lattice_mode(p);
    const size_t xb = sizeof(double) * size_t(N1) * L1 * d, yb = sizeof(double) * size_t(N2) * L2 * d;
    const size_t gb = sizeof(double) * size_t(M1) * N1 * (diag ? 1 : N2);
    const void *dX, *dY = nullptr, *dG;
    CHK(in_dev(c, B_IN0, X, xb, &dX));
    if (!diag && !sym) CHK(in_dev(c, B_IN1, Y, yb, &dY));
    CHK(in_dev(c, B_IN2, G, gb, &dG));
    void *dgX, *dgY = nullptr;
    CHK(out_dev(c, B_OUT0, gX, xb, &dgX));
    if (!diag && !sym) CHK(out_dev(c, B_OUT1, gY, yb, &dgY));
    double* dgb;
    CHK(gbase_begin(c, &dgb));
    // kernels without a differentiable base parameter skip the accumulation (one same-address atomic per wavefront otherwise)
    double* const kgb = (p->base_kernel == GPSIG_BASE_POLY || p->base_kernel == GPSIG_BASE_MIX) ? dgb : nullptr;
    WaveLaunchFn wfn = nullptr;
    Wave2LaunchFn w2x = nullptr, w2y = nullptr;            // scratch-free kernels with x resp. y as the register-resident side
    int wG = 0, wC = 0, w2xG = 0, w2yG = 0;
    const int drr = mode == MODE_PT_NODIFF ? 0 : 1;
    if ((c->grad_impl == 0 || c->grad_impl == 3 || c->grad_impl == 4) && N1 > 0 && N2 > 0) wfn = wave_plan(mode, L2 - drr, DP, M, &wG, &wC);
    if ((c->grad_impl == 0 || c->grad_impl == 4) && N1 > 0 && N2 > 0) wave2_plan(mode, L1 - drr, L2 - drr, DP, M, diag || sym, &w2x, &w2xG, &w2y, &w2yG);
    Wave2LaunchFn lfn = nullptr;                           // point kernels: scratch-free sweeps with Lam out
    int lG = 0, lC = 0;
    if ((c->grad_impl == 0 || c->grad_impl == 4) && N1 > 0 && N2 > 0) lfn = lam_undo_plan(mode, p->base_kernel, L1 - drr, L2 - drr, DP, M, &lG, &lC);
    bool fswap = false;
    int fG = 16;
    FusedGradLaunchFn ffn = (N1 > 0 && N2 > 0 && DP > 0) ? fused_grad_plan(c, p, mode, L1, L2, DP, diag, sym, &fswap, &fG) : nullptr;
    // where the fused reverse kernel is not built (more than 16 columns, long register sides) the wide route takes over; option wide = 1: wherever built
    // (beyond 8 columns, or where no wavefront kernel is built at all: at <= 8 columns the scratch-free sweeps measured 10-25 % ahead on the
    // reference's shapes -- profiles/r06_ab_small_widths.txt; grad_impl != 0: A/B runs of the exact-shape kernels)
    // (higher order: the point route's dM and contraction kernels cost more than the sweeps -- ho_dm_kernel evaluates every kappa four times with the
    // library's exp --, so the wide route's dgemms take RBF and the Matern families at every width)
    // (the dot-product families: beyond 32 columns, or by option -- up to there the feature route and the exact-shape kernels below keep them;
    // SignaturePoly, SignatureMix: beyond 64 columns -- DP == 0 --, or by option)
    const bool wide_rule = wide_base_param_kind(p->base_kernel) ? false : (wide_dot_kind(p->base_kernel) ? d > 32 : (d > 8 || (!w2x && !lfn && !wfn)));
    if (wide_ok && (c->wide == 1 || DP == 0 || wide_ho || (!ffn && c->grad_impl == 0 && wide_rule))) {
        CHK(wide_lat_backward(c, p, d, static_cast<const double*>(dX), static_cast<const double*>((diag || sym) ? nullptr : dY), N1, N2, L1, L2, diag,
                              static_cast<const double*>(dG), static_cast<double*>(dgX), static_cast<double*>(dgY), kgb));
        CHK(out_done(c, gX, dgX, xb));
        if (!diag && !sym) CHK(out_done(c, gY, dgY, yb));
        CHK(gbase_end(c, dgb, g_base));
        return finish(c);
    }
    bool by_features = false;      // the linear kernel, first order: through the feature contraction where that is cheaper (round 4)
    if (N1 > 0 && N2 > 0)
        CHK(sig_features_grad(c, p, d, static_cast<const double*>(dX), static_cast<const double*>(sym || diag ? dX : dY), N1, N2, L1, L2, diag, sym,
                              static_cast<const double*>(dG), static_cast<double*>(dgX), static_cast<double*>(dgY), &by_features));
    if (by_features) {
    } else if (N1 == 0 || N2 == 0) {
        if (xb) CHK(zero_async(c, dgX, xb));
        if (dgY && yb) CHK(zero_async(c, dgY, yb));
    } else if (p->order > 1 && M > 1) {
        // the symmetric Gram is taken as the cross Gram of X with itself: both sides' gradients land in gX
        CHK(seq_grad_ho(c, p, DP, mode, static_cast<const double*>(dX), static_cast<const double*>(sym || diag ? dX : dY), N1, N2, L1, L2, d, diag, sym,
                        static_cast<const double*>(dG), static_cast<double*>(dgX), static_cast<double*>(sym || diag ? dgX : dgY), kgb));
    } else if (ffn) {
        const double *Xd = static_cast<const double*>(dX), *Yd = static_cast<const double*>(sym ? dX : dY);
        double *gXd = static_cast<double*>(dgX), *gYd = static_cast<double*>(sym ? dgX : dgY);
        if (fswap) CHK(seq_grad_fused(c, p, ffn, fG, DP, mode == MODE_PT_DIFF, Yd, Xd, N2, N1, L2, L1, d, false, static_cast<const double*>(dG), 1, N2, gYd, gXd));
        else CHK(seq_grad_fused(c, p, ffn, fG, DP, mode == MODE_PT_DIFF, Xd, Yd, N1, N2, L1, L2, d, sym, static_cast<const double*>(dG), N2, 1, gXd, gYd));
    } else if (w2x) {
        const double* Xd = static_cast<const double*>(dX);
        const double* Gd = static_cast<const double*>(dG);
        CHK(zero_async(c, dgX, xb));
        if (diag) {
            // both roles of the pair (x_i, x_i) have the same derivative: twice the register-side gradient
            CHK(wave2_side(c, p, w2x, w2xG, mode, Xd, Xd, static_cast<double*>(dgX), N1, N1, L1, L1, d, true, Gd, N1, 1, 0, false, 2.0, kgb, 0.5));
        } else if (sym) {
            // k(x_s, x_r) = k(x_r, x_s): the gradient of x_r collects G[s][r] + G[r][s] over all s
            CHK(wave2_side(c, p, w2x, w2xG, mode, Xd, Xd, static_cast<double*>(dgX), N1, N1, L1, L1, d, false, Gd, N1 * N1, N1, 1, true, 1.0, kgb, 0.5));
        } else {
            const double* Yd = static_cast<const double*>(dY);
            CHK(zero_async(c, dgY, yb));
            CHK(wave2_side(c, p, w2y, w2yG, mode, Xd, Yd, static_cast<double*>(dgY), N1, N2, L1, L2, d, false, Gd, N1 * N2, N2, 1, false, 1.0, kgb, 1.0));
            CHK(wave2_side(c, p, w2x, w2xG, mode, Yd, Xd, static_cast<double*>(dgX), N2, N1, L2, L1, d, false, Gd, N1 * N2, 1, N2, false, 1.0, nullptr, 0.0));
        }
    } else if (lfn) {
        CHK(seq_grad_undo(c, p, lfn, lG, DP, mode, static_cast<const double*>(dX), static_cast<const double*>(sym || diag ? dX : dY), N1, N2, L1, L2, d,
                          diag, sym, static_cast<const double*>(dG), static_cast<double*>(dgX), static_cast<double*>(sym || diag ? dgX : dgY), kgb));
    } else if (wfn) {
        CHK(seq_grad_wave(c, p, wfn, wG, wC, DP, mode, static_cast<const double*>(dX), static_cast<const double*>(sym || diag ? dX : dY), N1, N2, L1, L2, d,
                          diag, sym, static_cast<const double*>(dG), static_cast<double*>(dgX), static_cast<double*>(sym || diag ? dgX : dgY), kgb));
    } else {
        const int64_t s1 = pad64(N1), s2 = pad64(N2);
        void *xT, *yT = nullptr, *gxT, *gyT = nullptr;
        const size_t xtb = sizeof(double) * size_t(L1) * DP * s1, ytb = sizeof(double) * size_t(L2) * DP * s2;
        CHK(ensure(c, B_GR0, xtb, &xT));
        CHK(ensure(c, B_GR2, xtb, &gxT));
        CHK(to_timemajor(c, static_cast<const double*>(dX), static_cast<double*>(xT), N1, L1, d, DP, s1));
        CHK(zero_async(c, gxT, xtb));
        if (!diag && !sym) {
            CHK(ensure(c, B_GR1, ytb, &yT));
            CHK(ensure(c, B_GR3, ytb, &gyT));
            CHK(to_timemajor(c, static_cast<const double*>(dY), static_cast<double*>(yT), N2, L2, d, DP, s2));
            CHK(zero_async(c, gyT, ytb));
        }
        const int dr = mode == MODE_PT_NODIFF ? 0 : 1;
        const int R1 = L1 - dr, R2 = L2 - dr;
        const size_t per_j = sizeof(double) * size_t(M) * size_t(R1 > 0 ? R1 : 0) * size_t(R2 > 0 ? R2 : 0) * size_t(s1);
        int64_t chunk = diag ? 1 : int64_t(scratch_budget(c) / (per_j ? per_j : 1));
        if (chunk < 1) chunk = 1;
        if (chunk > N2) chunk = N2;
        if (chunk > 65535) chunk = 65535;
        void* scr;
        CHK(ensure(c, B_GR4, per_j * size_t(chunk) + 64, &scr));
        SeqGradArgs A;
        memset(&A, 0, sizeof(A));
        A.xT = static_cast<const double*>(xT);
        A.yT = (diag || sym) ? A.xT : static_cast<const double*>(yT);
        A.gxT = static_cast<double*>(gxT);
        A.gyT = (diag || sym) ? A.gxT : static_cast<double*>(gyT);
        A.xstride = s1;
        A.ystride = (diag || sym) ? s1 : s2;
        A.N1 = int(N1); A.N2 = int(N2); A.L1 = L1; A.L2 = L2;
        A.M = M; A.kind = p->base_kernel; A.mode = mode;
        A.p0 = p->base_params[0]; A.p1 = p->base_params[1];
        A.diag = diag ? 1 : 0;
        A.G = static_cast<const double*>(dG);
        A.gm = diag ? N1 : N1 * N2; A.gi = diag ? 1 : N2; A.gj = diag ? 0 : 1;
        A.scratch = static_cast<double*>(scr);
        A.levels = nullptr;
        A.gbase = kgb;
        const unsigned gx_ = unsigned(s1 / 64);
        if (diag) {
            A.j0 = 0; A.nj = 1; A.pairs = s1;
            CHK(launch_seq(c, DP, dim3(gx_, 1), A));
        } else {
            for (int64_t j0 = 0; j0 < N2; j0 += chunk) {
                const int64_t nj = (N2 - j0 < chunk) ? N2 - j0 : chunk;
                A.j0 = int(j0); A.nj = int(nj); A.pairs = s1 * nj;
                CHK(launch_seq(c, DP, dim3(gx_, unsigned(nj)), A));
            }
        }
        CHK(from_timemajor(c, static_cast<const double*>(gxT), static_cast<double*>(dgX), N1, L1, d, DP, s1));
        if (!diag && !sym) CHK(from_timemajor(c, static_cast<const double*>(gyT), static_cast<double*>(dgY), N2, L2, d, DP, s2));
    }
    CHK(out_done(c, gX, dgX, xb));
    if (!diag && !sym) CHK(out_done(c, gY, dgY, yb));
    CHK(gbase_end(c, dgb, g_base));
    return finish(c);
}

int pad_rows(gpsig_ctx* c, const double* Z, double* ZP, int64_t rows, int d, int DP) {
    if (rows == 0) return GPSIG_OK;
    hipLaunchKernelGGL(grad_pad_rows_kernel, dim3(grid_for(rows * DP)), dim3(256), 0, c->stream, Z, ZP, rows, d, DP);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}
int unpad_rows(gpsig_ctx* c, const double* ZP, double* Z, int64_t rows, int d, int DP) {
    if (rows == 0) return GPSIG_OK;
    hipLaunchKernelGGL(grad_unpad_rows_kernel, dim3(grid_for(rows * d)), dim3(256), 0, c->stream, ZP, Z, rows, d, DP, 0);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

int pad_z(gpsig_ctx* c, bool collapse, const double* Z, double* ZP, int64_t rows, int d, int DP) {
    if (!collapse) return pad_rows(c, Z, ZP, rows, d, DP);
    if (rows == 0) return GPSIG_OK;
    hipLaunchKernelGGL(grad_pad_diff_rows_kernel, dim3(grid_for(rows * DP)), dim3(256), 0, c->stream, Z, ZP, rows, d, DP);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}
int unpad_z(gpsig_ctx* c, bool collapse, const double* ZP, double* Z, int64_t rows, int d, int DP) {
    if (!collapse) return unpad_rows(c, ZP, Z, rows, d, DP);
    if (rows == 0) return GPSIG_OK;
    hipLaunchKernelGGL(grad_unpad_pm_rows_kernel, dim3(grid_for(rows * d)), dim3(256), 0, c->stream, ZP, Z, rows, d, DP);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

}  // namespace

extern "C" {

int gpsig_seq_gram_levels_grad(gpsig_ctx* c, const gpsig_params* p, const void* X, const void* X2, int64_t N1, int64_t N2, int32_t L1,
                               int32_t L2, const void* G, void* gX, void* gX2, double* g_base) {
    if (!c) return GPSIG_ERR_INVALID;
    if (X2 && !gX2) return fail(c, GPSIG_ERR_INVALID, "gX2 is NULL");
    return seq_grad(c, p, X, X2, N1, N2, L1, L2, false, G, gX, gX2, g_base);
}

// The same gradient continued from what gpsig_seq_gram_levels_stash kept of the forward recursion (desc: the descriptor it returned): the fused
// reverse kernel's backward sweep only.  *taken == 0: the stash is gone (another evaluation has overwritten it) or was never written -- nothing
// was computed, call gpsig_seq_gram_levels_grad.  Device pointers, float64.
int gpsig_seq_gram_levels_grad_stash(gpsig_ctx* c, const gpsig_params* p, const void* X, const void* X2, int64_t N1, int64_t N2, int32_t L1,
                                     int32_t L2, const void* G, void* gX, void* gX2, const int64_t* desc, int32_t* taken) {
    if (!c || !p || !desc || !taken) return GPSIG_ERR_INVALID;
    *taken = 0;
    if (X2 && !gX2) return fail(c, GPSIG_ERR_INVALID, "gX2 is NULL");
    if (c->ptr_mode != GPSIG_PTR_DEVICE || p->dtype != GPSIG_F64 || c->grad_impl != 0) return GPSIG_OK;
    int d, DP;
    CHK(grad_check(c, p, &d, &DP));
    if (lattice_mode(p) != MODE_PT_DIFF || p->order > 1 || DP > 8 || N1 <= 0 || (X2 && N2 <= 0)) return GPSIG_OK;      // (the base kernel: by the lookup)
    HIPCHK(c, hipSetDevice(c->device));
    const bool sym = X2 == nullptr;
    bool done = false;
    CHK(seq_grad_fused_stash(c, p, DP, static_cast<const double*>(X), static_cast<const double*>(sym ? X : X2), N1, sym ? N1 : N2, L1, sym ? L1 : L2, d,
                             sym, static_cast<const double*>(G), static_cast<double*>(gX), static_cast<double*>(sym ? gX : gX2), desc, &done));
    *taken = done ? 1 : 0;
    return GPSIG_OK;
}

int gpsig_seq_diag_levels_grad(gpsig_ctx* c, const gpsig_params* p, const void* X, int64_t N, int32_t L, const void* G, void* gX,
                               double* g_base) {
    if (!c) return GPSIG_ERR_INVALID;
    return seq_grad(c, p, X, nullptr, N, N, L, L, true, G, gX, nullptr, g_base);
}

int gpsig_tens_gram_levels_grad(gpsig_ctx* c, const gpsig_params* p, const void* Z, int64_t T, int32_t increments, const void* G, void* gZ,
                                double* g_base) {
    int d, DP;
    CHK(grad_check(c, p, &d, &DP, 4096));
    if (T < 0 || T > 65535) return fail(c, GPSIG_ERR_INVALID, "bad number of tensors");
    const bool wide = T > 0 && wide_tens_available(c, p, T) && (c->wide == 1 || d > wide_auto_cols(p, 12));      // wide_api.hip
    if (DP == 0 && !wide) return fail(c, GPSIG_ERR_UNSUPPORTED, "gradients are built for at most 64 feature columns here (got %d)", d);
    const int M = p->num_levels, lt = M * (M + 1) / 2, E = increments ? 2 : 1;
    const int64_t rows = int64_t(lt) * T * E;
    const size_t zb = sizeof(double) * size_t(rows) * d, gb = sizeof(double) * size_t(M + 1) * T * T;
    const void *dZ, *dG;
    CHK(in_dev(c, B_IN0, Z, zb, &dZ));
    CHK(in_dev(c, B_IN2, G, gb, &dG));
    void* dgZ;
    CHK(out_dev(c, B_OUT0, gZ, zb, &dgZ));
    double* dgb;
    CHK(gbase_begin(c, &dgb));
    // kernels without a differentiable base parameter skip the accumulation (one same-address atomic per wavefront otherwise)
    double* const kgb = (p->base_kernel == GPSIG_BASE_POLY || p->base_kernel == GPSIG_BASE_MIX) ? dgb : nullptr;
    if (wide) {
        CHK(wide_tens_backward(c, p, d, static_cast<const double*>(dZ), T, increments, static_cast<const double*>(dG), static_cast<double*>(dgZ), kgb));
    } else if (T > 0) {
        void *zp, *gzp;
        CHK(ensure(c, B_GR0, sizeof(double) * size_t(rows) * DP, &zp));
        CHK(ensure(c, B_GR1, sizeof(double) * size_t(rows) * DP, &gzp));
        CHK(pad_rows(c, static_cast<const double*>(dZ), static_cast<double*>(zp), rows, d, DP));
        CHK(zero_async(c, gzp, sizeof(double) * size_t(rows) * DP));
        TensGradArgs A;
        memset(&A, 0, sizeof(A));
        A.z = static_cast<const double*>(zp); A.gz = static_cast<double*>(gzp);
        A.T = int(T); A.M = M; A.kind = p->base_kernel; A.incr = increments ? 1 : 0;
        A.p0 = p->base_params[0]; A.p1 = p->base_params[1];
        A.G = static_cast<const double*>(dG); A.gm = T * T; A.gt = T; A.gn = 1;
        A.gbase = kgb;
        if (c->grad_impl == 0) {
            const int64_t tb = (T + 63) / 64;
            int64_t slices = (1024 + tb - 1) / tb;
            if (slices > T) slices = T;
            void* part;
            A.part_stride = rows * DP;
            CHK(ensure(c, B_GR4, sizeof(double) * size_t(slices) * size_t(A.part_stride) + 64, &part));
            A.part = static_cast<double*>(part);
            CHK(launch_tens_row(c, DP, E, dim3(unsigned(tb), unsigned(slices), unsigned(M * (M + 1) / 2)), A));
            hipLaunchKernelGGL(tens_row_reduce_kernel, dim3(unsigned((A.part_stride + 255) / 256)), dim3(256), 0, c->stream, A.part,
                               static_cast<double*>(gzp), int(slices), A.part_stride);
            HIPCHK(c, hipGetLastError());
        } else {
            CHK(launch_tens(c, DP, dim3(unsigned((T + 63) / 64), unsigned(T)), A));
        }
        CHK(unpad_rows(c, static_cast<const double*>(gzp), static_cast<double*>(dgZ), rows, d, DP));
    }
    CHK(out_done(c, gZ, dgZ, zb));
    CHK(gbase_end(c, dgb, g_base));
    return finish(c);
}

int gpsig_tens_vs_seq_levels_grad(gpsig_ctx* c, const gpsig_params* p, const void* Z, const void* X, int64_t T, int64_t N, int32_t L,
                                  int32_t increments, const void* G, void* gZ, void* gX, double* g_base) {
    int d, DP;
    CHK(grad_check(c, p, &d, &DP, 4096));
    // wide state spaces (wide_api.hip): beyond the tile kernel's 8 columns, or wherever built when the option says so
    // (higher orders: at any width -- the tile kernel's reverse pass is first-order, the older kernels go through scratch memory operation by operation)
    // (the dot-product families: beyond 32 columns, or by option; SignaturePoly, SignatureMix: beyond 64)
    const bool wide = wide_tvs_available(c, p, d, T, N, L) && ((wide_dot_kind(p->base_kernel) || wide_base_param_kind(p->base_kernel)) ? (c->wide == 1 || d > wide_auto_cols(p, 32)) :
                                                               (c->wide == 1 || d > 8 || (p->num_levels > 6 && c->wide != 0) ||      /* (7 / 8 levels: no reverse tile instance -- 100 ms at T = 512, N = 2,048 on the older kernels) */
                                                                (p->order > 1 && p->num_levels > 1 && c->wide != 0 && !tvs_grad_tile_ho_available(c, p, d, L, increments))));
    if (DP == 0 && !wide) return fail(c, GPSIG_ERR_UNSUPPORTED, "gradients are built for at most 64 feature columns here (got %d)", d);
    if (T < 0 || N < 0 || L < 1) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    if (N > 0x7fffffff || T > 0x7fffffff) return fail(c, GPSIG_ERR_UNSUPPORTED, "more than 2^31 items");
    const int M = p->num_levels, lt = M * (M + 1) / 2;
    const bool collapse = increments && p->base_kernel == GPSIG_BASE_LINEAR;      // <z1, x> - <z0, x> = <z1 - z0, x>
    const int E = (increments && !collapse) ? 2 : 1;
    const int64_t rows = int64_t(lt) * T * E;                                      // padded rows the kernels see
    const size_t zb = sizeof(double) * size_t(lt) * T * (increments ? 2 : 1) * d, xb = sizeof(double) * size_t(N) * L * d, gb = sizeof(double) * size_t(M + 1) * T * N;
    const void *dZ, *dX, *dG;
    CHK(in_dev(c, B_IN0, Z, zb, &dZ));
    CHK(in_dev(c, B_IN1, X, xb, &dX));
    CHK(in_dev(c, B_IN2, G, gb, &dG));
    void *dgZ, *dgX;
    CHK(out_dev(c, B_OUT0, gZ, zb, &dgZ));
    CHK(out_dev(c, B_OUT1, gX, xb, &dgX));
    double* dgb;
    CHK(gbase_begin(c, &dgb));
    // kernels without a differentiable base parameter skip the accumulation (one same-address atomic per wavefront otherwise)
    double* const kgb = (p->base_kernel == GPSIG_BASE_POLY || p->base_kernel == GPSIG_BASE_MIX) ? dgb : nullptr;
    bool tiled = false;
    if (wide) {
        CHK(wide_tvs_backward(c, p, d, static_cast<const double*>(dZ), static_cast<const double*>(dX), static_cast<const double*>(dG), T, N, L, increments,
                              nullptr, nullptr, static_cast<double*>(dgZ), static_cast<double*>(dgX), nullptr, kgb));
        tiled = true;
    }
    if (!tiled && T > 0 && N > 0 && c->grad_impl == 0 && c->tvs_grad_tile != 0)
        CHK(tvs_grad_tile_device(c, p, d, static_cast<const double*>(dZ), static_cast<const double*>(dX), static_cast<const double*>(dG), T, N, L,
                                 increments, nullptr, nullptr, static_cast<double*>(dgZ), static_cast<double*>(dgX), nullptr, kgb, scratch_budget(c), &tiled));
    if (tiled) {
        // both gradients were written by the tile kernel's reductions
    } else if (T == 0 || N == 0) {
        if (zb) CHK(zero_async(c, dgZ, zb));
        if (xb) CHK(zero_async(c, dgX, xb));
    } else if (c->grad_impl == 0 && !(p->order > 1 && M > 1) && tvs_lanet_available(c, DP, M, L)) {
        void *zp, *gzp;
        CHK(ensure(c, B_GR0, sizeof(double) * size_t(rows) * DP, &zp));
        CHK(ensure(c, B_GR1, sizeof(double) * size_t(rows) * DP, &gzp));
        CHK(pad_z(c, collapse, static_cast<const double*>(dZ), static_cast<double*>(zp), rows, d, DP));
        CHK(zero_async(c, gzp, sizeof(double) * size_t(rows) * DP));
        CHK(zero_async(c, dgX, xb));
        TvsLaneTGradArgs A;
        memset(&A, 0, sizeof(A));
        A.z = static_cast<const double*>(zp); A.gz = static_cast<double*>(gzp);
        A.X = static_cast<const double*>(dX); A.gX = static_cast<double*>(dgX);
        A.T = int(T); A.N = int(N); A.L = L; A.d = d; A.M = M; A.kind = p->base_kernel; A.diff = p->difference ? 1 : 0;
        A.p0 = p->base_params[0]; A.p1 = p->base_params[1];
        A.G = static_cast<const double*>(dG); A.gm = T * N; A.gt = N; A.gn = 1;
        A.gbase = kgb;
        const int tpw = E == 2 ? 32 : 64;              // tensors per wavefront
        const int64_t tb = (T + tpw - 1) / tpw;
        int64_t runs = (2048 + tb - 1) / tb;
        if (runs > N) runs = N;
        if (runs > 65535) runs = 65535;
        A.nrun = int((N + runs - 1) / runs);
        runs = (N + A.nrun - 1) / A.nrun;
        // few workgroups: the serial sweep of one (tensor, sequence, level) chain bounds the launch -- one level per workgroup
        const unsigned zl = tb * runs < 1024 ? unsigned(M) : 1u;
        CHK(launch_tvs_lanet(c, DP, E == 2, dim3(unsigned(tb), unsigned(runs), zl), A));
        CHK(unpad_z(c, collapse, static_cast<const double*>(gzp), static_cast<double*>(dgZ), rows, d, DP));
    } else {
        const int64_t s = pad64(N);
        void *zp, *gzp, *xT, *gxT, *scr = nullptr;
        const size_t xtb = sizeof(double) * size_t(L) * DP * s;
        CHK(ensure(c, B_GR0, sizeof(double) * size_t(rows) * DP, &zp));
        CHK(ensure(c, B_GR1, sizeof(double) * size_t(rows) * DP, &gzp));
        CHK(ensure(c, B_GR2, xtb, &xT));
        CHK(ensure(c, B_GR3, xtb, &gxT));
        CHK(pad_z(c, collapse, static_cast<const double*>(dZ), static_cast<double*>(zp), rows, d, DP));
        CHK(to_timemajor(c, static_cast<const double*>(dX), static_cast<double*>(xT), N, L, d, DP, s));
        CHK(zero_async(c, gzp, sizeof(double) * size_t(rows) * DP));
        CHK(zero_async(c, gxT, xtb));
        const int R = p->difference ? L - 1 : L;
        const bool ho = p->order > 1 && M > 1;        // higher-order chains (signature_algs.py:129-160): one pair per thread with scratch
        const bool fused = !ho && c->grad_impl != 1 && tvs_fused_available(DP, M, E);     // grad_impl 2: one pair per thread, scratch-free
        const size_t nslots = ho ? size_t(TvsPairGrad<4>::ho_slots(M, p->order)) : size_t(lt + M * (M - 1) / 2);
        const size_t per_t = sizeof(double) * nslots * size_t(R > 0 ? R : 0) * size_t(s);
        int64_t chunk = int64_t(scratch_budget(c) / (per_t ? per_t : 1));
        if (chunk < 1) chunk = 1;
        if (chunk > T) chunk = T;
        if (chunk > 65535) chunk = 65535;
        if (!fused) CHK(ensure(c, B_GR4, per_t * size_t(chunk) + 64, &scr));
        TvsGradArgs A;
        memset(&A, 0, sizeof(A));
        A.z = static_cast<const double*>(zp); A.gz = static_cast<double*>(gzp);
        A.xT = static_cast<const double*>(xT); A.gxT = static_cast<double*>(gxT);
        A.xstride = s;
        A.T = int(T); A.N = int(N); A.L = L; A.M = M; A.kind = p->base_kernel; A.incr = E == 2 ? 1 : 0; A.diff = p->difference ? 1 : 0;
        A.order = ho ? p->order : 1;
        A.p0 = p->base_params[0]; A.p1 = p->base_params[1];
        A.G = static_cast<const double*>(dG); A.gm = T * N; A.gt = N; A.gn = 1;
        A.gbase = kgb;
        if (fused) {
            if (T > 65535) return fail(c, GPSIG_ERR_UNSUPPORTED, "more than 65535 inducing tensors");
            CHK(launch_tvs_fused(c, DP, E, dim3(unsigned(s / 64), unsigned(T)), A));
        } else {
            A.scratch = static_cast<double*>(scr);
            for (int64_t t0 = 0; t0 < T; t0 += chunk) {
                const int64_t nt = (T - t0 < chunk) ? T - t0 : chunk;
                A.t0 = int(t0); A.nt = int(nt); A.pairs = s * nt;
                CHK(launch_tvs(c, DP, dim3(unsigned(s / 64), unsigned(nt)), A));
            }
        }
        CHK(unpad_z(c, collapse, static_cast<const double*>(gzp), static_cast<double*>(dgZ), rows, d, DP));
        CHK(from_timemajor(c, static_cast<const double*>(gxT), static_cast<double*>(dgX), N, L, d, DP, s));
    }
    CHK(out_done(c, gZ, dgZ, zb));
    CHK(out_done(c, gX, dgX, xb));
    CHK(gbase_end(c, dgb, g_base));
    return finish(c);
}

}  // extern "C"

// ---- the recursions on GIVEN base-kernel lattices ("matrix route") ------------------------------------------------------------
// For state spaces wider than the gradient kernels' 64 columns, and for base kernels the kernels do not differentiate
// (SignatureSpectral: alpha, omega, gamma are trainable, gpsig/kernels.py:912-914), the caller builds the base-kernel tensor itself --
// a d-deep contraction: a library GEMM -- and differentiates it itself; what is left for this library is what the reference's
// signature_algs.py does AFTER its lines :25-26 / :114: the recursion on the increment lattices, any order, and its reverse pass.
// The lattices of a block of pairs live in scratch memory ((pairs, R1, R2) arrays, one pass over HBM per elementary operation, as in
// seq_grad_ho above): a path for minibatch-sized problems, not for BASELINE-sized Grams.
namespace {

// levels (forward == true: out (M+1, P)) or dL/ddM (forward == false: G (M+1, P) in, gdM (P, R1, R2) out) of dM (P, R1, R2)
int lattice_pass(gpsig_ctx* c, const gpsig_params* p, const double* dM, int64_t Ptot, int R1, int R2, bool forward, const double* Gup, double* out) {
    const int M = p->num_levels, D = p->order;
    const size_t cells = size_t(R1) * R2;
    if (forward) {
        hipLaunchKernelGGL(fill_pairs_kernel, dim3(grid_for(Ptot)), dim3(256), 0, c->stream, out, Ptot, 1.0);      // level 0 == 1
        HIPCHK(c, hipGetLastError());
    }
    if (Ptot == 0) return GPSIG_OK;
    if (cells == 0) {
        if (forward) CHK(zero_async(c, out + Ptot, sizeof(double) * size_t(M) * Ptot));
        return GPSIG_OK;
    }
    auto dm_of = [&](int m) { return m < D ? m : D; };
    // scratch slots (slot 0 = the caller's dM, the last one = the caller's gdM): R_m[r][s] for m = 2 .. M-1 (backward) or two
    // alternating grids (forward) | two grids of adjoints | two temporaries
    std::vector<int> roff(M + 2, 0);
    int nslots = 1;
    if (forward) {
        roff[0] = nslots; nslots += D * D;              // grid of the previous level
        roff[1] = nslots; nslots += D * D;              // grid being built
    } else {
        for (int m = 2; m <= M - 1; ++m) { roff[m] = nslots; nslots += dm_of(m) * dm_of(m); }
    }
    const int u0 = nslots, u1 = u0 + (forward ? 0 : D * D), t0 = u1 + (forward ? 0 : D * D), t1 = t0 + 1;
    nslots = t1 + 1;
    const size_t per_pair = sizeof(double) * cells * size_t(nslots - 1);
    int64_t chunk = int64_t(scratch_budget(c) / (per_pair ? per_pair : 1));
    if (chunk < 1) chunk = 1;
    if (chunk > Ptot) chunk = Ptot;
    void* scr;
    CHK(ensure(c, B_GR5, per_pair * size_t(chunk) + 64, &scr));
    for (int64_t p0 = 0; p0 < Ptot; p0 += chunk) {
        const int64_t npairs = Ptot - p0 < chunk ? Ptot - p0 : chunk, P = npairs * int64_t(cells);
        const double* const dm = dM + p0 * int64_t(cells);
        double* const base = static_cast<double*>(scr);
        double* const lam = forward ? nullptr : out + p0 * int64_t(cells);
        auto slot = [&](int k) -> double* { return k == 0 ? const_cast<double*>(dm) : base + int64_t(k - 1) * P; };
        const HoBlock B{p0, npairs, p0, 1, 1};
        auto mul = [&](const double* A_, const double* B_, double* dst, double scale, int acc) {
            hipLaunchKernelGGL(ho_mul_kernel, dim3(grid_for(P)), dim3(256), 0, c->stream, A_, B_, dst, P, scale, acc);
        };
        auto cum = [&](const double* src, double* dst, int axis, int reverse) {
            hipLaunchKernelGGL(ho_cumsum_kernel, dim3(grid_for(npairs * (axis == 0 ? R2 : R1), 64)), dim3(64), 0, c->stream, src, dst, npairs, R1,
                               R2, axis, reverse, 1.0, 0);
        };
        auto pairsum = [&](const double* src, int m, int acc) {
            hipLaunchKernelGGL(ho_pairsum_kernel, dim3(unsigned(npairs < 65535 ? npairs : 65535)), dim3(64), 0, c->stream, src, npairs, int64_t(cells),
                               out + int64_t(m) * Ptot + p0, acc);
        };
        if (forward) {
            // grids alternate between two sets: prev (level m-1), cur (level m); level 1's grid is dM itself
            int prev = roff[0], cur = roff[1];
            auto G1 = [&](int set, int m, int r, int s) -> double* { return m == 1 ? slot(0) : slot(set + r * D + s); };
            pairsum(slot(0), 1, 0);                                                                             // signature_algs.py:28 / :58
            for (int m = 2; m <= M; ++m) {
                const int dc = dm_of(m), dp = dm_of(m - 1);
                auto Rp = [&](int r, int s) { return G1(prev, m - 1, r, s); };
                auto sum_all = [&]() { for (int r = 0; r < dp; ++r) for (int s2 = 0; s2 < dp; ++s2) mul(Rp(r, s2), nullptr, slot(t0), 1.0, r + s2 > 0); };
                auto sum_col = [&](int j2) { for (int r = 0; r < dp; ++r) mul(Rp(r, j2), nullptr, slot(t0), 1.0, r > 0); };
                auto sum_row = [&](int j2) { for (int s2 = 0; s2 < dp; ++s2) mul(Rp(j2, s2), nullptr, slot(t0), 1.0, s2 > 0); };
                sum_all(); cum(slot(t0), slot(t1), 0, 0); cum(slot(t1), slot(t0), 1, 0);
                mul(slot(0), slot(t0), slot(cur), 1.0, 0);                                                      // :32 / :64
                for (int j = 2; j <= dc; ++j) {
                    sum_col(j - 2); cum(slot(t0), slot(t1), 0, 0);
                    mul(slot(0), slot(t1), slot(cur + j - 1), 1.0 / j, 0);                                      // :66
                    sum_row(j - 2); cum(slot(t0), slot(t1), 1, 0);
                    mul(slot(0), slot(t1), slot(cur + (j - 1) * D), 1.0 / j, 0);                                // :67
                    for (int k = 2; k <= dc; ++k) mul(slot(0), Rp(j - 2, k - 2), slot(cur + (j - 1) * D + k - 1), 1.0 / (double(j) * k), 0);   // :69
                }
                for (int r = 0; r < dc; ++r)
                    for (int s2 = 0; s2 < dc; ++s2) pairsum(slot(cur + r * D + s2), m, r + s2 > 0);             // :33 / :71
                std::swap(prev, cur);
            }
            HIPCHK(c, hipGetLastError());
            continue;
        }
        auto Rm = [&](int m, int r, int s2) { return m == 1 ? slot(0) : slot(roff[m] + r * dm_of(m) + s2); };
        auto bcast = [&](int m, double* dst, int acc) {
            hipLaunchKernelGGL(ho_bcast_kernel, dim3(grid_for(P)), dim3(256), 0, c->stream, Gup, int64_t(m) * Ptot, int64_t(1), int64_t(0), B, int64_t(cells),
                               dst, acc);
        };
        auto sum_all = [&](int m) { const int dp = dm_of(m); for (int r = 0; r < dp; ++r) for (int s2 = 0; s2 < dp; ++s2) mul(Rm(m, r, s2), nullptr, slot(t0), 1.0, r + s2 > 0); };
        auto sum_col = [&](int m, int j2) { const int dp = dm_of(m); for (int r = 0; r < dp; ++r) mul(Rm(m, r, j2), nullptr, slot(t0), 1.0, r > 0); };
        auto sum_row = [&](int m, int j2) { const int dp = dm_of(m); for (int s2 = 0; s2 < dp; ++s2) mul(Rm(m, j2, s2), nullptr, slot(t0), 1.0, s2 > 0); };
        for (int m = 2; m <= M - 1; ++m) {                                                                      // forward grids, as seq_grad_ho
            const int dc = dm_of(m);
            sum_all(m - 1); cum(slot(t0), slot(t1), 0, 0); cum(slot(t1), slot(t0), 1, 0);
            mul(slot(0), slot(t0), Rm(m, 0, 0), 1.0, 0);
            for (int j = 2; j <= dc; ++j) {
                sum_col(m - 1, j - 2); cum(slot(t0), slot(t1), 0, 0);
                mul(slot(0), slot(t1), Rm(m, 0, j - 1), 1.0 / j, 0);
                sum_row(m - 1, j - 2); cum(slot(t0), slot(t1), 1, 0);
                mul(slot(0), slot(t1), Rm(m, j - 1, 0), 1.0 / j, 0);
                for (int k = 2; k <= dc; ++k) mul(slot(0), Rm(m - 1, j - 2, k - 2), Rm(m, j - 1, k - 1), 1.0 / (double(j) * k), 0);
            }
        }
        int ucur = u0, unext = u1;
        auto U = [&](int set, int r, int s2) { return slot(set + r * D + s2); };
        for (int r = 0; r < dm_of(M); ++r) for (int s2 = 0; s2 < dm_of(M); ++s2) bcast(M, U(ucur, r, s2), 0);
        CHK(zero_async(c, lam, sizeof(double) * size_t(P)));
        for (int m = M; m >= 2; --m) {
            const int dc = dm_of(m), dp = dm_of(m - 1);
            sum_all(m - 1); cum(slot(t0), slot(t1), 0, 0); cum(slot(t1), slot(t0), 1, 0);
            mul(U(ucur, 0, 0), slot(t0), lam, 1.0, 1);
            for (int j = 2; j <= dc; ++j) {
                sum_col(m - 1, j - 2); cum(slot(t0), slot(t1), 0, 0);
                mul(U(ucur, 0, j - 1), slot(t1), lam, 1.0 / j, 1);
                sum_row(m - 1, j - 2); cum(slot(t0), slot(t1), 1, 0);
                mul(U(ucur, j - 1, 0), slot(t1), lam, 1.0 / j, 1);
                for (int k = 2; k <= dc; ++k) mul(U(ucur, j - 1, k - 1), Rm(m - 1, j - 2, k - 2), lam, 1.0 / (double(j) * k), 1);
            }
            mul(slot(0), U(ucur, 0, 0), slot(t0), 1.0, 0); cum(slot(t0), slot(t1), 0, 1); cum(slot(t1), slot(t0), 1, 1);
            for (int r = 0; r < dp; ++r)
                for (int s2 = 0; s2 < dp; ++s2) { bcast(m - 1, U(unext, r, s2), 0); mul(slot(t0), nullptr, U(unext, r, s2), 1.0, 1); }
            for (int j = 2; j <= dc; ++j) {
                mul(slot(0), U(ucur, 0, j - 1), slot(t0), 1.0 / j, 0); cum(slot(t0), slot(t1), 0, 1);
                for (int r = 0; r < dp; ++r) mul(slot(t1), nullptr, U(unext, r, j - 2), 1.0, 1);
                mul(slot(0), U(ucur, j - 1, 0), slot(t0), 1.0 / j, 0); cum(slot(t0), slot(t1), 1, 1);
                for (int s2 = 0; s2 < dp; ++s2) mul(slot(t1), nullptr, U(unext, j - 2, s2), 1.0, 1);
                for (int k = 2; k <= dc; ++k) mul(slot(0), U(ucur, j - 1, k - 1), U(unext, j - 2, k - 2), 1.0 / (double(j) * k), 1);
            }
            std::swap(ucur, unext);
        }
        mul(U(ucur, 0, 0), nullptr, lam, 1.0, 1);                                                               // level 1: R_1 = dM
        HIPCHK(c, hipGetLastError());
    }
    return GPSIG_OK;
}

int lattice_check(gpsig_ctx* c, const gpsig_params* p) {
    if (!c) return GPSIG_ERR_INVALID;
    if (!p) return fail(c, GPSIG_ERR_INVALID, "params is NULL");
    if (p->dtype != GPSIG_F64) return fail(c, GPSIG_ERR_UNSUPPORTED, "the lattice primitives are built for float64 only");
    if (p->num_levels < 1 || p->num_levels > GRAD_MAX_LEVELS) return fail(c, GPSIG_ERR_UNSUPPORTED, "num_levels outside [1, %d]", GRAD_MAX_LEVELS);
    if (p->order < 1 || p->order > p->num_levels) return fail(c, GPSIG_ERR_INVALID, "order=%d outside [1, num_levels]", p->order);
    HIPCHK(c, hipSetDevice(c->device));
    return GPSIG_OK;
}

}  // namespace

extern "C" {

int gpsig_lattice_levels(gpsig_ctx* c, const gpsig_params* p, const void* dM, int64_t P, int32_t R1, int32_t R2, void* out) {
    CHK(lattice_check(c, p));
    if (P < 0 || R1 < 0 || R2 < 0) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    const size_t mb = sizeof(double) * size_t(P) * R1 * R2, ob = sizeof(double) * size_t(p->num_levels + 1) * P;
    const void* dm;
    CHK(in_dev(c, B_IN0, dM, mb, &dm));
    void* dout;
    CHK(out_dev(c, B_OUT0, out, ob, &dout));
    CHK(lattice_pass(c, p, static_cast<const double*>(dm), P, R1, R2, true, nullptr, static_cast<double*>(dout)));
    CHK(out_done(c, out, dout, ob));
    return finish(c);
}

int gpsig_lattice_levels_grad(gpsig_ctx* c, const gpsig_params* p, const void* dM, int64_t P, int32_t R1, int32_t R2, const void* G, void* gdM) {
    CHK(lattice_check(c, p));
    if (P < 0 || R1 < 0 || R2 < 0) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    const size_t mb = sizeof(double) * size_t(P) * R1 * R2, gb = sizeof(double) * size_t(p->num_levels + 1) * P;
    const void *dm, *dG;
    CHK(in_dev(c, B_IN0, dM, mb, &dm));
    CHK(in_dev(c, B_IN2, G, gb, &dG));
    void* dg;
    CHK(out_dev(c, B_OUT0, gdM, mb, &dg));
    CHK(lattice_pass(c, p, static_cast<const double*>(dm), P, R1, R2, false, static_cast<const double*>(dG), static_cast<double*>(dg)));
    CHK(out_done(c, gdM, dg, mb));
    return finish(c);
}

int gpsig_chain_levels(gpsig_ctx* c, const gpsig_params* p, const void* m, int64_t P, int32_t R, void* out) {
    CHK(lattice_check(c, p));
    if (p->order > 1 && p->num_levels > 1) return fail(c, GPSIG_ERR_UNSUPPORTED, "the chain primitives are built for order 1");
    if (P < 0 || R < 0) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    const int M = p->num_levels, lt = M * (M + 1) / 2;
    const size_t mb = sizeof(double) * size_t(lt) * R * P, ob = sizeof(double) * size_t(M + 1) * P;
    const void* dm;
    CHK(in_dev(c, B_IN0, m, mb, &dm));
    void* dout;
    CHK(out_dev(c, B_OUT0, out, ob, &dout));
    if (P > 0) {
        hipLaunchKernelGGL(chain_levels_kernel, dim3(grid_for(P, 64)), dim3(64), 0, c->stream, static_cast<const double*>(dm), M, int64_t(R), P,
                           static_cast<double*>(dout));
        HIPCHK(c, hipGetLastError());
    }
    CHK(out_done(c, out, dout, ob));
    return finish(c);
}

int gpsig_chain_levels_grad(gpsig_ctx* c, const gpsig_params* p, const void* m, int64_t P, int32_t R, const void* G, void* gm) {
    CHK(lattice_check(c, p));
    if (p->order > 1 && p->num_levels > 1) return fail(c, GPSIG_ERR_UNSUPPORTED, "the chain primitives are built for order 1");
    if (P < 0 || R < 0) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    const int M = p->num_levels, lt = M * (M + 1) / 2;
    const size_t mb = sizeof(double) * size_t(lt) * R * P, gb = sizeof(double) * size_t(M + 1) * P;
    const void *dm, *dG;
    CHK(in_dev(c, B_IN0, m, mb, &dm));
    CHK(in_dev(c, B_IN2, G, gb, &dG));
    void* dg;
    CHK(out_dev(c, B_OUT0, gm, mb, &dg));
    if (P > 0 && R > 0) {
        hipLaunchKernelGGL(chain_levels_grad_kernel, dim3(grid_for(P, 64)), dim3(64), 0, c->stream, static_cast<const double*>(dm),
                           static_cast<const double*>(dG), M, int64_t(R), P, static_cast<double*>(dg));
        HIPCHK(c, hipGetLastError());
    }
    CHK(out_done(c, gm, dg, mb));
    return finish(c);
}

}  // extern "C"

extern "C" {

// The weighted level sum of gpsig_tens_vs_seq_weighted: gradients with respect to Z, X and the factors.  The tile kernel takes the
// (T, N) upstream gradient and the factors as they are; other shapes go through the level primitives (the level array and its
// upstream gradient in scratch memory).
int gpsig_tens_vs_seq_weighted_grad(gpsig_ctx* c, const gpsig_params* p, const void* Z, const void* X, int64_t T, int64_t N, int32_t L,
                                    int32_t increments, const void* fac, const void* G, const void* aux, void* gZ, void* gX, void* gfac, double* g_base) {
    int d, DP;
    CHK(grad_check(c, p, &d, &DP, 4096));
    // (higher orders: at any width -- the tile kernel's reverse pass is first-order, the older kernels go through scratch memory operation by operation)
    // (the dot-product families: beyond 32 columns, or by option; SignaturePoly, SignatureMix: beyond 64)
    const bool wide = wide_tvs_available(c, p, d, T, N, L) && ((wide_dot_kind(p->base_kernel) || wide_base_param_kind(p->base_kernel)) ? (c->wide == 1 || d > wide_auto_cols(p, 32)) :
                                                               (c->wide == 1 || d > 8 || (p->num_levels > 6 && c->wide != 0) ||      /* (7 / 8 levels: no reverse tile instance -- 100 ms at T = 512, N = 2,048 on the older kernels) */
                                                                (p->order > 1 && p->num_levels > 1 && c->wide != 0 && !tvs_grad_tile_ho_available(c, p, d, L, increments))));
    if (DP == 0 && !wide) return fail(c, GPSIG_ERR_UNSUPPORTED, "gradients are built for at most 64 feature columns here (got %d)", d);
    if (T < 0 || N < 0 || L < 1) return fail(c, GPSIG_ERR_INVALID, "bad sizes");
    if (N > 0x7fffffff || T > 0x7fffffff) return fail(c, GPSIG_ERR_UNSUPPORTED, "more than 2^31 items");
    const int M = p->num_levels, M1 = M + 1, lt = M * (M + 1) / 2;
    const size_t zb = sizeof(double) * size_t(lt) * T * (increments ? 2 : 1) * d, xb = sizeof(double) * size_t(N) * L * d;
    const size_t gb = sizeof(double) * size_t(T) * N, fb = sizeof(double) * size_t(N) * M1;
    const void *dZ, *dX, *dG, *dF;
    CHK(in_dev(c, B_IN0, Z, zb, &dZ));
    CHK(in_dev(c, B_IN1, X, xb, &dX));
    CHK(in_dev(c, B_IN2, G, gb, &dG));
    CHK(in_dev(c, B_TW2, fac, fb, &dF));
    void *dgZ, *dgX, *dgF;
    CHK(out_dev(c, B_OUT0, gZ, zb, &dgZ));
    CHK(out_dev(c, B_OUT1, gX, xb, &dgX));
    CHK(out_dev(c, B_OUT2, gfac, fb, &dgF));
    const bool has_base = p->base_kernel == GPSIG_BASE_POLY || p->base_kernel == GPSIG_BASE_MIX;
    bool tiled = false;
    if (wide) {
        double* dgb = nullptr;
        if (has_base) CHK(gbase_begin(c, &dgb));
        CHK(wide_tvs_backward(c, p, d, static_cast<const double*>(dZ), static_cast<const double*>(dX), static_cast<const double*>(dG), T, N, L, increments,
                              static_cast<const double*>(dF), c->ptr_mode == GPSIG_PTR_DEVICE ? static_cast<const double*>(aux) : nullptr,
                              static_cast<double*>(dgZ), static_cast<double*>(dgX), static_cast<double*>(dgF), dgb));
        if (has_base) CHK(gbase_end(c, dgb, g_base));
        else if (g_base && c->ptr_mode == GPSIG_PTR_HOST) g_base[0] = g_base[1] = 0.0;              // (no base parameter: zeros, as before)
        else if (g_base) CHK(zero_async(c, g_base, 2 * sizeof(double)));
        tiled = true;
    }
    if (!tiled && T > 0 && N > 0 && c->grad_impl == 0 && c->tvs_grad_tile != 0) {
        double* dgb;
        CHK(gbase_begin(c, &dgb));
        CHK(tvs_grad_tile_device(c, p, d, static_cast<const double*>(dZ), static_cast<const double*>(dX), static_cast<const double*>(dG), T, N, L,
                                 increments, static_cast<const double*>(dF), static_cast<const double*>(aux), static_cast<double*>(dgZ), static_cast<double*>(dgX),
                                 static_cast<double*>(dgF), has_base ? dgb : nullptr, scratch_budget(c), &tiled));
        if (tiled) CHK(gbase_end(c, dgb, g_base));
    }
    if (!tiled) {
        if (T == 0 || N == 0) {
            if (zb) CHK(zero_async(c, dgZ, zb));
            if (xb) CHK(zero_async(c, dgX, xb));
            if (fb) CHK(zero_async(c, dgF, fb));
            if (g_base && c->ptr_mode == GPSIG_PTR_HOST) g_base[0] = g_base[1] = 0.0;
            else if (g_base) CHK(zero_async(c, g_base, 2 * sizeof(double)));
        } else {
            void *lev, *glev, *tgb;
            CHK(ensure(c, B_TW0, sizeof(double) * size_t(M1) * T * N + 8, &lev));
            CHK(ensure(c, B_TW1, sizeof(double) * size_t(M1) * T * N + 8, &glev));
            CHK(ensure(c, B_GR7B, 2 * sizeof(double), &tgb));
            const int mode = c->ptr_mode;
            c->ptr_mode = GPSIG_PTR_DEVICE;                  // the operands are on the device by now
            int rc = gpsig_tens_vs_seq_levels(c, p, dZ, dX, T, N, L, increments, lev);
            if (rc == GPSIG_OK) {
                hipLaunchKernelGGL(weighted_upstream_levels_kernel, dim3(grid_for(int64_t(M1) * T * N)), dim3(256), 0, c->stream,
                                   static_cast<const double*>(dG), static_cast<const double*>(dF), M1, T, N, static_cast<double*>(glev));
                hipLaunchKernelGGL(weighted_gfac_kernel, dim3(grid_for(N * M1)), dim3(256), 0, c->stream, static_cast<const double*>(dG),
                                   static_cast<const double*>(lev), M1, T, N, static_cast<double*>(dgF));
                rc = gpsig_tens_vs_seq_levels_grad(c, p, dZ, dX, T, N, L, increments, glev, dgZ, dgX, static_cast<double*>(tgb));
            }
            c->ptr_mode = mode;
            CHK(rc);
            HIPCHK(c, hipGetLastError());
            if (g_base) HIPCHK(c, hipMemcpyAsync(g_base, tgb, 2 * sizeof(double), mode == GPSIG_PTR_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
        }
    }
    CHK(out_done(c, gZ, dgZ, zb));
    CHK(out_done(c, gX, dgX, xb));
    CHK(out_done(c, gfac, dgF, fb));
    return finish(c);
}

}  // extern "C"
