// launchers.hpp -- everything that crosses a translation unit of the library, declared once.
//
// The library is many small instance units (each instantiates a few kernel templates and exports a lookup function that returns a host
// launch stub) and a handful of host units that call them.  Every unit that defines one of the functions below and every unit that calls one
// includes this file, so the compiler checks each definition against the one declaration.  Declarations only: the argument structs are
// forward-declared (the stubs take them by reference), so this file pulls in no kernel code and changes nothing a unit instantiates.
//
// Adding a sequence-Gram instance unit: write the unit file (seq_inst.hpp / seq_inst_ho.hpp) and add its name to GPSIG_SEQ_UNITS /
// GPSIG_SEQ_HO_UNITS below.  The Makefile compiles every *.hip of the directory.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

struct gpsig_ctx;
struct gpsig_params;

namespace gpsig {
struct ScaleParams;
struct SeqGramArgs;
struct TvsArgs;
struct TvsLaneTArgs;
struct TvsTileArgs;
struct TvsGradTileArgs;
struct SigFeatArgs;
struct SigGramArgs;
struct SigReduceArgs;
struct SigFeatGradArgs;
struct WaveGradArgs;
struct Wave2Args;
struct WaveHoArgs;
struct FusedGradArgs;

// ---- host launch stubs -----------------------------------------------------------------------------------------------------------
typedef hipError_t (*SeqLaunchFn)(const SeqGramArgs&, int, size_t, hipStream_t);
typedef hipError_t (*TvsLaunchFn)(const TvsArgs&, hipStream_t);
typedef hipError_t (*TvsLaneTLaunchFn)(const TvsLaneTArgs&, hipStream_t);
typedef hipError_t (*TvsTileLaunchFn)(TvsTileArgs&, size_t, hipStream_t, int);
typedef hipError_t (*TvsGradTileLaunchFn)(const TvsGradTileArgs&, dim3, size_t, hipStream_t);
typedef hipError_t (*SigFeatLaunchFn)(const SigFeatArgs&, unsigned, size_t, hipStream_t);
typedef hipError_t (*SigFeatGradLaunchFn)(const SigFeatGradArgs&, unsigned, size_t, hipStream_t);
typedef hipError_t (*WaveLaunchFn)(const WaveGradArgs&, int, hipStream_t);
typedef hipError_t (*Wave2LaunchFn)(const Wave2Args&, int, size_t, hipStream_t);
typedef hipError_t (*WaveHoLaunchFn)(const WaveHoArgs&, int, size_t, hipStream_t);
typedef hipError_t (*FusedGradLaunchFn)(const FusedGradArgs&, int, size_t, hipStream_t);

// ---- sequence-Gram instance units --------------------------------------------------------------------------------------------------
// A regular unit (seq_inst.hpp) describes itself: element type, lattice mode, the base kernel it has at compile time (-1: none) and its
// lookup (G, C, D, MMAX, exact).  A higher-order unit (seq_inst_ho.hpp): element type, mode, the one padded width D it serves and its
// lookup (G, C, D, MMAX, OMAX).  The launchers of api.hip walk the tables these lists produce, in this order.
struct SeqUnit {
    bool f32;
    int mode, kind;
    SeqLaunchFn (*lookup)(int, int, int, int, bool);
};
struct SeqHoUnit {
    bool f32;
    int mode, D;
    SeqLaunchFn (*lookup)(int, int, int, int, int);
};
#define GPSIG_SEQ_UNITS_EX(X, V) X(V##_ex_g16_d4) X(V##_ex_g16_d8) X(V##_ex_g16_d16) X(V##_ex_g64_d4) X(V##_ex_g64_d8) X(V##_ex_g64_d16)
#define GPSIG_SEQ_UNITS(X)                                                                  \
    X(inc_exact) GPSIG_SEQ_UNITS_EX(X, inc) X(inc_g16) X(inc_g64)                           \
    X(ptd_exact) GPSIG_SEQ_UNITS_EX(X, ptd) X(ptd_g16) X(ptd_g64)                           \
    X(ptdrbf_exact) GPSIG_SEQ_UNITS_EX(X, ptdrbf)                                           \
    X(ptdm12_exact) X(ptdm32_exact) X(ptdm52_exact)                                         \
    X(ptd_spectral_g16) X(ptd_spectral_g64)                                                 \
    X(ptn_g16) X(ptn_g64)                                                                   \
    X(f32_inc_exact) GPSIG_SEQ_UNITS_EX(X, f32_inc) X(f32_inc_g16) X(f32_inc_g64)           \
    X(f32_ptdrbf_exact) GPSIG_SEQ_UNITS_EX(X, f32_ptdrbf)                                   \
    X(f32_ptd_exact) GPSIG_SEQ_UNITS_EX(X, f32_ptd) X(f32_ptd_g16) X(f32_ptd_g64)           \
    X(f32_ptn_g16) X(f32_ptn_g64)
#define GPSIG_SEQ_HO_UNITS_D(X, V) X(ho_##V##_d4) X(ho_##V##_d8) X(ho_##V##_d16) X(ho_##V##_d32)
#define GPSIG_SEQ_HO_UNITS(X)                                                                               \
    GPSIG_SEQ_HO_UNITS_D(X, inc) GPSIG_SEQ_HO_UNITS_D(X, ptd) GPSIG_SEQ_HO_UNITS_D(X, ptn)                  \
    GPSIG_SEQ_HO_UNITS_D(X, f32_inc) GPSIG_SEQ_HO_UNITS_D(X, f32_ptd) GPSIG_SEQ_HO_UNITS_D(X, f32_ptn)
#define GPSIG_SEQ_UNIT_DECL(n) SeqLaunchFn seq_lookup_##n(int, int, int, int, bool); extern const SeqUnit seq_lookup_##n##_unit;
#define GPSIG_SEQ_HO_UNIT_DECL(n) SeqLaunchFn seq_lookup_##n(int, int, int, int, int); extern const SeqHoUnit seq_lookup_##n##_unit;
GPSIG_SEQ_UNITS(GPSIG_SEQ_UNIT_DECL)
GPSIG_SEQ_HO_UNITS(GPSIG_SEQ_HO_UNIT_DECL)
#undef GPSIG_SEQ_UNIT_DECL
#undef GPSIG_SEQ_HO_UNIT_DECL
// the units with lookups of their own
SeqLaunchFn seq_lookup_ptdrbf_stash(int G, int C, int D, int MMAX);                           // seq_inst_ptdrbf_stash.hip
SeqLaunchFn seq_lookup_ptdmatern_stash(int kind, int G, int C, int D, int MMAX);
SeqLaunchFn seq_lookup_ho_ptdrbf_exact(int G, int C, int D, int M, int order);
SeqLaunchFn seq_lookup_ho_ptdrbf_exact_o4(int G, int C, int D, int M, int order);
SeqLaunchFn seq_lookup_ho_ptdm12_exact(int kind, int G, int C, int D, int M, int order);      // seq_inst_ho_exact.hpp: null for any other kind
SeqLaunchFn seq_lookup_ho_ptdm32_exact(int kind, int G, int C, int D, int M, int order);
SeqLaunchFn seq_lookup_ho_ptdm52_exact(int kind, int G, int C, int D, int M, int order);
bool seq_pk2_select(int rows, int d, int M, int* G, int* C, int* D);                          // seq_pk2_inst.hip
SeqLaunchFn seq_pk2_lookup(int G, int C, int D, int M, int mode, int pack, int waves);

// ---- tensor-vs-sequence kernels ----------------------------------------------------------------------------------------------------
TvsLaunchFn tvs_lookup(int M, int TT, bool incr, bool f32);                                   // tens_inst.hip, over tens_inst_{f64,f32}_*.hip
#define GPSIG_TENS_DECL(tag) TvsLaunchFn tvs_lookup_##tag##_lo(int, int, bool); TvsLaunchFn tvs_lookup_##tag##_m6(int, int, bool); \
                             TvsLaunchFn tvs_lookup_##tag##_m7(int, int, bool); TvsLaunchFn tvs_lookup_##tag##_m8(int, int, bool);
GPSIG_TENS_DECL(f64) GPSIG_TENS_DECL(f32)
#undef GPSIG_TENS_DECL
bool tvs_lanet_plan(int M, int d, bool incr, TvsLaneTLaunchFn* fns, int* ngroups);            // tens_inst_lanet.hip
int tvs_tile_width(int d);                                                                    // tvs_tile_inst.hip, over tvs_tile_inst_m*.hip
int tvs_tile_waves(int M, int D, int E, int kind);
TvsTileLaunchFn tvs_tile_lookup(int M, int NW, int D, bool incr, int kind);
TvsTileLaunchFn tvs_tile_lookup_m2(int, int, bool, int);
TvsTileLaunchFn tvs_tile_lookup_m3(int, int, bool, int);
TvsTileLaunchFn tvs_tile_lookup_m4(int, int, bool, int);
TvsTileLaunchFn tvs_tile_lookup_m5(int, int, bool, int);
TvsTileLaunchFn tvs_tile_lookup_m6(int, int, bool, int);
TvsTileLaunchFn tvs_tile_lookup_ho(int M, int NW, int D, bool incr);                          // tvs_tile_inst_ho.hip
TvsGradTileLaunchFn tvs_grad_tile_lookup_m1(int, int, bool);                                  // tvs_grad_tile_inst_m*.hip
TvsGradTileLaunchFn tvs_grad_tile_lookup_m2(int, int, bool);
TvsGradTileLaunchFn tvs_grad_tile_lookup_m3(int, int, bool);
TvsGradTileLaunchFn tvs_grad_tile_lookup_m4(int, int, bool);
TvsGradTileLaunchFn tvs_grad_tile_lookup_m5(int, int, bool);
TvsGradTileLaunchFn tvs_grad_tile_lookup_m6(int, int, bool);
TvsGradTileLaunchFn tvs_grad_tile_lookup_ho(int M, int D, bool paired, int kind);             // tvs_grad_tile_inst_ho.hip: SignatureRBF and the Matern families, order > 1
// tvs_grad_api.hip: the tile kernel of the tensor-vs-sequence reverse pass (tvs_grad_tile_kernel.hpp)
bool tvs_grad_tile_ho_available(const gpsig_ctx* c, const gpsig_params* p, int d, int L, int increments);
int tvs_grad_tile_device(gpsig_ctx* c, const gpsig_params* p, int d, const double* Z, const double* X, const double* G, int64_t Tn, int64_t N,
                         int L, int increments, const double* fac, const double* aux, double* gZ, double* gX, double* gfac, double* gb, size_t budget, bool* done);

// ---- explicit level features (sig_feat_kernel.hpp, sig_feat_grad_kernel.hpp) -------------------------------------------------------
SigFeatLaunchFn sig_feat_lookup(int d, int M);                       // sig_feat_inst.hip, over sig_feat_inst_{a..f}.hip
SigFeatLaunchFn sig_feat_pick_a(int d, int M);                       // d = 1 .. 4
SigFeatLaunchFn sig_feat_pick_b(int d, int M);                       // d = 5 .. 8
SigFeatLaunchFn sig_feat_pick_c(int d, int M);                       // d = 9 .. 12
SigFeatLaunchFn sig_feat_pick_d(int d, int M);                       // d = 13 .. 16
SigFeatLaunchFn sig_feat_pick_e(int d, int M);                       // d = 17 .. 24
SigFeatLaunchFn sig_feat_pick_f(int d, int M);                       // d = 25 .. 32
SigFeatGradLaunchFn sig_feat_grad_pick_a(int d, int M);              // sig_feat_grad_inst_{a..f}.hip: the same ranges
SigFeatGradLaunchFn sig_feat_grad_pick_b(int d, int M);
SigFeatGradLaunchFn sig_feat_grad_pick_c(int d, int M);
SigFeatGradLaunchFn sig_feat_grad_pick_d(int d, int M);
SigFeatGradLaunchFn sig_feat_grad_pick_e(int d, int M);
SigFeatGradLaunchFn sig_feat_grad_pick_f(int d, int M);
hipError_t sig_gram_launch(const SigGramArgs& G, int ntiles, hipStream_t stream, int dma, int* used_dma, int* folded);
hipError_t sig_reduce_launch(const SigReduceArgs& R, hipStream_t stream);
hipError_t sig_convert_launch(const void* in, void* out, int64_t n, bool widen, hipStream_t stream);
// sig_feat_api.hip: the forward side of the feature route, and what it shares with the reverse side (sig_feat_grad_api.hip).
// What every site of the route asks first: the linear or cosine family and a feature kernel built for (d, M) -- sig_feat_lookup is null outside
// 1 <= d <= 32 and (sig_feat_pick.hpp: the switch's default) outside 2 <= M <= 8, so no site tests those ranges itself --, then the width
// F = sum_m d^m and the row stride ld of the feature matrix.  The order is each site's own business.
struct SigShape { int d, M; bool cosine; int64_t F, ld; SigFeatLaunchFn ffn; };
bool sig_shape(const gpsig_params* p, int d, SigShape* s);
constexpr size_t SIG_FEAT_LDS_MAX = 150 * 1024, SIG_FEAT_GRAD_LDS_MAX = 158 * 1024;       // the feature kernel's / the reverse kernel's arrays of one sequence
bool sig_shape_fits(const SigShape& s, const gpsig_params* p, int L);          // at least one step, and the feature kernel's arrays within SIG_FEAT_LDS_MAX
// the one launch of sig_features_kernel: N sequences X into Phi (N, s.ld); every SigFeatArgs field that the sites set differently is an argument
int sig_launch_features(gpsig_ctx* c, const SigShape& s, const gpsig_params* p, const ScaleParams& P, int order, const double* X, int64_t N, int L,
                        const double* w, int normalize, double jitter, int norm_squared, int natural_order, double* Phi, double* dlev);
int sig_features_K(gpsig_ctx* c, const gpsig_params* p, bool raw, const void* X, const void* X2, int64_t N1, int64_t N2, int L1, int L2, int return_levels,
                   void* out, bool timed, int x_squared, int64_t row_begin, int64_t row_end, int compact, bool* done, bool row_block_call = false);
bool tvs_features_plan(gpsig_ctx* c, const gpsig_params* p, bool f64, int64_t Tn, int64_t N, int L);
int tens_vs_seq_features_device(gpsig_ctx* c, const gpsig_params* p, bool f64, const void* ZT, const void* ZS, const void* X, int64_t Tn, int64_t N, int L,
                                int increments, const double* w, void* out, bool* done);
// sig_feat_grad_api.hip: SignatureLinear's levels differentiated through the feature contraction
int sig_features_grad(gpsig_ctx* c, const gpsig_params* p, int d, const double* X, const double* Y, int64_t N1, int64_t N2, int L1, int L2, bool diag,
                      bool sym, const double* G, double* gX, double* gY, bool* done);

// ---- reverse pass of the sequence lattices (grad_wave_kernel.hpp, grad_wave_ho_kernel.hpp, grad_fused_kernel.hpp) --------------------
WaveLaunchFn wave_lookup_inc(int G, int C, int DP, int LQ);
WaveLaunchFn wave_lookup_ptd(int G, int C, int DP, int LQ);
WaveLaunchFn wave_lookup_ptn(int G, int C, int DP, int LQ);
Wave2LaunchFn wave2_lookup_inc(int G, int C, int DP, int LQ);
Wave2LaunchFn lam_undo_lookup_ptd_rbf(int G, int C, int DP, int LQ);
Wave2LaunchFn lam_undo_lookup_ptd_gen(int G, int C, int DP, int LQ);
Wave2LaunchFn lam_undo_lookup_ptn_rbf(int G, int C, int DP, int LQ);
Wave2LaunchFn lam_undo_lookup_ptn_gen(int G, int C, int DP, int LQ);
WaveHoLaunchFn wave_ho_lookup(int G, int C, int order, int M);        // grad_wave_ho_inst.hip: prefixes through an HBM slot
WaveHoLaunchFn wave_o1_lookup(int G, int C, int M);                   // first order from a dM lattice: seq_grad_wave_o1_kernel
WaveHoLaunchFn wave_ho_undo_lookup_g16(int C, int order, int M);      // grad_wave_ho_inst_u16.hip / _u32.hip / _u64.hip: scratch-free
WaveHoLaunchFn wave_ho_undo_lookup_g32(int C, int order, int M);
WaveHoLaunchFn wave_ho_undo_lookup_g64(int C, int order, int M);
WaveHoLaunchFn wave_ho_levels_lookup_g16(int C, int order, int M);    // the forward pass: seq_levels_wave_ho_kernel
WaveHoLaunchFn wave_ho_levels_lookup_g32(int C, int order, int M);
WaveHoLaunchFn wave_ho_levels_lookup_g64(int C, int order, int M);
FusedGradLaunchFn fused_grad_stash_lookup(int kind, int DP, int LQ);
FusedGradLaunchFn fused_grad_lookup_diff_g16(int kind, int DP, int LQ);
FusedGradLaunchFn fused_grad_lookup_diff_g32(int kind, int DP, int LQ);
FusedGradLaunchFn fused_grad_lookup_diff_g64(int kind, int DP, int LQ);
FusedGradLaunchFn fused_grad_lookup_nodiff_g16(int kind, int DP, int LQ);
FusedGradLaunchFn fused_grad_lookup_nodiff_g32(int kind, int DP, int LQ);
FusedGradLaunchFn fused_grad_lookup_nodiff_g64(int kind, int DP, int LQ);
// grad_api.hip: the sweeps of the higher-order reverse pass, shared by the point route and the wide route
struct HoSweeps { WaveHoLaunchFn fn; int G, C; size_t lds, slot; };
bool ho_sweeps_plan(const gpsig_ctx* c, const gpsig_params* p, int R1, int R2, HoSweeps* hs);
bool o1_sweeps_plan(const gpsig_ctx* c, const gpsig_params* p, int R1, int R2, HoSweeps* hs);
bool ho_levels_plan(const gpsig_ctx* c, const gpsig_params* p, int R1, int R2, HoSweeps* hs);
int ho_sweeps_launch(gpsig_ctx* c, const HoSweeps& hs, int M, int R1, int R2, const double* dM, double* lam, const double* G, int64_t gm, int64_t gi,
                     int64_t gj, int64_t N2, bool diag, int64_t pair0, int64_t npairs);
int ho_levels_launch(gpsig_ctx* c, const HoSweeps& hs, int M, int R1, int R2, const double* dM, double* out, int64_t gm, int64_t gi, int64_t gj, int64_t N2,
                     bool diag, int64_t pair0, int64_t npairs);

// ---- wide_api.hip: state spaces beyond the exact-shape kernels' columns (kernel arguments by dgemm, fused map / difference / recursion kernels)
bool wide_tvs_available(const gpsig_ctx* c, const gpsig_params* p, int d, int64_t Tn, int64_t N, int L);
int wide_tvs_forward(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& sz, int d, const double* Z, const double* Xs, int64_t Tn, int64_t N, int L,
                     int increments, const double* fx, const double* w, int sum_levels, double* out, double* aux);
int wide_tvs_backward(gpsig_ctx* c, const gpsig_params* p, int d, const double* Z, const double* X, const double* G, int64_t Tn, int64_t N, int L,
                      int increments, const double* fac, const double* aux, double* gZ, double* gX, double* gfac, double* g_base);
bool wide_tens_available(const gpsig_ctx* c, const gpsig_params* p, int64_t Tn);
int wide_tens_forward(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& sz, int d, const double* Z, int64_t Tn, int increments, const double* w,
                      int sum_levels, double* out);
int wide_tens_backward(gpsig_ctx* c, const gpsig_params* p, int d, const double* Z, int64_t Tn, int increments, const double* G, double* gZ, double* g_base);
bool wide_lat_available(const gpsig_ctx* c, const gpsig_params* p, int L1, int L2);
bool wide_lat_ho_available(const gpsig_ctx* c, const gpsig_params* p, int L1, int L2);
int wide_lat_forward(gpsig_ctx* c, const gpsig_params* p, int d, const double* Xs, const double* Ys, int64_t N1, int64_t N2, int L1, int L2, bool diag,
                     double* out);
int wide_lat_backward(gpsig_ctx* c, const gpsig_params* p, int d, const double* Xs, const double* Ys, int64_t N1, int64_t N2, int L1, int L2, bool diag,
                      const double* G, double* gX, double* gY, double* g_base);

// the forward side's own predicates (api.hip's evaluation entry points and level primitives): the three above, or exact-mode SignatureSpectral beyond 32
// columns (wide_spectral: the kernel object has opted in -- check_params --; forward only, the reverse entry points keep asking the three above).
// wide_spectral_refusal: why such a call is not served, as the context's error (GPSIG_ERR_UNSUPPORTED)
bool wide_spectral(const gpsig_params* p);
bool wide_tvs_fwd_available(const gpsig_ctx* c, const gpsig_params* p, int d, int64_t Tn, int64_t N, int L);
bool wide_tens_fwd_available(const gpsig_ctx* c, const gpsig_params* p, int64_t Tn);
bool wide_lat_fwd_available(const gpsig_ctx* c, const gpsig_params* p, int L1, int L2);
int wide_spectral_refusal(gpsig_ctx* c, const gpsig_params* p, bool lattice, int L2);

// what the ragged form of the route (wide_ragged_api.hip) shares with it: the argument budget of one chunk (option wide_chunk_mb), the columns per lane
// of a lattice of R2 columns and the wavefronts per lattice of a launch (option wide_lat_waves)
size_t wide_chunk_bytes(const gpsig_ctx* c);
int wide_lat_columns(int R2);
int wide_lat_waves(const gpsig_ctx* c, int C, int64_t lattices);

// ---- wide_ragged_api.hip: ragged batches in exact mode -- the entry points gpsig_kernel_*_ragged (include/gpsig_hip.h).  Kzz of the covariances is
// the dense call's: api.hip's evaluation of K_tens on device pointers, float64
int tens_gram_f64(gpsig_ctx* c, const gpsig_params* p, const void* Z, int64_t Tn, int increments, int return_levels, void* out);

// ---- wide_spectral_inst.hip: SignatureSpectral's kernel-argument array of the wide route (wide_spectral_kernel.hpp).  They return the hipError_t of the launch.
struct WideSpxArgs;
int wide_spx_prep_launch(hipStream_t stream, const double* gamma, int64_t count, double* g2);          // g2 = gamma^2
// nrm, ph (Q, rows): the norms sum_f g2_qf x_f^2 and the phases <omega_q, x> of the rows X (rows, ld)
int wide_spx_side_launch(hipStream_t stream, const double* X, int64_t rows, int64_t ld, int d, int Q, const double* omega, const double* g2, double* nrm,
                         double* ph);
int wide_spx_launch(hipStream_t stream, const WideSpxArgs& A);

// ---- spectral_kappa_inst.hip: the reverse pass of the batched kappa op gpsig_spectral_kappa / _grad (kernels: spectral_kappa_kernel.hpp; the entry
// points and the chunking: spectral_kappa_api.hip; the forward pass is the three launchers above).  They return the hipError_t of the launch.
struct SpecKappaArgs;
int spk_weights_launch(hipStream_t stream, const SpecKappaArgs& A);                                   // U_q and the per-tile sums of a chunk
// out[e] = (first ? 0 : out[e]) + part[0][e] + part[1][e] + ... + part[count - 1][e], e < width: every sum of the op, in this order
int spk_reduce_launch(hipStream_t stream, const double* part, int64_t count, int64_t width, int first, double* out);
int spk_scale_launch(hipStream_t stream, const SpecKappaArgs& A);                                     // AS_q = gamma_q^2 o A
int spk_rows_launch(hipStream_t stream, const SpecKappaArgs& A);                                      // dA of the chunk's rows
int spk_cols_launch(hipStream_t stream, const SpecKappaArgs& A);                                      // dB of the chunk's batch members
int spk_param_launch(hipStream_t stream, const SpecKappaArgs& A, int side);                           // per-slice sums of domega, dgamma: side 0 rows of A, 1 rows of B
int spk_finish_launch(hipStream_t stream, const SpecKappaArgs& A, double* dalpha, double* domega, double* dgamma);

// ---- lr_cross_spectral_inst.hip: gpsig_spectral_cross / gpsig_spectral_cross_grad beyond 32 columns (the entry points: spectral_cross_api.hip)
int spectral_cross_wide(gpsig_ctx* c, int Q, int family, int d, const double* P, int64_t n, const double* S, int cc, const double* alpha,
                        const double* omega, const double* gamma, double* K);
int spectral_cross_wide_grad(gpsig_ctx* c, int Q, int family, int d, const double* P, int64_t n, const double* S, int cc, const double* alpha,
                             const double* omega, const double* gamma, const double* G, double* dP, double* dS, double* dalpha, double* domega,
                             double* dgamma);
// what both, and the evaluation side's wide spectral route (lr_eval_spectral_wide_inst.hip), compute once per call, at `head` (Q d + 2 Q c doubles):
// gamma^2 (Q, d), the landmarks' norms sum_f g2_qf s_if^2 (Q, c) and their phases phi_q(S_i) (Q, c).  Returns the hipError_t of the launches.
int spectral_cross_prepare_launch(hipStream_t stream, const double* S, int cc, int d, int Q, const double* omega, const double* gamma, double* head);

// ---- lowrank_solver.hip: rocSOLVER / rocBLAS, opened at first use --------------------------------------------------------------------
bool solver_dsyevd(void** handle_slot, hipStream_t stream, int n, double* A, double* ev, double* work, int* info, std::string* err);
bool solver_dgemm(void** handle_slot, hipStream_t stream, bool transA, bool transB, int m, int n, int k, double alpha, const double* A, int lda,
                  const double* B, int ldb, double beta, double* C, int ldc, std::string* err);
bool solver_dgemm_batched(void** handle_slot, hipStream_t stream, bool transA, bool transB, int m, int n, int k, double alpha, const double* A, int lda,
                          int64_t sa, const double* B, int ldb, int64_t sb, double beta, double* C, int ldc, int64_t sc, int batch, std::string* err);
void solver_release(void* handle);
}  // namespace gpsig
