/* gpsig_hip.h -- C ABI of libgpsig_hip.so: the MI355X (gfx950) signature-kernel evaluation path.
 *
 * The reference (tgcsaba/GPSig) is pure Python on TensorFlow 1.15 / GPflow 1.5.1 and has no native
 * boundary of its own; the entry points below are what a GPflow-side binding for this path would
 * call instead of building the TF graph.  Each one names the reference method it replaces
 * (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - All arrays are row-major and contiguous.  Sequences are passed exactly as the reference's
 *     numpy-facing wrappers take them: X is (N, L*d) viewed as (N, L, d) (gpsig/kernels.py:417-418),
 *     Z is (lt, T, d) or (lt, T, 2, d) with lt = M(M+1)/2 (gpsig/inducing_variables.py:28-46).
 *   - "levels" outputs have a leading axis of num_levels+1 (level 0 == 1, gpsig/signature_algs.py:20).
 *   - Data pointers are host or device pointers according to gpsig_set_pointer_mode(); the
 *     hyper-parameter arrays inside gpsig_params are always HOST pointers.
 *   - Every function returns GPSIG_OK (0) or a negative error code; gpsig_last_error() gives text.
 *   - Caller owns all inputs and outputs.  Scratch memory is owned by the ctx.  One ctx per
 *     (device, stream); calls on different ctxs may run concurrently; a ctx is not re-entrant.
 *   - In device-pointer mode calls are asynchronous on the ctx stream; in host-pointer mode they
 *     return after the result has been copied back.
 *   - There is no CPU fallback anywhere behind this ABI.
 */
#ifndef GPSIG_HIP_H
#define GPSIG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPSIG_ABI_VERSION 1

enum gpsig_status {
    GPSIG_OK = 0,
    GPSIG_ERR_INVALID = -1,      /* bad argument (the Python shim raises ValueError) */
    GPSIG_ERR_UNSUPPORTED = -2,  /* valid in the reference, not built here yet (NotImplementedError) */
    GPSIG_ERR_HIP = -3,          /* HIP runtime failure (RuntimeError) */
    GPSIG_ERR_NOMEM = -4
};

/* static (state-space) kernels, gpsig/kernels.py:786-993 */
enum gpsig_base_kernel {
    GPSIG_BASE_LINEAR = 0,    /* SignatureLinear    _lin       :799-806 */
    GPSIG_BASE_RBF = 1,       /* SignatureRBF/Gauss _rbf       :862-864 */
    GPSIG_BASE_COSINE = 2,    /* SignatureCosine    _cos       :820-828 */
    GPSIG_BASE_POLY = 3,      /* SignaturePoly      _poly      :844-848  base_params = {gamma, degree} */
    GPSIG_BASE_MIX = 4,       /* SignatureMix       _mix       :881-892  base_params = {mixing} */
    GPSIG_BASE_MATERN12 = 5,  /* SignatureMatern12/Laplace/Exponential :955-958 */
    GPSIG_BASE_MATERN32 = 6,  /* SignatureMatern32  :974-977 */
    GPSIG_BASE_MATERN52 = 7,  /* SignatureMatern52  :991-993 */
    GPSIG_BASE_SPECTRAL = 8   /* SignatureSpectral  _spectral  :921-942  base_params = {Q, family (0 rbf, 1 exp, 2 mixed)};
                                 base_table = alpha[Q], omega[Q][d], gamma[Q][d]; needs lengthscales == NULL, num_lags == 0
                                 (as the reference: :907, and its gamma clashes with the lag weights of :82).
                                 At most 32 features.  base_params[2] is the kernel object's OPT-IN to low-rank evaluation beyond
                                 them: 0 (the default) refuses more than 32 features everywhere, as before; non-zero lets the low-rank
                                 entry points -- gpsig_lr_seq_features, _ragged, gpsig_lr_tens_features, gpsig_lr_draw,
                                 gpsig_lr_whitening, gpsig_lr_gather_points, gpsig_base_kernel_matrix, gpsig_lr_kernel / _diag and
                                 the normalised gpsig_kernel_Kdiag (which runs no base kernel) -- take 33 .. 4096 features: float64,
                                 num_components <= 64, num_levels <= 8 (see gpsig_lr_seq_features).  Up to 32 features the slot
                                 changes nothing, and every exact (non-low-rank) evaluation keeps refusing more whatever it holds.
                                 The opt-in is off until a follow-up flips the default.
                                 base_params[3] is the kernel object's OPT-IN to EXACT (non-low-rank) evaluation beyond 32 features
                                 (kernels.SignatureSpectral.spectral_wide), independent of [2]: 0 (the default) refuses as before, with
                                 the same messages and codes; non-zero lets the evaluation entry points and forward level primitives --
                                 gpsig_kernel_K, _Kdiag, _K_tens, _K_tens_vs_seq, _K_tens_n_seq_covs, _K_seq_n_seq_covs,
                                 gpsig_seq_gram_levels, gpsig_seq_diag_levels, gpsig_tens_gram_levels, gpsig_tens_vs_seq_levels,
                                 gpsig_tens_vs_seq_weighted -- take 33 .. 4096 features on the wide route (the argument array by
                                 wide_spx_kernel on the float64 matrix cores; two bitwise-equal points are at distance and phase
                                 exactly 0): float64, Q <= 64, num_levels <= 8, first-order sequence lattices of at most 512 columns,
                                 Kzx at orders <= 4, Kzz within 2 GB of argument blocks, dense batches, host and device pointers; the
                                 result does not depend on wide_chunk_mb bit for bit.  GPSIG_ERR_UNSUPPORTED with a message naming the
                                 bound: "... serves first-order sequence lattices only", "... sequence lattices of at most 512 columns",
                                 "... serves Kzx at orders <= 4", "... is built for num_levels <= 8", "... context option wide = 0
                                 refuses it", "graph recording: ... is served by the wide route only, which does not record", "the spectral base kernel is built
                                 for float64 only", "num_features=... outside [1, 4096]".  No gradient entry point takes the family;
                                 up to 32 features the slot changes no bit. */
};

enum gpsig_dtype { GPSIG_F64 = 0, GPSIG_F32 = 1 };
enum gpsig_pointer_mode { GPSIG_PTR_HOST = 0, GPSIG_PTR_DEVICE = 1 };

typedef struct gpsig_ctx gpsig_ctx;

/* Constructor state of gpsig.kernels.SignatureKernel (gpsig/kernels.py:18-88), constrained values. */
typedef struct gpsig_params {
    int32_t base_kernel;     /* enum gpsig_base_kernel */
    int32_t dtype;           /* enum gpsig_dtype: element type of every data pointer */
    int32_t num_features;    /* d: state-space dimension of ONE lag copy (kernels.py:54) */
    int32_t num_levels;      /* M (kernels.py:55) */
    int32_t order;           /* 1..M, already clamped as kernels.py:57 does */
    int32_t difference;      /* kernels.py:63 */
    int32_t normalization;   /* kernels.py:62 */
    int32_t num_lags;        /* kernels.py:70-82 */
    double sigma;            /* kernels.py:66 */
    double jitter;           /* gpflow.settings.jitter, 1e-6 (kernels.py:431,463,578) */
    double base_params[4];
    const double* variances;     /* host, M+1 entries (kernels.py:65) */
    const double* lengthscales;  /* host, d entries, or NULL = no scaling (kernels.py:84-88) */
    const double* lags;          /* host, num_lags entries (kernels.py:79), NULL if num_lags == 0 */
    const double* gamma;         /* host, num_lags+1 entries (kernels.py:80-82), NULL if num_lags == 0 */
    const double* base_table;    /* host, extra parameters of the base kernel (GPSIG_BASE_SPECTRAL), else NULL */
    int64_t base_table_len;      /* number of doubles in base_table */
} gpsig_params;

/* ---- context ----------------------------------------------------------------------------- */
int gpsig_abi_version(void);
/* stream: a hipStream_t cast to void*, or NULL for the default stream */
int gpsig_ctx_create(int device, void* stream, gpsig_ctx** out);
void gpsig_ctx_destroy(gpsig_ctx* ctx);
const char* gpsig_last_error(gpsig_ctx* ctx); /* ctx may be NULL: error of the last failed create */
int gpsig_set_pointer_mode(gpsig_ctx* ctx, int mode);
int gpsig_sync(gpsig_ctx* ctx);
/* Restrict the following K / Kzx calls to shard `index` of `count` (independent pair blocks, no
 * exchange).  Entries outside the shard are left untouched in the output.  (0, 1) = everything. */
int gpsig_set_shard(gpsig_ctx* ctx, int index, int count);
/* Tuning / debugging knobs; unknown names return GPSIG_ERR_INVALID.
 *   "glds"        1: stage x-side records with LDS-DMA (global_load_lds), 0: load + ds_write
 *   "exact"       1: allow the kernels specialised on num_levels, 0: generic kernels only
 *   "pk2"         float32 kernels with two y sequences per pair group on the packed v_pk_* instructions (seq_pk2_kernel.hpp):
 *                 1 (default) wherever they are the faster ones, 2 always where built, 0 never
 *   "f32_waves"   their wavefronts per workgroup on one LDS ring of x records: 4, 1, or 0 = by launch size
 *   "f32_pack"    their y sequences per pair group: 2 (packed) or 1 (the same code on scalar instructions; for A/B runs)
 *   "keep_reset"  1 (default): the first-order pair kernels clear a lane's accumulators at a pair boundary through the
 *                 recursion's own FMAs (acc = acc * keep + inc with keep = 0 for one step), 0: by an explicit reset in the
 *                 boundary block (round 1; for A/B runs)
 *   "max_run"     >0: x-side run length per task, 0: automatic
 *   "tensor_lanes" tensor-vs-sequence kernel: 1 one lane per tensor, 0 one lane per sequence, -1 automatic
 *   "grad_scratch_mb" lattice scratch of one gradient / fallback launch in MiB (default 4096)
 *   "grad_impl"   gradient kernels: 0 planner's choice, 1 one pair per thread with the lattice in HBM scratch, 2 one pair per
 *                 thread scratch-free (tensor vs sequence), 3 wavefront kernel with the lattice in HBM scratch, 4 scratch-free wavefront
 *                 kernels wherever they are built (rounds 3-4's choice: for the point kernels both sweeps in one wavefront, dL/d(increments)
 *                 through HBM to a contraction kernel per side).  0 additionally picks the fused reverse kernel of round 5 (an evaluator and a
 *                 sweeper wavefront per four sequence pairs, both sides contracted on chip) where it is built: RBF and the Matern families on
 *                 points with differences, order 1, at most 256 points on one side, at most 8 columns of state space, 2 to 6 levels
 *   "matern_fast" float64 sequence Grams of SignatureMatern12 / 32 / 52: 1 (default) compile-time instances on prescaled records where the exact
 *                 shapes are built (distances from coordinate differences, table exp), 0 the run-time-kind instances with the library sqrt / exp
 *   "grad_stash_mb" gpsig_seq_gram_levels_stash keeps at most this many MiB for the backward call (default 4096; 0: never)
 *   "tvs_grad_tile" reverse pass of the tensor-vs-sequence chains: 1 (default) the tile kernel (all levels in one reverse sweep per
 *                 sequence, d/dx summed in LDS, no atomics) where it is built (order 1, at most 8 columns, at most 6 levels), 0 the round-1 kernels
 *   "pinned_staging" host-pointer mode: 1 (default) transfers of 2 MiB and more run in 16 MiB chunks through two pinned buffers of the
 *                 context, the DMA of one chunk overlapping a threaded host copy of the previous one; 0 plain hipMemcpy on the caller's
 *                 (pageable) memory
 *   "sig_features" SignatureLinear and SignatureCosine, any order: the Gram as ONE contraction of explicit level features on the float64 matrix cores
 *                 (sig_feat_kernel.hpp: K_m(x, y) = <Phi_m(x), Phi_m(y)>, d^m numbers per level): -1 (default) where that costs fewer
 *                 flops than the lattice sweep and the feature matrices fit, 0 never, 1 wherever it is built (d <= 32 columns after lags, d^M <= 32768); float32 calls are
 *                 computed in float64 on this route (inputs widened, result rounded)
 *   "sig_features_keep" 1: the feature matrix built by the next such evaluation is kept and reused by the evaluations that follow with the
 *                 same sequence pointer, shape and parameters -- the row-block calls of one decomposed Gram (gpsig_kernel_K_symm_rows*);
 *                 the caller must not write the sequences until it sets the option back to 0 (which also drops the matrix's validity)
 *   "sig_gemm_dma" that contraction's operand slabs by LDS-DMA into an XOR-swizzled image, fragments prefetched across the barrier
 *                 (1, default) or staged through registers (0); bit-identical results
 *   "sig_features_grad" gpsig_seq_gram_levels_grad / gpsig_seq_diag_levels_grad of SignatureLinear / SignatureCosine (every order) through the same feature space
 *                 (features, one rocBLAS dgemm per level and side, a reverse sweep per sequence: csrc/sig_feat_grad_api.hip): -1 (default)
 *                 where a time model says it is cheaper than the pair kernels' reverse pass, 0 never, 1 wherever it is built
 *   "sig_graded"  that contraction's depth pieces: 1 (default) the last of the equal pieces is cut into finer ones of halving size where a
 *                 launch runs for several rounds of workgroups (they fill the slots that fall free at the end: 12 -> 11.5 rounds' time
 *                 at BASELINE configs[1]), 0 equal pieces throughout (round 3).  The split depends on the Gram's total size and depth
 *                 alone, so row blocks still reassemble the one-call Gram bit for bit
 *   "lr_jacobi"   gpsig_lr_draw: 1 (default) the landmark Gram's eigendecomposition by the one-workgroup Jacobi kernel (c <= 64), 0 rocSOLVER
 *   "tvs_zreg"    tensor-lane gradient: components in registers (1) or LDS (0), -1 automatic
 *   "tvs_features" K_tens_vs_seq / the Kzx of K_tens_n_seq_covs (level sum) of SignatureLinear / SignatureCosine as ONE product of the tensors'
 *                 rank-one level features and the sequences' level features (rocBLAS dgemm; round 4): -1 (default) where a time model
 *                 prefers it to the tile kernel, 0 never, 1 wherever built (float64, 2 <= num_levels <= 8, not inside a graph capture)
 *   "tvs_tile"    tensor-vs-sequence tile kernel (levels split over the waves of a workgroup, coalesced result tiles):
 *                 -1 wherever it is built and there are at least 32 tensors, 0 never, 1 also for fewer tensors
 *   "tvs_tile_nw" its waves per workgroup (1 or 2), 0 automatic
 *   "tens_tile"   tensor-vs-tensor kernel (Kzz): 1 (default) 16 x 16 tiles with the tensors staged in LDS, 0 one thread per entry
 *                 gathering its components from HBM (round 1)
 *   "spectral_wave" SignatureSpectral's sequence kernels: 1 (default) the wavefront kernels with the family at compile time where they
 *                 are built (float64, first order, differences, d <= 16), 0 one pair per thread (round 1)
 *   "diag_own"    diagonal pass of the pair kernel (level diagonals for normalisation, Kdiag): 1 (default) every pair group of a
 *                 wavefront sweeps its own sequence, 0 all groups sweep the same 64/G sequences and emit one pair each (round 1)
 *   "lr_gemm"     low-rank Gram products on the fp64 matrix cores: 1 (default) 128 x 128 tiles with k-slabs staged through LDS,
 *                 0 operand fragments read straight from L2 (round 1)
 *   "lr_fused"    low-rank sequence features (gpsig_lr_seq_features): 1 (default) one fused kernel, a workgroup per sequence with
 *                 the (width, length) intermediates in LDS, wherever they fit -- two arrays where a wavefront can hold its output
 *                 columns in registers (at most 64 time steps, components and rank bound), three otherwise; 2 always the three-array
 *                 form; 0 one elementwise kernel per reference op.  Float32 features (p->dtype = GPSIG_F32) have the two fused forms
 *                 only: 0 answers GPSIG_ERR_UNSUPPORTED for them.  Also gpsig_lr_tens_features: 0 the multi-pass route.
 *   "wide"        (round 6) the wide-state-space route (csrc/wide_api.hip): kernel arguments by rocBLAS dgemm on augmented rows, fused
 *                 map / difference / recursion kernels, behind the levels, weighted-sum, fused-evaluation entry points and their gradients.
 *                 -1 (default) where the exact-shape kernels are not built or lose: Kzx beyond 8 columns, the sequence lattices beyond
 *                 32 columns / their register sides (reverse pass: beyond 8 columns where no fused kernel is built), Kzz beyond 12 --
 *                 the reference's own run settings, benchmarks/run_gpsig_benchmarks.py:32; 0 never; 1 wherever built (float64,
 *                 RBF and the Matern families, at most 8 levels, lattices of at most 512 columns; order 1, and at order > 1 the
 *                 tensor-vs-sequence chains (orders <= 4) and the sequence lattices' reverse pass (<= 5 levels)).  Not taken inside
 *                 a graph capture, nor under "capture_routes".
 *   "capture_routes"  0 (default); 1: eager calls choose the routes a library graph capture chooses -- every route that does not record (the wide route,
 *                 "tvs_features", "sig_features_grad") answers "not built", as it does between gpsig_graph_begin and gpsig_graph_end.  Set it around the
 *                 warm-up call of a recording and set it back afterwards (see the graph section below).  A call that has no route but the wide one -- more
 *                 than 64 columns, exact-mode SignatureSpectral beyond 32 -- then returns GPSIG_ERR_UNSUPPORTED with "graph recording: ... is served by the
 *                 wide route only, which does not record"; so does a ragged (lengths) call, whose plan needs the host
 *   "wide_chunk_mb"  its argument chunk in HBM (0: "grad_scratch_mb", 4 GB by default: a latency-bound launch split in two takes twice as long)
 *   "wide_contract"  the two contractions of a reverse pass with the adjoint array (rows of at most 32 augmented columns) as one hand-written MFMA pass:
 *                 1 (default) part tiles of 16 rows in LDS with the second operands in registers (rows of at most 16 columns; wider: the first form),
 *                 3 part tiles of 32 rows, 2 the first form (whole 64 x 64 tiles and both operand blocks in LDS), 0 two rocBLAS dgemms (for A/B runs)
 *   "wide_lat_waves"  wavefronts per sequence lattice on the wide route: -1 (default) eight for a launch of at most 128 lattices of more than 256
 *                 columns, one otherwise; 0 always one; 1 two / four / eight wherever a lane would hold that many columns
 *   "wide_sym_fold"  1 (default): the reverse pass of a symmetric Gram on the wide route runs over the pairs i <= j with the upstream gradient
 *                 folded onto them (G + G^T above the diagonal); 0: over all ordered pairs (for A/B runs)
 *   "wide_few_cols"  widest state space (default 8) at which the tensor-vs-sequence FORWARD pass of at most 256 sequences against tensors with increments
 *                 takes the wide chains (SignatureRBF; the reverse tile kernel continues from their totals); "ho_g32": -1 (default) the higher-order
 *                 sweeps of 33 .. 64 lattice columns with two columns per lane at order >= 3, four otherwise; 0 always four; 1 always two
 *   "wide_o1_sweeps"  first-order reverse pass of sequence lattices of at most 64 columns on the wide route: 1 (default) four lattices per wavefront from a dM
 *                 lattice (seq_grad_wave_o1_kernel) for launches of 1,024 lattices or more, 2 wherever the shape fits, 0 the lattice kernels (one per wavefront)
 *   "tvs_grad_matern" 1 (default): the Matern families in the tensor-vs-sequence reverse tile kernel as a compile-time kind; 0: the run-time family (A/B runs)
 *   order > 1 and "grad_impl": the sequence recursion's reverse pass runs as two sweeps of a wavefront per pair (csrc/grad_wave_ho_kernel.hpp;
 *                 <= 5 levels, min(order, levels) <= 4, lattices of <= 512 columns): 0 scratch-free where the row totals fit LDS, 3 with
 *                 the prefixes in an HBM slot per pair group, any other value the lattice operations of rounds 2-5 (tests' A/B reference) */
int gpsig_set_option(gpsig_ctx* ctx, const char* name, int value);
/* Bytes of device memory the context holds in its scratch buffers now (staging, task lists, intermediates; they grow on demand and are
 * kept until the context is destroyed).  No synchronisation, no device call. */
int64_t gpsig_scratch_bytes(gpsig_ctx* ctx);
/* HIP-event timing of the dominant kernel (the pair recursion) launched by the calls since the last
 * reset, measured on the ctx stream: total milliseconds and number of launches (the first 4096 timed
 * launches after a reset; none inside a graph capture). */
int gpsig_timing_reset(gpsig_ctx* ctx);
int gpsig_timing_get(gpsig_ctx* ctx, double* kernel_ms, int64_t* launches, int64_t* pairs);
/* What the timed launches were: *kernel = "sig_gram_dma_kernel" (or "sig_gram_kernel", its register-staged form) when they were the matrix-core contraction of the explicit signature
 * features (option "sig_features"), NULL for the pair recursion / chain kernels; *flops = the floating-point operations those
 * launches executed on the matrix cores (whole tiles, padded depth), 0 otherwise. */
int gpsig_timing_info(gpsig_ctx* ctx, const char** kernel, double* flops);
/* Effective shader clock while the calls that follow run (diagnostics for benchmarks; no reference analogue): a single sleeping
 * wavefront per XCD (eight one-wave workgroups) on a stream of its own takes up to `samples` readings of s_memtime (shader cycles) against s_memrealtime (100 MHz),
 * duration_ms / (samples - 1) apart; _read tells it to take a last reading and leave, waits for it, and returns the mean /
 * smallest / largest clock between consecutive readings in GHz and the time the readings span (it leaves by itself after 1.25 x
 * duration_ms).  Read it before any device-wide synchronisation, which would wait for the probe.  float64-heavy kernels run
 * this chip at 2.0-2.2 GHz instead of 2.4 (DVFS), differently from box to box: a benchmark line should carry the value. */
int gpsig_clock_probe_start(gpsig_ctx* ctx, double duration_ms, int32_t samples);
int gpsig_clock_probe_read(gpsig_ctx* ctx, double* ghz_mean, double* ghz_min, double* ghz_max, double* covered_ms);
/* The last read's mean clock per sampled wavefront and the XCD each sat on (HW_REG_XCC_ID); ghz_mean above is their average. */
int gpsig_clock_probe_xcds(gpsig_ctx* ctx, double* ghz, int32_t* xcc, int32_t cap, int32_t* n);

/* ---- HIP graphs for launch-bound evaluations (no reference analogue) -------------------------------------
 * An end-to-end evaluation is 5-15 short kernels.  The calls made between gpsig_graph_begin and gpsig_graph_end are
 * recorded from the ctx stream instead of executed; gpsig_graph_launch replays them with one launch, reading and writing
 * the same device buffers (refresh the inputs in place).  What it saves is host time per evaluation; the device time of a
 * small evaluation is the serial sweep of one pair's lattice and is the same either way (profiles/r01_graph_latency.txt).
 * Conditions, all checked: device-pointer mode; a context created on a stream of its own (not the default stream);
 * every recorded call was made once before with the same shapes and
 * hyper-parameters on this ctx (so that scratch buffers, task lists and level weights are in place -- a call that would
 * allocate, upload or wait fails with GPSIG_ERR_INVALID and the capture ends); a graph is replayable until a later call
 * moves a scratch buffer (gpsig_graph_launch then returns GPSIG_ERR_INVALID: capture again).
 *
 * The warm-up must take the route the recording takes.  Several routes do not record (the wide route: rocBLAS may allocate; Kzx as a product of
 * level features; the feature contraction's reverse pass) and are the eager default at many shapes: beyond 8 columns for Kzx, 12 for Kzz, 16 / 32 for
 * the sequence Grams.  A plain warm-up there sizes only that route's buffers.  So make the warm-up call under option "capture_routes":
 *
 *     gpsig_set_option(ctx, "capture_routes", 1);   the call, once;   gpsig_set_option(ctx, "capture_routes", 0);
 *     gpsig_graph_begin(ctx);   the same call;   gpsig_graph_end(ctx, &g);
 *
 * The contract, for any call the library serves eagerly, after that warm-up on the same ctx -- a recording of the same call does exactly one of two things:
 *   it SUCCEEDS: every replay on new contents of the same buffers is bit-equal to an eager call under "capture_routes" = 1 (the route the recording took),
 *     and agrees with a float64 reference to the tolerance that route is held to; or
 *   it is REFUSED at the warm-up (GPSIG_ERR_UNSUPPORTED): the message opens with "graph recording:" and names what the caller can act on -- the bound
 *     (64 columns; 32 for exact-mode SignatureSpectral), "served by the wide route only, which does not record".  It never reads "a scratch buffer has to
 *     grow -- run the same calls once".  The context is usable afterwards: no capture is open, and an eager call (option back at 0) works.
 * The same holds for the reverse-side entry points (the *_grad functions): their route predicates ask the same question. */
typedef struct gpsig_graph gpsig_graph;
int gpsig_graph_begin(gpsig_ctx* ctx);
int gpsig_graph_end(gpsig_ctx* ctx, gpsig_graph** out);
int gpsig_graph_launch(gpsig_ctx* ctx, gpsig_graph* graph);
void gpsig_graph_destroy(gpsig_graph* graph);

/* ---- unnormalised level tensors (the signature_algs.py layer) ----------------------------- */
/* SignatureKernel._K_seq (kernels.py:208-237) -> signature_kern_first_order / _higher_order
 * (signature_algs.py:8-74) on the base-kernel tensor of (X, X2).  X2 == NULL: symmetric.
 * Inputs are used as given (no lengthscale division).  out: (M+1, N1, N2). */
int gpsig_seq_gram_levels(gpsig_ctx* ctx, const gpsig_params* p, const void* X, const void* X2,
                          int64_t N1, int64_t N2, int32_t L1, int32_t L2, void* out);
/* SignatureKernel._K_seq_diag (kernels.py:188-205).  out: (M+1, N). */
int gpsig_seq_diag_levels(gpsig_ctx* ctx, const gpsig_params* p, const void* X, int64_t N, int32_t L, void* out);
/* SignatureKernel._K_tens (kernels.py:263-283) -> tensor_kern (signature_algs.py:76-99).  out: (M+1, T, T). */
int gpsig_tens_gram_levels(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, int64_t T, int32_t increments, void* out);
/* SignatureKernel._K_tens_vs_seq (kernels.py:313-340) -> signature_kern_tens_vs_seq_first_order /
 * _higher_order (signature_algs.py:101-160).  out: (M+1, T, N). */
int gpsig_tens_vs_seq_levels(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, const void* X,
                             int64_t T, int64_t N, int32_t L, int32_t increments, void* out);

/* Weighted level sum of the tensor-vs-sequence levels,  out[t][n] = sum_m fac[n][m] * _K_tens_vs_seq(Z, X)[m][t][n]:  what
 * K_tens_vs_seq (kernels.py:572-588) and the Kzx of K_tens_n_seq_covs (:638 / :660, :667) are once the per-sequence factors
 * fac[n][m] = sigma variances[m] / sqrt(diag_m(x_n) + jitter) are known -- in one pass, the level sum taken in the kernel's
 * epilogue, without the (M+1, T, N) level array ever reaching memory.  It is the form a training step uses (the factors are
 * differentiable inputs; gpsig_tens_vs_seq_weighted_grad below).  Inputs are used as given, like the level primitives.
 * fac: (N, M+1), out: (T, N), element type p->dtype.
 * aux (optional; float64, device-pointer mode): gpsig_tens_vs_seq_aux_elems() doubles that receive the totals of every chain of
 * every (tensor, sequence) pair when the tile kernel evaluates the call (*aux_written = 1); handed to _weighted_grad they save its
 * forward sweep.  NULL, or *aux_written == 0 afterwards: the reverse pass rebuilds them itself. */
int gpsig_tens_vs_seq_weighted(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, const void* X, int64_t T, int64_t N,
                               int32_t L, int32_t increments, const void* fac, void* out, void* aux, int32_t* aux_written);
int64_t gpsig_tens_vs_seq_aux_elems(const gpsig_params* p, int64_t T, int64_t N);

/* ---- end-to-end kernel evaluations (scaling, lags, normalisation, sigma*variances, level sum) */
/* SignatureKernel.K (kernels.py:401-476).  out: (N1, N2), or (M+1, N1, N2) if return_levels. */
int gpsig_kernel_K(gpsig_ctx* ctx, const gpsig_params* p, const void* X, const void* X2,
                   int64_t N1, int64_t N2, int32_t L1, int32_t L2, int32_t return_levels, void* out);
/* Row-block form of the symmetric K(X) for multi-GPU runs (no reference analogue: the reference is single
 * device).  Every unordered pair {i, j} of the N sequences is owned by exactly one row: row j owns the
 * columns i with (j - i) mod N in [0, N/2] (ties at N/2, N even, go to the smaller index as column).  A rank
 * computes the owned entries of rows [row_begin, row_end) -- row_begin a multiple of 4 -- into `out_rows`,
 * a (row_end - row_begin, N) block; entries it does not own are left untouched.  The blocks of all ranks,
 * stacked, are turned into the full symmetric matrix by gpsig_symmetrize_owned_rows. */
int gpsig_kernel_K_symm_rows(gpsig_ctx* ctx, const gpsig_params* p, const void* X, int64_t N, int32_t L,
                             int64_t row_begin, int64_t row_end, void* out_rows);
/* out[r][c] = half[r][c] if row r owns column c, else half[c][r].  half, out: (N, N), distinct buffers. */
int gpsig_symmetrize_owned_rows(gpsig_ctx* ctx, int32_t dtype, const void* half, int64_t N, void* out);
/* The same two steps with COMPACT row blocks: row j's N/2+1 owned columns j-N/2 .. j (mod N) are stored side by side,
 * out_rows[(j - row_begin) * (N/2+1) + N/2 - ((j-i) mod N)] -- half the bytes to move between GPUs; the one slot per row of an
 * even N that belongs to the other row of its pair (the tie at distance N/2) is left untouched.  half: the stacked blocks,
 * (N, N/2+1); out: (N, N). */
int gpsig_kernel_K_symm_rows_compact(gpsig_ctx* ctx, const gpsig_params* p, const void* X, int64_t N, int32_t L,
                                     int64_t row_begin, int64_t row_end, void* out_rows);
int gpsig_symmetrize_compact_rows(gpsig_ctx* ctx, int32_t dtype, const void* half, int64_t N, void* out);
/* SignatureKernel.Kdiag (kernels.py:479-510).  out: (N,) or (M+1, N). */
int gpsig_kernel_Kdiag(gpsig_ctx* ctx, const gpsig_params* p, const void* X, int64_t N, int32_t L,
                       int32_t return_levels, void* out);
/* SignatureKernel.K_tens (kernels.py:513-536).  out: (T, T) or (M+1, T, T). */
int gpsig_kernel_K_tens(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, int64_t T, int32_t increments,
                        int32_t return_levels, void* out);
/* SignatureKernel.K_tens_vs_seq (kernels.py:539-588).  out: (T, N) or (M+1, T, N). */
int gpsig_kernel_K_tens_vs_seq(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, const void* X,
                               int64_t T, int64_t N, int32_t L, int32_t increments, int32_t return_levels, void* out);
/* SignatureKernel.K_tens_n_seq_covs (kernels.py:591-671).  Kxx is (N,) / (M+1, N) unless full_X_cov. */
int gpsig_kernel_K_tens_n_seq_covs(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, const void* X,
                                   int64_t T, int64_t N, int32_t L, int32_t increments, int32_t full_X_cov,
                                   int32_t return_levels, void* Kzz, void* Kzx, void* Kxx);
/* SignatureKernel.K_seq_n_seq_covs (kernels.py:674-761): X = inducing sequences, X2 = data. */
int gpsig_kernel_K_seq_n_seq_covs(gpsig_ctx* ctx, const gpsig_params* p, const void* X, const void* X2,
                                  int64_t N1, int64_t N2, int32_t L1, int32_t L2, int32_t full_X2_cov,
                                  int32_t return_levels, void* Kxx, void* Kxx2, void* Kx2x2);

/* ---- ragged batches in exact mode (no reference analogue: the reference pads).  Each entry point takes its dense twin's arguments plus
 * `lengths`, directly after each L: N int32 in the context's pointer mode, 1 <= lengths[n] <= L (GPSIG_ERR_INVALID otherwise, and for a NULL
 * `lengths` where one is required).  Sequence n is X[n, :lengths[n]], evaluated as that truncated sequence would be on its own: rows at or
 * beyond lengths[n] are never read (NaN there changes no bit), difference = 1 gives lengths[n] - 1 increments, normalisation uses the
 * sequence's own diagonal, and with num_lags > 0 the lag interpolation runs on the sequence's OWN axis i / (lengths[n] - 1) -- the query of lag
 * j at observation t is max(t / (lengths[n] - 1) - lag_j, 0); the lagged copies of a one-point sequence are the point itself.  Outputs,
 * factors, sigma * variances, the level sum and the return_levels layouts are the dense entry points'; Kzz is the dense call's.
 * Forward evaluation on the wide route (kernel arguments by a contraction over packed rows, then chain / lattice kernels), taken at any width.
 * The plan needs the lengths on the host: in device-pointer mode one copy of N int32 and a stream synchronisation.
 * Served: SignatureRBF and the Matern families, float64, num_levels <= 8, first order, sequence lattices of at most 512 columns (the longest
 * sequence of the right-hand / diagonal side, minus one with differences).  GPSIG_ERR_UNSUPPORTED, with the bound in the message: the other
 * base kernels, order > 1 with num_levels > 1, context option wide = 0, graph capture, p->dtype = GPSIG_F32, longer lattices.  The argument
 * chunks follow option wide_chunk_mb, in whole sequences; a result does not depend on it bit for bit (Kdiag) or beyond rounding (the dgemms). */
int gpsig_kernel_Kdiag_ragged(gpsig_ctx* ctx, const gpsig_params* p, const void* X, int64_t N, int32_t L, const int32_t* lengths,
                              int32_t return_levels, void* out);
int gpsig_kernel_K_tens_vs_seq_ragged(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, const void* X,
                                      int64_t T, int64_t N, int32_t L, const int32_t* lengths, int32_t increments, int32_t return_levels, void* out);
int gpsig_kernel_K_tens_n_seq_covs_ragged(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, const void* X,
                                          int64_t T, int64_t N, int32_t L, const int32_t* lengths, int32_t increments, int32_t full_X_cov,
                                          int32_t return_levels, void* Kzz, void* Kzx, void* Kxx);
/* lengths / lengths2: either may be NULL -- that side is dense, every sequence has its L1 / L2 rows.  X2 == NULL: symmetric (lengths2 unused). */
int gpsig_kernel_K_ragged(gpsig_ctx* ctx, const gpsig_params* p, const void* X, const void* X2,
                          int64_t N1, int64_t N2, int32_t L1, const int32_t* lengths, int32_t L2, const int32_t* lengths2,
                          int32_t return_levels, void* out);

/* ---- low-rank mode (low_rank=True): gpsig/low_rank_calculations.py, gpsig/signature_algs.py:162-222,
 * gpsig/kernels.py:239-311, :424-426, :442-458, :499-501, :525-527, :560-574.
 * Float types: the state (landmarks, whitening, projections) is float64 always.  p->dtype = GPSIG_F32 (float32 points, features and
 * Grams) is accepted by gpsig_lr_seq_features / gpsig_lr_seq_features_ragged / gpsig_lr_tens_features (the fused and the time-tiled kernels
 * only: option lr_fused != 0 and the float32 LDS footprint within bounds, else GPSIG_ERR_UNSUPPORTED), gpsig_lr_kernel / gpsig_lr_kernel_diag (float32 factors in, float32 out),
 * and gpsig_lr_draw / gpsig_lr_gather_points (float32 points, widened before any arithmetic: the state drawn is bitwise that of the
 * widened points).  The spectral base kernel included.  Every other low-rank entry point is float64 only.
 *
 * The reference draws landmarks and random projections with TensorFlow's RNG inside the graph; here they are
 * drawn by the caller and passed in (all HOST pointers), which makes the device code deterministic:
 *   landmarks  (c, d') scaled points, whitening (c, c) = U / sqrt(S + jitter) of the landmark Gram
 *              (low_rank_calculations.py:50-60);
 *   sketches   one per level 2..M: the projection of low_rank_calculations.py:104-193 stored by output column,
 *              out[j] = sum_{e in [colptr[j], colptr[j+1])} val[e] * A[i1[e]] * B[i2[e]].
 * Factor matrices Phi are (rows, F), F = 1 + c + (M-1) r, level blocks [1 | c | r | ... | r].
 * Host-side objects are uploaded once and recognised on later calls by a 64-bit FNV-1a hash of their dimensions and contents (an
 * evaluation hashes ~100 KB instead of uploading it); the parameter tables of the spectral kernel, wide lengthscales and the level
 * offsets are compared in full.  A recorded graph (gpsig_graph_*) reads these device copies: a later eager call on the same ctx
 * with other objects rewrites them in place, and replays of the earlier recording are refused. */
typedef struct gpsig_sketch {
    int32_t k1, k2, r, nnz;
    const int32_t* colptr;   /* r + 1 */
    const int32_t* i1;       /* nnz, < k1 */
    const int32_t* i2;       /* nnz, < k2 */
    const double* val;       /* nnz */
} gpsig_sketch;
typedef struct gpsig_lr_state gpsig_lr_state;   /* the same objects drawn and kept on the device: gpsig_lr_draw below */
typedef struct gpsig_lowrank {
    int32_t num_components;  /* c */
    int32_t rank_bound;      /* r */
    int32_t num_sketches;    /* M - 1 */
    const double* landmarks;
    const double* whitening;
    const gpsig_sketch* sketches;
    const gpsig_lr_state* device_state;   /* non-NULL: the three arrays above are ignored */
} gpsig_lowrank;
/* The random objects of one low-rank evaluation drawn ON THE DEVICE, as the reference draws them inside its graph at every
 * evaluation (low_rank_calculations.py:12-20, :47-57, :92-101, :104-127, :139-193): c landmark rows uniformly without replacement
 * among the scaled components of Z (or NULL), the scaled observations of X and of X2 (or NULL) -- in this order --, the jitter
 * diagonal, the whitening of the landmark Gram (a one-workgroup Jacobi eigendecomposition for c <= 64, rocSOLVER beyond), and one
 * projection per level 2..M; sparsity 0 'sqrt', 1 'log', 2 'lin'.  A counter-based generator (Philox-4x32-10) keyed by `seed`: the same
 * seed gives the same objects.  Device pointers; everything is queued on the ctx stream, nothing waits for the host.  *state: NULL to
 * create, or a state of this context to draw into again.  gpsig_lr_state_sizes / _export copy what was drawn to the host (for the
 * CPU restatement of the same evaluation); they wait for the stream.
 * SignatureSpectral beyond 32 features with the opt-in p->base_params[2] != 0: the landmark Gram here, in gpsig_lr_whitening and in
 * gpsig_base_kernel_matrix comes from a thread-per-pair kernel on the table in its (Q, d) layout, in the difference form (symmetric; at most
 * 64 landmarks are ever whitened for a state the feature entry points accept).  Without the opt-in refused, as before. */
int gpsig_lr_draw(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t sparsity, uint64_t seed,
                  const void* X, int64_t N, int32_t L, const void* X2, int64_t N2, int32_t L2, const void* Z, int64_t T,
                  int32_t increments, gpsig_lr_state** state);
void gpsig_lr_state_destroy(gpsig_lr_state* state);
int gpsig_lr_state_sizes(gpsig_ctx* ctx, const gpsig_lr_state* state, int32_t* sizes /* 5: c, d', r, projections, Jacobi sweeps */, int32_t* nnz);
int gpsig_lr_state_export(gpsig_ctx* ctx, const gpsig_lr_state* state, double* landmarks, double* jitter_diag, double* whitening,
                          double* eigenvalues, const gpsig_sketch* sketches);
/* scaled / lagged observations number idx[0..R) (flat index n*L + t) of X -> out (R, d') on the HOST (landmark candidates; float64 for
 * float32 X too) */
int gpsig_lr_gather_points(gpsig_ctx* ctx, const gpsig_params* p, const void* X, int64_t N, int32_t L, const int64_t* idx,
                           int64_t R, double* out_host);
/* kappa(A, B) of already scaled points, all on the HOST: A (na, d'), B (nb, d') -> out (na, nb) */
int gpsig_base_kernel_matrix(gpsig_ctx* ctx, const gpsig_params* p, const double* A_host, const double* B_host, int64_t na,
                             int64_t nb, int32_t d, double* out_host);
/* Nystrom whitening (low_rank_calculations.py:50-57, :60) of c landmarks S (c, d') -- already scaled points, HOST --:
 * W = kappa(S, S) + diag(jitter_diag) on the device, rocSOLVER dsyevd, whitening (c, c) = U / sqrt(eigenvalues + p->jitter) back
 * on the HOST (the layout gpsig_lowrank.whitening takes).  eigenvalues_host: (c) ascending, or NULL.  The reference draws
 * jitter_diag as settings.jitter * uniform(0, 1) per landmark (:52); it is an argument here so that the caller owns the RNG. */
int gpsig_lr_whitening(gpsig_ctx* ctx, const gpsig_params* p, const double* landmarks_host, int32_t c, int32_t d,
                       const double* jitter_diag_host, double* whitening_host, double* eigenvalues_host);
/* The same feature map for the TRAINING path (round 4): when the reference trains in low-rank mode the landmarks are gathered from the
 * scaled inputs and their Gram is decomposed inside the differentiated graph (low_rank_calculations.py:47-60), so landmarks S (c, d) and
 * whitening Wh (c, c) are functions of the trainable parameters and live on the device -- DEVICE pointers, like X (N, L, d: columns as
 * they come, no scaling inside, p->num_lags = 0) and Phi (N, F = 1 + c + (M-1) r); device-pointer mode only.  The projections of
 * levels 2..M are value-independent random objects: HOST arrays, kept on the device by content across calls.
 * _grad: dPhi (N, F) -> gX (N, L, d), gS (c, d), gWh (c, c), g_base[0] (the base kernel's own parameter, or NULL) -- what tf.gradients
 * returns for _K_seq_lr_feat (kernels.py:239-261) given the landmarks and the whitening; the caller chains gS and gWh through the
 * gather and the eigendecomposition (gpsig_amd/autodiff.py).  num_components <= 64 and num_components x d <= 4096 in _grad.
 * Sequence length: where a sequence's arrays fit the LDS the whole sequence is kept on chip (three arrays of max(c, r, d) rows forward,
 * four in _grad: at c = r = 50 up to L = 128 and L = 64); longer sequences are walked in time tiles of a multiple of 64 steps (64 at 64
 * rows, 256 at 16 rows), each direction on its own, with the same results up to rounding in _grad.  GPSIG_ERR_UNSUPPORTED only where a
 * single 64-step tile does not fit (more than about 75 rows in _grad), or where one workgroup's scratch of (c + (M-2) r) L doubles
 * exceeds 256 MB. */
int gpsig_lr_seq_features_dev(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                              const gpsig_sketch* sketches, const void* X, int64_t N, int32_t L, const double* S, const double* Wh, void* Phi);
int gpsig_lr_seq_features_grad(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                               const gpsig_sketch* sketches, const void* X, int64_t N, int32_t L, const double* S, const double* Wh,
                               const void* dPhi, void* gX, double* gS, double* gWh, double* g_base);
/* The same pair for a RAGGED batch: sequence n has lengths[n] points, 1 <= lengths[n] <= L, in rows of room for L (`lengths`: N int32 on
 * the DEVICE, directly after L).  Phi[n] is exactly the features of X[n, :lengths[n]] evaluated alone (with p->difference and lengths[n] = 1:
 * no steps, Phi[n] = [1, 0, .., 0]); the rows X[n, lengths[n]:] are never read and may hold anything, NaN included; _grad writes every gX row
 * exactly once, the padded points' rows as exact zeros, and stays deterministic.  Same checks, limits, typed refusals and plan as the pair above:
 * whole-sequence or time-tiled form, tile length, LDS and scratch sizes follow from L alone (the host never reads the lengths); the kernels
 * take each sequence's extent, tile count and scratch rows from its length, clamped to [1, L] on the device.  lengths == NULL with N > 0 is
 * GPSIG_ERR_INVALID.  Float64, the families of the pair above (GPSIG_BASE_SPECTRAL: GPSIG_ERR_UNSUPPORTED).  They follow the option
 * lr_fused_pad; the whole-sequence forms are built once each, at 512 threads, whatever lr_fused_variant and lr_grad_threads say (at 1024
 * threads the ragged reverse instance would keep scratch memory). */
int gpsig_lr_seq_features_ragged_dev(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                     const gpsig_sketch* sketches, const void* X, int64_t N, int32_t L, const int32_t* lengths, const double* S,
                                     const double* Wh, void* Phi);
int gpsig_lr_seq_features_ragged_grad(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                      const gpsig_sketch* sketches, const void* X, int64_t N, int32_t L, const int32_t* lengths, const double* S,
                                      const double* Wh, const void* dPhi, void* gX, double* gS, double* gWh, double* g_base);
/* The same pair for SignatureSpectral, whose parameters are trained: p->base_kernel = GPSIG_BASE_SPECTRAL, p->base_params = {Q, family};
 * alpha (Q), omega (Q, d), gamma (Q, d) are DEVICE pointers read on the device (p->base_table is ignored; no host round trip per step).
 * _grad: dPhi (N, F) -> gX (N, L, d), gS (c, d), gWh (c, c), dalpha (Q), domega (Q, d), dgamma (Q, d), all overwritten; deterministic
 * (no floating-point atomics, partial sums combined in a fixed order).  Limits: float64, device-pointer mode, num_lags = 0, order 1,
 * num_levels <= 8, Q <= 64, d <= 32, num_components <= 64, num_components x d <= 4096, a sequence's arrays within the LDS (longer sequences
 * and ragged batches: the _spectral_ragged pair below); outside them GPSIG_ERR_UNSUPPORTED.  gpsig_lr_seq_features_dev / _grad keep refusing the
 * spectral kernel. */
int gpsig_lr_seq_features_spectral_dev(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                       const gpsig_sketch* sketches, const void* X, int64_t N, int32_t L, const double* S, const double* Wh,
                                       const double* alpha, const double* omega, const double* gamma, void* Phi);
int gpsig_lr_seq_features_spectral_grad(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                        const gpsig_sketch* sketches, const void* X, int64_t N, int32_t L, const double* S, const double* Wh,
                                        const double* alpha, const double* omega, const double* gamma, const void* dPhi, void* gX,
                                        double* gS, double* gWh, double* dalpha, double* domega, double* dgamma);
/* The spectral pair for LONG and RAGGED batches: the same arguments with `lengths` directly after L, as the ragged pair above (N int32 on the
 * DEVICE, clamped to [1, L] by the kernels) -- but lengths == NULL is valid here and means that every sequence has L points: that is how long
 * dense batches are served.  Limits: those of the spectral pair except the sequence length.  Where a sequence's arrays fit the LDS the whole
 * sequence is kept on chip, longer ones are walked in time tiles, each direction on its own; the plan follows from L alone (the host never
 * reads the lengths).  GPSIG_ERR_UNSUPPORTED only where a single 64-step tile does not fit or where one workgroup's scratch -- the
 * (c + (M-2) r) L doubles of the other families plus c L for kxs, which _grad keeps so that kappa is evaluated once per point -- exceeds
 * 256 MB.  Phi[n] is the features of X[n, :lengths[n]] evaluated alone; the rows beyond a sequence's length are never read, by the feature
 * kernels or by the spectral cross op's reverse kernels, and may hold NaN; _grad writes every gX row exactly once, the padded points' rows as
 * exact zeros, and is bit-for-bit repeatable (fixed-order partial sums, no floating-point atomics).  N = 0: the summed outputs are zeroed.
 * One instance per form (whole-sequence forward and reverse 512 threads, tiled forward 1024, tiled reverse 512), whatever lr_fused,
 * lr_fused_variant and lr_grad_threads say; they follow lr_fused_pad. */
int gpsig_lr_seq_features_spectral_ragged_dev(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                              const gpsig_sketch* sketches, const void* X, int64_t N, int32_t L, const int32_t* lengths,
                                              const double* S, const double* Wh, const double* alpha, const double* omega, const double* gamma,
                                              void* Phi);
int gpsig_lr_seq_features_spectral_ragged_grad(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                               const gpsig_sketch* sketches, const void* X, int64_t N, int32_t L, const int32_t* lengths,
                                               const double* S, const double* Wh, const double* alpha, const double* omega, const double* gamma,
                                               const void* dPhi, void* gX, double* gS, double* gWh, double* dalpha, double* domega, double* dgamma);
/* The inducing tensors' feature map for the TRAINING path: _K_tens_lr_feat (kernels.py:285-311: Nystrom_map + tensor_kern_lr_feature) given
 * landmarks S (c, d) and whitening Wh (c, c) on the device, like the four sequence entry points above.  Z: T inducing tensors of
 * lt = M (M + 1) / 2 components, (lt, T, d) or, with `increments`, (lt, T, 2, d) -- already scaled (no lengthscales inside, p->num_lags = 0),
 * DEVICE pointer; Phi (T, F = 1 + c + (M-1) r) by the fused tensor kernels (one workgroup per tensor).
 * _grad: dPhi (T, F) -> gZ (Z's layout), gS (c, d), gWh (c, c), g_base[0] (the base kernel's own parameter, or NULL), all overwritten: one
 * kernel that repeats the forward pass in LDS and walks every level's chain of projections backwards, per-workgroup partial sums combined
 * in a fixed order (no floating-point atomics: bit-for-bit repeatable).  The Matern families take no gradient through a zero distance, as
 * the sequence pair.  The spectral pair takes alpha (Q), omega (Q, d), gamma (Q, d) as DEVICE pointers (p->base_params = {Q, family}) and also
 * returns dalpha, domega, dgamma.  T = 0: the summed outputs are zeroed.  Limits: float64, device-pointer mode (GPSIG_ERR_INVALID otherwise),
 * order 1, num_levels <= 8, num_components <= 64, num_components x d <= 4096, a tensor's arrays within the LDS (spectral: Q <= 64, d <= 32);
 * outside them GPSIG_ERR_UNSUPPORTED. */
int gpsig_lr_tens_features_dev(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                               const gpsig_sketch* sketches, const void* Z, int64_t T, int32_t increments, const double* S, const double* Wh,
                               void* Phi);
int gpsig_lr_tens_features_grad(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                const gpsig_sketch* sketches, const void* Z, int64_t T, int32_t increments, const double* S, const double* Wh,
                                const void* dPhi, void* gZ, double* gS, double* gWh, double* g_base);
int gpsig_lr_tens_features_spectral_dev(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                        const gpsig_sketch* sketches, const void* Z, int64_t T, int32_t increments, const double* S,
                                        const double* Wh, const double* alpha, const double* omega, const double* gamma, void* Phi);
int gpsig_lr_tens_features_spectral_grad(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                         const gpsig_sketch* sketches, const void* Z, int64_t T, int32_t increments, const double* S,
                                         const double* Wh, const double* alpha, const double* omega, const double* gamma, const void* dPhi,
                                         void* gZ, double* gS, double* gWh, double* dalpha, double* domega, double* dgamma);
/* SignatureSpectral's Nystrom cross matrix for the TRAINING path (kernels.py:921-942, low_rank_calculations.py:59): K (n, c) = kappa(P, S)
 * for points P (n, d) and landmarks S (c, d), the parameters alpha (Q), omega (Q, d), gamma (Q, d) read from DEVICE memory (they change at
 * every optimiser step: no trip through the host), family 0 = rbf, 1 = exp, 2 = mixed; 1 <= Q <= 64.  Device pointers, device-pointer
 * mode; asynchronous on the context's stream.  Limits: d <= 32 with any c >= 1 (a thread per pair); 33 <= d <= 4096 with c <= 64 (the d-deep
 * contractions on the float64 matrix cores: the squared distance of a component is xs + ss - 2 ip from three products accumulated in one
 * order, the phase a difference of two, so a landmark that IS one of the points is at distance and phase exactly 0 from it); outside them
 * GPSIG_ERR_UNSUPPORTED.
 * _grad: G = dL/dK (n, c) -> dP (n, d), dS (c, d), dalpha (Q), domega (Q, d), dgamma (Q, d), overwritten; deterministic (partial sums
 * combined in a fixed order, no floating-point atomics: two calls return the same bits).  The exponential envelope's sqrt has derivative 0 at
 * zero distance (a point paired with itself).  n = 0 zeroes the four sums.  Beyond 32 columns also: scratch stays inside the context's chunk
 * budget (wide_chunk_mb, else grad_scratch_mb) -- the points go in chunks whose sums are added in chunk order; the bits of dP do not depend
 * on the budget --, and an element with G == 0 contributes nothing whatever its point holds: a point all of whose G are zero (the padded rows
 * of a ragged batch: NaN in P, zeros in G) gets a dP row of exact zeros and takes no part in dS, dalpha, domega, dgamma. */
int gpsig_spectral_cross(gpsig_ctx* ctx, int32_t Q, int32_t family, int32_t d, const double* P, int64_t n, const double* S, int32_t c,
                         const double* alpha, const double* omega, const double* gamma, double* K);
int gpsig_spectral_cross_grad(gpsig_ctx* ctx, int32_t Q, int32_t family, int32_t d, const double* P, int64_t n, const double* S, int32_t c,
                              const double* alpha, const double* omega, const double* gamma, const double* G, double* dP, double* dS,
                              double* dalpha, double* domega, double* dgamma);
/* SignatureSpectral's kappa as a BATCHED op for exact-mode training (kernels.py:921-942): K (batch, m, n) = kappa(A_b[i], B_b[j]) for A (batch, m, d),
 * B (batch, n, d), contiguous float64; alpha (Q), omega (Q, d), gamma (Q, d) read from DEVICE memory; family as in gpsig_spectral_cross.  What the
 * matrix route's torch ops compute from the (batch, m, n, d) difference tensor, without that tensor: the d-deep contractions run on the float64 matrix
 * cores, a component's squared distance is nrm(a) + nrm(b) - 2 ip from three products accumulated in one order and its phase a difference of two, so
 * where a row of A and a row of B are bitwise equal the entry is exactly sum_q alpha_q.  A and B may be the same array (the rows' norms and phases are
 * then computed once).  Device pointers, device-pointer mode, asynchronous on the context's stream; not inside a graph capture.
 * Limits: 1 <= Q <= 64, 1 <= d <= 4096, m, n < 2^31; outside them GPSIG_ERR_UNSUPPORTED with the bound in the message.  batch, m or n equal to 0 is
 * served: nothing is launched.
 * _grad: G = dL/dK (batch, m, n) -> dA (batch, m, d), dB (batch, n, d), dalpha (Q), domega (Q, d), dgamma (Q, d), overwritten (dA and dB are two
 * arrays even where A and B are one: the caller adds them).  The exponential envelope's sqrt has derivative 0 at zero distance.  With batch, m or n
 * equal to 0 all five are written as zeros.  Scratch stays inside the context's chunk budget (wide_chunk_mb, else grad_scratch_mb): whole batch
 * members go in chunks, and rows of A in blocks of a multiple of 64 where one member exceeds it (a single 64-row block beyond the budget is still
 * served).  Sums inside a chunk are added slot by slot, the column-side and parameter sums of the chunks in chunk order: no floating-point atomics,
 * two identical calls return the same bits (a different budget may round the sums differently).  The two skinny products per chunk are rocBLAS GEMMs. */
int gpsig_spectral_kappa(gpsig_ctx* ctx, int32_t Q, int32_t family, int32_t d, const double* A, const double* B, int64_t batch, int64_t m, int64_t n,
                         const double* alpha, const double* omega, const double* gamma, double* K);
int gpsig_spectral_kappa_grad(gpsig_ctx* ctx, int32_t Q, int32_t family, int32_t d, const double* A, const double* B, int64_t batch, int64_t m,
                              int64_t n, const double* alpha, const double* omega, const double* gamma, const double* G, double* dA, double* dB,
                              double* dalpha, double* domega, double* dgamma);
/* The Nystrom cross matrix of the other families for the TRAINING path on WIDE state spaces (low_rank_calculations.py:59): K (n, c) =
 * kappa(P, S) for points P (n, d) and landmarks S (c, d), p->base_kernel in GPSIG_BASE_LINEAR .. GPSIG_BASE_MATERN52 with p->base_params as
 * the fused feature kernels read them, d = p->num_features; the d-deep contraction runs on the float64 matrix cores.  Device pointers,
 * device-pointer mode, float64, asynchronous on the context's stream.  Limits: 1 <= c <= 64, 1 <= d <= 4096, any n >= 0; outside them
 * GPSIG_ERR_UNSUPPORTED.  |P_t|^2 and |S_i|^2 are diagonals of matrix-core products with the inner product's own order of additions, so a
 * landmark that IS one of the points is at distance exactly 0 from it.
 * _grad: G = dL/dK (n, c) -> dP (n, d), dS (c, d), g_base[0] (the base kernel's own parameter, or NULL), overwritten; partial sums combined
 * in a fixed order, no floating-point atomics: two calls return the same bits (the number of partial sums of dS follows the option
 * wide_chunk_mb).  The Matern families take no gradient through a zero distance, as the feature pairs above.  An element with G == 0
 * contributes nothing whatever its point holds, and a point whose G are all zero gets a dP row of exact zeros: the padded rows of a ragged
 * batch may hold NaN.  n = 0: dS and g_base are zeroed.  Scratch: n (c + 1) doubles of the context's. */
int gpsig_lr_cross(gpsig_ctx* ctx, const gpsig_params* p, const double* P, int64_t n, const double* S, int32_t c, double* K);
int gpsig_lr_cross_grad(gpsig_ctx* ctx, const gpsig_params* p, const double* P, int64_t n, const double* S, int32_t c, const double* G, double* dP,
                        double* dS, double* g_base);
/* The training path's feature maps BEHIND that cross matrix: gpsig_lr_seq_features_dev / _grad and gpsig_lr_tens_features_dev / _grad without
 * their first phase.  kxs (N, L, c) = kappa(X, S) and kzs (lt T E, c) = kappa of Z's points in their flat order come from memory
 * (gpsig_lr_cross); the reverse passes return dkxs / dkzs in the same layouts (for gpsig_lr_cross_grad, which carries them on to the points,
 * the landmarks and the base parameter) and gWh (c, c), all overwritten and bit-for-bit repeatable.  p->num_features (the width the cross
 * matrix was computed at) is not used: the width enters neither the LDS plan nor a table, which have max(c, r) rows.  `lengths`: N int32 on
 * the DEVICE as the ragged pair takes them, or NULL (every sequence has L points); the kxs rows beyond a sequence's length are never read and
 * their dkxs rows are exact zeros.  Sequences go in time tiles (one tile where they fit).  Checks and refusals are those of the pairs above
 * (float64, device-pointer mode, order 1, num_levels <= 8, num_components <= 64, else GPSIG_ERR_UNSUPPORTED); the sequence pair also refuses
 * a 64-step tile that exceeds the LDS, the tensor pair a tensor's arrays that do.  N = 0 / T = 0: gWh is zeroed. */
int gpsig_lr_seq_features_kx_dev(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                 const gpsig_sketch* sketches, const double* kxs, int64_t N, int32_t L, const int32_t* lengths, const double* Wh,
                                 void* Phi);
int gpsig_lr_seq_features_kx_grad(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                  const gpsig_sketch* sketches, const double* kxs, int64_t N, int32_t L, const int32_t* lengths, const double* Wh,
                                  const void* dPhi, double* dkxs, double* gWh);
int gpsig_lr_tens_features_kx_dev(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                  const gpsig_sketch* sketches, const double* kzs, int64_t T, int32_t increments, const double* Wh, void* Phi);
int gpsig_lr_tens_features_kx_grad(gpsig_ctx* ctx, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t num_sketches,
                                   const gpsig_sketch* sketches, const double* kzs, int64_t T, int32_t increments, const double* Wh,
                                   const void* dPhi, double* dkzs, double* gWh);
/* SignatureKernel._K_seq_lr_feat (kernels.py:239-261): Nystrom_map + signature_kern_first_order_lr_feature.  Phi: (N, F).
 * With option lr_fused != 0 (the default): one fused kernel where a sequence's three (width, L) arrays fit the LDS; beyond that the
 * time-tiled kernels (csrc/lr_eval_tiled.hpp: tiles of a multiple of 64 time steps, one carried vector per level, the raw points scaled in
 * the kernel -- lengthscales and lags included), in float64 and float32, where at least one 64-step tile fits; SignatureSpectral's tiled
 * kernel is float64 only (float32: GPSIG_ERR_UNSUPPORTED there).  Where not even one tile holds the points -- 65 c + 138 max(c, r, d') doubles
 * exceed 156 KB: d' > 121 at c = r = 50, twice that in float32 -- the WIDE route: the Nystrom cross matrix on the float64 matrix cores from the
 * raw points (csrc/lr_cross_kernel.hpp, evaluation form; float32 points are widened value by value, so a landmark that is one of the points
 * stays at distance exactly 0), written to context scratch in the call's element type, then the feature kernels that take it from memory
 * (csrc/lr_kx.hpp; float32: the kx instance of the tiled kernel); sequences go in chunks whose cross matrix stays within wide_chunk_mb (else
 * grad_scratch_mb), and the result does not depend on the chunk count.  It serves the families of base_eval at num_components <= 64,
 * num_levels <= 8 and d' <= 4096 wherever max(c, r) rows fit a tile.  lr_fused = 0, SignatureSpectral or num_components > 64 beyond the
 * tiled kernels: the multi-pass route (float64 only; float32: GPSIG_ERR_UNSUPPORTED), which streams five (N, L, max(c, r)) arrays of
 * context-owned scratch.  The rule is csrc/lr_tile_plan.hpp: lr_eval_route.
 * SignatureSpectral beyond 32 features: refused (GPSIG_ERR_UNSUPPORTED, "at most 32 features") unless p->base_params[2] != 0, the kernel
 * object's opt-in (off by default).  With it, 33 .. 4096 features take ONE route, dense or ragged and at any lr_fused, 0 included: the
 * evaluation form of the spectral cross kernel (csrc/lr_eval_spectral_wide_inst.hip: the d-deep contractions on the float64 matrix cores from
 * the caller's raw points, the points' phases in the same walk, so that a landmark that is one of the points is at distance and phase exactly
 * 0), then the feature kernels above that take the cross matrix from memory, in the same chunks.  Float64, num_components <= 64,
 * num_levels <= 8, max(c, r) rows within a tile; outside that GPSIG_ERR_UNSUPPORTED with a message that names the bound -- float32 included
 * (the Python layer computes such a call in float64 and rounds).  The rule is csrc/lr_tile_plan.hpp: lr_spectral_eval_wide. */
int gpsig_lr_seq_features(gpsig_ctx* ctx, const gpsig_params* p, const gpsig_lowrank* lr, const void* X, int64_t N, int32_t L, void* Phi);
/* ... for a RAGGED batch: lengths (N int32, in the context's pointer mode like X; host pointers are copied in), sequence n is
 * X[n, :lengths[n]] and Phi[n] its features evaluated alone.  The rows beyond a sequence's length are never read (they may hold NaN);
 * lengths are clamped to [1, L] on the device.  A sequence of one point with p->difference has no steps: Phi[n] = [1, 0, .., 0].  Served by
 * the time-tiled kernels at every length and, where not even one tile holds the points, by the wide route (above: the padded rows are zeros
 * in the cross kernel's operand and their rows of the cross matrix are never written), whatever lr_fused says; float64 and float32,
 * SignatureSpectral in float64 only.
 * GPSIG_ERR_UNSUPPORTED: p->num_lags > 0 (the lag interpolation runs on the table's own time axis), float32 SignatureSpectral, and shapes
 * whose 64-step tile exceeds the LDS where the wide route does not apply (SignatureSpectral, num_components > 64, max(c, r) rows beyond a tile).
 * SignatureSpectral beyond 32 features with the opt-in p->base_params[2] != 0: the route of gpsig_lr_seq_features above -- the padded rows are
 * zeros in the spectral cross kernel's operand, are never read or written, and a wavefront whose 16 rows are all padding skips its arithmetic. */
int gpsig_lr_seq_features_ragged(gpsig_ctx* ctx, const gpsig_params* p, const gpsig_lowrank* lr, const void* X, int64_t N, int32_t L,
                                 const int32_t* lengths, void* Phi);
/* ... for a ragged batch WITH LAGS, each sequence on its own time axis (no reference analogue: the reference pads and interpolates on the
 * table's axis).  The contract, routes and refusals of gpsig_lr_seq_features_ragged, except that p->num_lags > 0 is served: sequence n is
 * X[n, :len] (len = lengths[n]) and Phi[n] the features of that truncated sequence evaluated on its own -- its axis is i / (len - 1), the query
 * of lag j at observation t is max(t / (len - 1) - lag_j, 0), bracket and value as gpsig/lags.py:20-32 with jitter 1e-6 -- equal to
 * gpsig_lr_seq_features on X[n:n+1, :len] with the same lr.  Rows at or beyond len are never read.  A sequence of ONE point has no axis (the
 * reference's formula is 0 / 0 there and the dense entry points return NaN at L = 1): its lagged copies are the point itself.  With full
 * lengths the bits are gpsig_lr_seq_features', with p->num_lags == 0 those of gpsig_lr_seq_features_ragged. */
int gpsig_lr_seq_features_ragged_lagged(gpsig_ctx* ctx, const gpsig_params* p, const gpsig_lowrank* lr, const void* X, int64_t N, int32_t L,
                                        const int32_t* lengths, void* Phi);
/* The TRAINING path's lag op for ragged batches (gpsig/lags.py:41-63 on per-sequence axes, the semantics above): X (N, L, d), lengths (N int32,
 * clamped to [1, L]), lags (p doubles, 1 <= p <= 8) -> out (N, L, p + 1, d): copy 0 is X, copy j the interpolation at lag j; the output rows at
 * or beyond a sequence's length repeat its row len - 1 (so that landmarks gathered from it are real points), the input rows there are never
 * read.  Device pointers, device-pointer mode, float64, asynchronous on the context's stream, d <= 4096.
 * _grad: G = dL/dout -> dX (N, L, d), every element written, rows at or beyond len exact zeros (the gradients of the repeated output rows go
 * to the sources of row len - 1), and dlags (p) = - sum G (x_r - x_l) / (t_r - t_l) over the queries that the clamp at 0 did not catch; a
 * sequence of one point contributes exactly zero to dlags.  No floating-point atomics: two calls return the same bits.  N = 0: dlags is
 * zeroed.  Scratch: N p doubles of the context's. */
int gpsig_seq_lags_ragged_dev(gpsig_ctx* ctx, const double* X, const int32_t* lengths, const double* lags, int64_t N, int32_t L, int32_t d,
                              int32_t p, double* out);
int gpsig_seq_lags_ragged_grad(gpsig_ctx* ctx, const double* X, const int32_t* lengths, const double* lags, const double* G, int64_t N,
                               int32_t L, int32_t d, int32_t p, double* dX, double* dlags);
/* SignatureKernel._K_tens_lr_feat (kernels.py:285-311): Nystrom_map + tensor_kern_lr_feature.  Phi: (T, F).  With lr_fused != 0 one fused kernel
 * where a tensor's arrays -- 8 (lt E (d' + 2 c) + lt c + 2 max(c, r)) bytes, half in float32 -- fit 64 KB of LDS; where they do without the
 * points (d' = 0) the wide route as for sequences (the cross matrix of Z's points in their flat order, then the kx instance of the fused
 * kernel; tensors in chunks), for the families of base_eval at num_components <= 64; else the multi-pass route (float64 only).
 * SignatureSpectral beyond 32 features with the opt-in p->base_params[2] != 0: the spectral cross kernel's evaluation form on Z's points in their
 * flat order, then the kx instance of the fused kernel, under the bounds of gpsig_lr_seq_features with the kzs footprint (d' = 0) within 64 KB
 * and T <= 2^31 - 1 (csrc/lr_tile_plan.hpp: lr_spectral_eval_tens_wide); without the opt-in refused, as before. */
int gpsig_lr_tens_features(gpsig_ctx* ctx, const gpsig_params* p, const gpsig_lowrank* lr, const void* Z, int64_t T,
                           int32_t increments, void* Phi);
/* Kernel matrix from factors: level Grams PhiA_m PhiB_m^T (fp64 MFMA; float32 factors: v_mfma_f32_16x16x4_f32), optional per-side level normalisation
 * 1/sqrt(|Phi_m|^2 + jitter) (kernels.py:457-469, :574-581), sigma*variances, level sum.  PhiB == NULL: symmetric, with
 * the jitter of kernels.py:431 on the diagonal when normalising.  out: (N1, N2) or (M+1, N1, N2). */
int gpsig_lr_kernel(gpsig_ctx* ctx, const gpsig_params* p, const gpsig_lowrank* lr, const void* PhiA, const void* PhiB, int64_t N1,
                    int64_t N2, int32_t normalize_a, int32_t normalize_b, int32_t return_levels, void* out);
/* diagonal sum_j Phi_m[n][j]^2 * sigma * variances[m] (kernels.py:499-510).  out: (N,) or (M+1, N). */
int gpsig_lr_kernel_diag(gpsig_ctx* ctx, const gpsig_params* p, const gpsig_lowrank* lr, const void* Phi, int64_t N,
                         int32_t return_levels, void* out);

/* ---- gradients (reverse mode) of the level primitives ------------------------------------------------------------
 * The reference has no gradient code: it trains through TensorFlow's autodiff of the graph these primitives stand
 * for (gpsig/training.py:149-164, gpsig/models.py:40-59).  Each function below takes the upstream gradient G of the
 * (M+1, ...) level array its forward counterpart returns and produces the gradients with respect to the inputs of
 * that primitive, i.e. what tf.gradients would return for _K_seq / _K_seq_diag / _K_tens / _K_tens_vs_seq
 * (gpsig/kernels.py:188-340) with order = 1.  As for the forward primitives, inputs are taken as they come (already
 * scaled, d = num_features * (num_lags + 1) columns); float64 only.  Outputs are overwritten.  g_base: 2 doubles in the
 * context's pointer mode or NULL; [0] receives the gradient with respect to base_params[0] (gamma of SignaturePoly,
 * kernels.py:844-848; mixing of SignatureMix, :881-892).  Option "grad_scratch_mb" bounds the lattice scratch. */
/* X2 == NULL: symmetric Gram, gX receives both roles of every sequence. */
int gpsig_seq_gram_levels_grad(gpsig_ctx* ctx, const gpsig_params* p, const void* X, const void* X2, int64_t N1, int64_t N2,
                               int32_t L1, int32_t L2, const void* G /* (M+1, N1, N2) */, void* gX, void* gX2, double* g_base);
/* The pair of them for a forward pass that will be differentiated (round 5; what the TensorFlow graph of the reference does implicitly -- the
 * forward op's intermediates are kept for its gradient op).  _levels_stash evaluates like gpsig_seq_gram_levels and, where the fused reverse
 * kernel can continue from it (SignatureRBF / SignatureMatern12 / 32 / 52 with differences, order 1, float64, at most 64 observations and 8
 * columns, num_levels 4 / 5, within
 * option "grad_stash_mb", default 4096; not inside a graph capture), keeps the forward recursion's row totals and final states in the context:
 * desc (8 integers) describes what was kept, desc[0] == 0 nothing.  _levels_grad_stash continues from it with the backward sweep only (*taken = 1),
 * or does nothing (*taken = 0: never kept, or another evaluation has overwritten it since) -- then call gpsig_seq_gram_levels_grad.  Device
 * pointers.  K(X) forward + backward of 1,024 sequences of 64 x 8, five levels: 17.0 -> 13 ms. */
int gpsig_seq_gram_levels_stash(gpsig_ctx* ctx, const gpsig_params* p, const void* X, const void* X2, int64_t N1, int64_t N2,
                                int32_t L1, int32_t L2, void* out, int64_t* desc /* 8 */);
int gpsig_seq_gram_levels_grad_stash(gpsig_ctx* ctx, const gpsig_params* p, const void* X, const void* X2, int64_t N1, int64_t N2,
                                     int32_t L1, int32_t L2, const void* G, void* gX, void* gX2, const int64_t* desc, int32_t* taken);
/* The explicit level features of the linear (cosine: of the unit vectors) kernel as an op of their own (round 4; no function of this name
 * in the reference: signature_algs.py:8-35 unrolled -- level m of SignatureLinear is <Phi_m(x), Phi_m(y)> -- and, for order > 1, the
 * truncated-exponential steps of :37-74; order = num_levels with difference on is the signature of the piecewise-linear path, what the
 * reference's notebook checks against esig).  out: (N, ld) doubles, ld = gpsig_seq_features_ld(p, L): columns [0, F) hold levels 1..M one
 * after the other, F = sum_m d^m, each in the natural order of its multi-indices (last index fastest, first index = earliest time), column F
 * is level 0 (= 1), the rest zeros.  With them the tensor-vs-sequence kernel of a rank-one tensor is <z_1 (x) .. (x) z_m, Phi_m(x)>
 * (signature_algs.py:101-127).  Inputs as they come (p->lengthscales NULL, no lags), float64; _ld returns 0 for shapes the feature kernels
 * are not built for (then _seq_features fails with GPSIG_ERR_UNSUPPORTED).  _grad: dPhi (N, ld) back through the feature sweep to gX
 * (N, L, d); Phi is the forward's output; device pointers.  Plain kernel launches on the context's stream: usable inside a graph capture. */
int64_t gpsig_seq_features_ld(const gpsig_params* p, int32_t L);
int gpsig_seq_features(gpsig_ctx* ctx, const gpsig_params* p, const void* X, int64_t N, int32_t L, void* out);
int gpsig_seq_features_grad(gpsig_ctx* ctx, const gpsig_params* p, const void* X, int64_t N, int32_t L, const void* Phi, const void* dPhi, void* gX);
/* The gradient of gpsig_kernel_K's level SUM (return_levels = 0) for SignatureLinear / SignatureCosine of every order through the
 * feature space (round 4): with K[i][j] = sum_m w_m <u_m(x_i), u_m(y_j)>, u_m = Phi_m / sqrt(|Phi_m|^2 + jitter) when p->normalization
 * (else Phi_m) and w_m = sigma variances[m], every level shares the upstream g (N1, N2), so ONE product g U(Y) over the whole feature
 * width (rocBLAS dgemm), the normalisation's reverse step per row and one reverse sweep per sequence give gX [, gX2] -- the
 * (M+1, N1, N2) level arrays of the level primitives and their upstream gradients never exist (what tf.gradients does through
 * kernels.py:401-476 for these kernels).  Inputs as they come, like the level primitives (p->lengthscales NULL, no lags); float64,
 * device-pointer mode.  X2 == NULL: symmetric Gram (a normalised one has a constant diagonal: no gradient from it).
 * g_weights: (M+1) doubles on the device or NULL; entries 1..M receive d/dw_m from the feature products; entry 0 (level 0 is constant)
 * and a normalised symmetric Gram's diagonal terms (trace of g) are plain sums of g left to the caller.
 * *taken = 0: the route does not apply (another base kernel, a shape the feature kernels are not built for, inside a graph capture,
 * option "sig_features_grad" 0 ...): nothing was written, use the level primitives.  g == NULL: only answer that question. */
int gpsig_kernel_K_grad(gpsig_ctx* ctx, const gpsig_params* p, const void* X, const void* X2, int64_t N1, int64_t N2, int32_t L1, int32_t L2,
                        const void* g /* (N1, N2) */, void* gX, void* gX2, void* g_weights, int32_t* taken);
int gpsig_seq_diag_levels_grad(gpsig_ctx* ctx, const gpsig_params* p, const void* X, int64_t N, int32_t L,
                               const void* G /* (M+1, N) */, void* gX, double* g_base);
int gpsig_tens_gram_levels_grad(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, int64_t T, int32_t increments,
                                const void* G /* (M+1, T, T) */, void* gZ, double* g_base);
int gpsig_tens_vs_seq_levels_grad(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, const void* X, int64_t T, int64_t N,
                                  int32_t L, int32_t increments, const void* G /* (M+1, T, N) */, void* gZ, void* gX,
                                  double* g_base);

/* Reverse pass of gpsig_tens_vs_seq_weighted: G (T, N) is the upstream gradient of the weighted sum; gZ, gX as above, gfac (N, M+1)
 * the gradient with respect to the factors (through which the level diagonals of the sequences, sigma and the variances are
 * reached: gpsig/kernels.py:572-581, :471).  float64.  aux: device pointer in either pointer mode. */
int gpsig_tens_vs_seq_weighted_grad(gpsig_ctx* ctx, const gpsig_params* p, const void* Z, const void* X, int64_t T, int64_t N,
                                    int32_t L, int32_t increments, const void* fac /* (N, M+1) */, const void* G /* (T, N) */,
                                    const void* aux /* what the forward call wrote, or NULL */, void* gZ, void* gX,
                                    void* gfac /* (N, M+1) */, double* g_base);

/* ---- the recursions on GIVEN increment lattices ("matrix route") ---------------------------------------------------------------
 * What gpsig/signature_algs.py does after it has differenced the base-kernel tensor (:25-26, :55-56 / :114): for callers that
 * build that tensor themselves -- state spaces wider than the gradient kernels' 64 columns, where it is a d-deep contraction and
 * belongs on a library GEMM, and base kernels whose parameters are differentiated outside this library (SignatureSpectral's alpha,
 * omega, gamma: gpsig/kernels.py:912-914).  The lattices of a block of pairs are held in scratch memory (option "grad_scratch_mb"):
 * sized for training minibatches, not for BASELINE-sized Grams.  float64.
 *   dM: (P, R1, R2) increment lattices of P pairs -> out (M+1, P): signature_kern_first_order / _higher_order (:28-35, :58-74), p->order;
 *   m:  (lt, R, P) component increments, pair index fastest -> out (M+1, P): signature_kern_tens_vs_seq_first_order (:116-127), order 1.
 * _grad: G (M+1, P) upstream -> the gradient with respect to dM / m, same layouts. */
int gpsig_lattice_levels(gpsig_ctx* ctx, const gpsig_params* p, const void* dM, int64_t P, int32_t R1, int32_t R2, void* out);
int gpsig_lattice_levels_grad(gpsig_ctx* ctx, const gpsig_params* p, const void* dM, int64_t P, int32_t R1, int32_t R2, const void* G, void* gdM);
int gpsig_chain_levels(gpsig_ctx* ctx, const gpsig_params* p, const void* m, int64_t P, int32_t R, void* out);
int gpsig_chain_levels_grad(gpsig_ctx* ctx, const gpsig_params* p, const void* m, int64_t P, int32_t R, const void* G, void* gm);

#ifdef __cplusplus
}
#endif
#endif /* GPSIG_HIP_H */
