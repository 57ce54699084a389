// sig_feat_api.hip -- the forward side of the feature route: SignatureLinear and SignatureCosine through explicit level features.
//
// For the linear kernel (the cosine kernel: of the unit vectors x / |x|, kernels.py:820-828) level m of a pair is <Phi_m(x), Phi_m(y)> with
// d^m numbers Phi_m per sequence (sig_feat_kernel.hpp), so a Gram is ONE contraction over the feature width on the float64 matrix cores.
// The reverse side and the feature op are sig_feat_grad_api.hip.  Entry points (declared in launchers.hpp, called from api.hip on device pointers):
//     sig_features_K               seq_K_device's first question (K, K_seq_n_seq_covs, gpsig_seq_gram_levels, the row blocks of
//                                  gpsig_kernel_K_symm_rows*): features of both sides (sig_features_kernel), the contraction in depth pieces
//                                  (sig_gram_launch), the pieces added in a fixed order (inside it: sig_gram_fold, or sig_reduce_launch).  float32 calls are widened, computed in
//                                  float64 and rounded.  *done = false leaves the call to the lattice kernels.
//     tvs_features_plan            whether Kzx of this shape is one product of the tensors' and the sequences' level features (a pure predicate:
//                                  the entry points ask it too, to skip the diagonal factors that the features carry themselves)
//     tens_vs_seq_features_device  ... and that product: square_small_kernel, sig_features_kernel, tens_level_features_kernel, one rocBLAS dgemm.
//                                  *done = false: the tile kernel.
// Shared with the reverse side: sig_shape / sig_shape_fits (family, lookup, F, ld; steps and LDS) and sig_launch_features (the one launch).
// What decides the routes: options "sig_features" / "tvs_features" (0 never, 1 wherever built, -1 the time models below, with their measured
// rates); a feature kernel built for (d, M); SIG_FEAT_LDS_MAX; the memory bounds at each site.  A one-column state space takes sig_features_K
// whatever the model says.  Differences between the sites that are meant are marked where they are.
// Scratch:  B_SF0  Phi(X) (N1, ld)                 B_SF1  Phi(X2) (N2, ld) / the tensors' features Zf (Tn, ld)
//           B_SF2  partial sums (pieces, NA, NB)    B_SF3, B_SF4  float32 calls: X, X2 widened      B_SF5  float32 calls: the float64 result
//           B_SFC  the tiles' arrival counters (sig_gram_fold)
//           B_TW2  Kzx: the squared level weights
// "sig_features_keep" remembers what B_SF0 holds (sf_valid, sf_X, sf_phi, sf_key).  Whoever else writes B_SF0 clears sf_valid:
// tens_vs_seq_features_device below, sig_features_grad and sig_features_sum_grad (sig_feat_grad_api.hip); the option's setter does too.
#include "api_common.hpp"
#include "launchers.hpp"
#include "sig_feat_kernel.hpp"

namespace {       // (at global scope, as they were in api.hip: the kernels keep their names)

// ---- the linear / cosine kernel's Kzx as a product of level features (round 4) ------------------------------------------------------
// An inducing tensor's level m is the rank-one tensor z_1 (x) .. (x) z_m (first factor <-> earliest time, signature_algs.py:118-125), and
// K_m(z, x) = <z_1 (x) .. (x) z_m, Phi_m(x)> with the level features of sig_feat_kernel.hpp (every order: :129-160 too).
// Zf[t][k]: the tensors' features in the layout of the sequences' (natural order, level-0 column = 1, zero padding).  ZT / ZS as
// prep_tensors_kernel leaves them: ZT[((t * d + f) * lt + c) * E + e], ZS[(t * lt + c) * E + e] = |z|^2.
static __global__ void tens_level_features_kernel(const double* __restrict__ ZT, const double* __restrict__ ZS, int lt, int E, int d, int64_t Tn,
                                                  int M, int unit, int64_t ld, double* __restrict__ Zf) {
    const int64_t total = Tn * ld;
    for (int64_t e = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; e < total; e += int64_t(gridDim.x) * blockDim.x) {
        const int64_t t = e / ld;
        int k = int(e - t * ld), m = 1, w = d, off = 0;
        while (m <= M && k >= off + w) { off += w; ++m; w *= d; }
        double v;
        if (m > M) {
            v = k == off ? 1.0 : 0.0;                                 // level 0, then the padding
        } else {
            int idx = k - off;
            const int c0 = m * (m - 1) / 2;
            v = 1.0;
            for (int j = m - 1; j >= 0; --j) {                        // last index fastest = the component paired with the latest time
                const int f = idx % d;
                idx /= d;
                const int c = c0 + j;
                double z = ZT[((t * d + f) * lt + c) * E + (E - 1)];
                if (unit) z *= rsqrt(ZS[(t * lt + c) * E + (E - 1)]);  // SignatureCosine: unit vectors (kernels.py:820-828)
                if (E == 2) {                                         // increments: k(z1, x) - k(z0, x) is linear in z (kernels.py:329-330)
                    double z0 = ZT[((t * d + f) * lt + c) * E];
                    if (unit) z0 *= rsqrt(ZS[(t * lt + c) * E]);
                    z -= z0;
                }
                v *= z;
            }
        }
        Zf[e] = v;
    }
}

static __global__ void square_small_kernel(const double* __restrict__ a, int n, double* __restrict__ b) {
    if (int(threadIdx.x) < n) b[threadIdx.x] = a[threadIdx.x] * a[threadIdx.x];
}

}  // namespace

namespace gpsig {

static_assert(SG_BM == SIG_PIECE_TILE && SG_BN == SIG_PIECE_TILE, "sig_piece_counts counts the contraction's tiles");

bool sig_shape(const gpsig_params* p, int d, SigShape* s) {
    // the linear kernel, and the cosine kernel as the linear kernel of the unit vectors x / |x| (kernels.py:820-828)
    s->cosine = p->base_kernel == GPSIG_BASE_COSINE;
    s->d = d; s->M = p->num_levels;
    if (!(p->base_kernel == GPSIG_BASE_LINEAR || s->cosine)) return false;
    s->ffn = sig_feat_lookup(d, s->M);
    if (!s->ffn) return false;
    s->F = sig_feature_count(d, s->M); s->ld = (s->F + 1 + 15) / 16 * 16;
    return true;
}

bool sig_shape_fits(const SigShape& s, const gpsig_params* p, int L) {
    return (p->difference ? L - 1 : L) >= 1 && sig_features_lds_bytes(s.d, s.M, L) <= SIG_FEAT_LDS_MAX;
}

int sig_launch_features(gpsig_ctx* c, const SigShape& s, const gpsig_params* p, const ScaleParams& P, int order, const double* X, int64_t N, int L,
                        const double* w, int normalize, double jitter, int norm_squared, int natural_order, double* Phi, double* dlev) {
    SigFeatArgs A;
    memset(&A, 0, sizeof(A));
    A.X = X; A.N = N; A.L = L; A.difference = p->difference ? 1 : 0; A.P = P;
    A.w = w; A.normalize = normalize; A.jitter = jitter; A.Phi = Phi; A.ld = s.ld; A.dlev = dlev;
    A.order = order; A.unit_points = s.cosine ? 1 : 0; A.norm_squared = norm_squared; A.natural_order = natural_order;
    // (workgroups of one or two wavefronts -- small d^M -- are latency-bound at 16 per CU: up to 16,384 of them; 0.667 -> 0.647 ms at configs[2])
    const int64_t cap = sig_threads(s.d, s.M) <= 128 ? 16384 : 4096;
    hipError_t e = s.ffn(A, unsigned(N < cap ? N : cap), sig_features_lds_bytes(s.d, s.M, L), c->stream);
    if (e != hipSuccess) return fail(c, GPSIG_ERR_HIP, "sig_features_kernel: %s", hipGetErrorString(e));
    return GPSIG_OK;
}

namespace {

// ---- sig_features_K, step by step ---------------------------------------------------------------------------------------------------
// what steps (b) and (c) decide for one call
struct SigGramPlan {
    bool sym, rows, symtiles;
    int64_t N1, N2, NA, NB, H, row_begin;         // the Gram is N1 x (sym ? N1 : N2); this call computes NA x NB of it
    int nti, ntj, ntiles, nsplit, graded;
};

// (a) Taken where it is the cheaper evaluation -- 2 sum_m d^m flops per entry on the matrix cores against the lattice sweep's
// L1 L2 (2d + 3M - 1) on the vector unit at about 0.6 of the GEMM's efficiency -- and a sequence's arrays fit the LDS.
bool sig_gram_route(gpsig_ctx* c, const gpsig_params* p, bool raw, bool sym, bool rows, int64_t N1, int64_t N2, int L1, int L2, int x_squared, SigShape* s) {
    // float32 calls too: computed in float64 (the matrix cores' own precision), inputs widened and the result rounded -- 29 -> 1.4 ms at
    // d = 16, num_levels = 3, and closer to the reference than a float32 recursion; not for row blocks (float64 only)
    const bool f32 = p->dtype == GPSIG_F32;
    if (c->sig_features == 0 || !(p->dtype == GPSIG_F64 || f32)) return false;       // (c->capturing is not asked here, unlike tvs_features_plan and the reverse side: it only keeps step (d) from asking the device)
    if (x_squared && (sym || raw || !p->normalization)) return false;       // (the quirk is a cross Gram's: its X side only)
    if (f32 && rows) return false;
    if (c->shard_n > 1) return false;             // gpsig_set_shard: "entries outside the shard are left untouched" is the pair kernels' contract
    const int M = p->num_levels, d = p->num_features * ((raw ? 0 : p->num_lags) + 1);
    if (p->order < 1 || p->order > M) return false;           // (refused, as tvs_features_plan does; the reverse side clamps the order)
    if (!sig_shape(p, d, s) || !sig_shape_fits(*s, p, L1) || !sig_shape_fits(*s, p, L2)) return false;
    // One-column state spaces take this route whatever the time model says (round 5): the pair recursion's sums over index tuples cancel by
    // orders of magnitude for scalar increments -- the float64 pair kernels AND the float64 CPU restatement are 2e-3 .. 5e-3 from an 80-bit evaluation on
    // case 779 of the round-5 sweep (tests/golden/fuzz_cases_r5.npz) -- while the per-sequence feature sums do not (8.7e-7 there, float32 rounding).
    if (c->sig_features < 0 && d != 1) {
        const int r1 = p->difference ? L1 - 1 : L1, r2 = p->difference ? L2 - 1 : L2;
        // (the higher-order pair kernels carry order^2 grids per level: 34 to 150 times the first order's time at configs[1]'s size)
        const double lattice = double(r1) * r2 * (2.0 * d + 3.0 * M - 1.0) * (p->order > 1 ? 8.0 : 1.0) * (s->cosine ? 1.5 : 1.0) * (f32 ? 0.5 : 1.0), feat = 2.0 * double(s->F);      // (the float32 pair kernels run at twice the float64 ones' rate)
        const double pairs = sym ? double(N1) * N1 / 2 : double(N1) * N2;
        if (!(feat * 0.6 < lattice)) return false;
        // small problems: the contraction is three or four launches with a floor of ~60 us plus its feature kernel (60 us per sequence
        // and CU at 32,768 top-level features), the pair kernels one launch with a floor of ~100 us; rates as measured
        // (tools/bench_crossover.py, profiles/r03_crossover.txt)
        const double seqs = double(N1) + (sym ? 0.0 : double(N2)), t_seq = 60e-6 * double(sig_ipow(d, M)) / 32768.0;
        const double t_feat_kernel = ceil(seqs / 256.0) * t_seq > 15e-6 ? ceil(seqs / 256.0) * t_seq : 15e-6;
        const double t_lattice = 100e-6 + pairs * lattice / (d > 8 ? 12.5e12 : 25e12), t_features = 60e-6 + t_feat_kernel + pairs * feat / 60e12;
        if (pairs < 1024.0 || !(t_features < t_lattice)) return false;
    }
    return true;
}

// (b) row_end > 0: the owned entries of rows [row_begin, row_end) (multi-GPU row blocks): NA rows against the NB sequences from row_begin - H on
SigGramPlan sig_gram_geometry(bool sym, bool rows, int64_t N1, int64_t N2, int64_t row_begin, int64_t row_end) {
    SigGramPlan g;
    g.sym = sym; g.rows = rows; g.N1 = N1; g.N2 = N2; g.row_begin = row_begin;
    g.NA = rows ? row_end - row_begin : N1; g.H = N1 / 2;
    g.NB = sym ? N1 : N2;
    if (rows) g.NB = (g.NA + g.H < N1) ? g.NA + g.H : N1;
    g.nti = int((g.NA + SG_BM - 1) / SG_BM); g.ntj = int((g.NB + SG_BN - 1) / SG_BN);
    g.symtiles = sym && !rows;
    g.ntiles = g.symtiles ? g.nti * (g.nti + 1) / 2 : g.nti * g.ntj;
    g.nsplit = g.graded = 1;          // (step (c) sets them)
    return g;
}

// (d) What the scratch buffers would have to grow by, against what the device has left: the pair recursion needs no such memory
// and is the better answer to a full device than an allocation error.
// (not for row blocks: the ranks of a sharded evaluation must all take the same route whatever each device has left -- there a
// full device is an allocation error of that rank, not a silent change of route that the other ranks do not follow)
struct SigBuf { int id; size_t bytes; };          // (0 bytes: not needed by this call)
bool sig_gram_headroom(const gpsig_ctx* c, const SigBuf (&bufs)[3], bool rows) {
    size_t extra = 0, held = 0;                   // (a buffer that grows is freed first)
    for (const SigBuf& b : bufs)
        if (b.bytes > c->buf[b.id].cap) { extra += b.bytes + b.bytes / 8 + 256; held += c->buf[b.id].cap; }
    if (!(extra > (size_t(1) << 30) && !c->capturing && !rows)) return true;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return true;
    return !(extra > free_b + held - (free_b + held) / 16);
}

// (e) "sig_features_keep": between the calls of ONE decomposed evaluation (the chunks of a rank's row block: parallel.ShardedGram) the
// features of the same sequences under the same parameters are built once.  The caller promises not to write X in between.
uint64_t sig_keep_key(const gpsig_params* p, bool raw, int x_squared, int64_t N1, int L1, int64_t ld) {
    const int32_t head[8] = {p->base_kernel, p->dtype, p->num_features, p->num_levels, p->order, p->difference, p->normalization, p->num_lags};
    const int64_t tail[4] = {N1, L1, (raw ? 1 : 0) + (x_squared ? 2 : 0), ld};
    uint64_t key = fnv1a(FNV1A_BASIS, head, sizeof(head));
    key = fnv1a(fnv1a(key, &p->sigma, sizeof(double)), &p->jitter, sizeof(double));
    key = fnv1a(key, p->variances, sizeof(double) * (p->num_levels + 1));
    if (p->lengthscales) key = fnv1a(key, p->lengthscales, sizeof(double) * p->num_features);
    if (p->num_lags > 0) key = fnv1a(fnv1a(key, p->lags, sizeof(double) * p->num_lags), p->gamma, sizeof(double) * (p->num_lags + 1));
    return fnv1a(key, tail, sizeof(tail));
}

// (f) float32 calls: the sequences widened into B_SF3 / B_SF4, the float64 result in B_SF5 (narrowed after the last level)
int sig_gram_stage_f32(gpsig_ctx* c, const gpsig_params* p, const SigGramPlan& g, int L1, int L2, int return_levels, const void** X, const void** X2,
                       void** out) {
    void *x64, *y64 = nullptr, *o64;
    const int64_t per1 = int64_t(L1) * p->num_features, per2 = int64_t(L2) * p->num_features;
    CHK(ensure(c, B_SF3, sizeof(double) * size_t(g.N1 * per1) + 64, &x64));
    HIPCHK(c, sig_convert_launch(*X, x64, g.N1 * per1, true, c->stream));
    if (!g.sym) {
        CHK(ensure(c, B_SF4, sizeof(double) * size_t(g.N2 * per2) + 64, &y64));
        HIPCHK(c, sig_convert_launch(*X2, y64, g.N2 * per2, true, c->stream));
    }
    CHK(ensure(c, B_SF5, sizeof(double) * size_t(return_levels ? p->num_levels + 1 : 1) * size_t(g.N1) * size_t(g.sym ? g.N1 : g.N2) + 64, &o64));
    *X = x64; *X2 = g.sym ? nullptr : y64; *out = o64;
    return GPSIG_OK;
}

// (g) one contraction and one reduce per level array (return_levels) or for the level sum
int sig_gram_levels(gpsig_ctx* c, const gpsig_params* p, const SigShape& s, const SigGramPlan& g, bool raw, int return_levels, int normalize,
                    const void* phi1, const void* phi2, void* part, void* out, bool timed, int compact) {
    const int M = s.M, d = s.d;
    const int64_t F = s.F, ld = s.ld, N1 = g.N1, NA = g.NA, NB = g.NB, H = g.H, row_begin = g.row_begin, Ncols = g.sym ? N1 : g.N2;
    const bool rows = g.rows;
    // level sums of the weights: the exact diagonal of the normalised symmetric Gram (kernels.py:430-433: (K_ii + jitter) / (K_ii + jitter))
    const int nlev = return_levels ? M + 1 : 1;
    for (int lv = 0; lv < nlev; ++lv) {
        int kb = 0, ke = int(F) + 1;                         // all levels and the level-0 column: the level sum is inside the contraction
        double dval = 0.0;
        if (return_levels) {
            if (lv == 0) { kb = int(F); ke = int(F) + 1; }
            else { kb = sig_feature_count(d, lv - 1); ke = sig_feature_count(d, lv); }
            dval = raw ? 0.0 : p->sigma * p->variances[lv];
        } else {
            for (int m = 0; m <= M; ++m) dval += p->sigma * p->variances[m];
        }
        SigGramArgs G;
        memset(&G, 0, sizeof(G));
        G.A = static_cast<const double*>(phi1) + (rows ? row_begin * ld : 0);
        G.B = static_cast<const double*>(g.sym ? phi1 : phi2);
        G.NA = NA; G.NB = NB; G.lda = ld; G.ldb = ld;
        G.b_off = rows ? ((row_begin - H) % N1 + N1) % N1 : 0; G.b_mod = g.sym ? N1 : g.N2;
        G.k_begin = kb; G.k_end = ke;
        G.band = (rows && NA + H <= N1) ? H : 0;      // column c of the block is sequence row_begin - H + c (no wrap inside the block): row i owns c in [i, i + H]
        const int nslab = (ke - kb + SG_BK - 1) / SG_BK;
        // (the per-level products of return_levels: equal pieces of their own, shorter depth)
        const int ns = sig_piece_bounds(nslab, g.nsplit, return_levels ? 1 : g.graded, G.bound);
        G.nsplit = ns; G.symmetric = g.symtiles ? 1 : 0; G.ntj = g.ntj; G.part = static_cast<double*>(part);
        SigReduceArgs R;
        memset(&R, 0, sizeof(R));
        R.part = static_cast<const double*>(part); R.nsplit = ns; R.NA = NA; R.NB = NB;
        R.out = static_cast<double*>(out) + (return_levels ? int64_t(lv) * N1 * Ncols : 0);
        R.so_i = Ncols; R.so_j = 1;
        R.mode = rows ? 2 : (g.symtiles ? 1 : 0);
        R.diag_set = (g.sym && normalize) ? 1 : 0; R.diag_value = dval;
        R.N = N1; R.r0 = row_begin; R.c0 = G.b_off; R.compact = compact;
        // The one-call symmetric product adds its pieces inside the LDS-DMA kernel (sig_gram_fold): the workgroup that finishes a tile's
        // last piece does what the reduce kernel would, under the multiplies of the others.  Row blocks, general products, the per-level
        // products and the staging kernel keep the reduce kernels.  The tiles' arrival counters are zero when a launch begins: an eager
        // call zeroes them on the stream, in whole 16 bytes from the start of their block (a fresh block, or counters that an
        // abandoned launch left behind), and every tile's last arriver sets its counter back to zero.  A capture records NO memset: with
        // a memset node ahead of the contraction a replayed graph left the result untouched at 10 tiles x 5 pieces (nobody drew a last
        // ticket; tests/test_gpu_graph.py, test_replay_of_the_feature_contraction), without it the replays are the eager call's bits.
        // The block cannot be new inside a capture (a buffer that has to grow refuses it), so the warm-up call has left it zero.
        if (R.mode == 1 && !return_levels && c->sig_gemm_dma) {
            void* cnt = nullptr;
            const size_t cnt_bytes = (sizeof(int) * size_t(g.ntiles) + 15) / 16 * 16;
            CHK(ensure(c, B_SFC, cnt_bytes, &cnt));
            if (ns > 1 && !c->capturing) HIPCHK(c, hipMemsetAsync(cnt, 0, cnt_bytes, c->stream));
            G.fold = 1; G.cnt = static_cast<int*>(cnt);
            G.out = R.out; G.so_i = R.so_i; G.so_j = R.so_j; G.diag_set = R.diag_set; G.diag_value = R.diag_value;
        }
        hipEvent_t e0 = nullptr, e1 = nullptr;
        bool on = false;
        if (timed) CHK(timing_begin(c, &e0, &e1, &on));
        // the LDS-DMA form reads whole slabs: only where the columns behind k_end are the zero padding of the feature rows
        int used_dma = 0, folded = 0;
        HIPCHK(c, sig_gram_launch(G, g.ntiles, c->stream, (c->sig_gemm_dma && !return_levels) ? 1 : 0, &used_dma, &folded));
        if (on) {
            HIPCHK(c, hipEventRecord(e1, c->stream));
            c->t_launches += 1;
            c->t_pairs += NA * NB;
            c->t_kernel = used_dma ? "sig_gram_dma_kernel" : "sig_gram_kernel";
            // what is executed: the LDS-DMA form computes 36 of the 64 16 x 16 blocks of a symmetric product's diagonal tiles
            const double tiles_done = double(g.ntiles) - ((used_dma && g.symtiles) ? double(g.nti) * 28.0 / 64.0 : 0.0);
            c->t_flops += 2.0 * tiles_done * SG_BM * SG_BN * double(nslab) * SG_BK;
        }
        if (!folded) HIPCHK(c, sig_reduce_launch(R, c->stream));
    }
    return GPSIG_OK;
}

}  // namespace

// ---- SignatureLinear / SignatureCosine: the Gram as a contraction of explicit level features (sig_feat_kernel.hpp) ------------------
int sig_features_K(gpsig_ctx* c, const gpsig_params* p, bool raw, const void* X, const void* X2, int64_t N1, int64_t N2, int L1, int L2,
                   int return_levels, void* out, bool timed, int x_squared, int64_t row_begin, int64_t row_end, int compact, bool* done,
                   bool row_block_call) {
    *done = false;
    const bool sym = X2 == nullptr, f32 = p->dtype == GPSIG_F32;
    // (row_block_call: an EMPTY row block -- a rank that owns no rows -- takes the decisions of a non-empty one and returns before launching)
    const bool rows = row_end > 0 || row_block_call;
    SigShape s;
    if (!sig_gram_route(c, p, raw, sym, rows, N1, N2, L1, L2, x_squared, &s)) return GPSIG_OK;                  // (a)
    SigGramPlan g = sig_gram_geometry(sym, rows, N1, N2, row_begin, row_end);                                  // (b)
    const int nslab_all = int((s.ld + SG_BK - 1) / SG_BK);
    sig_piece_counts(N1, N2, sym, nslab_all, c->sig_graded != 0, &g.nsplit, &g.graded);                        // (c)
    // the exception to that model's rule: 40 GiB of partial sums -- of THIS call's NA x NB entries, not of the full problem
    const size_t part_one = sizeof(double) * size_t(g.NA) * g.NB;
    while (g.nsplit > 1 && part_one * size_t(g.nsplit - 1 + g.graded) > (size_t(40) << 30)) { --g.nsplit; g.graded = 1; }
    const int npieces = g.nsplit - 1 + g.graded;
    const size_t feat_bytes = sizeof(double) * size_t(s.ld) * (size_t(N1) + (sym ? 0 : size_t(N2)));
    if (feat_bytes + part_one * size_t(npieces) > (size_t(96) << 30)) return GPSIG_OK;
    const SigBuf bufs[3] = {{B_SF0, sizeof(double) * size_t(s.ld) * N1 + 64}, {B_SF1, sym ? 0 : sizeof(double) * size_t(s.ld) * N2 + 64},
                            {B_SF2, part_one * size_t(npieces) + 64}};
    if (!sig_gram_headroom(c, bufs, rows)) return GPSIG_OK;                                                     // (d)
    if (rows && g.NA <= 0) { *done = true; return GPSIG_OK; }        // an empty row block: the route is decided, there is nothing to compute
    const double* w = nullptr;
    if (!raw) CHK(upload_weights(c, p, &w));
    ScaleParams sp;
    CHK(scale_params(c, p, !raw, &sp));
    void* dev[3] = {nullptr, nullptr, nullptr};       // phi1, phi2, part
    for (int i = 0; i < 3; ++i)
        if (bufs[i].bytes) CHK(ensure(c, bufs[i].id, bufs[i].bytes, &dev[i]));
    void* const phi1 = dev[0];
    void* out32 = nullptr;                    // float32 calls: where the rounded result goes
    const void* const X_given = X;            // (the caller's pointer: what "sig_features_keep" recognises)
    if (f32) {                                                                                                  // (f)
        out32 = out;
        CHK(sig_gram_stage_f32(c, p, g, L1, L2, return_levels, &X, &X2, &out));
    }
    const int normalize = (!raw && p->normalization) ? 1 : 0;
    const uint64_t key = sig_keep_key(p, raw, x_squared, N1, L1, s.ld);                                         // (e)
    const bool reuse = c->sf_keep && c->sf_valid && c->sf_X == X_given && c->sf_phi == phi1 && c->sf_key == key;
    // (natural_order = 0, where the Kzx product and the reverse side ask for 1: both sides of this contraction come from the same kernel, in its own order)
    if (N1 > 0 && !reuse)
        CHK(sig_launch_features(c, s, p, sp, p->order, static_cast<const double*>(X), N1, L1, w, normalize, p->jitter, x_squared ? 1 : 0, 0,
                                static_cast<double*>(phi1), nullptr));
    c->sf_valid = c->sf_keep != 0 && N1 > 0;
    c->sf_X = X_given; c->sf_phi = phi1; c->sf_key = key;
    if (!sym && N2 > 0)
        CHK(sig_launch_features(c, s, p, sp, p->order, static_cast<const double*>(X2), N2, L2, w, normalize, p->jitter, 0, 0,
                                static_cast<double*>(dev[1]), nullptr));
    if (g.NA <= 0 || g.NB <= 0) { *done = true; return GPSIG_OK; }
    CHK(sig_gram_levels(c, p, s, g, raw, return_levels, normalize, phi1, dev[1], dev[2], out, timed, compact));  // (g)
    if (out32) HIPCHK(c, sig_convert_launch(out, out32, int64_t(return_levels ? s.M + 1 : 1) * N1 * (sym ? N1 : N2), false, c->stream));
    *done = true;
    return GPSIG_OK;
}

// f64: the call's element type (Kzx of a float32 call stays on the pair kernels)
bool tvs_features_plan(gpsig_ctx* c, const gpsig_params* p, bool f64, int64_t Tn, int64_t N, int L) {
    if (!f64 || c->tvs_features == 0 || routes_as_captured(c)) return false;         // (inside a capture the route is refused outright, as on the reverse side)
    const int M = p->num_levels;
    if (p->order < 1 || p->order > M || Tn <= 0 || N <= 0 || Tn > 0x3fffffff || N > 0x3fffffff) return false;       // (the order: refused, as sig_features_K does)
    SigShape s;
    if (!sig_shape(p, p->num_features * (p->num_lags + 1), &s) || !sig_shape_fits(s, p, L)) return false;
    for (int m = 0; m <= M; ++m)
        if (!(p->sigma * p->variances[m] >= 0.0)) return false;             // (the weights go in squared: sqrt(w^2 / (diag + jitter)))
    if (sizeof(double) * size_t(s.ld) * (size_t(N) + size_t(Tn)) > (size_t(16) << 30)) return false;
    if (c->tvs_features < 0) {
        // rates as measured at BASELINE configs[2] (512 x 16,384, L = 50, d = 6, M = 4): the tile kernel 1.05 ms, here 0.18 + 0.42 ms
        const int lt = M * (M + 1) / 2;
        const double t_tile = 40e-6 + double(Tn) * double(N) * L * lt / 4.0e12;
        const double t_seq = 60e-6 * double(sig_ipow(s.d, M)) / 32768.0, rounds = ceil(double(N) / 256.0);
        const double t_feat = 80e-6 + (rounds * t_seq > 15e-6 ? rounds * t_seq : 15e-6) + 2.0 * double(Tn) * double(N) * double(s.ld) / 50e12;
        if (!(t_feat < t_tile)) return false;
    }
    return true;
}

// Kzx = sum_m w_m / sqrt(K_m(x, x) + jitter) K_m(z, x) (kernels.py:572-588) of the linear / cosine kernel as ONE product of the tensors' and the
// sequences' level features (rocBLAS dgemm): the weights and the normalisation ride on the sequences' features.  *done = false: the tile kernel.
int tens_vs_seq_features_device(gpsig_ctx* c, const gpsig_params* p, bool f64, const void* ZT, const void* ZS, const void* X, int64_t Tn, int64_t N,
                                int L, int increments, const double* w, void* out, bool* done) {
    *done = false;
    if (!tvs_features_plan(c, p, f64, Tn, N, L)) return GPSIG_OK;
    SigShape s;
    sig_shape(p, p->num_features * (p->num_lags + 1), &s);            // (the plan has said yes to it)
    const int M = s.M;
    const int64_t ld = s.ld;
    void *phi, *zf, *w2;
    CHK(ensure(c, B_SF0, sizeof(double) * size_t(ld) * N + 64, &phi));
    CHK(ensure(c, B_SF1, sizeof(double) * size_t(ld) * Tn + 64, &zf));
    CHK(ensure(c, B_TW2, sizeof(double) * 16, &w2));
    c->sf_valid = false;                          // (B_SF0 no longer holds what "sig_features_keep" remembers)
    hipLaunchKernelGGL(square_small_kernel, dim3(1), dim3(64), 0, c->stream, w, M + 1, static_cast<double*>(w2));
    HIPCHK(c, hipGetLastError());
    ScaleParams sp;
    CHK(scale_params(c, p, true, &sp));
    CHK(sig_launch_features(c, s, p, sp, p->order, static_cast<const double*>(X), N, L, static_cast<const double*>(w2), p->normalization ? 1 : 0,
                            p->jitter, 0, 1, static_cast<double*>(phi), nullptr));
    hipLaunchKernelGGL(tens_level_features_kernel, dim3(grid_for(Tn * ld)), dim3(256), 0, c->stream, static_cast<const double*>(ZT),
                       static_cast<const double*>(ZS), M * (M + 1) / 2, increments ? 2 : 1, s.d, Tn, M, s.cosine ? 1 : 0, ld, static_cast<double*>(zf));
    HIPCHK(c, hipGetLastError());
    hipEvent_t e0, e1;
    bool timed;
    CHK(timing_begin(c, &e0, &e1, &timed));
    // row-major out (T, N) = Zf (T, ld) Phi (N, ld)^T  ==  column-major out^T (N x T) = Phi_cm^T (N x ld) Zf_cm (ld x T)
    std::string err;
    if (!solver_dgemm(&c->blas_handle, c->stream, true, false, int(N), int(Tn), int(ld), 1.0, static_cast<const double*>(phi), int(ld),
                      static_cast<const double*>(zf), int(ld), 0.0, static_cast<double*>(out), int(N), &err))
        return fail(c, GPSIG_ERR_HIP, "%s", err.c_str());
    if (timed) {
        HIPCHK(c, hipEventRecord(e1, c->stream));
        c->t_launches += 1;
        c->t_pairs += Tn * N;
        c->t_kernel = "tvs_features_dgemm";
        c->t_flops += 2.0 * double(Tn) * double(N) * double(ld);
    }
    *done = true;
    return GPSIG_OK;
}

}  // namespace gpsig
