// lr_api.hip -- the low-rank evaluation path: features of sequences and of inducing tensors from landmarks, whitening and projections that the
// CALLER owns (host arrays, or a gpsig_lr_draw state on the device), their Gram products, and the draw itself.  (The training path, lr_grad_api.hip,
// takes landmarks and whitening as device pointers: there they are functions of the trained parameters.)  Entry points:
//     gpsig_lr_gather_points, gpsig_base_kernel_matrix, gpsig_lr_whitening     the pieces of a host-side draw (gpsig_amd/low_rank.py)
//     gpsig_lr_seq_features / _ragged / _ragged_lagged                         sequences (N, L, d): lr_seq_features, then lr_seq_features_t
//     gpsig_lr_tens_features                                                  inducing tensors (lt, T, E, d'): lr_tens_features_t
//     gpsig_lr_kernel, gpsig_lr_kernel_diag                                    Gram products of feature matrices (lr_kernel_t, lr_kernel_diag_t)
//     gpsig_lr_draw, gpsig_lr_state_destroy / _sizes / _export                 the device-side draw (lr_draw_kernels.hpp) and its state
// The routes of a feature call, and where each one's rule lives (all in lr_tile_plan.hpp; the host code here asks, it does not restate):
//     fused         one workgroup per sequence / tensor, intermediates in LDS (lr_fused_kernel.hpp)          lr_eval_route, lr_eval_tens_route
//     tiled         sequences beyond the fused kernels and every ragged batch: 64-step tiles (lr_eval_tiled.hpp)     lr_eval_route
//     wide          state spaces beyond every kernel that holds the points in LDS: the Nystrom cross matrix from the matrix cores in chunks,
//                   then feature kernels that read it from memory (lr_eval_wide.hpp)                           lr_eval_route, lr_eval_tens_route
//     spectral wide the same two loops for SignatureSpectral beyond the 32 columns of its packed table, for a kernel object that opts in
//                   (spectral_wide: base_params[2] != 0), with the spectral cross kernel's evaluation form in the cross launcher's place
//                   (lr_eval_spectral_wide.hpp)                                                 lr_spectral_eval_wide, lr_spectral_eval_tens_wide
//     multi-pass    one kernel per reference op (lowrank_kernels.hpp), float64 only: lr_fused = 0, or nothing above fits     what the rules leave
// A feature call decides its route, refuses, and only then stages: lr_upload, in_dev, out_dev happen once per call, after every refusal.
// What the routes share:
//     LrDev, lr_upload / lr_state_dev   the device view of a gpsig_lowrank: host arrays uploaded by content (ContentUpload, ctx.hpp; the
//                                       projections hashed by fnv1a_sketch as lr_grad_api.hip's upload_sketches hashes them) or a drawn state as it is
//     lr_state_args                     what a feature kernel reads of the state, in the call's float type
//     lr_seq_args                       the fields the fused and the tiled sequence kernels' argument blocks have in common
//     lr_wide_open, lr_spectral_wide_open     what the wide loops set up before their first chunk
//     lr_gemm, lr_level_offsets         the Gram products' and the multi-pass routes' GEMM (A B^T), the level boundaries of a row of Phi
//     landmark_gram                     kappa(S, S) for a whitening, from the packed spectral table or -- spectral_wide -- the (Q, d) one
// Scratch: B_LR0 landmarks, whitening and projections of a host state (lr_upload); B_LR1 the level offsets; B_LR2 the wide routes' chunk of kxs /
// kzs, the multi-pass routes' kxs, the Gram products' A-side level factors; B_LR3 the landmarks' norms (wide), feat (multi-pass), B-side factors;
// B_LR4 gamma^2 and the landmarks' norms and phases (spectral wide), U (multi-pass), the scaled A side; B_LR5 / B_LR6 the multi-pass routes' two
// running products, B_LR5 the scaled B side; B_LR7 the transposed whitening of a host state (multi-pass); B_LR2 .. B_LR5 also hold the operands of
// gpsig_lr_gather_points, gpsig_base_kernel_matrix and gpsig_lr_whitening.  B_LRF32: the state narrowed to float32, once per float32 call.
// B_SPECW: SignatureSpectral's table in its own (Q, d) layout (B_SPEC, the packed one, is api.hip's spectral_table).  B_LR8 belongs to the training
// path.  check_params, scale_params, spectral_table, base_p, upload_weights and the ENTER macros are api.hip's (api_common.hpp).
#include <algorithm>
#include <new>
#include <type_traits>

#include "api_common.hpp"
#include "launchers.hpp"
#include "aux_kernels.hpp"
#include "lowrank_kernels.hpp"
#include "lr_fused_args.hpp"
#include "lr_eval_tiled.hpp"
#include "lr_eval_wide.hpp"
#include "lr_eval_spectral_wide.hpp"
#include "lr_draw_kernels.hpp"

using namespace gpsig;

void gpsig::lr_detach_states(gpsig_ctx* c) {
    for (gpsig_lr_state* st : c->lr_states) { st->device = c->device; st->ctx = nullptr; }
}

namespace {

// BASE_SPECTRAL beyond SPECTRAL_STRIDE columns with the kernel object's opt-in: the calls that take the kernels of lr_eval_spectral_wide_inst.hip
bool spectral_wide(const gpsig_params* p) {
    return p->base_kernel == GPSIG_BASE_SPECTRAL && p->base_params[2] != 0.0 && p->num_features > SPECTRAL_STRIDE;
}

}  // namespace

// ... and their table: alpha[Q], omega[Q][d], gamma[Q][d] as the caller holds it, on the device in B_SPECW.  Compared in full and uploaded only
// when changed, as api.hip's spectral_table; a change refuses the replays of recorded graphs in the same way.  (Exact mode's wide route takes the
// same table: wide_api.hip.)
int gpsig::spectral_table_wide(gpsig_ctx* c, const gpsig_params* p, const double** dev) {
    const size_t n = size_t(p->base_table_len);
    void* dp;
    CHK(ensure(c, B_SPECW, sizeof(double) * n, &dp));
    if (!(c->spec_wide_base == dp && c->last_spec_wide.size() == n && memcmp(c->last_spec_wide.data(), p->base_table, sizeof(double) * n) == 0)) {
        CHK(no_capture(c, "the spectral kernel's table changed"));
        ++c->alloc_gen;                  // a recorded graph read the old contents of this buffer: its replays are refused from here on
        c->spec_wide_base = nullptr;
        c->last_spec_wide.assign(p->base_table, p->base_table + n);
        HIPCHK(c, hipMemcpyAsync(dp, c->last_spec_wide.data(), sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
        CHK(host_sync(c));
        c->spec_wide_base = dp;
    }
    *dev = static_cast<const double*>(dp);
    return GPSIG_OK;
}

namespace {

// kappa(A, B) (na, nb) of rows of d columns for a landmark Gram (gpsig_lr_whitening, gpsig_lr_draw, gpsig_base_kernel_matrix): the thread-per-pair
// kernel of every family on the packed table, or -- spectral_wide -- its twin with row stride d
int landmark_gram(gpsig_ctx* c, const gpsig_params* p, const double* A, const double* B, int64_t na, int64_t nb, int d, double* out) {
    if (spectral_wide(p)) {
        const double* tab;
        CHK(spectral_table_wide(c, p, &tab));
        const int rc = lr_spx_gram_launch(c->stream, A, B, na, nb, d, int(p->base_params[0]), int(p->base_params[1]), tab, out);
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral landmark Gram: %s", hipGetErrorString(hipError_t(rc)));
        return GPSIG_OK;
    }
    const double* spec;
    CHK(spectral_table(c, p, &spec));
    hipLaunchKernelGGL(base_kernel_matrix_kernel<double>, dim3(grid_for(na * nb)), dim3(256), 0, c->stream, A, B, na, nb, d, int(p->base_kernel),
                       p->base_params[0], p->base_params[1], spec, out);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

// ---- the state (float64; float32 features and Grams are computed from a float64 state) ------------------------------------------
struct LrDev {                 // device copies of a gpsig_lowrank
    const double* S; const double* Wh;
    int c, r, nsk;
    std::vector<const int32_t*> colptr, i1, i2;
    std::vector<const double*> val;
    std::vector<const LrEntry*> ent;        // the same entries packed (value, i1, i2) for the fused feature kernel
    std::vector<int64_t> nent;              // entries of ent[i] that may be read (nnz; the capacity for a device-drawn state)
    std::vector<int> k1, k2;
};

// entries a projection is given room for: the expected number plus twelve standard deviations (never more than all of them)
int32_t lr_sketch_capacity(int64_t D, int r, int sparsity) {
    if (sparsity == 2) return int32_t(r);
    const double s = sparsity == 0 ? sqrt(double(D)) : double(D) / log(double(D));
    const double mean = double(D) * r / (s < 1.0 ? 1.0 : s);
    double cap = mean + 12.0 * sqrt(mean) + 64.0;
    if (cap > double(D) * r) cap = double(D) * r;
    return int32_t(cap);
}

int lr_state_layout(gpsig_lr_state* st) {
    using gpsig::LrEntry;
    size_t o = 0;
    auto take = [&](size_t n, size_t align = 16) { o = (o + align - 1) / align * align; const size_t at = o; o += n; return at; };
    const int c = st->c;
    const size_t o_idx = take(sizeof(int64_t) * (size_t(c) + size_t(st->r) + 8));
    const size_t o_S = take(sizeof(double) * size_t(c) * st->d_eff);
    const size_t o_jd = take(sizeof(double) * c), o_W = take(sizeof(double) * size_t(c) * c), o_Wh = take(sizeof(double) * size_t(c) * c);
    const size_t o_WhT = take(sizeof(double) * size_t(c) * c), o_ev = take(sizeof(double) * c), o_work = take(sizeof(double) * c);
    const size_t o_info = take(sizeof(int) * 4);
    size_t o_sk[gpsig::LR_FUSED_MAX_SKETCHES][6];
    int k2 = c;
    for (int i = 0; i < st->nsk; ++i) {
        gpsig_lr_state::Sk& s = st->sk[i];
        s.k1 = c; s.k2 = k2;
        s.cap = lr_sketch_capacity(int64_t(c) * k2, st->r, st->sparsity);
        o_sk[i][0] = take(sizeof(int32_t) * (size_t(st->r) + 1));
        o_sk[i][1] = take(sizeof(int32_t) * (size_t(st->r) + 1));
        o_sk[i][2] = take(sizeof(int32_t) * size_t(s.cap));
        o_sk[i][3] = take(sizeof(int32_t) * size_t(s.cap));
        o_sk[i][4] = take(sizeof(double) * size_t(s.cap));
        o_sk[i][5] = take(sizeof(LrEntry) * (size_t(s.cap) + 1));
        k2 = st->r;
    }
    if (o > st->bytes) {
        if (st->block) { (void)hipStreamSynchronize(st->ctx->stream); (void)hipFree(st->block); st->block = nullptr; st->bytes = 0; }
        if (hipMalloc(&st->block, o + 256) != hipSuccess) return GPSIG_ERR_NOMEM;
        st->bytes = o + 256;
    }
    char* b = static_cast<char*>(st->block);
    st->idx = reinterpret_cast<int64_t*>(b + o_idx);
    st->S = reinterpret_cast<double*>(b + o_S); st->jd = reinterpret_cast<double*>(b + o_jd); st->W = reinterpret_cast<double*>(b + o_W);
    st->Wh = reinterpret_cast<double*>(b + o_Wh); st->WhT = reinterpret_cast<double*>(b + o_WhT); st->ev = reinterpret_cast<double*>(b + o_ev);
    st->work = reinterpret_cast<double*>(b + o_work); st->info = reinterpret_cast<int*>(b + o_info);
    for (int i = 0; i < st->nsk; ++i) {
        gpsig_lr_state::Sk& s = st->sk[i];
        s.counts = reinterpret_cast<int32_t*>(b + o_sk[i][0]); s.colptr = reinterpret_cast<int32_t*>(b + o_sk[i][1]);
        s.i1 = reinterpret_cast<int32_t*>(b + o_sk[i][2]); s.i2 = reinterpret_cast<int32_t*>(b + o_sk[i][3]);
        s.val = reinterpret_cast<double*>(b + o_sk[i][4]); s.ent = reinterpret_cast<LrEntry*>(b + o_sk[i][5]);
    }
    return GPSIG_OK;
}

// the LrDev view of a device-resident state (what lr_upload builds from host arrays)
void lr_state_dev(const gpsig_lr_state* st, LrDev* D) {
    D->c = st->c; D->r = st->r; D->nsk = st->nsk;
    D->S = st->S; D->Wh = st->Wh;
    for (int i = 0; i < st->nsk; ++i) {
        D->colptr.push_back(st->sk[i].colptr); D->i1.push_back(st->sk[i].i1); D->i2.push_back(st->sk[i].i2);
        D->val.push_back(st->sk[i].val); D->ent.push_back(st->sk[i].ent); D->nent.push_back(st->sk[i].cap);
        D->k1.push_back(st->sk[i].k1); D->k2.push_back(st->sk[i].k2);
    }
}

int lr_check(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr) {
    if (!lr) return fail(c, GPSIG_ERR_INVALID, "lowrank descriptor is NULL");
    if (p->order != 1 && p->num_levels > 1) return fail(c, GPSIG_ERR_UNSUPPORTED, "Low-rank mode not implemented for order higher than 1.");
    if (lr->num_components < 1 || lr->rank_bound < 1) return fail(c, GPSIG_ERR_INVALID, "num_components and rank_bound must be positive");
    if (lr->num_sketches != p->num_levels - 1) return fail(c, GPSIG_ERR_INVALID, "need one sketch per level 2..num_levels");
    if (lr->device_state) {                  // drawn on the device (gpsig_lr_draw): nothing on the host to check
        const gpsig_lr_state* st = lr->device_state;
        if (st->ctx != c) return fail(c, GPSIG_ERR_INVALID, "the low-rank state belongs to another context");
        if (st->c != lr->num_components || st->r != lr->rank_bound || st->nsk != lr->num_sketches)
            return fail(c, GPSIG_ERR_INVALID, "the low-rank state was drawn for other sizes");
        return GPSIG_OK;
    }
    if (!lr->landmarks || !lr->whitening || (lr->num_sketches > 0 && !lr->sketches)) return fail(c, GPSIG_ERR_INVALID, "NULL low-rank array");
    int k2 = lr->num_components;
    for (int i = 0; i < lr->num_sketches; ++i) {
        const gpsig_sketch& sk = lr->sketches[i];
        if (sk.k1 != lr->num_components || sk.k2 != k2 || sk.r != lr->rank_bound)
            return fail(c, GPSIG_ERR_INVALID, "sketch %d has shape (%d, %d) -> %d, expected (%d, %d) -> %d", i, sk.k1, sk.k2, sk.r,
                        lr->num_components, k2, lr->rank_bound);
        k2 = lr->rank_bound;
    }
    return GPSIG_OK;
}

// upload landmarks, whitening and sketches into one scratch block -- unless the block already holds exactly these (content hash):
// the random objects of one evaluation go through several calls, and every upload is a host synchronisation
int lr_upload(gpsig_ctx* c, const gpsig_lowrank* lr, int d_eff, LrDev* D) {
    if (lr->device_state) {                  // already where the kernels read it
        if (lr->device_state->d_eff != d_eff) return fail(c, GPSIG_ERR_INVALID, "the low-rank state was drawn for %d columns, the call has %d", lr->device_state->d_eff, d_eff);
        lr_state_dev(lr->device_state, D);
        return GPSIG_OK;
    }
    const int cc = lr->num_components;
    uint64_t hsh = FNV1A_BASIS;
    const int64_t dims[4] = {cc, d_eff, lr->rank_bound, lr->num_sketches};
    hsh = fnv1a(hsh, dims, sizeof(dims));
    hsh = fnv1a(hsh, lr->landmarks, sizeof(double) * size_t(cc) * d_eff);
    hsh = fnv1a(hsh, lr->whitening, sizeof(double) * size_t(cc) * cc);
    for (int i = 0; i < lr->num_sketches; ++i) hsh = fnv1a_sketch(hsh, lr->sketches[i]);
    size_t bytes = sizeof(double) * (size_t(cc) * d_eff + size_t(cc) * cc);
    for (int i = 0; i < lr->num_sketches; ++i)
        bytes += sizeof(int32_t) * (size_t(lr->sketches[i].r) + 1 + 2 * size_t(lr->sketches[i].nnz)) + sizeof(double) * size_t(lr->sketches[i].nnz) +
                 sizeof(LrEntry) * size_t(lr->sketches[i].nnz) + 96;
    ContentUpload up(c->lr_cache);
    CHK(up.open(c, B_LR0, bytes + 64, hsh, size_t(2 + 5 * lr->num_sketches)));
    D->c = cc; D->r = lr->rank_bound; D->nsk = lr->num_sketches;
    D->S = up.place<double>(lr->landmarks, sizeof(double) * size_t(cc) * d_eff, 8);
    D->Wh = up.place<double>(lr->whitening, sizeof(double) * size_t(cc) * cc, 8);
    for (int i = 0; i < lr->num_sketches; ++i) {
        const gpsig_sketch& sk = lr->sketches[i];
        D->colptr.push_back(up.place<int32_t>(sk.colptr, sizeof(int32_t) * (size_t(sk.r) + 1), 8));
        D->i1.push_back(up.place<int32_t>(sk.i1, sizeof(int32_t) * size_t(sk.nnz), 8));
        D->i2.push_back(up.place<int32_t>(sk.i2, sizeof(int32_t) * size_t(sk.nnz), 8));
        D->val.push_back(up.place<double>(sk.val, sizeof(double) * size_t(sk.nnz), 8));
        std::vector<LrEntry> packed;
        if (!up.cached) {
            packed.resize(size_t(sk.nnz) + 1);
            for (int64_t e = 0; e < sk.nnz; ++e) packed[size_t(e)] = LrEntry{sk.val[e], sk.i1[e], sk.i2[e]};
        }
        D->ent.push_back(up.place<LrEntry>(packed.data(), sizeof(LrEntry) * size_t(sk.nnz), 16));
        D->nent.push_back(sk.nnz);
        D->k1.push_back(sk.k1); D->k2.push_back(sk.k2);
    }
    return up.commit(c, "the low-rank objects changed and have to be uploaded");
}

// the whitening transposed, as the multi-pass routes' GEMM reads it (feat = kxs Wh = kxs (Wh^T)^T): a device-drawn state keeps one,
// a host state's is made here into B_LR7
int lr_whitening_t(gpsig_ctx* c, const gpsig_lowrank* lr, int cc, const double** wht) {
    void* d;
    CHK(ensure(c, B_LR7, sizeof(double) * size_t(cc) * cc + 8, &d));
    if (lr->device_state) {
        *wht = lr->device_state->WhT;
        return GPSIG_OK;
    }
    std::vector<double> t(size_t(cc) * cc);
    for (int a = 0; a < cc; ++a)
        for (int b = 0; b < cc; ++b) t[size_t(b) * cc + a] = lr->whitening[size_t(a) * cc + b];
    HIPCHK(c, hipMemcpyAsync(d, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, c->stream));
    CHK(host_sync(c));
    *wht = static_cast<const double*>(d);
    return GPSIG_OK;
}

int lr_gemm(gpsig_ctx* c, const double* A, const double* B, int64_t N1, int64_t N2, int K, int64_t lda, int64_t ldb, double* C_,
            int64_t ldc) {
    if (N1 <= 0 || N2 <= 0) return GPSIG_OK;
    if (c->lr_gemm != 0 && N1 * N2 >= int64_t(GEMM_BM) * GEMM_BN) {       // 128 x 128 tiles through LDS
        dim3 grid((unsigned)((N2 + GEMM_BN - 1) / GEMM_BN), (unsigned)((N1 + GEMM_BM - 1) / GEMM_BM));
        hipLaunchKernelGGL(gemm_abt_f64_tiled_kernel, grid, dim3(256), 0, c->stream, A, B, N1, N2, K, lda, ldb, C_, ldc);
        HIPCHK(c, hipGetLastError());
        return GPSIG_OK;
    }
    dim3 grid((unsigned)((N2 + 63) / 64), (unsigned)((N1 + 63) / 64));
    hipLaunchKernelGGL(gemm_abt_f64_mfma_kernel, grid, dim3(256), 0, c->stream, A, B, N1, N2, K, lda, ldb, C_, ldc);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

// where level m's features start in a row of Phi: off[m] .. off[m + 1], F = off[M + 1]
std::vector<int32_t> lr_level_offsets_host(int M, int cc, int r) {
    std::vector<int32_t> off(M + 2);
    off[0] = 0; off[1] = 1;
    if (M >= 1) off[2] = 1 + cc;
    for (int m = 2; m <= M; ++m) off[m + 1] = off[m] + r;
    return off;
}

// ... and their device copy in B_LR1
int lr_level_offsets(gpsig_ctx* c, int M, int cc, int r, const int32_t** dev_off, int* F) {
    const std::vector<int32_t> off = lr_level_offsets_host(M, cc, r);
    *F = off[M + 1];
    void* d;
    CHK(ensure(c, B_LR1, sizeof(int32_t) * off.size(), &d));
    if (!(c->lr_off_base == d && c->lr_off_key[0] == M && c->lr_off_key[1] == cc && c->lr_off_key[2] == r)) {     // (M, c, r) define them
        CHK(no_capture(c, "the low-rank level offsets have to be uploaded"));
        ++c->alloc_gen;                  // a recorded graph read the old contents of this buffer: its replays are refused from here on
        c->lr_off_base = nullptr;
        HIPCHK(c, hipMemcpyAsync(d, off.data(), sizeof(int32_t) * off.size(), hipMemcpyHostToDevice, c->stream));
        CHK(host_sync(c));
        c->lr_off_base = d; c->lr_off_key[0] = M; c->lr_off_key[1] = cc; c->lr_off_key[2] = r;
    }
    *dev_off = static_cast<const int32_t*>(d);
    return GPSIG_OK;
}

// ---- float32 calls.  The state (landmarks, whitening, projections) stays float64 -- drawn and whitened in float64 --; what the float32 feature
// kernels read of it, and the spectral table, are narrowed on the device once per call into B_LRF32.
int lr_gemm(gpsig_ctx* c, const float* A, const float* B, int64_t N1, int64_t N2, int K, int64_t lda, int64_t ldb, float* C_, int64_t ldc) {
    if (N1 <= 0 || N2 <= 0) return GPSIG_OK;
    dim3 grid((unsigned)((N2 + GEMM_BN - 1) / GEMM_BN), (unsigned)((N1 + GEMM_BM - 1) / GEMM_BM));
    hipLaunchKernelGGL(gemm_abt_f32_tiled_kernel, grid, dim3(256), 0, c->stream, A, B, N1, N2, K, lda, ldb, C_, ldc);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

// what the fused kernels read of the state: float64 where lr_upload put it, float32 narrowed on the device once per call into B_LRF32
template <typename Args>
int lr_state_args(gpsig_ctx* c, const gpsig_params* p, const LrDev& D, int d_eff, const double* spec, Args* A) {
    if constexpr (std::is_same<typename Args::value_type, double>::value) {
        A->S = D.S; A->Wh = D.Wh; A->spec = spec;
        for (int i = 0; i < D.nsk; ++i) A->sk[i] = LrFusedSketch{D.colptr[i], D.ent[i]};
        return GPSIG_OK;
    } else {
        const int64_t nS = int64_t(D.c) * d_eff, nW = int64_t(D.c) * D.c;
        const int64_t nspec = spec ? int64_t(p->base_params[0]) * (1 + 2 * SPECTRAL_STRIDE) : 0;
        auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
        size_t bytes = up16(sizeof(float) * nS) + up16(sizeof(float) * nW) + up16(sizeof(float) * nspec);
        for (int i = 0; i < D.nsk; ++i) bytes += sizeof(LrEntryF32) * size_t(D.nent[i]) + 16;
        void* base;
        CHK(ensure(c, B_LRF32, bytes + 16, &base));
        char* b = static_cast<char*>(base);
        float* S = reinterpret_cast<float*>(b); b += up16(sizeof(float) * nS);
        float* Wh = reinterpret_cast<float*>(b); b += up16(sizeof(float) * nW);
        float* sp = reinterpret_cast<float*>(b); b += up16(sizeof(float) * nspec);
        int rc = lr_narrow_launch(c->stream, D.S, nS, S);
        if (rc == 0) rc = lr_narrow_launch(c->stream, D.Wh, nW, Wh);
        if (rc == 0 && spec) rc = lr_narrow_launch(c->stream, spec, nspec, sp);
        for (int i = 0; i < D.nsk && rc == 0; ++i) {
            LrEntryF32* e = reinterpret_cast<LrEntryF32*>(b);
            rc = lr_narrow_entries_launch(c->stream, D.ent[i], D.nent[i], e);
            A->sk[i] = LrFusedSketchF32{D.colptr[i], e};
            b += sizeof(LrEntryF32) * size_t(D.nent[i]) + 16;
        }
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "narrowing the low-rank state to float32: %s", hipGetErrorString(hipError_t(rc)));
        A->S = S; A->Wh = Wh; A->spec = spec ? sp : nullptr;
        return GPSIG_OK;
    }
}

// low-rank Gram products (gpsig_lr_kernel / gpsig_lr_kernel_diag) in the features' float type: factors, scaling and the GEMM in T, level
// weights and jitter from their float64 host values
template <typename T>
int lr_kernel_t(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* PhiA, const void* PhiB, int64_t N1, int64_t N2,
                int32_t normalize_a, int32_t normalize_b, int32_t return_levels, void* out) {
    const int M = p->num_levels, M1 = M + 1, cc = lr->num_components, r = lr->rank_bound;
    const bool sym = PhiB == nullptr;
    if (sym) N2 = N1;
    const int32_t* off;
    int F;
    CHK(lr_level_offsets(c, M, cc, r, &off, &F));
    const void *dA, *dB;
    CHK(in_dev(c, B_IN0, PhiA, sizeof(T) * size_t(N1) * F, &dA));
    if (sym) dB = dA; else CHK(in_dev(c, B_IN1, PhiB, sizeof(T) * size_t(N2) * F, &dB));
    const size_t ob = sizeof(T) * size_t(N1) * N2 * (return_levels ? M1 : 1);
    void* dout;
    CHK(out_dev(c, B_OUT0, out, ob, &dout));
    const double* w;
    CHK(upload_weights(c, p, &w));
    void *fa, *fb, *sa, *sb;
    CHK(ensure(c, B_LR2, sizeof(T) * size_t(N1) * M1 + 8, &fa));
    CHK(ensure(c, B_LR3, sizeof(T) * size_t(N2) * M1 + 8, &fb));
    CHK(ensure(c, B_LR4, sizeof(T) * size_t(N1) * F + 8, &sa));
    CHK(ensure(c, B_LR5, sizeof(T) * size_t(N2) * F + 8, &sb));
    if (N1 <= 0 || N2 <= 0) return finish(c);
    // per-row level factors: A side carries sigma*variances, both sides 1/sqrt(|Phi_m|^2 + jitter) when normalising
    hipLaunchKernelGGL(lr_level_factors_kernel<T>, dim3(grid_for(N1 * M1)), dim3(256), 0, c->stream, static_cast<const T*>(dA), N1,
                       int64_t(F), M1, off, w, p->jitter, int(normalize_a != 0), static_cast<T*>(fa));
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(lr_level_factors_kernel<T>, dim3(grid_for(N2 * M1)), dim3(256), 0, c->stream, static_cast<const T*>(dB), N2,
                       int64_t(F), M1, off, static_cast<const double*>(nullptr), p->jitter, int((sym ? normalize_a : normalize_b) != 0),
                       static_cast<T*>(fb));
    HIPCHK(c, hipGetLastError());
    const bool jit_diag = sym && normalize_a;         // kernels.py:431
    // one product per level over the level's own columns, or (level -1) one over all of them
    const std::vector<int32_t> hoff = lr_level_offsets_host(M, cc, r);
    for (int m = return_levels ? 0 : -1; m <= (return_levels ? M : -1); ++m) {
        const int wdt = m < 0 ? F : hoff[m + 1] - hoff[m];
        hipLaunchKernelGGL(lr_scale_factors_kernel<T>, dim3(grid_for(N1 * wdt)), dim3(256), 0, c->stream, static_cast<const T*>(dA),
                           N1, int64_t(F), M1, off, static_cast<const T*>(fa), m, static_cast<T*>(sa), int64_t(wdt));
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(lr_scale_factors_kernel<T>, dim3(grid_for(N2 * wdt)), dim3(256), 0, c->stream, static_cast<const T*>(dB),
                           N2, int64_t(F), M1, off, static_cast<const T*>(fb), m, static_cast<T*>(sb), int64_t(wdt));
        HIPCHK(c, hipGetLastError());
        T* om = static_cast<T*>(dout) + size_t(m < 0 ? 0 : m) * N1 * N2;
        CHK(lr_gemm(c, static_cast<const T*>(sa), static_cast<const T*>(sb), N1, N2, wdt, wdt, wdt, om, N2));
        if (jit_diag) {
            hipLaunchKernelGGL(lr_add_jitter_diag_kernel<T>, dim3(grid_for(N1)), dim3(256), 0, c->stream, om, N1, M1,
                               static_cast<const T*>(fa), static_cast<const T*>(fb), p->jitter, m);
            HIPCHK(c, hipGetLastError());
        }
    }
    CHK(out_done(c, out, dout, ob));
    return finish(c);
}

template <typename T>
int lr_kernel_diag_t(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* Phi, int64_t N, int32_t return_levels,
                     void* out) {
    const int M = p->num_levels, M1 = M + 1;
    const int32_t* off;
    int F;
    CHK(lr_level_offsets(c, M, lr->num_components, lr->rank_bound, &off, &F));
    const void* dP;
    CHK(in_dev(c, B_IN0, Phi, sizeof(T) * size_t(N) * F, &dP));
    const size_t ob = sizeof(T) * size_t(N) * (return_levels ? M1 : 1);
    void* dout;
    CHK(out_dev(c, B_OUT0, out, ob, &dout));
    const double* w;
    CHK(upload_weights(c, p, &w));
    if (N > 0) {
        hipLaunchKernelGGL(lr_level_diag_kernel<T>, dim3(grid_for(N * M1)), dim3(256), 0, c->stream, static_cast<const T*>(dP), N,
                           int64_t(F), M1, off, w, int(return_levels != 0), static_cast<T*>(dout));
        HIPCHK(c, hipGetLastError());
    }
    CHK(out_done(c, out, dout, ob));
    return finish(c);
}

// The multi-pass routes (float64): one kernel per reference op, the only route for shapes beyond the LDS (lr_fused = 0, or a sequence's
// or tensor's arrays too large).  Scaled points, state and spectral table as the fused routes'.
int lr_seq_features_passes(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const ScaleParams& s, const LrDev& D, const double* dX,
                           int64_t N, int32_t L, const double* spec, void* Phi, void* dPhi) {
    const int M = p->num_levels, cc = D.c, r = D.r, F = 1 + cc + (M - 1) * r;
    const int l = p->difference ? L - 1 : L;
    double* phi = static_cast<double*>(dPhi);
    double p0, p1;
    base_p(p, &p0, &p1);
    void *kxs, *feat, *U, *Pa, *Pb;
    const int wmax = cc > r ? cc : r;
    CHK(ensure(c, B_LR2, sizeof(double) * size_t(N) * L * cc + 8, &kxs));
    CHK(ensure(c, B_LR3, sizeof(double) * size_t(N) * L * cc + 8, &feat));
    CHK(ensure(c, B_LR4, sizeof(double) * size_t(N) * (l > 0 ? l : 1) * cc + 8, &U));
    CHK(ensure(c, B_LR5, sizeof(double) * size_t(N) * (l > 0 ? l : 1) * wmax + 8, &Pa));
    CHK(ensure(c, B_LR6, sizeof(double) * size_t(N) * (l > 0 ? l : 1) * wmax + 8, &Pb));
    if (N <= 0) return finish(c);
    // Nystrom features (low_rank_calculations.py:59-60): kappa(X, S) then the whitening GEMM on the matrix cores
    if (p->base_kernel == GPSIG_BASE_SPECTRAL) {
        const int rc = lr_seq_cross_spectral_launch(c->stream, dX, N, int(L), s, D.S, cc, int(p0), int(p1), spec,
                                                    static_cast<double*>(kxs));
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral Nystrom cross kernel: %s", hipGetErrorString(hipError_t(rc)));
    } else {
        hipLaunchKernelGGL(lr_seq_cross_kernel<double>, dim3(grid_for(N * L * cc)), dim3(256), 0, c->stream, dX, N, int(L), s, D.S, cc,
                           int(p->base_kernel), p0, p1, static_cast<double*>(kxs));
        HIPCHK(c, hipGetLastError());
    }
    // feat = kxs (NL, c) * Wh (c, c) on the transposed whitening
    const double* wht;
    CHK(lr_whitening_t(c, lr, cc, &wht));
    CHK(lr_gemm(c, static_cast<const double*>(kxs), wht, N * L, cc, cc, cc, cc, static_cast<double*>(feat), cc));
    // level 0 and level 1 (signature_algs.py:177-182)
    hipLaunchKernelGGL(fill_kernel<double>, dim3(grid_for(N * F)), dim3(256), 0, c->stream, phi, N * F, 0.0);
    HIPCHK(c, hipGetLastError());
    if (l > 0) {
        hipLaunchKernelGGL(lr_time_diff_kernel<double>, dim3(grid_for(N * l * cc)), dim3(256), 0, c->stream,
                           static_cast<const double*>(feat), N, int(L), cc, int(p->difference), static_cast<double*>(U));
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(lr_timesum_kernel<double>, dim3(grid_for(N * cc)), dim3(256), 0, c->stream, static_cast<const double*>(U), N, l,
                           cc, phi, int64_t(F), 1);
        HIPCHK(c, hipGetLastError());
        // P = U; for level i: P = excumsum_t(P); P = sketch(U, P); Phi_i = sum_t P     (signature_algs.py:184-191)
        HIPCHK(c, hipMemcpyAsync(Pa, U, sizeof(double) * size_t(N) * l * cc, hipMemcpyDeviceToDevice, c->stream));
        double *cur = static_cast<double*>(Pa), *nxt = static_cast<double*>(Pb);
        int kw = cc;
        for (int i = 2; i <= M; ++i) {
            hipLaunchKernelGGL(lr_excumsum_kernel<double>, dim3(grid_for(N * kw)), dim3(256), 0, c->stream, cur, N, l, kw, phi, int64_t(F), 0, 0);
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL(lr_sketch_kernel<double>, dim3(grid_for(N * l * r)), dim3(256), 0, c->stream, static_cast<const double*>(U),
                               int64_t(cc), static_cast<const double*>(cur), int64_t(kw), N * l, r, D.colptr[i - 2], D.i1[i - 2], D.i2[i - 2],
                               D.val[i - 2], nxt, int64_t(r));
            HIPCHK(c, hipGetLastError());
            hipLaunchKernelGGL(lr_timesum_kernel<double>, dim3(grid_for(N * r)), dim3(256), 0, c->stream, static_cast<const double*>(nxt), N, l,
                               r, phi, int64_t(F), 1 + cc + (i - 2) * r);
            HIPCHK(c, hipGetLastError());
            double* t = cur; cur = nxt; nxt = t;
            kw = r;
        }
    }
    hipLaunchKernelGGL(fill_strided_kernel<double>, dim3(grid_for(N)), dim3(256), 0, c->stream, phi, N, int64_t(F), 1.0);
    HIPCHK(c, hipGetLastError());
    CHK(out_done(c, Phi, dPhi, sizeof(double) * size_t(N) * F));
    return finish(c);
}

int lr_tens_features_passes(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const ScaleParams& s, const LrDev& D, const double* dZ,
                            int64_t T, int E, const double* spec, void* Phi, void* dPhi) {
    const int M = p->num_levels, lt = M * (M + 1) / 2, cc = D.c, r = D.r, F = 1 + cc + (M - 1) * r;
    const int increments = E == 2;
    double* phi = static_cast<double*>(dPhi);
    double p0, p1;
    base_p(p, &p0, &p1);
    const int64_t rows = int64_t(lt) * T * E;
    void *kxs, *feat, *U, *Ra, *Rb;
    const int wmax = cc > r ? cc : r;
    CHK(ensure(c, B_LR2, sizeof(double) * size_t(rows) * cc + 8, &kxs));
    CHK(ensure(c, B_LR3, sizeof(double) * size_t(rows) * cc + 8, &feat));
    CHK(ensure(c, B_LR4, sizeof(double) * size_t(lt) * T * cc + 8, &U));
    CHK(ensure(c, B_LR5, sizeof(double) * size_t(T) * wmax + 8, &Ra));
    CHK(ensure(c, B_LR6, sizeof(double) * size_t(T) * wmax + 8, &Rb));
    const double* wht;
    CHK(lr_whitening_t(c, lr, cc, &wht));
    if (p->base_kernel == GPSIG_BASE_SPECTRAL) {
        const int rc = lr_tens_cross_spectral_launch(c->stream, dZ, rows, s, D.S, cc, int(p0), int(p1), spec,
                                                     static_cast<double*>(kxs));
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral Nystrom cross kernel: %s", hipGetErrorString(hipError_t(rc)));
    } else {
        hipLaunchKernelGGL(lr_tens_cross_kernel<double>, dim3(grid_for(rows * cc)), dim3(256), 0, c->stream, dZ, rows, s, D.S, cc,
                           int(p->base_kernel), p0, p1, static_cast<double*>(kxs));
        HIPCHK(c, hipGetLastError());
    }
    CHK(lr_gemm(c, static_cast<const double*>(kxs), wht, rows, cc, cc, cc, cc, static_cast<double*>(feat), cc));
    // increments: F(z[.,1]) - F(z[.,0]) (kernels.py:304); rows are ((k*T + t)*E + e): a "time difference" over e with L = E
    if (increments) {
        hipLaunchKernelGGL(lr_time_diff_kernel<double>, dim3(grid_for(int64_t(lt) * T * cc)), dim3(256), 0, c->stream,
                           static_cast<const double*>(feat), int64_t(lt) * T, 2, cc, 1, static_cast<double*>(U));
        HIPCHK(c, hipGetLastError());
    } else {
        HIPCHK(c, hipMemcpyAsync(U, feat, sizeof(double) * size_t(lt) * T * cc, hipMemcpyDeviceToDevice, c->stream));
    }
    hipLaunchKernelGGL(fill_kernel<double>, dim3(grid_for(T * F)), dim3(256), 0, c->stream, phi, T * F, 0.0);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(fill_strided_kernel<double>, dim3(grid_for(T)), dim3(256), 0, c->stream, phi, T, int64_t(F), 1.0);
    HIPCHK(c, hipGetLastError());
    // tensor_kern_lr_feature (signature_algs.py:211-221): R = U[k]; R = sketch_{j-1}(U[k'], R)
    const double* Ud = static_cast<const double*>(U);
    int k = 0;
    for (int i = 1; i <= M; ++i) {
        const double* R = Ud + size_t(k) * T * cc;
        int kw = cc;
        ++k;
        double *cur = static_cast<double*>(Ra), *nxt = static_cast<double*>(Rb);
        for (int j = 1; j < i; ++j) {
            hipLaunchKernelGGL(lr_sketch_kernel<double>, dim3(grid_for(T * r)), dim3(256), 0, c->stream, Ud + size_t(k) * T * cc, int64_t(cc), R,
                               int64_t(kw), T, r, D.colptr[j - 1], D.i1[j - 1], D.i2[j - 1], D.val[j - 1], cur, int64_t(r));
            HIPCHK(c, hipGetLastError());
            R = cur;
            kw = r;
            double* t = cur; cur = nxt; nxt = t;
            ++k;
        }
        const int off = i == 1 ? 1 : 1 + cc + (i - 2) * r;
        hipLaunchKernelGGL(copy_block_kernel<double>, dim3(grid_for(T * kw)), dim3(256), 0, c->stream, R, T, kw, int64_t(kw), phi, int64_t(F), off);
        HIPCHK(c, hipGetLastError());
    }
    CHK(out_done(c, Phi, dPhi, sizeof(double) * size_t(T) * F));
    return finish(c);
}

// ---- The wide routes: state spaces beyond every kernel that holds the points in LDS (which calls: lr_eval_route / lr_eval_tens_route,
// lr_tile_plan.hpp).  The Nystrom cross matrix comes from the float64 matrix cores, straight from the caller's raw points (lr_cross_eval_kernel,
// lr_cross_kernel.hpp), into B_LR2 in the call's element type; the feature kernels that take it from memory follow (lr_eval_wide.hpp).  Sequences
// (tensors) go in chunks whose kxs stay within the wide route's chunk budget, each a cross launch and a feature launch on its slice: they are
// independent, so the result does not depend on the chunk count.  `spectral`: the same two loops for SignatureSpectral beyond the 32 columns of
// its packed table (spectral_wide; which calls: lr_spectral_eval_wide / lr_spectral_eval_tens_wide, lr_tile_plan.hpp; float64 only).  There the
// cross matrix comes from the evaluation form of the spectral cross kernel (lr_eval_spectral_wide_inst.hip), which computes the points' phases in
// its own walk; gamma^2 and the landmarks' norms and phases are the training op's kernels on S, once per call, in B_LR4.
size_t lr_wide_chunk_bytes(const gpsig_ctx* c) {     // (as lr_cross_inst.hip: chunk_budget)
    if (c->wide_chunk_mb > 0) return size_t(c->wide_chunk_mb) << 20;
    return size_t(c->grad_scratch_mb > 0 ? c->grad_scratch_mb : 4096) << 20;
}

// what both wide routes set up: the feature kernels' view of the state (lr_state_args: float32 narrowed once per call), |S_i|^2 in B_LR3, the chunk
// (objects of `per` bytes of kxs each) and its buffer (`norms` false: SignatureSpectral has norms of its own -- A then only carries the kxs buffer)
template <typename T, typename Entry>
int lr_wide_open(gpsig_ctx* c, const gpsig_params* p, const LrDev& D, int d_eff, int64_t count, size_t per, LrEvalWideFeat<T, Entry>* W,
                 LrCrossEvalArgs<T>* A, int64_t* chunk, bool norms) {
    std::conditional_t<std::is_same<T, float>::value, LrEvalTiledArgsF32, LrEvalTiledArgs> st{};
    CHK(lr_state_args(c, p, D, d_eff, nullptr, &st));
    W->Wh = st.Wh;
    for (int i = 0; i < D.nsk; ++i) W->sk[i] = st.sk[i];
    W->c = D.c; W->r = D.r; W->M = p->num_levels; W->difference = p->difference;
    const int64_t fit = int64_t(lr_wide_chunk_bytes(c) / per);
    *chunk = std::max<int64_t>(1, std::min<int64_t>(fit, count));
    void *kxs, *sn;
    CHK(ensure(c, B_LR2, per * size_t(*chunk) + 64, &kxs));
    CHK(ensure(c, B_LR3, sizeof(double) * LR_EVAL_WIDE_MAX_C + 64, &sn));
    double p0, p1;
    base_p(p, &p0, &p1);
    A->S = D.S; A->c = D.c; A->kind = int(p->base_kernel); A->p0 = p0; A->p1 = p1;
    A->sn = static_cast<const double*>(sn);
    A->K = static_cast<T*>(kxs);
    W->kxs = static_cast<const T*>(kxs);
    if (count > 0 && norms) {
        const int rc = lr_cross_norms_launch(c->stream, D.S, D.c, d_eff, static_cast<double*>(sn));
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "Nystrom cross kernel (landmark norms): %s", hipGetErrorString(hipError_t(rc)));
    }
    return GPSIG_OK;
}

int lr_spectral_wide_refused(gpsig_ctx* c, LrSpectralWide w, bool tensors, size_t lds) {
    const int lo = int(SPECTRAL_STRIDE), hi = LR_EVAL_WIDE_MAX_D;
    switch (w) {
    case LR_SPX_F32: return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank SignatureSpectral features beyond %d columns are built for float64 only", lo);
    case LR_SPX_COMPONENTS:
        return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank SignatureSpectral features beyond %d columns are built for num_components <= %d", lo, LR_EVAL_WIDE_MAX_C);
    case LR_SPX_LEVELS:
        return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank SignatureSpectral features beyond %d columns are built for num_levels <= %d", lo, LR_FUSED_MAX_SKETCHES + 1);
    case LR_SPX_COLUMNS: return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank SignatureSpectral features are built for at most %d columns", hi);
    case LR_SPX_TENSORS: return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank SignatureSpectral tensor features beyond %d columns take at most 2^31 - 1 tensors", lo);
    default: break;
    }
    if (tensors)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank SignatureSpectral tensor features beyond %d columns need a tensor's kzs arrays (%zu bytes) within %zu "
                    "bytes of LDS", lo, lds, LR_TENS_FUSED_MAX_LDS);
    return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank SignatureSpectral features beyond %d columns need one 64-step tile of max(num_components, rank_bound) "
                "rows in the LDS (%zu bytes of %zu)", lo, lds, LR_FUSED_MAX_LDS);
}

// what a spectral call sets up behind lr_wide_open: the table, gamma^2 and the landmarks' norms and phases
int lr_spectral_wide_open(gpsig_ctx* c, const gpsig_params* p, const LrDev& D, int64_t count, LrSpxEvalArgs* A) {
    const int Q = int(p->base_params[0]), d = p->num_features;
    const double* tab;
    CHK(spectral_table_wide(c, p, &tab));
    void* head;
    CHK(ensure(c, B_LR4, sizeof(double) * (size_t(Q) * d + 2 * size_t(Q) * D.c) + 64, &head));
    double* const g2 = static_cast<double*>(head);
    A->d = d; A->S = D.S; A->c = D.c; A->Q = Q; A->family = int(p->base_params[1]);
    A->alpha = tab; A->omega = tab + Q;
    A->g2 = g2; A->ss = g2 + size_t(Q) * d; A->phS = A->ss + size_t(Q) * D.c;
    if (count > 0) {
        const int rc = spectral_cross_prepare_launch(c->stream, D.S, D.c, d, Q, A->omega, tab + Q + size_t(Q) * d, g2);
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral cross kernel (landmark norms and phases): %s", hipGetErrorString(hipError_t(rc)));
    }
    return GPSIG_OK;
}

template <typename T>
int lr_seq_features_wide(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& s, const LrDev& D, const T* dX, int64_t N, int32_t L,
                         const int32_t* dlen, bool spectral, void* Phi, void* dPhi) {
    using Entry = std::conditional_t<std::is_same<T, float>::value, LrEntryF32, LrEntry>;
    const int F = 1 + D.c + (p->num_levels - 1) * D.r;
    LrEvalWideFeat<T, Entry> W{};
    LrCrossEvalArgs<T> A{};
    LrSpxEvalArgs B{};
    int64_t chunk;
    CHK(lr_wide_open(c, p, D, s.d_eff(), N, sizeof(T) * size_t(L) * D.c, &W, &A, &chunk, !spectral));
    if (spectral) CHK(lr_spectral_wide_open(c, p, D, N, &B));
    A.L = L; A.P = s;
    B.L = L;
    W.L = L;
    for (int64_t n0 = 0; n0 < N; n0 += chunk) {
        const int64_t nn = std::min<int64_t>(chunk, N - n0);
        const T* X0 = dX + n0 * int64_t(L) * p->num_features;
        const int32_t* len = dlen ? dlen + n0 : nullptr;
        if (spectral) {
            if constexpr (std::is_same<T, double>::value) {
                B.X = X0; B.n = nn * L; B.lengths = len; B.K = A.K;
                const int rc = lr_spx_eval_seq_launch(c->stream, B);
                if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral cross kernel (evaluation form): %s", hipGetErrorString(hipError_t(rc)));
            }
        } else {
            A.X = X0; A.n = nn * L; A.lengths = len;
            const int rc = lr_cross_eval_seq_launch(c->stream, A);
            if (rc != 0) return fail(c, GPSIG_ERR_HIP, "Nystrom cross kernel (evaluation form): %s", hipGetErrorString(hipError_t(rc)));
        }
        W.N = nn; W.lengths = len;
        W.Phi = static_cast<T*>(dPhi) + n0 * int64_t(F);
        const int rc = lr_eval_wide_seq_launch(c->stream, W, c->lr_fused_pad);
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "tiled low-rank feature kernel (kxs from memory): %s", hipGetErrorString(hipError_t(rc)));
    }
    CHK(out_done(c, Phi, dPhi, sizeof(T) * size_t(N) * F));
    return finish(c);
}

template <typename T>
int lr_tens_features_wide(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& s, const LrDev& D, const T* dZ, int64_t T_, int lt, int E,
                          bool spectral, void* Phi, void* dPhi) {
    using Entry = std::conditional_t<std::is_same<T, float>::value, LrEntryF32, LrEntry>;
    const int F = 1 + D.c + (p->num_levels - 1) * D.r;
    LrEvalWideFeat<T, Entry> W{};
    LrCrossEvalArgs<T> A{};
    LrSpxEvalArgs B{};
    int64_t chunk;
    CHK(lr_wide_open(c, p, D, s.d_eff(), T_, sizeof(T) * size_t(lt) * E * D.c, &W, &A, &chunk, !spectral));
    if (spectral) CHK(lr_spectral_wide_open(c, p, D, T_, &B));
    A.X = dZ; A.P = s; A.T = T_; A.E = E;
    B.T = T_; B.E = E;
    W.L = lt; W.E = E;
    for (int64_t t0 = 0; t0 < T_; t0 += chunk) {
        const int64_t nt = std::min<int64_t>(chunk, T_ - t0);
        if (spectral) {
            if constexpr (std::is_same<T, double>::value) {
                B.X = dZ; B.K = A.K; B.t0 = t0; B.nt = nt; B.n = int64_t(lt) * nt * E;
                const int rc = lr_spx_eval_tens_launch(c->stream, B);
                if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral cross kernel (evaluation form, tensors): %s", hipGetErrorString(hipError_t(rc)));
            }
        } else {
            A.t0 = t0; A.nt = nt; A.n = int64_t(lt) * nt * E;
            const int rc = lr_cross_eval_tens_launch(c->stream, A);
            if (rc != 0) return fail(c, GPSIG_ERR_HIP, "Nystrom cross kernel (evaluation form, tensors): %s", hipGetErrorString(hipError_t(rc)));
        }
        W.N = nt;
        W.Phi = static_cast<T*>(dPhi) + t0 * int64_t(F);
        const int rc = lr_eval_wide_tens_launch(c->stream, W);
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "fused low-rank tensor feature kernel (kzs from memory): %s", hipGetErrorString(hipError_t(rc)));
    }
    CHK(out_done(c, Phi, dPhi, sizeof(T) * size_t(T_) * F));
    return finish(c);
}

// the fields the fused and the tiled sequence kernels' argument blocks have in common, and the state in the call's float type
template <typename T, typename Args>
int lr_seq_args(gpsig_ctx* c, const gpsig_params* p, const ScaleParams& s, const LrDev& D, const double* spec, const void* dX, int64_t N, int32_t L,
                void* dPhi, Args* A) {
    double p0, p1;
    base_p(p, &p0, &p1);
    A->X = static_cast<const T*>(dX); A->N = N; A->L = L; A->P = s;
    A->c = D.c; A->r = D.r; A->M = p->num_levels; A->difference = p->difference; A->kind = int(p->base_kernel); A->p0 = T(p0); A->p1 = T(p1);
    A->Phi = static_cast<T*>(dPhi);
    return lr_state_args(c, p, D, s.d_eff(), spec, A);
}

// gpsig_lr_seq_features / _ragged / _ragged_lagged in T.  Whole sequences (`ragged` false): the fused kernels (lr_fused_kernel.hpp: one
// workgroup per sequence, intermediates in LDS) where a sequence's arrays fit; beyond them, with lr_fused != 0, the time-tiled kernels of
// lr_eval_tiled.hpp where at least one 64-step tile fits (float32: the families of base_eval only); beyond those the wide route above (the
// families of base_eval, c <= 64, both float types); else the multi-pass route -- float64 only: for float32 that is UNSUPPORTED, and the Python
// layer computes the call in float64 and rounds it.  lr_fused = 0 is the multi-pass route at every shape.  The rule is lr_eval_route
// (lr_tile_plan.hpp).  float64 tests the three-array footprint before it may pick either fused form, float32 the footprint of the form it picks.
// Ragged (`lengths`: N int32 in the context's pointer mode): the tiled kernels at every length -- a short batch is a one-tile walk --, the wide
// route beyond them, whatever lr_fused says; there is no multi-pass form.  SignatureSpectral beyond its packed table (spectral_wide) has the one
// route, dense or ragged, at any lr_fused: lr_spectral_eval_wide takes it or names the bound that refuses it.
template <typename T>
int lr_seq_features_t(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* X, int64_t N, int32_t L, bool ragged,
                      const int32_t* lengths, void* Phi) {
    constexpr bool f32 = std::is_same<T, float>::value;
    const int M = p->num_levels, cc = lr->num_components, r = lr->rank_bound, F = 1 + cc + (M - 1) * r;
    ScaleParams s;
    CHK(scale_params(c, p, true, &s));
    const int d_eff = s.d_eff();
    // the route, and its refusals: nothing is uploaded for a call that is refused
    const bool spx = spectral_wide(p);
    // two arrays in LDS instead of three where a wavefront can hold its output columns in registers (lr_fused2): a third workgroup per CU
    const bool two = c->lr_fused == 1 && lr_fused2_ok(cc, r, L);
    LrEvalRoute route = LR_EVAL_WIDE;
    if (spx) {
        const LrSpectralWide w = lr_spectral_eval_wide(f32, cc, r, d_eff, L, M, p->difference, c->lr_fused_pad);
        if (w != LR_SPX_WIDE) return lr_spectral_wide_refused(c, w, false, lr_eval_tiled_lds_bytes(false, cc, r, 0, LR_TILE_STEP, c->lr_fused_pad));
    } else {
        const size_t lds = !f32 ? lr_fused_lds_bytes(cc, r, d_eff, L, c->lr_fused_pad)
                           : two ? lr_fused2_lds_bytes_f32(cc, r, d_eff, L, c->lr_fused_pad) : lr_fused_lds_bytes_f32(cc, r, d_eff, L, c->lr_fused_pad);
        route = lr_eval_route(f32, cc, r, d_eff, L, M, p->difference, ragged, c->lr_fused, p->base_kernel == GPSIG_BASE_SPECTRAL, c->lr_fused_pad);
        if (ragged && route == LR_EVAL_REFUSE)
            return fail(c, GPSIG_ERR_UNSUPPORTED, "ragged low-rank features need one 64-step tile of the tiled kernels in the LDS (%zu bytes), at most %d "
                        "levels, and float64 for SignatureSpectral", lr_eval_tiled_lds_bytes(f32, cc, r, d_eff, LR_TILE_STEP, c->lr_fused_pad), LR_FUSED_MAX_SKETCHES + 1);
        if (route == LR_EVAL_REFUSE)
            return fail(c, GPSIG_ERR_UNSUPPORTED, "float32 low-rank features are built for the fused kernels only (lr_fused != 0, %zu bytes of LDS)", lds);
    }
    // the state, the points (raw: num_features columns), the lengths and the output, once
    LrDev D;
    CHK(lr_upload(c, lr, d_eff, &D));
    const void* dX;
    CHK(in_dev(c, B_IN0, X, sizeof(T) * size_t(N) * L * p->num_features, &dX));
    const void* dlen = nullptr;
    if (ragged) CHK(in_dev(c, B_IN1, lengths, sizeof(int32_t) * size_t(N), &dlen));
    void* dPhi;
    CHK(out_dev(c, B_OUT0, Phi, sizeof(T) * size_t(N) * F, &dPhi));
    if (route == LR_EVAL_WIDE)
        return lr_seq_features_wide<T>(c, p, s, D, static_cast<const T*>(dX), N, L, static_cast<const int32_t*>(dlen), spx, Phi, dPhi);
    const double* spec = nullptr;        // BASE_SPECTRAL: its parameter table (p0 = Q, p1 = family), read by the spectral instances
    if (!f32 || N > 0) CHK(spectral_table(c, p, &spec));                     // (float32 uploads nothing for an empty call)
    if (route == LR_EVAL_PASSES) return lr_seq_features_passes(c, p, lr, s, D, static_cast<const double*>(dX), N, L, spec, Phi, dPhi);
    if (N <= 0) return finish(c);
    const bool tiled = route == LR_EVAL_TILED;
    int rc;
    if (tiled) {
        std::conditional_t<f32, LrEvalTiledArgsF32, LrEvalTiledArgs> A{};
        A.lengths = static_cast<const int32_t*>(dlen);
        CHK(lr_seq_args<T>(c, p, s, D, spec, dX, N, L, dPhi, &A));
        rc = lr_eval_tiled_launch(c->stream, A, c->lr_fused_pad);
    } else {
        std::conditional_t<f32, LrFusedArgsF32, LrFusedArgs> A{};
        CHK(lr_seq_args<T>(c, p, s, D, spec, dX, N, L, dPhi, &A));
        rc = lr_fused_launch(c->stream, A, c->lr_fused_pad, two, c->lr_fused_variant);
    }
    if (rc != 0)
        return fail(c, GPSIG_ERR_HIP, f32 ? "%s float32 low-rank feature kernel: %s" : "%s low-rank feature kernel: %s", tiled ? "tiled" : "fused",
                    hipGetErrorString(hipError_t(rc)));
    CHK(out_done(c, Phi, dPhi, sizeof(T) * size_t(N) * F));
    return finish(c);
}

// gpsig_lr_tens_features in T: the fused kernel where a tensor's arrays fit 64 KB of LDS; where they do without the points, the wide route;
// else the multi-pass route (float64 only, as above).  The rule is lr_eval_tens_route (lr_tile_plan.hpp); spectral_wide: lr_spectral_eval_tens_wide.
template <typename T>
int lr_tens_features_t(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* Z, int64_t T_, int32_t increments, void* Phi) {
    constexpr bool f32 = std::is_same<T, float>::value;
    const int M = p->num_levels, lt = M * (M + 1) / 2, E = increments ? 2 : 1, cc = lr->num_components, r = lr->rank_bound, F = 1 + cc + (M - 1) * r;
    ScaleParams s;
    CHK(scale_params(c, p, true, &s));
    const int d_eff = s.d_eff();
    const bool spx = spectral_wide(p);
    LrEvalRoute route = LR_EVAL_WIDE;
    if (spx) {
        const LrSpectralWide w = lr_spectral_eval_tens_wide(f32, cc, r, d_eff, M, E, T_);
        if (w != LR_SPX_WIDE) return lr_spectral_wide_refused(c, w, true, lr_tens_fused_lds_bytes(cc, r, 0, lt, E));
    } else {
        const size_t lds = f32 ? lr_tens_fused_lds_bytes_f32(cc, r, d_eff, lt, E) : lr_tens_fused_lds_bytes(cc, r, d_eff, lt, E);
        route = lr_eval_tens_route(f32, cc, r, d_eff, M, E, c->lr_fused, p->base_kernel == GPSIG_BASE_SPECTRAL, T_);
        if (route == LR_EVAL_REFUSE)
            return fail(c, GPSIG_ERR_UNSUPPORTED, "float32 low-rank tensor features are built for the fused kernel only (lr_fused != 0, %zu bytes of LDS)", lds);
    }
    LrDev D;
    CHK(lr_upload(c, lr, d_eff, &D));
    const void* dZ;
    CHK(in_dev(c, B_IN0, Z, sizeof(T) * size_t(lt) * T_ * E * d_eff, &dZ));
    void* dPhi;
    CHK(out_dev(c, B_OUT0, Phi, sizeof(T) * size_t(T_) * F, &dPhi));
    if (T_ <= 0) return finish(c);
    if (route == LR_EVAL_WIDE) return lr_tens_features_wide<T>(c, p, s, D, static_cast<const T*>(dZ), T_, lt, E, spx, Phi, dPhi);
    double p0, p1;
    base_p(p, &p0, &p1);
    const double* spec;
    CHK(spectral_table(c, p, &spec));
    if (route != LR_EVAL_FUSED) return lr_tens_features_passes(c, p, lr, s, D, static_cast<const double*>(dZ), T_, E, spec, Phi, dPhi);
    std::conditional_t<f32, LrTensFusedArgsF32, LrTensFusedArgs> A{};
    A.Z = static_cast<const T*>(dZ); A.T = T_; A.lt = lt; A.E = E; A.P = s;
    A.c = cc; A.r = r; A.M = M; A.kind = int(p->base_kernel); A.p0 = T(p0); A.p1 = T(p1);
    A.Phi = static_cast<T*>(dPhi);
    CHK(lr_state_args(c, p, D, d_eff, spec, &A));
    const int rc = lr_tens_fused_launch(c->stream, A);
    if (rc != 0)
        return fail(c, GPSIG_ERR_HIP, f32 ? "fused float32 low-rank tensor feature kernel: %s" : "fused low-rank tensor feature kernel: %s", hipGetErrorString(hipError_t(rc)));
    CHK(out_done(c, Phi, dPhi, sizeof(T) * size_t(T_) * F));
    return finish(c);
}

// the three sequence entry points: dense, ragged (`lengths`), and ragged with lags on each sequence's own time axis.  The kernels of
// lr_seq_features_t's ragged routes take a sequence's length as the axis of its lag interpolation (scaled_point's seq_len; lr_cross_eval_kernel's
// brackets) wherever a call has lengths -- only gpsig_lr_seq_features_ragged_lagged (`lags_ok`) sends them lags
int lr_seq_features(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* X, int64_t N, int32_t L, bool ragged,
                    const int32_t* lengths, bool lags_ok, void* Phi) {
    ENTER_LR(c, p);
    CHK(lr_check(c, p, lr));
    if (ragged && !lags_ok && p->num_lags > 0)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "per-sequence lengths are not built for num_lags > 0: the lag interpolation runs on the table's own time axis");
    if (ragged && !lengths && N > 0) return fail(c, GPSIG_ERR_INVALID, "null lengths pointer");
    return p->dtype == GPSIG_F32 ? lr_seq_features_t<float>(c, p, lr, X, N, L, ragged, lengths, Phi)
                                 : lr_seq_features_t<double>(c, p, lr, X, N, L, ragged, lengths, Phi);
}

}  // namespace

extern "C" {

int gpsig_lr_gather_points(gpsig_ctx* c, const gpsig_params* p, const void* X, int64_t N, int32_t L, const int64_t* idx, int64_t R,
                           double* out_host) {
    ENTER_LR(c, p);
    const bool f32 = p->dtype == GPSIG_F32;      // float32 points, gathered into float64 landmarks (each value widened, then scaled)
    if (!idx || !out_host || R < 0) return fail(c, GPSIG_ERR_INVALID, "bad landmark request");
    for (int64_t k = 0; k < R; ++k)
        if (idx[k] < 0 || idx[k] >= N * L) return fail(c, GPSIG_ERR_INVALID, "landmark index out of range");
    ScaleParams s;
    CHK(scale_params(c, p, true, &s));
    const int d_eff = s.d_eff();
    const void* dX;
    CHK(in_dev(c, B_IN0, X, (f32 ? sizeof(float) : sizeof(double)) * size_t(N) * L * p->num_features, &dX));
    void *didx, *dout;
    CHK(ensure(c, B_LR2, sizeof(int64_t) * size_t(R) + 8, &didx));
    CHK(ensure(c, B_LR3, sizeof(double) * size_t(R) * d_eff + 8, &dout));
    if (R > 0) {
        HIPCHK(c, hipMemcpyAsync(didx, idx, sizeof(int64_t) * size_t(R), hipMemcpyHostToDevice, c->stream));
        if (f32)
            hipLaunchKernelGGL(lr_gather_points_f32_kernel, dim3(grid_for(R * d_eff)), dim3(256), 0, c->stream,
                               static_cast<const float*>(dX), L, s, static_cast<const int64_t*>(didx), R, static_cast<double*>(dout));
        else
            hipLaunchKernelGGL(lr_gather_points_kernel<double>, dim3(grid_for(R * d_eff)), dim3(256), 0, c->stream,
                               static_cast<const double*>(dX), L, s, static_cast<const int64_t*>(didx), R, static_cast<double*>(dout));
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(out_host, dout, sizeof(double) * size_t(R) * d_eff, hipMemcpyDeviceToHost, c->stream));
    }
    CHK(host_sync(c));
    return GPSIG_OK;
}

int gpsig_base_kernel_matrix(gpsig_ctx* c, const gpsig_params* p, const double* A_host, const double* B_host, int64_t na, int64_t nb,
                             int32_t d, double* out_host) {
    ENTER_GRAM(c, p);
    if (!A_host || !B_host || !out_host || na < 0 || nb < 0 || d < 1) return fail(c, GPSIG_ERR_INVALID, "bad base-kernel-matrix request");
    void *da, *db, *dout;
    CHK(ensure(c, B_LR2, sizeof(double) * size_t(na) * d + 8, &da));
    CHK(ensure(c, B_LR3, sizeof(double) * size_t(nb) * d + 8, &db));
    CHK(ensure(c, B_LR4, sizeof(double) * size_t(na) * nb + 8, &dout));
    if (na > 0 && nb > 0) {
        HIPCHK(c, hipMemcpyAsync(da, A_host, sizeof(double) * size_t(na) * d, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(db, B_host, sizeof(double) * size_t(nb) * d, hipMemcpyHostToDevice, c->stream));
        CHK(landmark_gram(c, p, static_cast<const double*>(da), static_cast<const double*>(db), na, nb, int(d), static_cast<double*>(dout)));
        HIPCHK(c, hipMemcpyAsync(out_host, dout, sizeof(double) * size_t(na) * nb, hipMemcpyDeviceToHost, c->stream));
    }
    CHK(host_sync(c));
    return GPSIG_OK;
}

int gpsig_lr_whitening(gpsig_ctx* c, const gpsig_params* p, const double* S_host, int32_t nc, int32_t d, const double* jitter_diag_host,
                       double* Wh_host, double* ev_host) {
    ENTER_GRAM(c, p);
    if (!S_host || !jitter_diag_host || !Wh_host || nc < 1 || d < 1) return fail(c, GPSIG_ERR_INVALID, "bad whitening request");
    CHK(no_capture(c, "the Nystrom whitening copies to and from the host"));
    void *dS, *dW, *dJ, *dWh;
    CHK(ensure(c, B_LR2, sizeof(double) * size_t(nc) * d + 8, &dS));
    CHK(ensure(c, B_LR4, sizeof(double) * size_t(nc) * nc + 8, &dW));
    CHK(ensure(c, B_LR3, sizeof(double) * size_t(nc) * 3 + 64, &dJ));
    CHK(ensure(c, B_LR5, sizeof(double) * size_t(nc) * nc + 8, &dWh));
    double* const dEv = static_cast<double*>(dJ) + nc;
    double* const dWork = static_cast<double*>(dJ) + 2 * size_t(nc);
    int* const dInfo = reinterpret_cast<int*>(static_cast<double*>(dJ) + 3 * size_t(nc));
    HIPCHK(c, hipMemcpyAsync(dS, S_host, sizeof(double) * size_t(nc) * d, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dJ, jitter_diag_host, sizeof(double) * size_t(nc), hipMemcpyHostToDevice, c->stream));
    const int64_t total = int64_t(nc) * nc;
    CHK(landmark_gram(c, p, static_cast<const double*>(dS), static_cast<const double*>(dS), int64_t(nc), int64_t(nc), int(d),
                      static_cast<double*>(dW)));                                                          // low_rank_calculations.py:51
    hipLaunchKernelGGL(add_diag_kernel, dim3((nc + 255) / 256), dim3(256), 0, c->stream, static_cast<double*>(dW),
                       static_cast<const double*>(dJ), int(nc));
    HIPCHK(c, hipGetLastError());
    std::string err;
    if (!solver_dsyevd(&c->blas_handle, c->stream, nc, static_cast<double*>(dW), dEv, dWork, dInfo, &err))    // :55
        return fail(c, GPSIG_ERR_HIP, "%s", err.c_str());
    hipLaunchKernelGGL(eig_sign_kernel, dim3((nc + 63) / 64), dim3(64), 0, c->stream, static_cast<const double*>(dW), int(nc), dWork);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(whiten_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, c->stream, static_cast<const double*>(dW),
                       static_cast<const double*>(dEv), static_cast<const double*>(dWork), int(nc), p->jitter, static_cast<double*>(dWh));
    HIPCHK(c, hipGetLastError());
    int info = 0;
    HIPCHK(c, hipMemcpyAsync(Wh_host, dWh, sizeof(double) * size_t(total), hipMemcpyDeviceToHost, c->stream));
    if (ev_host) HIPCHK(c, hipMemcpyAsync(ev_host, dEv, sizeof(double) * size_t(nc), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&info, dInfo, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    CHK(host_sync(c));
    if (info != 0) return fail(c, GPSIG_ERR_HIP, "rocsolver_dsyevd did not converge (info = %d)", info);
    return GPSIG_OK;
}

int gpsig_lr_seq_features(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* X, int64_t N, int32_t L, void* Phi) {
    return lr_seq_features(c, p, lr, X, N, L, false, nullptr, true, Phi);
}

int gpsig_lr_seq_features_ragged(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* X, int64_t N, int32_t L,
                                 const int32_t* lengths, void* Phi) {
    return lr_seq_features(c, p, lr, X, N, L, true, lengths, false, Phi);
}

int gpsig_lr_seq_features_ragged_lagged(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* X, int64_t N, int32_t L,
                                        const int32_t* lengths, void* Phi) {
    return lr_seq_features(c, p, lr, X, N, L, true, lengths, true, Phi);
}

int gpsig_lr_tens_features(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* Z, int64_t T, int32_t increments,
                           void* Phi) {
    ENTER_LR(c, p);
    CHK(lr_check(c, p, lr));
    return p->dtype == GPSIG_F32 ? lr_tens_features_t<float>(c, p, lr, Z, T, increments, Phi) : lr_tens_features_t<double>(c, p, lr, Z, T, increments, Phi);
}

int gpsig_lr_kernel(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* PhiA, const void* PhiB, int64_t N1, int64_t N2,
                    int32_t normalize_a, int32_t normalize_b, int32_t return_levels, void* out) {
    ENTER_LR(c, p);
    if (!lr) return fail(c, GPSIG_ERR_INVALID, "lowrank descriptor is NULL");
    return p->dtype == GPSIG_F32 ? lr_kernel_t<float>(c, p, lr, PhiA, PhiB, N1, N2, normalize_a, normalize_b, return_levels, out)
                                 : lr_kernel_t<double>(c, p, lr, PhiA, PhiB, N1, N2, normalize_a, normalize_b, return_levels, out);
}

int gpsig_lr_kernel_diag(gpsig_ctx* c, const gpsig_params* p, const gpsig_lowrank* lr, const void* Phi, int64_t N, int32_t return_levels,
                         void* out) {
    ENTER_LR(c, p);
    if (!lr) return fail(c, GPSIG_ERR_INVALID, "lowrank descriptor is NULL");
    return p->dtype == GPSIG_F32 ? lr_kernel_diag_t<float>(c, p, lr, Phi, N, return_levels, out) : lr_kernel_diag_t<double>(c, p, lr, Phi, N, return_levels, out);
}

int gpsig_lr_draw(gpsig_ctx* c, const gpsig_params* p, int32_t num_components, int32_t rank_bound, int32_t sparsity, uint64_t seed,
                  const void* X, int64_t N, int32_t L, const void* X2, int64_t N2, int32_t L2, const void* Z, int64_t T, int32_t increments,
                  gpsig_lr_state** inout) {
    ENTER_LR(c, p);
    if (!inout) return fail(c, GPSIG_ERR_INVALID, "null state slot");
    if (c->ptr_mode != GPSIG_PTR_DEVICE) return fail(c, GPSIG_ERR_INVALID, "gpsig_lr_draw takes device pointers (the host-side draw is gpsig_amd/low_rank.py)");
    if (num_components < 1 || rank_bound < 1 || sparsity < 0 || sparsity > 2) return fail(c, GPSIG_ERR_INVALID, "bad low-rank sizes");
    if (num_components > LR_DRAW_MAX || rank_bound > LR_DRAW_MAX) return fail(c, GPSIG_ERR_UNSUPPORTED, "the device-side draw takes at most %d components / rank bound", LR_DRAW_MAX);
    const int M = p->num_levels, nsk = M - 1;
    if (nsk > LR_FUSED_MAX_SKETCHES) return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank mode is built for num_levels <= %d", LR_FUSED_MAX_SKETCHES + 1);
    ScaleParams s;
    CHK(scale_params(c, p, true, &s));
    const int d_eff = s.d_eff();
    const int lt = M * (M + 1) / 2;
    const int64_t ztot = Z ? int64_t(lt) * T * (increments ? 2 : 1) : 0;
    const int64_t total = ztot + (X ? N * L : 0) + (X2 ? N2 * L2 : 0);
    if (num_components > total) return fail(c, GPSIG_ERR_INVALID, "num_components exceeds the number of available points");
    if (sparsity == 2 && nsk > 0 && (rank_bound > int64_t(num_components) * num_components || (nsk > 1 && rank_bound > int64_t(num_components) * rank_bound)))
        return fail(c, GPSIG_ERR_INVALID, "rank_bound exceeds the number of coordinate pairs");
    gpsig_lr_state* st = *inout;
    if (st && st->ctx != c) return fail(c, GPSIG_ERR_INVALID, "the state belongs to another context");
    if (!st) {
        st = new (std::nothrow) gpsig_lr_state();
        if (!st) return fail(c, GPSIG_ERR_NOMEM, "out of host memory");
        st->ctx = c;
    }
    if (!st->ctx) return fail(c, GPSIG_ERR_INVALID, "the state's context has been destroyed");
    st->c = num_components; st->d_eff = d_eff; st->r = rank_bound; st->nsk = nsk; st->sparsity = sparsity;
    CHK(no_capture(c, "a low-rank draw may have to allocate"));
    if (lr_state_layout(st) != GPSIG_OK) { if (!*inout) delete st; return fail(c, GPSIG_ERR_NOMEM, "hipMalloc failed for the low-rank state"); }
    if (!*inout) c->lr_states.push_back(st);
    *inout = st;
    const PhiloxKey key{uint32_t(seed), uint32_t(seed >> 32)};
    const int cc = st->c;
    HIPCHK(c, hipMemsetAsync(st->info, 0, sizeof(int) * 4, c->stream));
    hipLaunchKernelGGL(lr_draw_indices_kernel, dim3(1), dim3(64), 0, c->stream, total, cc, key, uint32_t(LRS_LANDMARKS), st->idx);
    HIPCHK(c, hipGetLastError());
    // float32 points: the landmarks are gathered widened to float64, and everything below is the float64 draw of the widened points
    if (p->dtype == GPSIG_F32)
        hipLaunchKernelGGL(lr_gather_landmarks_f32_kernel, dim3(grid_for(int64_t(cc) * d_eff)), dim3(256), 0, c->stream, st->idx, cc,
                           static_cast<const float*>(Z), ztot, static_cast<const float*>(X), X ? N : 0, int(L), static_cast<const float*>(X2),
                           X2 ? N2 : 0, int(L2), s, key, p->jitter, st->S, st->jd);
    else
        hipLaunchKernelGGL(lr_gather_landmarks_kernel, dim3(grid_for(int64_t(cc) * d_eff)), dim3(256), 0, c->stream, st->idx, cc,
                           static_cast<const double*>(Z), ztot, static_cast<const double*>(X), X ? N : 0, int(L), static_cast<const double*>(X2),
                           X2 ? N2 : 0, int(L2), s, key, p->jitter, st->S, st->jd);
    HIPCHK(c, hipGetLastError());
    // the projections depend on the seed only: they are drawn on a side stream while the main one decomposes the landmark Gram
    if (!c->side_stream) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->side_stream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->side_fork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->side_join, hipEventDisableTiming));
    }
    HIPCHK(c, hipEventRecord(c->side_fork, c->stream));            // after the memset of info and everything queued before this draw
    HIPCHK(c, hipStreamWaitEvent(c->side_stream, c->side_fork, 0));
    hipStream_t const ss = c->side_stream;
    // W = kappa(S, S) + diag(jd)                                                          low_rank_calculations.py:51-52
    CHK(landmark_gram(c, p, static_cast<const double*>(st->S), static_cast<const double*>(st->S), int64_t(cc), int64_t(cc), d_eff, st->W));
    hipLaunchKernelGGL(add_diag_kernel, dim3((cc + 255) / 256), dim3(256), 0, c->stream, st->W, static_cast<const double*>(st->jd), cc);
    HIPCHK(c, hipGetLastError());
    // eigendecomposition (:55), sign convention, U / sqrt(S + jitter) (:56-57, :60)
    if (cc <= LR_JACOBI_MAX && c->lr_jacobi != 0) {
        const size_t lds = sizeof(double) * (2 * size_t(cc) * (cc + 1) + 2 * size_t(LR_JACOBI_MAX));
        // (the kernel has read W into LDS long before it writes the eigenvectors over it)
        hipLaunchKernelGGL(lr_jacobi_eig_kernel, dim3(1), dim3(LR_JACOBI_THREADS), lds, c->stream, static_cast<const double*>(st->W), cc, st->W, st->ev, st->info);
        HIPCHK(c, hipGetLastError());
    } else {
        std::string err;
        if (!solver_dsyevd(&c->blas_handle, c->stream, cc, st->W, st->ev, st->work, st->info, &err)) return fail(c, GPSIG_ERR_HIP, "%s", err.c_str());
    }
    hipLaunchKernelGGL(eig_sign_kernel, dim3((cc + 63) / 64), dim3(64), 0, c->stream, static_cast<const double*>(st->W), cc, st->work);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(whiten_kernel, dim3(unsigned((int64_t(cc) * cc + 255) / 256)), dim3(256), 0, c->stream, static_cast<const double*>(st->W),
                       static_cast<const double*>(st->ev), static_cast<const double*>(st->work), cc, p->jitter, st->Wh);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(lr_transpose_kernel, dim3(unsigned((cc * cc + 255) / 256)), dim3(256), 0, c->stream, static_cast<const double*>(st->Wh), cc, st->WhT);
    HIPCHK(c, hipGetLastError());
    // one projection per level 2..M (signature_algs.py:184-191)
    for (int i = 0; i < nsk; ++i) {
        gpsig_lr_state::Sk& k = st->sk[i];
        const int64_t D = int64_t(k.k1) * k.k2;
        if (sparsity == 2) {
            hipLaunchKernelGGL(lr_draw_lin_kernel, dim3(1), dim3(64), 0, ss, D, st->r, k.k1, key, uint32_t(i), k.colptr, k.i1, k.i2, k.val, k.ent);
            HIPCHK(c, hipGetLastError());
            continue;
        }
        const double sv = sparsity == 0 ? sqrt(double(D)) : double(D) / log(double(D));       // low_rank_calculations.py:172-175
        const double inv_s = sv < 1.0 ? 1.0 : 1.0 / sv, scale = sqrt((sv < 1.0 ? 1.0 : sv) / double(st->r));   // :192
        for (int fill = 0; fill < 2; ++fill) {
            hipLaunchKernelGGL(lr_draw_sparse_kernel, dim3(unsigned(st->r)), dim3(64), 0, ss, D, st->r, k.k1, inv_s, scale, key, uint32_t(i), fill,
                               k.cap, k.counts, static_cast<const int32_t*>(k.colptr), k.i1, k.i2, k.val, k.ent);
            HIPCHK(c, hipGetLastError());
            if (!fill) {
                hipLaunchKernelGGL(lr_colptr_kernel, dim3(1), dim3(64), 0, ss, static_cast<const int32_t*>(k.counts), st->r, k.cap, k.colptr,
                                   st->info + 1);
                HIPCHK(c, hipGetLastError());
            }
        }
    }
    HIPCHK(c, hipEventRecord(c->side_join, ss));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->side_join, 0));
    // A failed draw (eigensolver not converged, a projection over its capacity) must not give silently wrong features: nothing on the
    // evaluation path reads the flags back (that would be a host synchronisation per evaluation), so the whitening is turned into NaNs
    // and every feature, product and covariance computed from this state is NaN; gpsig_lr_state_sizes reports the cause.
    hipLaunchKernelGGL(lr_poison_kernel, dim3(unsigned((int64_t(cc) * cc + 255) / 256)), dim3(256), 0, c->stream, static_cast<const int*>(st->info), cc, st->Wh, st->WhT);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

void gpsig_lr_state_destroy(gpsig_lr_state* st) {
    if (!st) return;
    if (gpsig_ctx* c = st->ctx) {            // still attached: wait for what reads the block, leave the context's registry
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        for (size_t i = 0; i < c->lr_states.size(); ++i)
            if (c->lr_states[i] == st) { c->lr_states.erase(c->lr_states.begin() + i); break; }
    } else {
        (void)hipSetDevice(st->device);      // the context went first (it synchronised its streams then): only the block is left
    }
    if (st->block) (void)hipFree(st->block);
    delete st;
}

// sizes[0..4] = c, d_eff, r, number of projections, Jacobi sweeps taken (0: rocSOLVER); nnz[i] = entries of projection i.  Waits for the draw.
int gpsig_lr_state_sizes(gpsig_ctx* c, const gpsig_lr_state* st, int32_t* sizes, int32_t* nnz) {
    if (!c || !st || !sizes) return GPSIG_ERR_INVALID;
    if (st->ctx != c) return fail(c, GPSIG_ERR_INVALID, "the low-rank state belongs to another (or a destroyed) context");
    HIPCHK(c, hipSetDevice(c->device));
    sizes[0] = st->c; sizes[1] = st->d_eff; sizes[2] = st->r; sizes[3] = st->nsk; sizes[4] = 0;
    int info[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(info, st->info, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    for (int i = 0; i < st->nsk && nnz; ++i)
        HIPCHK(c, hipMemcpyAsync(&nnz[i], st->sk[i].colptr + st->r, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    sizes[4] = info[2];
    if (info[0] != 0) return fail(c, GPSIG_ERR_HIP, "the eigendecomposition of the landmark Gram did not converge (info = %d)", info[0]);
    if (info[1] != 0) return fail(c, GPSIG_ERR_HIP, "a random projection drew more entries than its capacity (a 12-sigma event: draw again)");
    return GPSIG_OK;
}

// Copies of what was drawn, all HOST pointers: landmarks (c, d'), jitter_diag (c), whitening (c, c), eigenvalues (c) -- any may be
// NULL --, and for projection i the arrays of sketches[i] (colptr r+1, i1 / i2 / val nnz[i] as reported by gpsig_lr_state_sizes).
int gpsig_lr_state_export(gpsig_ctx* c, const gpsig_lr_state* st, double* landmarks, double* jitter_diag, double* whitening, double* eigenvalues,
                          const gpsig_sketch* sketches) {
    if (!c || !st) return GPSIG_ERR_INVALID;
    if (st->ctx != c) return fail(c, GPSIG_ERR_INVALID, "the low-rank state belongs to another (or a destroyed) context");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cc = size_t(st->c);
    if (landmarks) HIPCHK(c, hipMemcpyAsync(landmarks, st->S, sizeof(double) * cc * st->d_eff, hipMemcpyDeviceToHost, c->stream));
    if (jitter_diag) HIPCHK(c, hipMemcpyAsync(jitter_diag, st->jd, sizeof(double) * cc, hipMemcpyDeviceToHost, c->stream));
    if (whitening) HIPCHK(c, hipMemcpyAsync(whitening, st->Wh, sizeof(double) * cc * cc, hipMemcpyDeviceToHost, c->stream));
    if (eigenvalues) HIPCHK(c, hipMemcpyAsync(eigenvalues, st->ev, sizeof(double) * cc, hipMemcpyDeviceToHost, c->stream));
    for (int i = 0; i < st->nsk && sketches; ++i) {
        const gpsig_sketch& h = sketches[i];
        const gpsig_lr_state::Sk& k = st->sk[i];
        if (h.nnz < 0 || h.nnz > k.cap) return fail(c, GPSIG_ERR_INVALID, "projection %d: %d entries asked for, capacity %d", i, h.nnz, k.cap);
        HIPCHK(c, hipMemcpyAsync(const_cast<int32_t*>(h.colptr), k.colptr, sizeof(int32_t) * (size_t(st->r) + 1), hipMemcpyDeviceToHost, c->stream));
        if (h.nnz) {
            HIPCHK(c, hipMemcpyAsync(const_cast<int32_t*>(h.i1), k.i1, sizeof(int32_t) * size_t(h.nnz), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(const_cast<int32_t*>(h.i2), k.i2, sizeof(int32_t) * size_t(h.nnz), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(const_cast<double*>(h.val), k.val, sizeof(double) * size_t(h.nnz), hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return GPSIG_OK;
}

}  // extern "C"
