// lr_grad_api.hip -- the low-rank training path: the feature maps of sequences and of inducing tensors with the landmarks and the whitening
// ON THE DEVICE, and their reverse passes.
//
// When the reference trains in low-rank mode, the Nystrom landmarks are gathered from the scaled inputs and their Gram is decomposed
// inside the differentiated graph (gpsig/low_rank_calculations.py:47-60): landmarks and whitening are functions of the trainable
// parameters, new at every step, and live where the step runs.  gpsig_lr_seq_features (lr_api.hip) takes them from the host (or from a
// gpsig_lr_draw state) because the evaluation path's caller owns them; the entry points here take device pointers.  Each map has a forward
// entry (`_dev`: Phi) and a reverse one (`_grad`: dPhi -> d points, dS, dWh and the base kernel's parameters):
//     gpsig_lr_seq_features_dev / _grad                   sequences (N, L, d): lr_fused_kernel.hpp / lr_grad_kernel.hpp; where a sequence's arrays
//                                                         exceed the LDS (lr_tile_plan.hpp) the time-tiled kernels of lr_tiled_kernel.hpp, each
//                                                         direction on its own
//     gpsig_lr_seq_features_ragged_dev / _ragged_grad     ... with N per-sequence lengths on the device: the same host paths (seq_features_dev /
//                                                         seq_features_grad, one optional pointer) and the ragged instances of the same four
//                                                         kernels (lr_ragged_inst.hip); checks and plan follow from L alone
//     gpsig_lr_seq_features_spectral_dev / _grad          SignatureSpectral, whose alpha, omega, gamma are trained and so are device pointers too:
//                                                         the whole-sequence spectral instances, nothing beyond the LDS
//     gpsig_lr_seq_features_spectral_ragged_dev / _grad   ... long and ragged batches (`lengths` may be NULL: L points each): the lengths-aware
//                                                         instances of lr_spectral_tiled_inst.hip, whole sequence or time-tiled
//     gpsig_lr_tens_features_dev / _grad                  inducing tensors (lt, T, E, d) (_K_tens_lr_feat, kernels.py:285-311): the fused tensor
//     gpsig_lr_tens_features_spectral_dev / _grad         kernels of lr_fused_kernel.hpp (lr_tens_fused_launch) / lr_tens_grad_kernel.hpp
//     gpsig_lr_seq_features_kx_dev / _kx_grad             the maps BEHIND the Nystrom cross matrix, for state spaces too wide for the kernels above:
//     gpsig_lr_tens_features_kx_dev / _kx_grad            kxs (N, L, c) / kzs (lt T E, c) come from memory (gpsig_lr_cross, lr_cross_inst.hip), the
//                                                         reverse passes stop at dkxs / dkzs and sum dWh alone (lr_kx.hpp, lr_kx_inst.hip); the
//                                                         width d enters neither a plan nor a table
// What they share:
//     LrCall, open()      the call's sizes, landmarks, whitening and projections; check() and the entry's own size / NULL test.  An entry's
//                         plan and LDS refusals follow, then upload_sketches: the projections are value-independent random objects that come from
//                         the host once per draw, are kept on the device by content (with the two transposed copies the reverse pass gathers over:
//                         ContentUpload, ctx.hpp, as lr_api.hip's lr_upload) and reused by every call that passes the same ones
//     forward_fields, reverse_fields     the fields the argument blocks of one direction have in common
//     spectral_table      alpha, omega, gamma packed into the table of the spectral forward instances, on the device (no host round trip)
//     zero_outputs        an empty batch
//     reduce_partials     the per-workgroup partial sums added up in workgroup order: deterministic
//     spectral_reverse    the spectral reverse passes.  Their kernels stop at dkxs (a row of c per point, in B_LRDK), which the spectral cross
//                         op's reverse kernels take on to d points, dS, dalpha, domega, dgamma.  Above LR_SPECTRAL_DKXS_BUDGET bytes of dkxs the
//                         sequences (tensors) go in chunks that fit it: each chunk's dS and parameter sums are added to the outputs in chunk order,
//                         the dWh partials of all chunks are reduced once in workgroup order -- deterministic either way.  A chunk of tensors is
//                         lt runs of Z, one per component, each handed to the cross op in turn.
// Scratch: B_GR0 partial sums, B_GR1 the per-workgroup E_i (the spectral sequence kernels: and kxs of a whole sequence, c L doubles more, inside
// the plan's budget), B_LRDK dkxs, B_GR2 the cross op's partials (own buffers: none of them can be resized while another one's reader is
// queued; ensure() waits for the stream before it frees anything anyway).
#include "ctx.hpp"
#include "lr_grad_kernel.hpp"
#include "lr_kx.hpp"
#include "lr_tens_grad_kernel.hpp"
#include "lr_spectral_tiled.hpp"
#include "lr_tiled_kernel.hpp"

#include <algorithm>
#include <type_traits>
#include <vector>

using namespace gpsig;

namespace {

constexpr size_t LR_SPECTRAL_DKXS_BUDGET = size_t(256) << 20;      // bytes of dkxs per chunk of sequences (spectral reverse pass)

// the projections of levels 2 .. M on the device: by output column, by first operand index, by second operand index
int upload_sketches(gpsig_ctx* c, int cc, int r, int nsk, const gpsig_sketch* sk, LrGradSketch* out) {
    if (nsk < 0 || nsk > LR_FUSED_MAX_SKETCHES) return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank mode is built for num_levels <= %d", LR_FUSED_MAX_SKETCHES + 1);
    if (nsk > 0 && !sk) return fail(c, GPSIG_ERR_INVALID, "NULL sketch array");
    uint64_t h = FNV1A_BASIS;
    int k2 = cc;
    size_t bytes = 64;
    for (int i = 0; i < nsk; ++i) {
        const gpsig_sketch& s = sk[i];
        if (s.k1 != cc || s.k2 != k2 || s.r != r || s.nnz < 0 || !s.colptr || (s.nnz > 0 && (!s.i1 || !s.i2 || !s.val)))
            return fail(c, GPSIG_ERR_INVALID, "sketch %d has shape (%d, %d) -> %d, expected (%d, %d) -> %d", i, s.k1, s.k2, s.r, cc, k2, r);
        h = fnv1a_sketch(h, s);
        bytes += 3 * (sizeof(LrEntry) * (size_t(s.nnz) + 1) + 16) + sizeof(int32_t) * (size_t(s.r) + size_t(s.k1) + size_t(s.k2) + 3) + 48;
        k2 = r;
    }
    ContentUpload up(c->lr_sketch_cache);
    CHK(up.open(c, B_LR8, bytes, h, size_t(6 * nsk)));
    for (int i = 0; i < nsk; ++i) {
        const gpsig_sketch& s = sk[i];
        std::vector<LrEntry> e0, e1, e2;
        std::vector<int32_t> p1, p2;
        if (!up.cached) {
            const size_t nnz = size_t(s.nnz);
            e0.resize(nnz + 1); e1.resize(nnz + 1); e2.resize(nnz + 1);
            p1.assign(size_t(s.k1) + 1, 0); p2.assign(size_t(s.k2) + 1, 0);
            for (size_t e = 0; e < nnz; ++e) {
                if (s.i1[e] < 0 || s.i1[e] >= s.k1 || s.i2[e] < 0 || s.i2[e] >= s.k2) return fail(c, GPSIG_ERR_INVALID, "sketch %d: entry %zu out of range", i, e);
                e0[e] = LrEntry{s.val[e], s.i1[e], s.i2[e]};
                ++p1[size_t(s.i1[e]) + 1]; ++p2[size_t(s.i2[e]) + 1];
            }
            for (int k = 0; k < s.k1; ++k) p1[size_t(k) + 1] += p1[size_t(k)];
            for (int k = 0; k < s.k2; ++k) p2[size_t(k) + 1] += p2[size_t(k)];
            std::vector<int32_t> n1(p1.begin(), p1.end() - 1), n2(p2.begin(), p2.end() - 1);
            for (int j = 0; j < s.r; ++j)                              // entries in their given order: a row's entries keep it
                for (int32_t e = s.colptr[j]; e < s.colptr[j + 1]; ++e) {
                    e1[size_t(n1[size_t(s.i1[e])]++)] = LrEntry{s.val[e], s.i2[e], j};
                    e2[size_t(n2[size_t(s.i2[e])]++)] = LrEntry{s.val[e], s.i1[e], j};
                }
        }
        LrGradSketch& g = out[i];
        g.colptr = up.place<int32_t>(s.colptr, sizeof(int32_t) * (size_t(s.r) + 1), 16);
        g.ent = up.place<LrEntry>(e0.data(), sizeof(LrEntry) * size_t(s.nnz), 16);
        g.ptr1 = up.place<int32_t>(p1.data(), sizeof(int32_t) * (size_t(s.k1) + 1), 16);
        g.ent1 = up.place<LrEntry>(e1.data(), sizeof(LrEntry) * size_t(s.nnz), 16);
        g.ptr2 = up.place<int32_t>(p2.data(), sizeof(int32_t) * (size_t(s.k2) + 1), 16);
        g.ent2 = up.place<LrEntry>(e2.data(), sizeof(LrEntry) * size_t(s.nnz), 16);
    }
    return up.commit(c, "the projections of a low-rank evaluation have to be uploaded");
}

int check(gpsig_ctx* c, const gpsig_params* p, int cc, int r, int nsk, bool spectral = false) {
    if (!c) return GPSIG_ERR_INVALID;
    if (!p) return fail(c, GPSIG_ERR_INVALID, "params is NULL");
    if (p->dtype != GPSIG_F64) return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank mode is built for float64 only");
    if (spectral) {                  // the spectral entry points: the limits of the reverse pass and of the cross op, UNSUPPORTED beyond them
        if (p->base_kernel != GPSIG_BASE_SPECTRAL) return fail(c, GPSIG_ERR_INVALID, "the spectral entry points take the spectral base kernel");
        const int Q = int(p->base_params[0]), family = int(p->base_params[1]), d = p->num_features;
        if (Q < 1 || double(Q) != p->base_params[0] || family < 0 || family > 2 || double(family) != p->base_params[1])
            return fail(c, GPSIG_ERR_INVALID, "spectral kernel: bad number of components / family");
        if (Q > 64) return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral training path is built for at most 64 components");
        if (d > SPECTRAL_STRIDE) return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral base kernel is built for at most %d features", int(SPECTRAL_STRIDE));
        if (p->num_lags != 0 || (p->order != 1 && p->num_levels > 1)) return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral training path is built for order 1 without lags");
        if (nsk > LR_FUSED_MAX_SKETCHES) return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank mode is built for num_levels <= %d", LR_FUSED_MAX_SKETCHES + 1);
        if (cc > 64 || int64_t(cc) * d > int64_t(LR_GRAD_KS) * LR_GRAD_THREADS)
            return fail(c, GPSIG_ERR_UNSUPPORTED, "the spectral training path is built for num_components <= 64 and num_components x columns <= %d", LR_GRAD_KS * LR_GRAD_THREADS);
    } else if (p->base_kernel == GPSIG_BASE_SPECTRAL) {
        return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank mode is not built for the spectral base kernel");
    }
    if (!spectral && (p->base_kernel < GPSIG_BASE_LINEAR || p->base_kernel > GPSIG_BASE_MATERN52)) return fail(c, GPSIG_ERR_INVALID, "unknown base kernel %d", p->base_kernel);
    if (p->num_levels < 1) return fail(c, GPSIG_ERR_INVALID, "num_levels must be >= 1");
    if (p->order != 1 && p->num_levels > 1) return fail(c, GPSIG_ERR_UNSUPPORTED, "Low-rank mode not implemented for order higher than 1.");
    if (cc < 1 || r < 1) return fail(c, GPSIG_ERR_INVALID, "num_components and rank_bound must be positive");
    if (nsk != p->num_levels - 1) return fail(c, GPSIG_ERR_INVALID, "need one sketch per level 2..num_levels");
    if (c->ptr_mode != GPSIG_PTR_DEVICE) return fail(c, GPSIG_ERR_INVALID, "the training-path low-rank entry points take device pointers");
    if (p->num_features < 1 || p->num_lags != 0) return fail(c, GPSIG_ERR_INVALID, "the level primitives take their columns as they come (num_lags = 0)");
    HIPCHK(c, hipSetDevice(c->device));
    return GPSIG_OK;
}

// what the helpers below take of a call: its sizes (F = 1 + c + (M - 1) r columns of Phi; Q and family of a spectral call), the landmarks, the
// whitening and, once upload_sketches has run, the projections
struct LrCall {
    gpsig_ctx* c; const gpsig_params* p;
    int cc, r, nsk, M, d, F, Q, family;
    const double *S, *Wh;
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
};
// the spectral entry points' parameters and what their reverse passes add up over the points
struct LrSpectral {
    const double *alpha, *omega, *gamma;
    double *gS, *dalpha, *domega, *dgamma;
};

// how every entry point opens: check(), then `bad` -- the entry's own size / NULL test (of its arguments alone, so it is evaluated beforehand).
// The entry's plan and LDS refusals come next, then upload_sketches into k->gs.
int open(LrCall* k, gpsig_ctx* c, const gpsig_params* p, int cc, int r, int nsk, const double* S, const double* Wh, bool spectral, bool bad) {
    CHK(check(c, p, cc, r, nsk, spectral));
    k->c = c; k->p = p; k->cc = cc; k->r = r; k->nsk = nsk; k->M = p->num_levels; k->d = p->num_features;
    k->F = 1 + cc + (k->M - 1) * r;
    k->Q = spectral ? int(p->base_params[0]) : 0; k->family = spectral ? int(p->base_params[1]) : 0;
    k->S = S; k->Wh = Wh;
    if (bad) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    return GPSIG_OK;
}

// ... and the tensor entry points, whose own checks come before the NULL test: the reverse kernel's per-thread tables and the LDS footprints of
// both directions
int tens_open(LrCall* k, gpsig_ctx* c, const gpsig_params* p, int cc, int r, int nsk, const double* S, const double* Wh, bool spectral, int64_t T, int E,
              bool bad) {
    CHK(open(k, c, p, cc, r, nsk, S, Wh, spectral, false));
    const int M = k->M, d = k->d, lt = M * (M + 1) / 2;
    if (T < 0 || T > 0x7fffffff) return fail(c, GPSIG_ERR_INVALID, "bad number of tensors");
    if (M - 1 > LR_FUSED_MAX_SKETCHES) return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank mode is built for num_levels <= %d", LR_FUSED_MAX_SKETCHES + 1);
    if (cc > 64 || int64_t(cc) * d > int64_t(LR_GRAD_KS) * LR_GRAD_THREADS)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "the low-rank reverse pass is built for num_components <= 64 and num_components x columns <= %d", LR_GRAD_KS * LR_GRAD_THREADS);
    const size_t lds = std::max(lr_tens_grad_lds_bytes(cc, r, d, lt, E, M), lr_tens_fused_lds_bytes(cc, r, d, lt, E));
    if (lds > LR_FUSED_MAX_LDS) return fail(c, GPSIG_ERR_UNSUPPORTED, "a tensor's low-rank arrays (%zu bytes) exceed the LDS", lds);
    if (bad) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    return GPSIG_OK;
}

// the plan of one direction of the sequence kernels (from L alone): refused where not even the smallest tile fits the LDS ...
int forward_plan(const LrCall& k, int L, LrTileDir* D) {
    *D = lr_tile_dir(false, k.cc, k.r, k.d, L, k.p->difference ? L - 1 : L, k.c->lr_fused_pad);
    if (!D->untiled && D->TL == 0)
        return fail(k.c, GPSIG_ERR_UNSUPPORTED, "a %d-step tile of a sequence's low-rank arrays (%zu bytes) exceeds the LDS", LR_TILE_STEP,
                    lr_tiled_fused_lds_bytes(k.cc, k.r, k.d, LR_TILE_STEP, k.c->lr_fused_pad));
    return GPSIG_OK;
}
// ... and in the reverse pass, for launches of at most `nb` sequences, also where one workgroup's scratch (`extra` doubles beyond the E_i)
// exceeds its budget
int reverse_plan(const LrCall& k, int L, int64_t N, int64_t nb, int64_t extra, LrTilePlan* plan) {
    *plan = lr_tile_plan(k.cc, k.r, k.d, L, k.M, k.p->difference, k.c->lr_fused_pad, nb, extra);
    if (!plan->rev.untiled && plan->rev.TL == 0)
        return fail(k.c, GPSIG_ERR_UNSUPPORTED, "a %d-step tile of a sequence's low-rank arrays (%zu bytes) exceeds the LDS in the reverse pass", LR_TILE_STEP,
                    lr_tiled_grad_lds_bytes(k.cc, k.r, k.d, LR_TILE_STEP, k.c->lr_fused_pad));
    if (N > 0 && plan->grid == 0)
        return fail(k.c, GPSIG_ERR_UNSUPPORTED, "one workgroup's scratch for a sequence of %d steps (%lld bytes) exceeds the reverse pass's budget", plan->l,
                    (long long)(plan->escr_stride * int64_t(sizeof(double))));
    return GPSIG_OK;
}

// alpha (Q), omega (Q, d), gamma (Q, d) -> the table layout of the spectral fused instances: alpha[Q], omega[Q][SPECTRAL_STRIDE],
// gamma[Q][SPECTRAL_STRIDE], zero beyond the d features
__global__ __launch_bounds__(256) void lr_spectral_pack_kernel(const double* __restrict__ alpha, const double* __restrict__ omega,
                                                               const double* __restrict__ gamma, int Q, int d, double* __restrict__ tab) {
    const int n = Q * (1 + 2 * SPECTRAL_STRIDE);
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += gridDim.x * blockDim.x) {
        double v = 0.0;
        if (q < Q) {
            v = alpha[q];
        } else {
            const int k = q - Q, which = k / (Q * SPECTRAL_STRIDE), rem = k - which * Q * SPECTRAL_STRIDE;
            const int row = rem / SPECTRAL_STRIDE, f = rem - row * SPECTRAL_STRIDE;
            if (f < d) v = (which ? gamma : omega)[row * d + f];
        }
        tab[q] = v;
    }
}

// ... packed on the device, in B_SPECD
int spectral_table(const LrCall& k, const double* alpha, const double* omega, const double* gamma, const double** tab) {
    void* t;
    const int ntab = k.Q * (1 + 2 * SPECTRAL_STRIDE);
    CHK(ensure(k.c, B_SPECD, sizeof(double) * size_t(ntab) + 64, &t));
    hipLaunchKernelGGL(lr_spectral_pack_kernel, dim3(unsigned((ntab + 255) / 256)), dim3(256), 0, k.c->stream, alpha, omega, gamma, k.Q, k.d,
                       static_cast<double*>(t));
    HIPCHK(k.c, hipGetLastError());
    *tab = static_cast<const double*>(t);
    return GPSIG_OK;
}

// an empty batch: the sums over it are zeros (g_base may be NULL; `sp`: the spectral parameters' sums in its place)
int zero_outputs(const LrCall& k, double* gS, double* gWh, double* g_base, const LrSpectral* sp = nullptr) {
    gpsig_ctx* c = k.c;
    CHK(zero_async(c, gS, sizeof(double) * size_t(k.cc) * k.d));
    CHK(zero_async(c, gWh, sizeof(double) * size_t(k.cc) * k.cc));
    if (g_base) CHK(zero_async(c, g_base, sizeof(double)));
    if (sp) {
        CHK(zero_async(c, sp->dalpha, sizeof(double) * size_t(k.Q)));
        CHK(zero_async(c, sp->domega, sizeof(double) * size_t(k.Q) * k.d));
        CHK(zero_async(c, sp->dgamma, sizeof(double) * size_t(k.Q) * k.d));
    }
    return GPSIG_OK;
}

// the partial sums of `nparts` workgroups added up in workgroup order: rows of dS (c d), dWh (c c) and the base parameter's one, or with
// `dwh_only` (the spectral reverse kernels) of dWh alone
int reduce_partials(const LrCall& k, const void* part, int64_t nparts, bool dwh_only, double* gS, double* gWh, double* g_base) {
    const int64_t nS = dwh_only ? 0 : int64_t(k.cc) * k.d, nW = int64_t(k.cc) * k.cc, width = nS + nW + (dwh_only ? 0 : 1);
    hipLaunchKernelGGL(lr_grad_reduce_kernel, dim3(unsigned((width + 255) / 256)), dim3(256), 0, k.c->stream, static_cast<const double*>(part), int(nparts), width,
                       gS, nS, gWh, nW, g_base);
    HIPCHK(k.c, hipGetLastError());
    return GPSIG_OK;
}

// the fields the forward argument blocks share (LrFusedArgs, LrTensFusedArgs; the launchers derive F, lp and rows_b) ...
template <typename Args>
void forward_fields(const LrCall& k, const double* spec, void* Phi, Args* A) {
    A->P.d_in = k.d;
    A->S = k.S; A->Wh = k.Wh;
    A->c = k.cc; A->r = k.r; A->M = k.M; A->kind = int(k.p->base_kernel);
    A->p0 = k.p->base_params[0]; A->p1 = k.p->base_params[1];
    A->spec = spec;
    for (int i = 0; i < k.nsk; ++i) A->sk[i] = LrFusedSketch{k.gs[i].colptr, k.gs[i].ent};
    A->Phi = static_cast<double*>(Phi);
}
// ... and the reverse ones (LrGradArgs, LrTensGradArgs)
template <typename Args>
void reverse_fields(const LrCall& k, Args* A) {
    A->d = k.d;
    A->S = k.S; A->Wh = k.Wh;
    A->c = k.cc; A->r = k.r; A->M = k.M; A->kind = int(k.p->base_kernel);
    A->p0 = k.p->base_params[0]; A->p1 = k.p->base_params[1];
    for (int i = 0; i < k.nsk; ++i) A->sk[i] = k.gs[i];
    A->F = k.F;
}

// the LrFusedArgs fields of a call on device-resident landmarks and whitening
void fused_args(const LrCall& k, const void* X, int64_t N, int L, const double* spec, void* Phi, LrFusedArgs* A) {
    A->X = static_cast<const double*>(X); A->N = N; A->L = L;
    A->difference = k.p->difference;
    forward_fields(k, spec, Phi, A);
}

// the fused feature kernels (lr_fused_inst.hip) on device-resident landmarks and whitening: the caller scaled the inputs (no lengthscales,
// no lags); `two` picks the two-array form, else the three-array instance of lr_fused_variant
int fused_features(const LrCall& k, const void* X, int64_t N, int L, const double* spec, bool two, void* Phi, const char* what,
                   const int32_t* lengths = nullptr) {
    gpsig_ctx* c = k.c;
    LrFusedRaggedArgs A{};                       // (with `lengths` the ragged instance of the three-array form, lr_ragged_inst.hip)
    A.lengths = lengths;
    fused_args(k, X, N, L, spec, Phi, &A);
    const int rc = lengths ? lr_ragged_fused_launch(c->stream, A, c->lr_fused_pad)
                           : lr_fused_launch(c->stream, static_cast<const LrFusedArgs&>(A), c->lr_fused_pad, two, c->lr_fused_variant);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "%s: %s", what, hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

// the LrGradArgs fields the sequence reverse passes fill the same way; the caller sets the sequences, dPhi, part and what is its own
void grad_args(const LrCall& k, int L, void* escr, int64_t escr_stride, LrGradArgs* A) {
    A->L = L;
    A->difference = k.p->difference;
    reverse_fields(k, A);
    A->escr = static_cast<double*>(escr); A->escr_stride = escr_stride;
    A->lp = lr_fused_stride(L, k.c->lr_fused_pad);
    A->rows_b = lr_grad_rows(k.cc, k.r, k.d);
}

// the tiled kernels' arguments (lr_tiled_kernel.hpp) from the plan of one direction
void tiled_args(const LrCall& k, int L, const LrTileDir& D, bool reverse, LrTiledArgs* A) {
    grad_args(k, L, nullptr, 0, A);
    A->lp = D.lp; A->TL = D.TL; A->ntiles = D.ntiles;
    A->rows_b = reverse ? lr_grad_rows(k.cc, k.r, k.d) : lr_fused_rows(k.cc, k.r, k.d);
}

// the reverse kernel in the workgroup size lr_grad_threads picks: one workgroup per CU at these LDS sizes, 1024 threads give the scalar
// loads of the projections' entries twice the wavefronts to hide behind
template <typename Args>
int grad_launch(gpsig_ctx* c, const Args& A, unsigned grid, size_t lds) {
    // (the tiled form is built at 512 threads alone: at 1024, 128 registers a thread, it would keep scratch memory)
    const bool wide = c->lr_grad_threads != 512 && !std::is_same<Args, LrTiledArgs>::value;
    void (*kern)(Args);
    if constexpr (std::is_same<Args, LrGradSpectralArgs>::value)
        kern = wide ? lr_seq_features_grad_spectral_kernel<1024> : lr_seq_features_grad_spectral_kernel<512>;
    else if constexpr (std::is_same<Args, LrTiledArgs>::value)
        kern = lr_seq_features_grad_tiled_kernel<512>;
    else
        kern = wide ? lr_seq_features_grad_kernel<1024> : lr_seq_features_grad_kernel<512>;
    const int rc = lr_launch(kern, grid, wide ? 1024 : 512, lds, c->stream, A);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "low-rank reverse kernel: %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

// the fused tensor kernels (lr_fused_inst.hip) on device-resident landmarks and whitening: already-scaled tensors, no lengthscales, no lags
int tens_features(const LrCall& k, const void* Z, int64_t T, int E, const double* spec, void* Phi, const char* what) {
    LrTensFusedArgs A{};
    A.Z = static_cast<const double*>(Z); A.T = T; A.lt = k.M * (k.M + 1) / 2; A.E = E;
    forward_fields(k, spec, Phi, &A);
    const int rc = lr_tens_fused_launch(k.c->stream, A);
    if (rc != 0) return fail(k.c, GPSIG_ERR_HIP, "%s: %s", what, hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

void tens_grad_args(const LrCall& k, const void* Z, int64_t T, int E, const void* dPhi, LrTensGradArgs* A) {
    A->Z = static_cast<const double*>(Z); A->T = T; A->lt = k.M * (k.M + 1) / 2; A->E = E;
    reverse_fields(k, A);
    A->dPhi = static_cast<const double*>(dPhi);
}

template <typename Args>
int tens_grad_launch(gpsig_ctx* c, const Args& A, unsigned grid) {
    void (*kern)(Args);
    if constexpr (std::is_same<Args, LrTensGradSpectralArgs>::value) kern = lr_tens_features_grad_spectral_kernel;
    else kern = lr_tens_features_grad_kernel;
    const int rc = lr_launch(kern, grid, LR_TENS_GRAD_THREADS, lr_tens_grad_lds_bytes(A.c, A.r, A.d, A.lt, A.E, A.M), c->stream, A);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "low-rank tensor reverse kernel: %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

// the launch result of a ragged reverse instance (lr_ragged_inst.hip), as grad_launch reports its own
int ragged_rc(gpsig_ctx* c, int rc) {
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "low-rank reverse kernel (ragged): %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

// the spectral cross op's reverse pass on n rows of L points P with their dkxs G: dP, and dS and the parameters' sums stored or, with
// `accumulate`, added.  `lengths` (n of them, or NULL): the lengths-aware kernels.
int cross_grad(const LrCall& k, const LrSpectral& sp, const double* P, int64_t n, int L, const int32_t* lengths, const double* G, double* dP, double* part,
               bool accumulate) {
    const int rc = lengths ? spectral_cross_grad_len_launch(k.c->stream, k.Q, k.family, k.d, P, n, L, lengths, k.S, k.cc, sp.alpha, sp.omega, sp.gamma, G, dP,
                                                            part, sp.gS, sp.dalpha, sp.domega, sp.dgamma, accumulate)
                           : spectral_cross_grad_launch(k.c->stream, k.Q, k.family, k.d, P, n * L, k.S, k.cc, sp.alpha, sp.omega, sp.gamma, G, dP, part, sp.gS,
                                                        sp.dalpha, sp.domega, sp.dgamma, accumulate);
    if (rc != 0) return fail(k.c, GPSIG_ERR_HIP, "spectral cross reverse pass: %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

// sequences (tensors) per chunk of a spectral reverse pass: dkxs of a chunk, `each` doubles per sequence, within the budget
int64_t spectral_chunk(int64_t n, int64_t each) {
    return std::min<int64_t>(n, std::max<int64_t>(1, int64_t(LR_SPECTRAL_DKXS_BUDGET) / (each * int64_t(sizeof(double)))));
}

// one chunk: sequences (tensors) n0 .. n0 + nn - 1, the workgroups of its launch, their dWh partials and scratch, the chunk's dkxs and the
// cross op's partials
struct LrChunk {
    int64_t n0, nn;
    unsigned grid;
    double *part, *escr, *dk, *cpart;
};

// the spectral reverse passes over n > 0 sequences (tensors) in chunks of nb, a chunk on min(its size, gmax) workgroups: `reverse` launches
// the reverse kernel on a chunk, `cross` takes the chunk's dkxs through the cross op (accumulating from the second chunk on); then the dWh
// partials of all workgroups are reduced.  Scratch in doubles: escr_each per workgroup (0: none), dk_each per sequence, cross_doubles.
template <typename Reverse, typename Cross>
int spectral_reverse(const LrCall& k, int64_t n, int64_t nb, int64_t gmax, size_t escr_each, size_t dk_each, size_t cross_doubles, double* gS, double* gWh,
                     Reverse reverse, Cross cross) {
    gpsig_ctx* c = k.c;
    const int64_t cc2 = int64_t(k.cc) * k.cc;
    int64_t nparts = 0;                                                // workgroups over all chunks: one dWh partial each
    for (int64_t n0 = 0; n0 < n; n0 += nb) nparts += std::min(std::min(nb, n - n0), gmax);
    void *part, *escr = nullptr, *dk, *cpart;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(nparts) * size_t(cc2) + 64, &part));
    if (escr_each) CHK(ensure(c, B_GR1, sizeof(double) * size_t(gmax) * escr_each + 64, &escr));
    CHK(ensure(c, B_LRDK, sizeof(double) * size_t(nb) * dk_each + 64, &dk));
    CHK(ensure(c, B_GR2, sizeof(double) * cross_doubles + 64, &cpart));
    int64_t at = 0;
    for (int64_t n0 = 0; n0 < n; n0 += nb) {
        const int64_t nn = std::min(nb, n - n0);
        const LrChunk ch{n0, nn, unsigned(std::min(nn, gmax)), static_cast<double*>(part) + at * cc2, static_cast<double*>(escr), static_cast<double*>(dk),
                         static_cast<double*>(cpart)};
        CHK(reverse(ch));
        CHK(cross(ch));
        at += ch.grid;
    }
    return reduce_partials(k, part, nparts, true, gS, gWh, nullptr);
}

// the host path of gpsig_lr_seq_features_dev and of its ragged twin (`lengths`: NULL, or N per-sequence lengths on the device): checks and plan
// are those of L either way -- the plan does not depend on the lengths, so the host never reads them
int seq_features_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* X,
                     int64_t N, int32_t L, const int32_t* lengths, const double* S, const double* Wh, void* Phi) {
    LrCall k;
    CHK(open(&k, c, p, cc, r, nsk, S, Wh, false, N < 0 || L < 1 || (N > 0 && (!X || !S || !Wh || !Phi))));
    // always the three-array form (the instance of lr_fused_variant): lr_fused does not apply here; beyond the LDS its time-tiled form
    LrTileDir D;
    CHK(forward_plan(k, L, &D));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (N == 0) return GPSIG_OK;
    if (D.untiled) return fused_features(k, X, N, L, nullptr, false, Phi, "fused low-rank feature kernel", lengths);
    LrTiledRaggedArgs A{};
    tiled_args(k, L, D, false, &A);
    A.X = static_cast<const double*>(X); A.N = N;
    A.Phi = static_cast<double*>(Phi);
    A.lengths = lengths;
    const unsigned grid = unsigned(N < (1 << 20) ? N : (1 << 20));
    const int rc = lengths ? lr_ragged_tiled_launch(c->stream, A, grid, D.lds)
                           : lr_launch(lr_seq_features_tiled_kernel<1024>, grid, 1024, D.lds, c->stream, static_cast<const LrTiledArgs&>(A));
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "tiled low-rank feature kernel: %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

// ... and of gpsig_lr_seq_features_grad and its ragged twin
int seq_features_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* X,
                      int64_t N, int32_t L, const int32_t* lengths, const double* S, const double* Wh, const void* dPhi, void* gX, double* gS,
                      double* gWh, double* g_base) {
    LrCall k;
    CHK(open(&k, c, p, cc, r, nsk, S, Wh, false, N < 0 || L < 1 || !gS || !gWh || (N > 0 && (!X || !S || !Wh || !dPhi || !gX))));
    if (cc > 64 || int64_t(cc) * k.d > int64_t(LR_GRAD_KS) * LR_GRAD_THREADS)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "the low-rank reverse pass is built for num_components <= 64 and num_components x columns <= %d", LR_GRAD_KS * LR_GRAD_THREADS);
    LrTilePlan plan;
    CHK(reverse_plan(k, L, N, N, 0, &plan));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (N == 0) return zero_outputs(k, gS, gWh, g_base);
    // one workgroup per CU at these LDS sizes, two rounds' worth of them (512); fewer where the tiled form's scratch would exceed its budget
    const unsigned grid = unsigned(plan.grid);
    const size_t lds = plan.rev.lds;
    void *part, *escr;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(grid) * size_t(int64_t(cc) * k.d + int64_t(cc) * cc + 1) + 64, &part));
    CHK(ensure(c, B_GR1, sizeof(double) * size_t(grid) * size_t(plan.escr_stride) + 64, &escr));
    const auto batch = [&](auto* A) {                                  // what the whole-sequence and the tiled block take alike
        A->escr = static_cast<double*>(escr); A->escr_stride = plan.escr_stride;
        A->X = static_cast<const double*>(X); A->N = N;
        A->dPhi = static_cast<const double*>(dPhi);
        A->gX = static_cast<double*>(gX);
        A->part = static_cast<double*>(part);
        A->lengths = lengths;
    };
    if (plan.rev.untiled) {
        LrGradRaggedArgs A{};
        grad_args(k, L, nullptr, 0, &A);
        batch(&A);
        if (lengths) CHK(ragged_rc(c, lr_ragged_grad_launch(c->stream, A, grid, lds)));
        else CHK(grad_launch(c, static_cast<const LrGradArgs&>(A), grid, lds));
    } else {
        LrTiledRaggedArgs A{};
        tiled_args(k, L, plan.rev, true, &A);
        batch(&A);
        if (lengths) CHK(ragged_rc(c, lr_ragged_grad_tiled_launch(c->stream, A, grid, lds)));
        else CHK(grad_launch(c, static_cast<const LrTiledArgs&>(A), grid, lds));
    }
    return reduce_partials(k, part, grid, false, gS, gWh, g_base);
}

// the host path of gpsig_lr_seq_features_spectral_grad (`whole_only`: the whole-sequence spectral instances in the workgroup size lr_grad_threads
// picks, nothing beyond the LDS) and of its lengths-aware twin (whole sequences or time tiles; `lengths` may be NULL)
int spectral_seq_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* X, int64_t N,
                      int32_t L, const int32_t* lengths, bool whole_only, const double* S, const double* Wh, const LrSpectral& sp, const void* dPhi,
                      void* gX, double* gWh) {
    LrCall k;
    CHK(open(&k, c, p, cc, r, nsk, S, Wh, true,
             N < 0 || L < 1 || !sp.gS || !gWh || !sp.dalpha || !sp.domega || !sp.dgamma ||
                 (N > 0 && (!X || !S || !Wh || !sp.alpha || !sp.omega || !sp.gamma || !dPhi || !gX))));
    const int d = k.d;
    // sequences per chunk; the plan of a chunk, with kxs (c, L) in each workgroup's scratch.  Whole sequences: min(chunk, 512) workgroups, as the
    // other families' reverse pass (tests/emu/test_lr_tile_plan.cpp holds the plan to the numbers this pass was written with)
    const int64_t nb = spectral_chunk(N, int64_t(L) * cc);
    LrTilePlan plan;
    if (whole_only) {
        plan = lr_tile_plan(cc, r, d, L, k.M, p->difference, c->lr_fused_pad, nb, int64_t(cc) * L);
        const size_t lds = lr_grad_lds_bytes(cc, r, d, L, c->lr_fused_pad);
        if (lds > LR_FUSED_MAX_LDS) return fail(c, GPSIG_ERR_UNSUPPORTED, "a sequence's low-rank arrays (%zu bytes) exceed the LDS in the reverse pass", lds);
    } else {
        CHK(reverse_plan(k, L, N, nb, int64_t(cc) * L, &plan));
    }
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (N == 0) return zero_outputs(k, sp.gS, gWh, nullptr, &sp);
    LrGradSpectralLenArgs W{};                                          // whole sequences ...
    LrTiledSpectralArgs T{};                                            // ... or time tiles
    if (plan.rev.untiled) {
        grad_args(k, L, nullptr, plan.escr_stride, &W);
        W.alpha = sp.alpha; W.omega = sp.omega; W.gamma = sp.gamma;
    } else {
        tiled_args(k, L, plan.rev, true, &T);
        T.escr_stride = plan.escr_stride;
        T.alpha = sp.alpha; T.omega = sp.omega; T.gamma = sp.gamma; T.ld = d;
    }
    W.kxs_off = T.kxs_off = plan.escr_stride - int64_t(cc) * L - 8;
    LrGradArgs& A = plan.rev.untiled ? static_cast<LrGradArgs&>(W) : static_cast<LrGradArgs&>(T);
    return spectral_reverse(
        k, N, nb, plan.grid, size_t(plan.escr_stride), size_t(L) * cc, spectral_cross_grad_part_doubles(nb * L, cc, d, k.Q), sp.gS, gWh,
        [&](const LrChunk& ch) -> int {
            A.X = static_cast<const double*>(X) + ch.n0 * int64_t(L) * d; A.N = ch.nn;
            A.dPhi = static_cast<const double*>(dPhi) + ch.n0 * int64_t(k.F);
            A.part = ch.part; A.escr = ch.escr;
            W.dkxs = T.dkxs = ch.dk;
            W.lengths = T.lengths = lengths ? lengths + ch.n0 : nullptr;
            if (whole_only) return grad_launch(c, static_cast<const LrGradSpectralArgs&>(W), ch.grid, plan.rev.lds);
            const int rc = plan.rev.untiled ? lr_spectral_len_grad_launch(c->stream, W, ch.grid, plan.rev.lds)
                                            : lr_spectral_grad_tiled_launch(c->stream, T, ch.grid, plan.rev.lds);
            if (rc != 0) return fail(c, GPSIG_ERR_HIP, "low-rank spectral reverse kernel (lengths-aware): %s", hipGetErrorString(hipError_t(rc)));
            return GPSIG_OK;
        },
        [&](const LrChunk& ch) -> int {
            return cross_grad(k, sp, A.X, ch.nn, L, W.lengths, ch.dk, static_cast<double*>(gX) + ch.n0 * int64_t(L) * d, ch.cpart, ch.n0 > 0);
        });
}

// ---- the entry points behind the cross matrix (lr_kx.hpp): what open() leaves to them.  p->num_features is the width of the points kxs was
// computed from and is not used: the plans have max(c, r) rows.
int kx_open(LrCall* k, gpsig_ctx* c, const gpsig_params* p, int cc, int r, int nsk, const double* Wh, bool bad) {
    CHK(open(k, c, p, cc, r, nsk, nullptr, Wh, false, false));
    k->d = 0;
    if (k->M - 1 > LR_FUSED_MAX_SKETCHES) return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank mode is built for num_levels <= %d", LR_FUSED_MAX_SKETCHES + 1);
    if (cc > 64) return fail(c, GPSIG_ERR_UNSUPPORTED, "the low-rank training path is built for num_components <= 64");
    if (bad) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    return GPSIG_OK;
}
int kx_plan(const LrCall& k, bool reverse, int L, LrTileDir* D) {
    *D = lr_kx_tile_dir(reverse, k.cc, k.r, L, k.p->difference ? L - 1 : L, k.c->lr_fused_pad);
    if (D->TL == 0)
        return fail(k.c, GPSIG_ERR_UNSUPPORTED, "a %d-step tile of a sequence's low-rank arrays (%zu bytes) exceeds the LDS", LR_TILE_STEP,
                    reverse ? lr_tiled_grad_lds_bytes(k.cc, k.r, 0, LR_TILE_STEP, k.c->lr_fused_pad)
                            : lr_tiled_fused_lds_bytes(k.cc, k.r, 0, LR_TILE_STEP, k.c->lr_fused_pad));
    return GPSIG_OK;
}
int kx_tens_open(LrCall* k, gpsig_ctx* c, const gpsig_params* p, int cc, int r, int nsk, const double* Wh, int64_t T, int E, bool bad) {
    CHK(kx_open(k, c, p, cc, r, nsk, Wh, false));
    const int lt = k->M * (k->M + 1) / 2;
    if (T < 0 || T > 0x7fffffff) return fail(c, GPSIG_ERR_INVALID, "bad number of tensors");
    const size_t lds = std::max(lr_tens_grad_lds_bytes(cc, r, 0, lt, E, k->M), lr_tens_fused_lds_bytes(cc, r, 0, lt, E));
    if (lds > LR_FUSED_MAX_LDS) return fail(c, GPSIG_ERR_UNSUPPORTED, "a tensor's low-rank arrays (%zu bytes) exceed the LDS", lds);
    if (bad) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    return GPSIG_OK;
}

}  // namespace

extern "C" {

int gpsig_lr_seq_features_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* X,
                              int64_t N, int32_t L, const double* S, const double* Wh, void* Phi) {
    return seq_features_dev(c, p, cc, r, nsk, sketches, X, N, L, nullptr, S, Wh, Phi);
}

int gpsig_lr_seq_features_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* X,
                               int64_t N, int32_t L, const double* S, const double* Wh, const void* dPhi, void* gX, double* gS, double* gWh,
                               double* g_base) {
    return seq_features_grad(c, p, cc, r, nsk, sketches, X, N, L, nullptr, S, Wh, dPhi, gX, gS, gWh, g_base);
}

// ... of a ragged batch: sequence n has lengths[n] points (N int32 on the device, 1 <= lengths[n] <= L; the kernels clamp)
int gpsig_lr_seq_features_ragged_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                     const void* X, int64_t N, int32_t L, const int32_t* lengths, const double* S, const double* Wh, void* Phi) {
    if (c && N > 0 && !lengths) return fail(c, GPSIG_ERR_INVALID, "lengths is NULL");
    return seq_features_dev(c, p, cc, r, nsk, sketches, X, N, L, lengths, S, Wh, Phi);
}

int gpsig_lr_seq_features_ragged_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                      const void* X, int64_t N, int32_t L, const int32_t* lengths, const double* S, const double* Wh,
                                      const void* dPhi, void* gX, double* gS, double* gWh, double* g_base) {
    if (c && N > 0 && !lengths) return fail(c, GPSIG_ERR_INVALID, "lengths is NULL");
    return seq_features_grad(c, p, cc, r, nsk, sketches, X, N, L, lengths, S, Wh, dPhi, gX, gS, gWh, g_base);
}

int gpsig_lr_seq_features_spectral_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                       const void* X, int64_t N, int32_t L, const double* S, const double* Wh, const double* alpha,
                                       const double* omega, const double* gamma, void* Phi) {
    LrCall k;
    CHK(open(&k, c, p, cc, r, nsk, S, Wh, true, N < 0 || L < 1 || (N > 0 && (!X || !S || !Wh || !alpha || !omega || !gamma || !Phi))));
    // the two-array kernel where lr_fused == 1 and it is built, else the three-array one (also for lr_fused == 0); the footprint of that form
    const bool two = c->lr_fused == 1 && lr_fused2_ok(cc, r, L);
    const size_t lds = two ? lr_fused2_lds_bytes(cc, r, k.d, L, c->lr_fused_pad) : lr_fused_lds_bytes(cc, r, k.d, L, c->lr_fused_pad);
    if (lds > LR_FUSED_MAX_LDS) return fail(c, GPSIG_ERR_UNSUPPORTED, "a sequence's low-rank arrays (%zu bytes) exceed the LDS", lds);
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (N == 0) return GPSIG_OK;
    const double* tab;
    CHK(spectral_table(k, alpha, omega, gamma, &tab));
    return fused_features(k, X, N, L, tab, two, Phi, "fused low-rank spectral feature kernel");
}

int gpsig_lr_seq_features_spectral_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                        const void* X, int64_t N, int32_t L, const double* S, const double* Wh, const double* alpha,
                                        const double* omega, const double* gamma, const void* dPhi, void* gX, double* gS, double* gWh,
                                        double* dalpha, double* domega, double* dgamma) {
    return spectral_seq_grad(c, p, cc, r, nsk, sketches, X, N, L, nullptr, true, S, Wh, {alpha, omega, gamma, gS, dalpha, domega, dgamma}, dPhi, gX, gWh);
}

// ... of long and ragged batches: `lengths` directly after L (N int32 on the device, the kernels clamp to [1, L]; NULL: L points each).  Sequences
// beyond the LDS go in time tiles; the plan follows from L alone.
int gpsig_lr_seq_features_spectral_ragged_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                              const void* X, int64_t N, int32_t L, const int32_t* lengths, const double* S, const double* Wh,
                                              const double* alpha, const double* omega, const double* gamma, void* Phi) {
    LrCall k;
    CHK(open(&k, c, p, cc, r, nsk, S, Wh, true, N < 0 || L < 1 || (N > 0 && (!X || !S || !Wh || !alpha || !omega || !gamma || !Phi))));
    LrTileDir D;
    CHK(forward_plan(k, L, &D));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (N == 0) return GPSIG_OK;
    const double* tab;
    CHK(spectral_table(k, alpha, omega, gamma, &tab));
    int rc;
    if (D.untiled) {
        LrFusedSpectralLenArgs A{};
        fused_args(k, X, N, L, tab, Phi, &A);
        A.lengths = lengths;
        rc = lr_spectral_len_fused_launch(c->stream, A, c->lr_fused_pad);
    } else {
        LrTiledSpectralArgs A{};
        tiled_args(k, L, D, false, &A);
        A.X = static_cast<const double*>(X); A.N = N;
        A.Phi = static_cast<double*>(Phi);
        A.alpha = tab; A.omega = tab + k.Q; A.gamma = tab + k.Q + k.Q * SPECTRAL_STRIDE; A.ld = SPECTRAL_STRIDE;
        A.lengths = lengths;
        rc = lr_spectral_tiled_launch(c->stream, A, unsigned(N < (1 << 20) ? N : (1 << 20)), D.lds);
    }
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "low-rank spectral feature kernel (lengths-aware): %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

int gpsig_lr_seq_features_spectral_ragged_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                               const void* X, int64_t N, int32_t L, const int32_t* lengths, const double* S, const double* Wh,
                                               const double* alpha, const double* omega, const double* gamma, const void* dPhi, void* gX, double* gS,
                                               double* gWh, double* dalpha, double* domega, double* dgamma) {
    return spectral_seq_grad(c, p, cc, r, nsk, sketches, X, N, L, lengths, false, S, Wh, {alpha, omega, gamma, gS, dalpha, domega, dgamma}, dPhi, gX, gWh);
}

int gpsig_lr_tens_features_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* Z,
                               int64_t T, int32_t increments, const double* S, const double* Wh, void* Phi) {
    LrCall k;
    const int E = increments ? 2 : 1;
    CHK(tens_open(&k, c, p, cc, r, nsk, S, Wh, false, T, E, T > 0 && (!Z || !S || !Wh || !Phi)));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (T == 0) return GPSIG_OK;
    return tens_features(k, Z, T, E, nullptr, Phi, "fused low-rank tensor feature kernel");
}

int gpsig_lr_tens_features_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* Z,
                                int64_t T, int32_t increments, const double* S, const double* Wh, const void* dPhi, void* gZ, double* gS, double* gWh,
                                double* g_base) {
    LrCall k;
    const int E = increments ? 2 : 1;
    CHK(tens_open(&k, c, p, cc, r, nsk, S, Wh, false, T, E, !gS || !gWh || (T > 0 && (!Z || !S || !Wh || !dPhi || !gZ))));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (T == 0) return zero_outputs(k, gS, gWh, g_base);
    const unsigned grid = unsigned(T < 512 ? T : 512);                 // as the sequences' reverse pass: the partial sums stay bounded
    void* part;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(grid) * size_t(int64_t(cc) * k.d + int64_t(cc) * cc + 1) + 64, &part));
    LrTensGradArgs A{};
    tens_grad_args(k, Z, T, E, dPhi, &A);
    A.t0 = 0; A.nt = T;
    A.gZ = static_cast<double*>(gZ);
    A.part = static_cast<double*>(part);
    CHK(tens_grad_launch(c, A, grid));
    return reduce_partials(k, part, grid, false, gS, gWh, g_base);
}

int gpsig_lr_tens_features_spectral_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                        const void* Z, int64_t T, int32_t increments, const double* S, const double* Wh, const double* alpha,
                                        const double* omega, const double* gamma, void* Phi) {
    LrCall k;
    const int E = increments ? 2 : 1;
    CHK(tens_open(&k, c, p, cc, r, nsk, S, Wh, true, T, E, T > 0 && (!Z || !S || !Wh || !alpha || !omega || !gamma || !Phi)));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (T == 0) return GPSIG_OK;
    const double* tab;
    CHK(spectral_table(k, alpha, omega, gamma, &tab));
    return tens_features(k, Z, T, E, tab, Phi, "fused low-rank spectral tensor feature kernel");
}

int gpsig_lr_tens_features_spectral_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                         const void* Z, int64_t T, int32_t increments, const double* S, const double* Wh, const double* alpha,
                                         const double* omega, const double* gamma, const void* dPhi, void* gZ, double* gS, double* gWh,
                                         double* dalpha, double* domega, double* dgamma) {
    LrCall k;
    const int E = increments ? 2 : 1;
    CHK(tens_open(&k, c, p, cc, r, nsk, S, Wh, true, T, E,
                  !gS || !gWh || !dalpha || !domega || !dgamma || (T > 0 && (!Z || !S || !Wh || !alpha || !omega || !gamma || !dPhi || !gZ))));
    const LrSpectral sp{alpha, omega, gamma, gS, dalpha, domega, dgamma};
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (T == 0) return zero_outputs(k, gS, gWh, nullptr, &sp);
    const int d = k.d, lt = k.M * (k.M + 1) / 2;
    const int64_t nb = spectral_chunk(T, int64_t(lt) * E * cc);
    const bool whole = nb == T;                                        // one launch: dkx is in the flat point order of Z
    LrTensGradSpectralArgs A{};
    tens_grad_args(k, Z, T, E, dPhi, &A);
    A.alpha = alpha; A.omega = omega; A.gamma = gamma;
    return spectral_reverse(
        k, T, nb, 512, 0, size_t(lt) * E * cc, spectral_cross_grad_part_doubles(whole ? int64_t(lt) * T * E : nb * E, cc, d, k.Q), gS, gWh,
        [&](const LrChunk& ch) -> int {
            A.t0 = ch.n0; A.nt = ch.nn;
            A.part = ch.part; A.dkx = ch.dk;
            return tens_grad_launch(c, A, ch.grid);
        },
        [&](const LrChunk& ch) -> int {
            // the chunk's points: component k's are the run (k T + n0) E .. of Z's flat rows, nn E of them; their dkx rows k nn E ..
            for (int j = 0; j < (whole ? 1 : lt); ++j) {
                const int64_t row0 = (int64_t(j) * T + ch.n0) * E, n = whole ? int64_t(lt) * T * E : ch.nn * E;
                CHK(cross_grad(k, sp, static_cast<const double*>(Z) + row0 * d, n, 1, nullptr, ch.dk + int64_t(j) * ch.nn * E * cc,
                               static_cast<double*>(gZ) + row0 * d, ch.cpart, ch.n0 > 0 || j > 0));
            }
            return GPSIG_OK;
        });
}

// ---- behind the cross matrix: kxs (N, L, c) = kappa(X, S) from gpsig_lr_cross; `lengths` may be NULL (L points each)
int gpsig_lr_seq_features_kx_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const double* kxs,
                                 int64_t N, int32_t L, const int32_t* lengths, const double* Wh, void* Phi) {
    LrCall k;
    CHK(kx_open(&k, c, p, cc, r, nsk, Wh, N < 0 || L < 1 || (N > 0 && (!kxs || !Wh || !Phi))));
    LrTileDir D;
    CHK(kx_plan(k, false, L, &D));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (N == 0) return GPSIG_OK;
    LrTiledKxArgs A{};
    tiled_args(k, L, D, false, &A);
    A.X = kxs; A.d = cc; A.N = N;                    // (the bodies step through X in rows of d: lr_kx.hpp)
    A.Phi = static_cast<double*>(Phi);
    A.lengths = lengths;
    const int rc = lr_kx_tiled_launch(c->stream, A, unsigned(N < (1 << 20) ? N : (1 << 20)), D.lds);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "tiled low-rank feature kernel (kxs from memory): %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

int gpsig_lr_seq_features_kx_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const double* kxs,
                                  int64_t N, int32_t L, const int32_t* lengths, const double* Wh, const void* dPhi, double* dkxs, double* gWh) {
    LrCall k;
    CHK(kx_open(&k, c, p, cc, r, nsk, Wh, N < 0 || L < 1 || !gWh || (N > 0 && (!kxs || !Wh || !dPhi || !dkxs))));
    LrTileDir D;
    CHK(kx_plan(k, true, L, &D));
    // min(N, 512) workgroups, fewer where their E_i scratch would exceed its budget (lr_tile_plan's rule, here for every length)
    const int64_t escr_stride = lr_escr_stride(cc, r, k.M, p->difference ? L - 1 : L);
    const int64_t grid = std::min<int64_t>(std::min<int64_t>(N, LR_TILE_MAX_GRID), int64_t(LR_TILE_SCRATCH_BUDGET / (sizeof(double) * size_t(escr_stride))));
    if (N > 0 && grid == 0)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "one workgroup's scratch for a sequence of %d points (%lld bytes) exceeds the reverse pass's budget", L,
                    (long long)(escr_stride * int64_t(sizeof(double))));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (N == 0) return zero_async(c, gWh, sizeof(double) * size_t(cc) * cc);
    void *part, *escr;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(grid) * size_t(cc) * cc + 64, &part));
    CHK(ensure(c, B_GR1, sizeof(double) * size_t(grid) * size_t(escr_stride) + 64, &escr));
    LrTiledKxArgs A{};
    tiled_args(k, L, D, true, &A);
    A.escr = static_cast<double*>(escr); A.escr_stride = escr_stride;
    A.X = kxs; A.d = cc; A.N = N;
    A.dPhi = static_cast<const double*>(dPhi);
    A.dkxs = dkxs;
    A.part = static_cast<double*>(part);
    A.lengths = lengths;
    const int rc = lr_kx_grad_tiled_launch(c->stream, A, unsigned(grid), D.lds);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "tiled low-rank reverse kernel (kxs from memory): %s", hipGetErrorString(hipError_t(rc)));
    return reduce_partials(k, part, grid, true, nullptr, gWh, nullptr);
}

// ... and the inducing tensors': kzs (lt T E, c) = kappa of Z's points in their flat order
int gpsig_lr_tens_features_kx_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const double* kzs,
                                  int64_t T, int32_t increments, const double* Wh, void* Phi) {
    LrCall k;
    const int E = increments ? 2 : 1;
    CHK(kx_tens_open(&k, c, p, cc, r, nsk, Wh, T, E, T > 0 && (!kzs || !Wh || !Phi)));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (T == 0) return GPSIG_OK;
    LrTensKxArgs A{};
    A.T = T; A.lt = k.M * (k.M + 1) / 2; A.E = E;
    forward_fields(k, nullptr, Phi, &A);
    A.kzs = kzs;
    const int rc = lr_kx_tens_launch(c->stream, A);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "fused low-rank tensor feature kernel (kzs from memory): %s", hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

int gpsig_lr_tens_features_kx_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const double* kzs,
                                   int64_t T, int32_t increments, const double* Wh, const void* dPhi, double* dkzs, double* gWh) {
    LrCall k;
    const int E = increments ? 2 : 1;
    CHK(kx_tens_open(&k, c, p, cc, r, nsk, Wh, T, E, !gWh || (T > 0 && (!kzs || !Wh || !dPhi || !dkzs))));
    CHK(upload_sketches(c, cc, r, nsk, sketches, k.gs));
    if (T == 0) return zero_async(c, gWh, sizeof(double) * size_t(cc) * cc);
    const unsigned grid = unsigned(T < 512 ? T : 512);                 // as gpsig_lr_tens_features_grad
    void* part;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(grid) * size_t(cc) * cc + 64, &part));
    LrTensGradKxArgs A{};
    tens_grad_args(k, nullptr, T, E, dPhi, &A);
    A.t0 = 0; A.nt = T;                                                // one launch: dkzs is in the flat point order of Z
    A.part = static_cast<double*>(part);
    A.dkx = dkzs;
    A.kzs = kzs;
    const int rc = lr_kx_tens_grad_launch(c->stream, A, grid);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "low-rank tensor reverse kernel (kzs from memory): %s", hipGetErrorString(hipError_t(rc)));
    return reduce_partials(k, part, grid, true, nullptr, gWh, nullptr);
}

}  // extern "C"
