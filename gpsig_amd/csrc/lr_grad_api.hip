// lr_grad_api.hip -- low-rank sequence features with the landmarks and the whitening ON THE DEVICE, and their reverse pass (round 4).
//
// When the reference trains in low-rank mode, the Nystrom landmarks are gathered from the scaled inputs and their Gram is decomposed
// inside the differentiated graph (gpsig/low_rank_calculations.py:47-60): landmarks and whitening are functions of the trainable
// parameters, new at every step, and live where the step runs.  gpsig_lr_seq_features (api.hip) takes them from the host (or from a
// gpsig_lr_draw state) because the evaluation path's caller owns them; the training path's two entry points take device pointers:
//     gpsig_lr_seq_features_dev    Phi (N, F) = the fused feature kernel of lr_fused_kernel.hpp on (X, S, Wh), launched by
//                                  lr_fused_inst.hip (fused_features below: the evaluation path's arguments on device pointers)
//     gpsig_lr_seq_features_grad   dPhi (N, F) -> dX, dS, dWh, d base parameter: lr_grad_kernel.hpp
// Where a sequence's arrays exceed the LDS (lr_fused_lds_bytes / lr_grad_lds_bytes, lr_tile_plan.hpp), the same two entry points launch the
// time-tiled kernels of lr_tiled_kernel.hpp, each direction on its own: shapes that fit keep the whole-sequence kernels.  The tiled reverse
// pass keeps the E_i of a whole sequence per workgroup in B_GR1; the plan shrinks the grid to hold that within LR_TILE_SCRATCH_BUDGET.
// Ragged batches: gpsig_lr_seq_features_ragged_dev / _ragged_grad take N per-sequence lengths on the device and share the host paths of the pair
// above (seq_features_dev / seq_features_grad below, one optional pointer): same checks and plan, which follow from L alone, then the ragged
// instances of the same four kernels (lr_ragged_inst.hip).
// and SignatureSpectral's pair, whose parameters (alpha, omega, gamma) are trained and so come as device pointers too:
//     gpsig_lr_seq_features_spectral_dev    Phi by the spectral fused instances on a table packed on the device (no host round trip)
//     gpsig_lr_seq_features_spectral_grad   lr_seq_features_grad_spectral_kernel: dPhi -> dWh and dkxs (N, L, c) in scratch; then the
//                                           spectral cross op's reverse kernels: dkxs -> dX, dS, dalpha, domega, dgamma
// dkxs takes N L c doubles.  Above LR_SPECTRAL_DKXS_BUDGET bytes the sequences go in chunks that fit it: each chunk's dS and parameter sums
// are added to the outputs in chunk order, the dWh partials of all chunks are reduced once in workgroup order -- deterministic either way.
// Scratch: B_GR0 dWh partials, B_GR1 the per-workgroup E_i and kxs, B_LRDK dkxs, B_GR2 the cross op's partials (own buffers: none of them
// can be resized while another one's reader is queued; ensure() waits for the stream before it frees anything anyway).
// Long and ragged SignatureSpectral batches: gpsig_lr_seq_features_spectral_ragged_dev / _ragged_grad take the spectral pair's arguments and an
// optional `lengths` (NULL: every sequence has L points).  Checks and plan follow from L alone, as for the other families; then the spectral
// instances of lr_spectral_tiled_inst.hip, whole sequence or time-tiled, each direction on its own.  The reverse kernels stop at dkxs and keep kxs
// of a whole sequence next to the E_i in B_GR1 (c L doubles more per workgroup, inside the plan's budget); dkxs goes to the lengths-aware
// reverse kernels of the spectral cross op, in chunks of LR_SPECTRAL_DKXS_BUDGET as above.
// The inducing tensors' feature map (_K_tens_lr_feat, kernels.py:285-311) has the same two pairs:
//     gpsig_lr_tens_features_dev / _spectral_dev     Phi (T, F) by the fused tensor kernels of lr_fused_kernel.hpp (lr_tens_fused_launch)
//     gpsig_lr_tens_features_grad / _spectral_grad   lr_tens_grad_kernel.hpp: dPhi -> dZ, dS, dWh, d base parameter; the spectral instance stops
//                                                    at dkx (lt T E, c), which the cross op's reverse kernels take with Z viewed (lt T E, d)
// Above the dkx budget the tensors go in chunks: a chunk's points are lt runs of Z, one per component, each handed to the cross op in turn.
// The projections of an evaluation are value-independent random objects: they come from the host once per draw, are kept on the
// device by content (with the two transposed copies the reverse pass gathers over: ContentUpload, ctx.hpp, as api.hip's lr_upload)
// and reused by every call that passes the same ones.
#include "ctx.hpp"
#include "lr_grad_kernel.hpp"
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
        const int64_t sd[4] = {s.k1, s.k2, s.r, s.nnz};
        h = fnv1a(h, sd, sizeof(sd));
        h = fnv1a(h, s.colptr, sizeof(int32_t) * (size_t(s.r) + 1));
        h = fnv1a(h, s.i1, sizeof(int32_t) * size_t(s.nnz));
        h = fnv1a(h, s.i2, sizeof(int32_t) * size_t(s.nnz));
        h = fnv1a(h, s.val, sizeof(double) * size_t(s.nnz));
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

// the LrFusedArgs fields of a call on device-resident landmarks and whitening (the launchers derive F, lp and rows_b)
void fused_args(const gpsig_params* p, int cc, int r, int nsk, const LrGradSketch* gs, const void* X, int64_t N, int L, const double* S,
                const double* Wh, const double* spec, void* Phi, LrFusedArgs* A) {
    A->X = static_cast<const double*>(X); A->N = N; A->L = L;
    A->P.d_in = p->num_features;
    A->S = S; A->Wh = Wh;
    A->c = cc; A->r = r; A->M = p->num_levels; A->difference = p->difference; A->kind = int(p->base_kernel);
    A->p0 = p->base_params[0]; A->p1 = p->base_params[1];
    A->spec = spec;
    for (int i = 0; i < nsk; ++i) A->sk[i] = LrFusedSketch{gs[i].colptr, gs[i].ent};
    A->Phi = static_cast<double*>(Phi);
}

// the fused feature kernels (lr_fused_inst.hip) on device-resident landmarks and whitening: the caller scaled the inputs (no lengthscales,
// no lags); `two` picks the two-array form, else the three-array instance of lr_fused_variant
int fused_features(gpsig_ctx* c, const gpsig_params* p, int cc, int r, int nsk, const LrGradSketch* gs, const void* X, int64_t N, int L,
                   const double* S, const double* Wh, const double* spec, bool two, void* Phi, const char* what, const int32_t* lengths = nullptr) {
    LrFusedRaggedArgs A{};                       // (with `lengths` the ragged instance of the three-array form, lr_ragged_inst.hip)
    A.lengths = lengths;
    fused_args(p, cc, r, nsk, gs, X, N, L, S, Wh, spec, Phi, &A);
    const int rc = lengths ? lr_ragged_fused_launch(c->stream, A, c->lr_fused_pad)
                           : lr_fused_launch(c->stream, static_cast<const LrFusedArgs&>(A), c->lr_fused_pad, two, c->lr_fused_variant);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "%s: %s", what, hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

// the LrGradArgs fields both reverse passes fill the same way; the caller sets the sequences, dPhi, part and what is its own
void grad_args(const gpsig_ctx* c, const gpsig_params* p, int cc, int r, int nsk, const LrGradSketch* gs, int L, const double* S, const double* Wh,
               void* escr, int64_t escr_stride, LrGradArgs* A) {
    const int M = p->num_levels, d = p->num_features;
    A->L = L; A->d = d;
    A->S = S; A->Wh = Wh;
    A->c = cc; A->r = r; A->M = M; A->difference = p->difference; A->kind = int(p->base_kernel);
    A->p0 = p->base_params[0]; A->p1 = p->base_params[1];
    for (int i = 0; i < nsk; ++i) A->sk[i] = gs[i];
    A->F = 1 + cc + (M - 1) * r;
    A->escr = static_cast<double*>(escr); A->escr_stride = escr_stride;
    A->lp = lr_fused_stride(L, c->lr_fused_pad);
    A->rows_b = lr_grad_rows(cc, r, d);
}

// the tiled kernels' arguments (lr_tiled_kernel.hpp) from the plan of one direction
void tiled_args(const gpsig_ctx* c, const gpsig_params* p, int cc, int r, int nsk, const LrGradSketch* gs, int L, const double* S, const double* Wh,
                const LrTileDir& D, bool reverse, LrTiledArgs* A) {
    grad_args(c, p, cc, r, nsk, gs, L, S, Wh, nullptr, 0, A);
    A->lp = D.lp; A->TL = D.TL; A->ntiles = D.ntiles;
    A->rows_b = reverse ? lr_grad_rows(cc, r, A->d) : lr_fused_rows(cc, r, A->d);
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

// what the tensor entry points take beyond check(): the reverse kernel's per-thread tables and the LDS footprints of both directions
int tens_check(gpsig_ctx* c, const gpsig_params* p, int cc, int r, int64_t T, int E) {
    const int M = p->num_levels, d = p->num_features, lt = M * (M + 1) / 2;
    if (T < 0 || T > 0x7fffffff) return fail(c, GPSIG_ERR_INVALID, "bad number of tensors");
    if (M - 1 > LR_FUSED_MAX_SKETCHES) return fail(c, GPSIG_ERR_UNSUPPORTED, "low-rank mode is built for num_levels <= %d", LR_FUSED_MAX_SKETCHES + 1);
    if (cc > 64 || int64_t(cc) * d > int64_t(LR_GRAD_KS) * LR_GRAD_THREADS)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "the low-rank reverse pass is built for num_components <= 64 and num_components x columns <= %d", LR_GRAD_KS * LR_GRAD_THREADS);
    const size_t lds = std::max(lr_tens_grad_lds_bytes(cc, r, d, lt, E, M), lr_tens_fused_lds_bytes(cc, r, d, lt, E));
    if (lds > LR_FUSED_MAX_LDS) return fail(c, GPSIG_ERR_UNSUPPORTED, "a tensor's low-rank arrays (%zu bytes) exceed the LDS", lds);
    return GPSIG_OK;
}

// the fused tensor kernels (lr_fused_inst.hip) on device-resident landmarks and whitening: already-scaled tensors, no lengthscales, no lags
int tens_features(gpsig_ctx* c, const gpsig_params* p, int cc, int r, int nsk, const LrGradSketch* gs, const void* Z, int64_t T, int E, const double* S,
                  const double* Wh, const double* spec, void* Phi, const char* what) {
    LrTensFusedArgs A{};
    A.Z = static_cast<const double*>(Z); A.T = T; A.lt = p->num_levels * (p->num_levels + 1) / 2; A.E = E;
    A.P.d_in = p->num_features;
    A.S = S; A.Wh = Wh;
    A.c = cc; A.r = r; A.M = p->num_levels; A.kind = int(p->base_kernel);
    A.p0 = p->base_params[0]; A.p1 = p->base_params[1];
    A.spec = spec;
    for (int i = 0; i < nsk; ++i) A.sk[i] = LrFusedSketch{gs[i].colptr, gs[i].ent};
    A.Phi = static_cast<double*>(Phi);
    const int rc = lr_tens_fused_launch(c->stream, A);
    if (rc != 0) return fail(c, GPSIG_ERR_HIP, "%s: %s", what, hipGetErrorString(hipError_t(rc)));
    return GPSIG_OK;
}

void tens_grad_args(const gpsig_params* p, int cc, int r, int nsk, const LrGradSketch* gs, const void* Z, int64_t T, int E, const double* S,
                    const double* Wh, const void* dPhi, LrTensGradArgs* A) {
    const int M = p->num_levels;
    A->Z = static_cast<const double*>(Z); A->T = T; A->lt = M * (M + 1) / 2; A->E = E; A->d = p->num_features;
    A->S = S; A->Wh = Wh;
    A->c = cc; A->r = r; A->M = M; A->kind = int(p->base_kernel);
    A->p0 = p->base_params[0]; A->p1 = p->base_params[1];
    for (int i = 0; i < nsk; ++i) A->sk[i] = gs[i];
    A->dPhi = static_cast<const double*>(dPhi); A->F = 1 + cc + (M - 1) * r;
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

// the host path of gpsig_lr_seq_features_dev and of its ragged twin (`lengths`: NULL, or N per-sequence lengths on the device): checks and plan
// are those of L either way -- the plan does not depend on the lengths, so the host never reads them
int seq_features_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* X,
                     int64_t N, int32_t L, const int32_t* lengths, const double* S, const double* Wh, void* Phi) {
    CHK(check(c, p, cc, r, nsk));
    if (N < 0 || L < 1 || (N > 0 && (!X || !S || !Wh || !Phi))) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    // always the three-array form (the instance of lr_fused_variant): lr_fused does not apply here; beyond the LDS its time-tiled form
    const LrTileDir D = lr_tile_dir(false, cc, r, p->num_features, L, p->difference ? L - 1 : L, c->lr_fused_pad);
    if (!D.untiled && D.TL == 0)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "a %d-step tile of a sequence's low-rank arrays (%zu bytes) exceeds the LDS", LR_TILE_STEP,
                    lr_tiled_fused_lds_bytes(cc, r, p->num_features, LR_TILE_STEP, c->lr_fused_pad));
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    if (N == 0) return GPSIG_OK;
    if (D.untiled) return fused_features(c, p, cc, r, nsk, gs, X, N, L, S, Wh, nullptr, false, Phi, "fused low-rank feature kernel", lengths);
    LrTiledRaggedArgs A{};
    tiled_args(c, p, cc, r, nsk, gs, L, S, Wh, D, false, &A);
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
    CHK(check(c, p, cc, r, nsk));
    if (N < 0 || L < 1 || !gS || !gWh || (N > 0 && (!X || !S || !Wh || !dPhi || !gX))) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    const int M = p->num_levels, d = p->num_features;
    if (cc > 64 || int64_t(cc) * d > int64_t(LR_GRAD_KS) * LR_GRAD_THREADS)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "the low-rank reverse pass is built for num_components <= 64 and num_components x columns <= %d", LR_GRAD_KS * LR_GRAD_THREADS);
    const LrTilePlan plan = lr_tile_plan(cc, r, d, L, M, p->difference, c->lr_fused_pad, N);
    const size_t lds = plan.rev.lds;
    if (!plan.rev.untiled && plan.rev.TL == 0)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "a %d-step tile of a sequence's low-rank arrays (%zu bytes) exceeds the LDS in the reverse pass", LR_TILE_STEP,
                    lr_tiled_grad_lds_bytes(cc, r, d, LR_TILE_STEP, c->lr_fused_pad));
    if (N > 0 && plan.grid == 0)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "one workgroup's scratch for a sequence of %d steps (%lld bytes) exceeds the reverse pass's budget", plan.l,
                    (long long)(plan.escr_stride * int64_t(sizeof(double))));
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    const int64_t width = int64_t(cc) * d + int64_t(cc) * cc + 1;
    if (N == 0) {
        CHK(zero_async(c, gS, sizeof(double) * size_t(cc) * d));
        CHK(zero_async(c, gWh, sizeof(double) * size_t(cc) * cc));
        if (g_base) CHK(zero_async(c, g_base, sizeof(double)));
        return GPSIG_OK;
    }
    // one workgroup per CU at these LDS sizes, two rounds' worth of them (512); fewer where the tiled form's scratch would exceed its budget
    const unsigned grid = unsigned(plan.grid);
    const int64_t escr_stride = plan.escr_stride;
    void *part, *escr;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(grid) * size_t(width) + 64, &part));
    CHK(ensure(c, B_GR1, sizeof(double) * size_t(grid) * size_t(escr_stride) + 64, &escr));
    if (plan.rev.untiled) {
        LrGradRaggedArgs A{};
        grad_args(c, p, cc, r, nsk, gs, L, S, Wh, escr, escr_stride, &A);
        A.X = static_cast<const double*>(X); A.N = N;
        A.dPhi = static_cast<const double*>(dPhi);
        A.gX = static_cast<double*>(gX);
        A.part = static_cast<double*>(part);
        A.lengths = lengths;
        if (lengths) CHK(ragged_rc(c, lr_ragged_grad_launch(c->stream, A, grid, lds)));
        else CHK(grad_launch(c, static_cast<const LrGradArgs&>(A), grid, lds));
    } else {
        LrTiledRaggedArgs A{};
        tiled_args(c, p, cc, r, nsk, gs, L, S, Wh, plan.rev, true, &A);
        A.escr = static_cast<double*>(escr); A.escr_stride = escr_stride;
        A.X = static_cast<const double*>(X); A.N = N;
        A.dPhi = static_cast<const double*>(dPhi);
        A.gX = static_cast<double*>(gX);
        A.part = static_cast<double*>(part);
        A.lengths = lengths;
        if (lengths) CHK(ragged_rc(c, lr_ragged_grad_tiled_launch(c->stream, A, grid, lds)));
        else CHK(grad_launch(c, static_cast<const LrTiledArgs&>(A), grid, lds));
    }
    hipLaunchKernelGGL(lr_grad_reduce_kernel, dim3(unsigned((width + 255) / 256)), dim3(256), 0, c->stream, static_cast<const double*>(part), int(grid), width,
                       gS, int64_t(cc) * d, gWh, int64_t(cc) * cc, g_base);
    HIPCHK(c, hipGetLastError());
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
    CHK(check(c, p, cc, r, nsk, true));
    if (N < 0 || L < 1 || (N > 0 && (!X || !S || !Wh || !alpha || !omega || !gamma || !Phi))) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    const int d = p->num_features, Q = int(p->base_params[0]);
    // the two-array kernel where lr_fused == 1 and it is built, else the three-array one (also for lr_fused == 0); the footprint of that form
    const bool two = c->lr_fused == 1 && lr_fused2_ok(cc, r, L);
    const size_t lds = two ? lr_fused2_lds_bytes(cc, r, d, L, c->lr_fused_pad) : lr_fused_lds_bytes(cc, r, d, L, c->lr_fused_pad);
    if (lds > LR_FUSED_MAX_LDS) return fail(c, GPSIG_ERR_UNSUPPORTED, "a sequence's low-rank arrays (%zu bytes) exceed the LDS", lds);
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    if (N == 0) return GPSIG_OK;
    void* tab;
    const int ntab = Q * (1 + 2 * SPECTRAL_STRIDE);
    CHK(ensure(c, B_SPECD, sizeof(double) * size_t(ntab) + 64, &tab));
    hipLaunchKernelGGL(lr_spectral_pack_kernel, dim3(unsigned((ntab + 255) / 256)), dim3(256), 0, c->stream, alpha, omega, gamma, Q, d,
                       static_cast<double*>(tab));
    HIPCHK(c, hipGetLastError());
    return fused_features(c, p, cc, r, nsk, gs, X, N, L, S, Wh, static_cast<const double*>(tab), two, Phi, "fused low-rank spectral feature kernel");
}

int gpsig_lr_seq_features_spectral_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                        const void* X, int64_t N, int32_t L, const double* S, const double* Wh, const double* alpha,
                                        const double* omega, const double* gamma, const void* dPhi, void* gX, double* gS, double* gWh,
                                        double* dalpha, double* domega, double* dgamma) {
    CHK(check(c, p, cc, r, nsk, true));
    if (N < 0 || L < 1 || !gS || !gWh || !dalpha || !domega || !dgamma ||
        (N > 0 && (!X || !S || !Wh || !alpha || !omega || !gamma || !dPhi || !gX)))
        return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    const int M = p->num_levels, d = p->num_features, F = 1 + cc + (M - 1) * r, Q = int(p->base_params[0]), family = int(p->base_params[1]);
    const size_t lds = lr_grad_lds_bytes(cc, r, d, L, c->lr_fused_pad);
    if (lds > LR_FUSED_MAX_LDS) return fail(c, GPSIG_ERR_UNSUPPORTED, "a sequence's low-rank arrays (%zu bytes) exceed the LDS in the reverse pass", lds);
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    if (N == 0) {
        CHK(zero_async(c, gS, sizeof(double) * size_t(cc) * d));
        CHK(zero_async(c, gWh, sizeof(double) * size_t(cc) * cc));
        CHK(zero_async(c, dalpha, sizeof(double) * size_t(Q)));
        CHK(zero_async(c, domega, sizeof(double) * size_t(Q) * d));
        CHK(zero_async(c, dgamma, sizeof(double) * size_t(Q) * d));
        return GPSIG_OK;
    }
    // sequences per chunk: dkxs of a chunk within the budget
    const int64_t per_seq = int64_t(L) * cc * int64_t(sizeof(double));
    const int64_t nb = std::min<int64_t>(N, std::max<int64_t>(1, int64_t(LR_SPECTRAL_DKXS_BUDGET) / per_seq));
    const int l = p->difference ? L - 1 : L;
    const unsigned gmax = unsigned(nb < 512 ? nb : 512);              // as the other families' reverse pass
    const int64_t kxs_off = (int64_t(cc) + int64_t(M > 2 ? M - 2 : 0) * r) * (l > 0 ? l : 1);
    const int64_t escr_stride = kxs_off + int64_t(cc) * L + 8;
    int64_t nparts = 0;                                                // workgroups over all chunks: one dWh partial each
    for (int64_t n0 = 0; n0 < N; n0 += nb) nparts += std::min<int64_t>(N - n0, 512);
    void *part, *escr, *dk, *cpart;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(nparts) * size_t(cc) * cc + 64, &part));
    CHK(ensure(c, B_GR1, sizeof(double) * size_t(gmax) * size_t(escr_stride) + 64, &escr));
    CHK(ensure(c, B_LRDK, sizeof(double) * size_t(nb) * size_t(L) * cc + 64, &dk));
    CHK(ensure(c, B_GR2, sizeof(double) * spectral_cross_grad_part_doubles(nb * L, cc, d, Q) + 64, &cpart));
    LrGradSpectralArgs A{};
    grad_args(c, p, cc, r, nsk, gs, L, S, Wh, escr, escr_stride, &A);
    A.alpha = alpha; A.omega = omega; A.gamma = gamma;
    A.dkxs = static_cast<double*>(dk); A.kxs_off = kxs_off;
    int64_t at = 0;
    for (int64_t n0 = 0; n0 < N; n0 += nb) {
        const int64_t nn = std::min(nb, N - n0);
        const unsigned grid = unsigned(nn < 512 ? nn : 512);
        const double* Xc = static_cast<const double*>(X) + n0 * int64_t(L) * d;
        A.X = Xc; A.N = nn;
        A.dPhi = static_cast<const double*>(dPhi) + n0 * int64_t(F);
        A.part = static_cast<double*>(part) + at * int64_t(cc) * cc;
        CHK(grad_launch(c, A, grid, lds));
        const int rc = spectral_cross_grad_launch(c->stream, Q, family, d, Xc, nn * L, S, cc, alpha, omega, gamma, A.dkxs,
                                                  static_cast<double*>(gX) + n0 * int64_t(L) * d, static_cast<double*>(cpart), gS, dalpha, domega,
                                                  dgamma, n0 > 0);
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral cross reverse pass: %s", hipGetErrorString(hipError_t(rc)));
        at += grid;
    }
    hipLaunchKernelGGL(lr_grad_reduce_kernel, dim3(unsigned((int64_t(cc) * cc + 255) / 256)), dim3(256), 0, c->stream, static_cast<const double*>(part),
                       int(nparts), int64_t(cc) * cc, gS, int64_t(0), gWh, int64_t(cc) * cc, static_cast<double*>(nullptr));
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

// ... of long and ragged batches: `lengths` directly after L (N int32 on the device, the kernels clamp to [1, L]; NULL: L points each).  Sequences
// beyond the LDS go in time tiles; the plan follows from L alone.
int gpsig_lr_seq_features_spectral_ragged_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                              const void* X, int64_t N, int32_t L, const int32_t* lengths, const double* S, const double* Wh,
                                              const double* alpha, const double* omega, const double* gamma, void* Phi) {
    CHK(check(c, p, cc, r, nsk, true));
    if (N < 0 || L < 1 || (N > 0 && (!X || !S || !Wh || !alpha || !omega || !gamma || !Phi))) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    const int d = p->num_features, Q = int(p->base_params[0]);
    const LrTileDir D = lr_tile_dir(false, cc, r, d, L, p->difference ? L - 1 : L, c->lr_fused_pad);
    if (!D.untiled && D.TL == 0)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "a %d-step tile of a sequence's low-rank arrays (%zu bytes) exceeds the LDS", LR_TILE_STEP,
                    lr_tiled_fused_lds_bytes(cc, r, d, LR_TILE_STEP, c->lr_fused_pad));
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    if (N == 0) return GPSIG_OK;
    void* tabv;
    const int ntab = Q * (1 + 2 * SPECTRAL_STRIDE);
    CHK(ensure(c, B_SPECD, sizeof(double) * size_t(ntab) + 64, &tabv));
    const double* tab = static_cast<const double*>(tabv);
    hipLaunchKernelGGL(lr_spectral_pack_kernel, dim3(unsigned((ntab + 255) / 256)), dim3(256), 0, c->stream, alpha, omega, gamma, Q, d,
                       static_cast<double*>(tabv));
    HIPCHK(c, hipGetLastError());
    int rc;
    if (D.untiled) {
        LrFusedSpectralLenArgs A{};
        fused_args(p, cc, r, nsk, gs, X, N, L, S, Wh, tab, Phi, &A);
        A.lengths = lengths;
        rc = lr_spectral_len_fused_launch(c->stream, A, c->lr_fused_pad);
    } else {
        LrTiledSpectralArgs A{};
        tiled_args(c, p, cc, r, nsk, gs, L, S, Wh, D, false, &A);
        A.X = static_cast<const double*>(X); A.N = N;
        A.Phi = static_cast<double*>(Phi);
        A.alpha = tab; A.omega = tab + Q; A.gamma = tab + Q + Q * SPECTRAL_STRIDE; A.ld = SPECTRAL_STRIDE;
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
    CHK(check(c, p, cc, r, nsk, true));
    if (N < 0 || L < 1 || !gS || !gWh || !dalpha || !domega || !dgamma ||
        (N > 0 && (!X || !S || !Wh || !alpha || !omega || !gamma || !dPhi || !gX)))
        return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    const int M = p->num_levels, d = p->num_features, F = 1 + cc + (M - 1) * r, Q = int(p->base_params[0]), family = int(p->base_params[1]);
    // sequences per chunk: dkxs of a chunk within the budget; the plan of a chunk, with kxs (c, L) in each workgroup's scratch
    const int64_t per_seq = int64_t(L) * cc * int64_t(sizeof(double));
    const int64_t nb = std::min<int64_t>(N, std::max<int64_t>(1, int64_t(LR_SPECTRAL_DKXS_BUDGET) / per_seq));
    const LrTilePlan plan = lr_tile_plan(cc, r, d, L, M, p->difference, c->lr_fused_pad, nb, int64_t(cc) * L);
    if (!plan.rev.untiled && plan.rev.TL == 0)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "a %d-step tile of a sequence's low-rank arrays (%zu bytes) exceeds the LDS in the reverse pass", LR_TILE_STEP,
                    lr_tiled_grad_lds_bytes(cc, r, d, LR_TILE_STEP, c->lr_fused_pad));
    if (N > 0 && plan.grid == 0)
        return fail(c, GPSIG_ERR_UNSUPPORTED, "one workgroup's scratch for a sequence of %d steps (%lld bytes) exceeds the reverse pass's budget", plan.l,
                    (long long)(plan.escr_stride * int64_t(sizeof(double))));
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    if (N == 0) {
        CHK(zero_async(c, gS, sizeof(double) * size_t(cc) * d));
        CHK(zero_async(c, gWh, sizeof(double) * size_t(cc) * cc));
        CHK(zero_async(c, dalpha, sizeof(double) * size_t(Q)));
        CHK(zero_async(c, domega, sizeof(double) * size_t(Q) * d));
        CHK(zero_async(c, dgamma, sizeof(double) * size_t(Q) * d));
        return GPSIG_OK;
    }
    const int64_t escr_stride = plan.escr_stride, kxs_off = escr_stride - int64_t(cc) * L - 8;
    int64_t nparts = 0;                                                // workgroups over all chunks: one dWh partial each
    for (int64_t n0 = 0; n0 < N; n0 += nb) nparts += std::min<int64_t>(std::min(nb, N - n0), plan.grid);
    void *part, *escr, *dk, *cpart;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(nparts) * size_t(cc) * cc + 64, &part));
    CHK(ensure(c, B_GR1, sizeof(double) * size_t(plan.grid) * size_t(escr_stride) + 64, &escr));
    CHK(ensure(c, B_LRDK, sizeof(double) * size_t(nb) * size_t(L) * cc + 64, &dk));
    CHK(ensure(c, B_GR2, sizeof(double) * spectral_cross_grad_part_doubles(nb * L, cc, d, Q) + 64, &cpart));
    LrGradSpectralLenArgs W{};                                          // whole sequences ...
    LrTiledSpectralArgs T{};                                            // ... or time tiles
    if (plan.rev.untiled) {
        grad_args(c, p, cc, r, nsk, gs, L, S, Wh, escr, escr_stride, &W);
        W.alpha = alpha; W.omega = omega; W.gamma = gamma;
        W.dkxs = static_cast<double*>(dk); W.kxs_off = kxs_off;
    } else {
        tiled_args(c, p, cc, r, nsk, gs, L, S, Wh, plan.rev, true, &T);
        T.escr = static_cast<double*>(escr); T.escr_stride = escr_stride;
        T.alpha = alpha; T.omega = omega; T.gamma = gamma; T.ld = d;
        T.dkxs = static_cast<double*>(dk); T.kxs_off = kxs_off;
    }
    int64_t at = 0;
    for (int64_t n0 = 0; n0 < N; n0 += nb) {
        const int64_t nn = std::min(nb, N - n0);
        const unsigned grid = unsigned(std::min<int64_t>(nn, plan.grid));
        const double* Xc = static_cast<const double*>(X) + n0 * int64_t(L) * d;
        const int32_t* lc = lengths ? lengths + n0 : nullptr;
        LrGradArgs& A = plan.rev.untiled ? static_cast<LrGradArgs&>(W) : static_cast<LrGradArgs&>(T);
        A.X = Xc; A.N = nn;
        A.dPhi = static_cast<const double*>(dPhi) + n0 * int64_t(F);
        A.part = static_cast<double*>(part) + at * int64_t(cc) * cc;
        W.lengths = T.lengths = lc;
        int rc = plan.rev.untiled ? lr_spectral_len_grad_launch(c->stream, W, grid, plan.rev.lds)
                                  : lr_spectral_grad_tiled_launch(c->stream, T, grid, plan.rev.lds);
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "low-rank spectral reverse kernel (lengths-aware): %s", hipGetErrorString(hipError_t(rc)));
        double* gXc = static_cast<double*>(gX) + n0 * int64_t(L) * d;
        double* dkp = static_cast<double*>(dk);
        rc = lc ? spectral_cross_grad_len_launch(c->stream, Q, family, d, Xc, nn, L, lc, S, cc, alpha, omega, gamma, dkp, gXc,
                                                 static_cast<double*>(cpart), gS, dalpha, domega, dgamma, n0 > 0)
                : spectral_cross_grad_launch(c->stream, Q, family, d, Xc, nn * L, S, cc, alpha, omega, gamma, dkp, gXc, static_cast<double*>(cpart), gS,
                                             dalpha, domega, dgamma, n0 > 0);
        if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral cross reverse pass: %s", hipGetErrorString(hipError_t(rc)));
        at += grid;
    }
    hipLaunchKernelGGL(lr_grad_reduce_kernel, dim3(unsigned((int64_t(cc) * cc + 255) / 256)), dim3(256), 0, c->stream, static_cast<const double*>(part),
                       int(nparts), int64_t(cc) * cc, gS, int64_t(0), gWh, int64_t(cc) * cc, static_cast<double*>(nullptr));
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

int gpsig_lr_tens_features_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* Z,
                               int64_t T, int32_t increments, const double* S, const double* Wh, void* Phi) {
    CHK(check(c, p, cc, r, nsk));
    const int E = increments ? 2 : 1;
    CHK(tens_check(c, p, cc, r, T, E));
    if (T > 0 && (!Z || !S || !Wh || !Phi)) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    if (T == 0) return GPSIG_OK;
    return tens_features(c, p, cc, r, nsk, gs, Z, T, E, S, Wh, nullptr, Phi, "fused low-rank tensor feature kernel");
}

int gpsig_lr_tens_features_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches, const void* Z,
                                int64_t T, int32_t increments, const double* S, const double* Wh, const void* dPhi, void* gZ, double* gS, double* gWh,
                                double* g_base) {
    CHK(check(c, p, cc, r, nsk));
    const int E = increments ? 2 : 1, d = p->num_features;
    CHK(tens_check(c, p, cc, r, T, E));
    if (!gS || !gWh || (T > 0 && (!Z || !S || !Wh || !dPhi || !gZ))) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    if (T == 0) {
        CHK(zero_async(c, gS, sizeof(double) * size_t(cc) * d));
        CHK(zero_async(c, gWh, sizeof(double) * size_t(cc) * cc));
        if (g_base) CHK(zero_async(c, g_base, sizeof(double)));
        return GPSIG_OK;
    }
    const int64_t width = int64_t(cc) * d + int64_t(cc) * cc + 1;
    const unsigned grid = unsigned(T < 512 ? T : 512);                 // as the sequences' reverse pass: the partial sums stay bounded
    void* part;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(grid) * size_t(width) + 64, &part));
    LrTensGradArgs A{};
    tens_grad_args(p, cc, r, nsk, gs, Z, T, E, S, Wh, dPhi, &A);
    A.t0 = 0; A.nt = T;
    A.gZ = static_cast<double*>(gZ);
    A.part = static_cast<double*>(part);
    CHK(tens_grad_launch(c, A, grid));
    hipLaunchKernelGGL(lr_grad_reduce_kernel, dim3(unsigned((width + 255) / 256)), dim3(256), 0, c->stream, static_cast<const double*>(part), int(grid), width,
                       gS, int64_t(cc) * d, gWh, int64_t(cc) * cc, g_base);
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

int gpsig_lr_tens_features_spectral_dev(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                        const void* Z, int64_t T, int32_t increments, const double* S, const double* Wh, const double* alpha,
                                        const double* omega, const double* gamma, void* Phi) {
    CHK(check(c, p, cc, r, nsk, true));
    const int E = increments ? 2 : 1, d = p->num_features, Q = int(p->base_params[0]);
    CHK(tens_check(c, p, cc, r, T, E));
    if (T > 0 && (!Z || !S || !Wh || !alpha || !omega || !gamma || !Phi)) return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    if (T == 0) return GPSIG_OK;
    void* tab;
    const int ntab = Q * (1 + 2 * SPECTRAL_STRIDE);
    CHK(ensure(c, B_SPECD, sizeof(double) * size_t(ntab) + 64, &tab));
    hipLaunchKernelGGL(lr_spectral_pack_kernel, dim3(unsigned((ntab + 255) / 256)), dim3(256), 0, c->stream, alpha, omega, gamma, Q, d,
                       static_cast<double*>(tab));
    HIPCHK(c, hipGetLastError());
    return tens_features(c, p, cc, r, nsk, gs, Z, T, E, S, Wh, static_cast<const double*>(tab), Phi, "fused low-rank spectral tensor feature kernel");
}

int gpsig_lr_tens_features_spectral_grad(gpsig_ctx* c, const gpsig_params* p, int32_t cc, int32_t r, int32_t nsk, const gpsig_sketch* sketches,
                                         const void* Z, int64_t T, int32_t increments, const double* S, const double* Wh, const double* alpha,
                                         const double* omega, const double* gamma, const void* dPhi, void* gZ, double* gS, double* gWh,
                                         double* dalpha, double* domega, double* dgamma) {
    CHK(check(c, p, cc, r, nsk, true));
    const int E = increments ? 2 : 1, M = p->num_levels, lt = M * (M + 1) / 2, d = p->num_features, Q = int(p->base_params[0]),
              family = int(p->base_params[1]);
    CHK(tens_check(c, p, cc, r, T, E));
    if (!gS || !gWh || !dalpha || !domega || !dgamma || (T > 0 && (!Z || !S || !Wh || !alpha || !omega || !gamma || !dPhi || !gZ)))
        return fail(c, GPSIG_ERR_INVALID, "bad sizes / NULL pointer");
    LrGradSketch gs[LR_FUSED_MAX_SKETCHES];
    CHK(upload_sketches(c, cc, r, nsk, sketches, gs));
    if (T == 0) {
        CHK(zero_async(c, gS, sizeof(double) * size_t(cc) * d));
        CHK(zero_async(c, gWh, sizeof(double) * size_t(cc) * cc));
        CHK(zero_async(c, dalpha, sizeof(double) * size_t(Q)));
        CHK(zero_async(c, domega, sizeof(double) * size_t(Q) * d));
        CHK(zero_async(c, dgamma, sizeof(double) * size_t(Q) * d));
        return GPSIG_OK;
    }
    // tensors per chunk: dkx of a chunk within the budget
    const int64_t per_tens = int64_t(lt) * E * cc * int64_t(sizeof(double));
    const int64_t nb = std::min<int64_t>(T, std::max<int64_t>(1, int64_t(LR_SPECTRAL_DKXS_BUDGET) / per_tens));
    const bool whole = nb == T;                                        // one launch: dkx is in the flat point order of Z
    int64_t nparts = 0;                                                // workgroups over all chunks: one dWh partial each
    for (int64_t n0 = 0; n0 < T; n0 += nb) nparts += std::min<int64_t>(std::min(nb, T - n0), 512);
    void *part, *dk, *cpart;
    CHK(ensure(c, B_GR0, sizeof(double) * size_t(nparts) * size_t(cc) * cc + 64, &part));
    CHK(ensure(c, B_LRDK, sizeof(double) * size_t(nb) * size_t(lt) * E * cc + 64, &dk));
    CHK(ensure(c, B_GR2, sizeof(double) * spectral_cross_grad_part_doubles(whole ? int64_t(lt) * T * E : nb * E, cc, d, Q) + 64, &cpart));
    LrTensGradSpectralArgs A{};
    tens_grad_args(p, cc, r, nsk, gs, Z, T, E, S, Wh, dPhi, &A);
    A.alpha = alpha; A.omega = omega; A.gamma = gamma;
    A.dkx = static_cast<double*>(dk);
    const double* Zd = static_cast<const double*>(Z);
    int64_t at = 0;
    for (int64_t n0 = 0; n0 < T; n0 += nb) {
        const int64_t nn = std::min(nb, T - n0);
        const unsigned grid = unsigned(nn < 512 ? nn : 512);
        A.t0 = n0; A.nt = nn;
        A.part = static_cast<double*>(part) + at * int64_t(cc) * cc;
        CHK(tens_grad_launch(c, A, grid));
        // the chunk's points: component k's are the run (k T + n0) E .. of Z's flat rows, nn E of them; their dkx rows k nn E ..
        for (int k = 0; k < (whole ? 1 : lt); ++k) {
            const int64_t row0 = (int64_t(k) * T + n0) * E, n = whole ? int64_t(lt) * T * E : nn * E;
            const int rc = spectral_cross_grad_launch(c->stream, Q, family, d, Zd + row0 * d, n, S, cc, alpha, omega, gamma,
                                                      A.dkx + int64_t(k) * nn * E * cc, static_cast<double*>(gZ) + row0 * d,
                                                      static_cast<double*>(cpart), gS, dalpha, domega, dgamma, n0 > 0 || k > 0);
            if (rc != 0) return fail(c, GPSIG_ERR_HIP, "spectral cross reverse pass: %s", hipGetErrorString(hipError_t(rc)));
        }
        at += grid;
    }
    hipLaunchKernelGGL(lr_grad_reduce_kernel, dim3(unsigned((int64_t(cc) * cc + 255) / 256)), dim3(256), 0, c->stream, static_cast<const double*>(part),
                       int(nparts), int64_t(cc) * cc, gS, int64_t(0), gWh, int64_t(cc) * cc, static_cast<double*>(nullptr));
    HIPCHK(c, hipGetLastError());
    return GPSIG_OK;
}

}  // extern "C"
