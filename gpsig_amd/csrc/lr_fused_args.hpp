// lr_fused_args.hpp -- argument block and launcher of the fused low-rank feature kernel (lr_fused_kernel.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"

namespace gpsig {

// Landmarks, whitening matrix and sketch entries are read-only for the whole launch and addressed wave-uniformly: in the
// constant address space the compiler may serve them through the scalar unit (s_load) instead of broadcasting vector loads.
template <typename T>
using lr_const_ptr = const __attribute__((address_space(4))) T*;
template <typename T>
__device__ __forceinline__ lr_const_ptr<T> lr_as_const(const T* p) { return (lr_const_ptr<T>)(p); }

struct LrEntry { double val; int32_t i1, i2; };     // one entry of a sketch, stored by output column (16 bytes: one s_load_dwordx4)

struct LrFusedSketch { const int32_t* colptr; const LrEntry* ent; };

constexpr int LR_FUSED_MAX_SKETCHES = 7;            // levels 2 .. 8
constexpr size_t LR_FUSED_MAX_LDS = 156 * 1024;     // of the 160 KB a CU has (one workgroup per CU at that size)

struct LrFusedArgs {
    using value_type = double;
    const double* X; int64_t N; int L;
    ScaleParams P;
    const double* S;        // landmarks (c, d_eff), scaled points
    const double* Wh;       // whitening (c, c) row-major: feat[j] = sum_i kxs[i] * Wh[i][j]
    int c, r, M, difference, kind;
    double p0, p1;
    LrFusedSketch sk[LR_FUSED_MAX_SKETCHES];
    double* Phi; int F;
    int lp;                 // row stride of the LDS arrays, in doubles (odd, > number of time steps rounded up to 64)
    int rows_b;             // rows of the two work arrays: max(c, r, d_eff)
    const double* spec;     // BASE_SPECTRAL: spectral_table()'s device table (p0 = Q, p1 = family); the spectral instances only
};

inline int lr_fused_stride(int L, int pad) { return (L + 63) / 64 * 64 + pad; }
inline size_t lr_fused_lds_bytes(int c, int r, int d_eff, int L, int pad = 1) {
    const int lp = lr_fused_stride(L, pad);
    int kb = c > r ? c : r;
    if (d_eff > kb) kb = d_eff;
    return sizeof(double) * size_t(lp) * (size_t(c) + 2 * size_t(kb));
}

// Feature map of inducing tensors (gpsig/kernels.py:285-311 _K_tens_lr_feat, signature_algs.py:194-222 tensor_kern_lr_feature),
// one workgroup per tensor: its lt * E components are whitened and chained through the sketches in LDS.
struct LrTensFusedArgs {
    using value_type = double;
    const double* Z; int64_t T; int lt, E;      // Z (lt, T, E, d_eff) as the caller gives it
    ScaleParams P;
    const double* S; const double* Wh;
    int c, r, M, kind;
    double p0, p1;
    LrFusedSketch sk[LR_FUSED_MAX_SKETCHES];
    double* Phi; int F;
    const double* spec;     // BASE_SPECTRAL table, as LrFusedArgs::spec
};
inline size_t lr_tens_fused_lds_bytes(int c, int r, int d_eff, int lt, int E) {
    const size_t rows = size_t(lt) * E, w = size_t(c > r ? c : r);
    return sizeof(double) * (rows * (size_t(d_eff) + 2 * size_t(c)) + size_t(lt) * c + 2 * w);
}
int lr_tens_fused_launch(hipStream_t stream, const LrTensFusedArgs& A);

// two-array form (lr_seq_features_fused2_kernel): usable for L <= 64 and at most 8 output columns per wavefront of the 512-thread workgroup
inline bool lr_fused2_ok(int c, int r, int L) { return L <= 64 && c <= 64 && r <= 64; }
inline size_t lr_fused2_lds_bytes(int c, int r, int d_eff, int L, int pad = 1) {
    int kb = c > r ? c : r;
    if (d_eff > kb) kb = d_eff;
    return sizeof(double) * size_t(lr_fused_stride(L, pad)) * 2 * size_t(kb);
}
int lr_fused2_launch(hipStream_t stream, const LrFusedArgs& A, unsigned grid);

// lr_fused_inst.hip: launches the kernel on `stream` with `grid` workgroups; returns the hipError_t of the launch
int lr_fused_launch(hipStream_t stream, const LrFusedArgs& A, unsigned grid, int variant);

// ---- float32 forms (lr_fused_inst.hip: lr_seq_features_fused{,2}{,_spectral}_f32_kernel, lr_tens_features_fused{,_spectral}_f32_kernel).
// The same bodies on float: points, landmarks, whitening, sketch values, spectral table and features in float32, phase 1 on the hardware
// transcendentals.  The state stays float64 (drawn and whitened in float64); lr_narrow_launch converts what the kernels read once per call.
struct LrEntryF32 { float val; int32_t i1, i2, pad; };  // 16 bytes as LrEntry: one s_load_dwordx4 per entry
struct LrFusedSketchF32 { const int32_t* colptr; const LrEntryF32* ent; };

struct LrFusedArgsF32 {
    using value_type = float;
    const float* X; int64_t N; int L;
    ScaleParams P;
    const float* S;
    const float* Wh;
    int c, r, M, difference, kind;
    float p0, p1;
    LrFusedSketchF32 sk[LR_FUSED_MAX_SKETCHES];
    float* Phi; int F;
    int lp;                 // row stride of the LDS arrays, in floats (odd)
    int rows_b;
    const float* spec;      // the spectral table in float32 (same layout as spectral_table()'s)
};
struct LrTensFusedArgsF32 {
    using value_type = float;
    const float* Z; int64_t T; int lt, E;
    ScaleParams P;
    const float* S; const float* Wh;
    int c, r, M, kind;
    float p0, p1;
    LrFusedSketchF32 sk[LR_FUSED_MAX_SKETCHES];
    float* Phi; int F;
    const float* spec;
};
inline size_t lr_fused_lds_bytes_f32(int c, int r, int d_eff, int L, int pad = 1) { return lr_fused_lds_bytes(c, r, d_eff, L, pad) / 2; }
inline size_t lr_fused2_lds_bytes_f32(int c, int r, int d_eff, int L, int pad = 1) { return lr_fused2_lds_bytes(c, r, d_eff, L, pad) / 2; }
inline size_t lr_tens_fused_lds_bytes_f32(int c, int r, int d_eff, int lt, int E) { return lr_tens_fused_lds_bytes(c, r, d_eff, lt, E) / 2; }
// the kind / spectral switch as the float64 launchers; fused2 where lr_fused2_ok, else the three-array form (one instance each: 512 threads,
// 8 entries per scalar-load batch)
int lr_fused_f32_launch(hipStream_t stream, const LrFusedArgsF32& A, unsigned grid, bool two_arrays);
int lr_tens_fused_f32_launch(hipStream_t stream, const LrTensFusedArgsF32& A);
// out[i] = float(in[i]) for n values, and the sketch entries (value narrowed, indices copied); returns the hipError_t of the launch
int lr_narrow_launch(hipStream_t stream, const double* in, int64_t n, float* out);
int lr_narrow_entries_launch(hipStream_t stream, const LrEntry* in, int64_t n, LrEntryF32* out);

// lr_spectral_inst.hip: the same kernels with SignatureSpectral's kappa in phase 1 (A.kind == BASE_SPECTRAL; the launchers above hand over)
int lr_fused_spectral_launch(hipStream_t stream, const LrFusedArgs& A, unsigned grid, size_t lds);
int lr_fused2_spectral_launch(hipStream_t stream, const LrFusedArgs& A, unsigned grid, size_t lds);
int lr_tens_fused_spectral_launch(hipStream_t stream, const LrTensFusedArgs& A, size_t lds);
// ... and the multi-pass route's Nystrom cross matrices (lowrank_kernels.hpp: lr_seq_cross_kernel / lr_tens_cross_kernel)
int lr_seq_cross_spectral_launch(hipStream_t stream, const double* X, int64_t N, int L, ScaleParams P, const double* S, int c, int Q, int family,
                                 const double* spec, double* out);
int lr_tens_cross_spectral_launch(hipStream_t stream, const double* Z, int64_t rows, ScaleParams P, const double* S, int c, int Q, int family,
                                  const double* spec, double* out);
// ... and the reverse pass of kappa(P, S) (n points, c landmarks, the parameters alpha (Q), omega (Q, d), gamma (Q, d) on the device) given
// G = dL/dK (n, c): dP (n, d) overwritten; dS (c, d), dalpha, domega, dgamma overwritten, or added to with `accumulate` (the chunks of one
// call, in order); `part` holds spectral_cross_grad_part_doubles(n, c, d, Q) doubles of per-workgroup partial sums.  Returns the hipError_t.
size_t spectral_cross_grad_part_doubles(int64_t n, int c, int d, int Q);
int spectral_cross_grad_launch(hipStream_t stream, int Q, int family, int d, const double* P, int64_t n, const double* S, int c,
                               const double* alpha, const double* omega, const double* gamma, const double* G, double* dP, double* part,
                               double* dS, double* dalpha, double* domega, double* dgamma, bool accumulate);

}  // namespace gpsig
