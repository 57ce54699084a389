// lr_fused_args.hpp -- argument blocks and launchers of the fused low-rank feature kernels (lr_fused_kernel.hpp), float64 and float32.
// lr_fused_inst.hip instantiates the kernels and exports one launcher per form; lr_api.hip (evaluation) and lr_grad_api.hip (training
// path) fill only what their callers decide: points, scaling, landmarks, whitening, base parameters, spectral table and projections.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aux_kernels.hpp"
#include "lr_tile_plan.hpp"       // LR_FUSED_MAX_LDS, lr_fused_stride, lr_fused_lds_bytes (HIP-free: the tile plan needs them too)

namespace gpsig {

// Landmarks, whitening matrix and sketch entries are read-only for the whole launch and addressed wave-uniformly: in the
// constant address space the compiler may serve them through the scalar unit (s_load) instead of broadcasting vector loads.
template <typename T>
using lr_const_ptr = const __attribute__((address_space(4))) T*;
template <typename T>
__device__ __forceinline__ lr_const_ptr<T> lr_as_const(const T* p) { return (lr_const_ptr<T>)(p); }

struct LrEntry { double val; int32_t i1, i2; };     // one entry of a sketch, stored by output column (16 bytes: one s_load_dwordx4)
// the float32 forms' entries: the same 16 bytes, one s_load_dwordx4 per entry
struct LrEntryF32 { float val; int32_t i1, i2, pad; };

template <typename Entry>
struct LrSketch { const int32_t* colptr; const Entry* ent; };
using LrFusedSketch = LrSketch<LrEntry>;
using LrFusedSketchF32 = LrSketch<LrEntryF32>;

// (LR_FUSED_MAX_SKETCHES = 7, levels 2 .. 8: lr_tile_plan.hpp)

// The float32 forms run the same bodies on float: points, landmarks, whitening, sketch values, spectral table and features in float32,
// phase 1 on the hardware transcendentals.  The state stays float64 (drawn and whitened in float64); lr_narrow_launch converts what the
// kernels read once per call.
template <typename V, typename Entry>
struct LrFusedFields {
    using value_type = V;
    const V* X; int64_t N; int L;
    ScaleParams P;
    const V* S;             // landmarks (c, d_eff), scaled points
    const V* Wh;            // whitening (c, c) row-major: feat[j] = sum_i kxs[i] * Wh[i][j]
    int c, r, M, difference, kind;
    V p0, p1;
    LrSketch<Entry> sk[LR_FUSED_MAX_SKETCHES];
    V* Phi; int F;
    int lp;                 // row stride of the LDS arrays, in values (odd, > number of time steps rounded up to 64)
    int rows_b;             // rows of the two work arrays: max(c, r, d_eff)
    const V* spec;          // BASE_SPECTRAL: spectral_table()'s device table (p0 = Q, p1 = family); the spectral instances only
};
struct LrFusedArgs : LrFusedFields<double, LrEntry> {};
struct LrFusedArgsF32 : LrFusedFields<float, LrEntryF32> {};

// Ragged batches: sequence n has lengths[n] points of the L its rows have room for (N int32 on the device).  The ragged instances of the
// sequence kernels (lr_ragged_inst.hip) are the same bodies on an argument block that carries the pointer: lr_ragged<Args> marks the block,
// lr_seq_points gives a sequence's extent -- L for every other block, so that their instances stay the code they were.  Strides, tile
// lengths and LDS sizes are those of L for both.
struct LrFusedRaggedArgs : LrFusedArgs { const int32_t* lengths; };
template <typename Args> struct lr_ragged { static constexpr bool value = false; };
template <> struct lr_ragged<LrFusedRaggedArgs> { static constexpr bool value = true; };
// lengths[n] through the scalar unit (n is the same for the whole workgroup), clamped to [1, L]: whatever the memory holds, a sequence's
// indices stay inside its own L x d block
__device__ __forceinline__ int lr_ragged_length(const int32_t* lengths, int64_t n, int L) {
    const int v = __builtin_amdgcn_readfirstlane(lr_as_const(lengths)[n]);
    return v < 1 ? 1 : (v > L ? L : v);
}
// blocks whose `lengths` may be NULL, meaning L points for every sequence (the spectral instances, lr_spectral_tiled.hpp): one wave-uniform branch
template <typename Args> struct lr_ragged_nullable { static constexpr bool value = false; };
template <typename Args>
__device__ __forceinline__ int lr_seq_points(const Args& A, int64_t n, int L) {
    if constexpr (lr_ragged_nullable<Args>::value) return A.lengths ? lr_ragged_length(A.lengths, n, L) : L;
    else if constexpr (lr_ragged<Args>::value) return lr_ragged_length(A.lengths, n, L);
    else return L;
}

// (the two-array form's lr_fused2_ok / lr_fused2_lds_bytes, the tensor kernel's lr_tens_fused_lds_bytes and the float32 footprints are HIP-free
// and live in lr_tile_plan.hpp, next to the route predicates that read them)

// Feature map of inducing tensors (gpsig/kernels.py:285-311 _K_tens_lr_feat, signature_algs.py:194-222 tensor_kern_lr_feature),
// one workgroup per tensor: its lt * E components are whitened and chained through the sketches in LDS.
template <typename V, typename Entry>
struct LrTensFusedFields {
    using value_type = V;
    const V* Z; int64_t T; int lt, E;           // Z (lt, T, E, d_eff) as the caller gives it
    ScaleParams P;
    const V* S; const V* Wh;
    int c, r, M, kind;
    V p0, p1;
    LrSketch<Entry> sk[LR_FUSED_MAX_SKETCHES];
    V* Phi; int F;
    const V* spec;          // BASE_SPECTRAL table, as LrFusedArgs::spec
};
struct LrTensFusedArgs : LrTensFusedFields<double, LrEntry> {};
struct LrTensFusedArgsF32 : LrTensFusedFields<float, LrEntryF32> {};
// blocks of the tensor kernels, forward and reverse, that carry `kzs` (lt T E, c): kappa of the tensors' points against the landmarks comes from
// memory in Z's flat point order instead of being evaluated (lr_kx.hpp; their d is 0: no point is read).  One compile-time branch.
template <typename Args> struct lr_tens_kx { static constexpr bool value = false; };

// lr_fused_inst.hip: the sequence route's launchers.  The caller fills the arguments except F, lp and rows_b, which the launcher derives
// (with the LDS row padding `pad`), and launches one workgroup per sequence (at most 2^20: the kernel strides over the rest).
// `two_arrays` picks lr_seq_features_fused2 (the caller checked lr_fused2_ok), else the three-array form: in float64 the instance
// `variant` (0-3) selects, in float32 the one instance built (512 threads, 8 entries per scalar-load batch).  A.kind == BASE_SPECTRAL
// launches the spectral instances.  Return the hipError_t of the launch.
int lr_fused_launch(hipStream_t stream, LrFusedArgs A, int pad, bool two_arrays, int variant);
int lr_fused_launch(hipStream_t stream, LrFusedArgsF32 A, int pad, bool two_arrays, int variant);
// lr_ragged_inst.hip: the three-array float64 form with per-sequence lengths (one instance: 512 threads, 8 entries per scalar-load batch)
int lr_ragged_fused_launch(hipStream_t stream, LrFusedRaggedArgs A, int pad);
// ... and the tensor route's: F derived, one workgroup per tensor
int lr_tens_fused_launch(hipStream_t stream, LrTensFusedArgs A);
int lr_tens_fused_launch(hipStream_t stream, LrTensFusedArgsF32 A);
// out[i] = float(in[i]) for n values, and the sketch entries (value narrowed, indices copied); returns the hipError_t of the launch
int lr_narrow_launch(hipStream_t stream, const double* in, int64_t n, float* out);
int lr_narrow_entries_launch(hipStream_t stream, const LrEntry* in, int64_t n, LrEntryF32* out);

// Launches a low-rank kernel with `lds` bytes of dynamic LDS.  Beyond the default 48 KB it has to be requested, on every launch that
// needs it: a process-wide cache of the granted size would be wrong on a second device and racy between contexts.  Returns the hipError_t.
template <typename Args>
int lr_launch(void (*kern)(Args), unsigned grid, unsigned threads, size_t lds, hipStream_t stream, const Args& A) {
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return int(e);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, A);
    return int(hipGetLastError());
}

// spectral_cross_api.hip: the multi-pass route's Nystrom cross matrices with SignatureSpectral's kappa (lowrank_kernels.hpp:
// lr_seq_cross_kernel / lr_tens_cross_kernel)
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
// ... and for the points of N sequences in rows of L (point p = n L + t), of which sequence n has
// lengths[n] (N int32 on the device, clamped to [1, L]): a point with t >= lengths[n] is not read, its dP row is stored as exact zeros and it
// adds nothing to dS, dalpha, domega, dgamma.  Same partial sums in the same order as spectral_cross_grad_launch on n = N L points.
int spectral_cross_grad_len_launch(hipStream_t stream, int Q, int family, int d, const double* P, int64_t N, int L, const int32_t* lengths,
                                   const double* S, int c, const double* alpha, const double* omega, const double* gamma, const double* G, double* dP,
                                   double* part, double* dS, double* dalpha, double* domega, double* dgamma, bool accumulate);

}  // namespace gpsig
