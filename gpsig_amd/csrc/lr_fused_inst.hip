// lr_fused_inst.hip -- the fused low-rank feature kernels, float64 and float32, plain and spectral, and their launchers (own translation
// unit: lr_api.hip and lr_grad_api.hip only see the arguments, lr_fused_args.hpp).
#include "lr_fused_kernel.hpp"

namespace gpsig {

namespace {
// what every caller of the sequence route would derive the same way: F, the LDS row stride, the work arrays' rows, the grid
template <typename Args>
void seq_fields(Args& A, int pad, unsigned* grid) {
    A.F = 1 + A.c + (A.M - 1) * A.r;
    A.lp = lr_fused_stride(A.L, pad);
    A.rows_b = A.c > A.r ? A.c : A.r;
    if (A.P.d_eff() > A.rows_b) A.rows_b = A.P.d_eff();
    *grid = unsigned(A.N < (int64_t(1) << 20) ? A.N : (int64_t(1) << 20));
}
}  // namespace

// SignatureSpectral's instances (its kappa in phase 1), the two-array form and float32: one instance each, 512 threads and 8 entries per
// scalar-load batch (the family's phase 1 -- Q components of 3d multiply-adds, an exp and a cos per pair -- is not worth a variant search)
int lr_fused_launch(hipStream_t stream, LrFusedArgs A, int pad, bool two_arrays, int variant) {
    unsigned grid;
    seq_fields(A, pad, &grid);
    const bool spec = A.kind == BASE_SPECTRAL;
    if (two_arrays) {
        const size_t lds = lr_fused2_lds_bytes(A.c, A.r, A.P.d_eff(), A.L, pad);
        return spec ? lr_launch(lr_seq_features_fused2_spectral_kernel<512, 8>, grid, 512, lds, stream, A)
                    : lr_launch(lr_seq_features_fused2_kernel<512, 8>, grid, 512, lds, stream, A);
    }
    const size_t lds = lr_fused_lds_bytes(A.c, A.r, A.P.d_eff(), A.L, pad);
    if (spec) return lr_launch(lr_seq_features_fused_spectral_kernel<512, 8>, grid, 512, lds, stream, A);
    // BASELINE configs[2]'s sequences (L=50, c=r=50, 'sqrt'), same box: 256 threads / 4 entries per batch 4.32 ms, 256 / 8 3.84,
    // 512 / 4 2.71, 512 / 8 2.57, 1024 / 4 3.09, 1024 / 8 4.01 (profiles/r02_lowrank.txt)
    switch (variant) {
        case 1: return lr_launch(lr_seq_features_fused_kernel<256, 4>, grid, 256, lds, stream, A);
        case 2: return lr_launch(lr_seq_features_fused_kernel<256, 8>, grid, 256, lds, stream, A);
        case 3: return lr_launch(lr_seq_features_fused_kernel<512, 4>, grid, 512, lds, stream, A);
        default: return lr_launch(lr_seq_features_fused_kernel<512, 8>, grid, 512, lds, stream, A);
    }
}

int lr_fused_launch(hipStream_t stream, LrFusedArgsF32 A, int pad, bool two_arrays, int /*variant: the float64 instances'*/) {
    unsigned grid;
    seq_fields(A, pad, &grid);
    const bool spec = A.kind == BASE_SPECTRAL;
    if (two_arrays) {
        const size_t lds = lr_fused2_lds_bytes_f32(A.c, A.r, A.P.d_eff(), A.L, pad);
        return spec ? lr_launch(lr_seq_features_fused2_spectral_f32_kernel<512, 8>, grid, 512, lds, stream, A)
                    : lr_launch(lr_seq_features_fused2_f32_kernel<512, 8>, grid, 512, lds, stream, A);
    }
    const size_t lds = lr_fused_lds_bytes_f32(A.c, A.r, A.P.d_eff(), A.L, pad);
    return spec ? lr_launch(lr_seq_features_fused_spectral_f32_kernel<512, 8>, grid, 512, lds, stream, A)
                : lr_launch(lr_seq_features_fused_f32_kernel<512, 8>, grid, 512, lds, stream, A);
}

int lr_tens_fused_launch(hipStream_t stream, LrTensFusedArgs A) {
    A.F = 1 + A.c + (A.M - 1) * A.r;
    const size_t lds = lr_tens_fused_lds_bytes(A.c, A.r, A.P.d_eff(), A.lt, A.E);
    return A.kind == BASE_SPECTRAL ? lr_launch(lr_tens_features_fused_spectral_kernel, unsigned(A.T), LR_TENS_THREADS, lds, stream, A)
                                   : lr_launch(lr_tens_features_fused_kernel, unsigned(A.T), LR_TENS_THREADS, lds, stream, A);
}

int lr_tens_fused_launch(hipStream_t stream, LrTensFusedArgsF32 A) {
    A.F = 1 + A.c + (A.M - 1) * A.r;
    const size_t lds = lr_tens_fused_lds_bytes_f32(A.c, A.r, A.P.d_eff(), A.lt, A.E);
    return A.kind == BASE_SPECTRAL ? lr_launch(lr_tens_features_fused_spectral_f32_kernel, unsigned(A.T), LR_TENS_THREADS, lds, stream, A)
                                   : lr_launch(lr_tens_features_fused_f32_kernel, unsigned(A.T), LR_TENS_THREADS, lds, stream, A);
}

// ---- float32: what the kernels read of the float64 state, narrowed on the device
namespace {
__global__ __launch_bounds__(256) void lr_narrow_kernel(const double* __restrict__ in, int64_t n, float* __restrict__ out) {
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) out[i] = float(in[i]);
}

__global__ __launch_bounds__(256) void lr_narrow_entries_kernel(const LrEntry* __restrict__ in, int64_t n, LrEntryF32* __restrict__ out) {
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
        out[i] = LrEntryF32{float(in[i].val), in[i].i1, in[i].i2, 0};
}

unsigned narrow_grid(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return unsigned(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}
}  // namespace

int lr_narrow_launch(hipStream_t stream, const double* in, int64_t n, float* out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(lr_narrow_kernel, dim3(narrow_grid(n)), dim3(256), 0, stream, in, n, out);
    return int(hipGetLastError());
}

int lr_narrow_entries_launch(hipStream_t stream, const LrEntry* in, int64_t n, LrEntryF32* out) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(lr_narrow_entries_kernel, dim3(narrow_grid(n)), dim3(256), 0, stream, in, n, out);
    return int(hipGetLastError());
}

}  // namespace gpsig
