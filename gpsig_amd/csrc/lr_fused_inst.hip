// lr_fused_inst.hip -- the fused low-rank feature kernel and its launcher (own translation unit: api.hip only sees the arguments).
#include "lr_fused_kernel.hpp"

namespace gpsig {

namespace {
template <int THREADS, int UNROLL>
int launch(hipStream_t stream, const LrFusedArgs& A, unsigned grid, size_t lds) {
    if (lds > 48 * 1024) {                           // dynamic LDS beyond the default has to be requested: per launch (no process-wide cache of what
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(lr_seq_features_fused_kernel<THREADS, UNROLL>),   // one device was granted)
                                           hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return int(e);
    }
    hipLaunchKernelGGL((lr_seq_features_fused_kernel<THREADS, UNROLL>), dim3(grid), dim3(THREADS), lds, stream, A);
    return int(hipGetLastError());
}
}  // namespace

int lr_fused_launch(hipStream_t stream, const LrFusedArgs& A, unsigned grid, int variant) {
    const size_t lds = sizeof(double) * size_t(A.lp) * (size_t(A.c) + 2 * size_t(A.rows_b));
    if (A.kind == BASE_SPECTRAL) return lr_fused_spectral_launch(stream, A, grid, lds);
    // BASELINE configs[2]'s sequences (L=50, c=r=50, 'sqrt'), same box: 256 threads / 4 entries per batch 4.32 ms, 256 / 8 3.84,
    // 512 / 4 2.71, 512 / 8 2.57, 1024 / 4 3.09, 1024 / 8 4.01 (profiles/r02_lowrank.txt)
    switch (variant) {
        case 1: return launch<256, 4>(stream, A, grid, lds);
        case 2: return launch<256, 8>(stream, A, grid, lds);
        case 3: return launch<512, 4>(stream, A, grid, lds);
        default: return launch<512, 8>(stream, A, grid, lds);
    }
}

int lr_fused2_launch(hipStream_t stream, const LrFusedArgs& A, unsigned grid) {
    const size_t lds = sizeof(double) * size_t(A.lp) * 2 * size_t(A.rows_b);
    if (A.kind == BASE_SPECTRAL) return lr_fused2_spectral_launch(stream, A, grid, lds);
    auto kern = lr_seq_features_fused2_kernel<512, 8>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return int(e);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, stream, A);
    return int(hipGetLastError());
}

int lr_tens_fused_launch(hipStream_t stream, const LrTensFusedArgs& A) {
    const size_t lds = lr_tens_fused_lds_bytes(A.c, A.r, A.P.d_eff(), A.lt, A.E);
    if (A.kind == BASE_SPECTRAL) return lr_tens_fused_spectral_launch(stream, A, lds);
    hipLaunchKernelGGL(lr_tens_features_fused_kernel, dim3(unsigned(A.T)), dim3(LR_TENS_THREADS), lds, stream, A);
    return int(hipGetLastError());
}

// ---- SignatureSpectral: the same kernels with its kappa in phase 1, one instance each (the family's phase 1 -- Q components of 3d
// multiply-adds, an exp and a cos per pair -- is not worth a variant search of its own)
int lr_fused_spectral_launch(hipStream_t stream, const LrFusedArgs& A, unsigned grid, size_t lds) {
    auto kern = lr_seq_features_fused_spectral_kernel<512, 8>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return int(e);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, stream, A);
    return int(hipGetLastError());
}

int lr_fused2_spectral_launch(hipStream_t stream, const LrFusedArgs& A, unsigned grid, size_t lds) {
    auto kern = lr_seq_features_fused2_spectral_kernel<512, 8>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return int(e);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, stream, A);
    return int(hipGetLastError());
}

int lr_tens_fused_spectral_launch(hipStream_t stream, const LrTensFusedArgs& A, size_t lds) {
    hipLaunchKernelGGL(lr_tens_features_fused_spectral_kernel, dim3(unsigned(A.T)), dim3(LR_TENS_THREADS), lds, stream, A);
    return int(hipGetLastError());
}

// ---- float32 forms: one instance each (512 threads, 8 entries per scalar-load batch: the float64 default)
namespace {
template <typename K, typename Args>
int launch_f32(K kern, hipStream_t stream, const Args& A, unsigned grid, unsigned threads, size_t lds) {
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return int(e);
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, stream, A);
    return int(hipGetLastError());
}

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

int lr_fused_f32_launch(hipStream_t stream, const LrFusedArgsF32& A, unsigned grid, bool two_arrays) {
    if (two_arrays) {
        const size_t lds = sizeof(float) * size_t(A.lp) * 2 * size_t(A.rows_b);
        return A.kind == BASE_SPECTRAL ? launch_f32(lr_seq_features_fused2_spectral_f32_kernel<512, 8>, stream, A, grid, 512, lds)
                                       : launch_f32(lr_seq_features_fused2_f32_kernel<512, 8>, stream, A, grid, 512, lds);
    }
    const size_t lds = sizeof(float) * size_t(A.lp) * (size_t(A.c) + 2 * size_t(A.rows_b));
    return A.kind == BASE_SPECTRAL ? launch_f32(lr_seq_features_fused_spectral_f32_kernel<512, 8>, stream, A, grid, 512, lds)
                                   : launch_f32(lr_seq_features_fused_f32_kernel<512, 8>, stream, A, grid, 512, lds);
}

int lr_tens_fused_f32_launch(hipStream_t stream, const LrTensFusedArgsF32& A) {
    const size_t lds = lr_tens_fused_lds_bytes_f32(A.c, A.r, A.P.d_eff(), A.lt, A.E);
    return A.kind == BASE_SPECTRAL ? launch_f32(lr_tens_features_fused_spectral_f32_kernel, stream, A, unsigned(A.T), LR_TENS_THREADS, lds)
                                   : launch_f32(lr_tens_features_fused_f32_kernel, stream, A, unsigned(A.T), LR_TENS_THREADS, lds);
}

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
