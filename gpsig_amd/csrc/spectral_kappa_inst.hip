// spectral_kappa_inst.hip -- the kernels of spectral_kappa_kernel.hpp (the reverse pass of the batched SignatureSpectral kappa op) and their launchers;
// called from spectral_kappa_api.hip.
#include "ctx.hpp"
#define GPSIG_SPK_KERNELS
#include "spectral_kappa_kernel.hpp"

namespace gpsig {

int spk_weights_launch(hipStream_t stream, const SpecKappaArgs& A) {
    if (A.nb <= 0 || A.nr <= 0 || A.n <= 0) return int(hipSuccess);
    hipLaunchKernelGGL(spk_weights_kernel, dim3(unsigned(A.ncb), unsigned(A.nrb < 65535 ? A.nrb : 65535), unsigned(A.nb < 65535 ? A.nb : 65535)),
                       dim3(SPK_THREADS), 0, stream, A);
    return int(hipGetLastError());
}

int spk_reduce_launch(hipStream_t stream, const double* part, int64_t count, int64_t width, int first, double* out) {
    if (width <= 0) return int(hipSuccess);
    hipLaunchKernelGGL(spk_reduce_kernel, dim3(grid_for(width)), dim3(256), 0, stream, part, count, width, first, out);
    return int(hipGetLastError());
}

int spk_scale_launch(hipStream_t stream, const SpecKappaArgs& A) {
    hipLaunchKernelGGL(spk_scale_kernel, dim3(grid_for(A.nb * A.Q * A.nr * A.d)), dim3(256), 0, stream, A);
    return int(hipGetLastError());
}

int spk_rows_launch(hipStream_t stream, const SpecKappaArgs& A) {
    hipLaunchKernelGGL(spk_rows_kernel, dim3(grid_for(A.nb * A.nr * A.d)), dim3(256), 0, stream, A);
    return int(hipGetLastError());
}

int spk_cols_launch(hipStream_t stream, const SpecKappaArgs& A) {
    hipLaunchKernelGGL(spk_cols_kernel, dim3(grid_for(A.nb * A.n * A.d)), dim3(256), 0, stream, A);
    return int(hipGetLastError());
}

int spk_param_launch(hipStream_t stream, const SpecKappaArgs& A, int side) {
    const int64_t rows = A.nb * (side ? A.n : A.nr), nsl = (rows + SPK_SLICE - 1) / SPK_SLICE;
    hipLaunchKernelGGL(spk_param_kernel, dim3(unsigned(nsl < 65535 ? nsl : 65535), unsigned(A.Q)), dim3(64), 0, stream, A, side);
    return int(hipGetLastError());
}

int spk_finish_launch(hipStream_t stream, const SpecKappaArgs& A, double* dalpha, double* domega, double* dgamma) {
    hipLaunchKernelGGL(spk_finish_kernel, dim3(grid_for(A.Q + 2 * int64_t(A.Q) * A.d)), dim3(256), 0, stream, A, dalpha, domega, dgamma);
    return int(hipGetLastError());
}

}  // namespace gpsig
