// wide_spectral_inst.hip -- the kernels of wide_spectral_kernel.hpp (SignatureSpectral's kernel-argument array of the wide route, exact mode beyond
// 32 columns) and their launchers; called from wide_api.hip.
#define GPSIG_WIDE_SPX_KERNELS
#include "wide_spectral_kernel.hpp"

namespace gpsig {

int wide_spx_prep_launch(hipStream_t stream, const double* gamma, int64_t count, double* g2) {
    if (count <= 0) return int(hipSuccess);
    hipLaunchKernelGGL(wide_spx_prep_kernel, dim3(unsigned((count + 255) / 256)), dim3(256), 0, stream, gamma, count, g2);
    return int(hipGetLastError());
}

int wide_spx_side_launch(hipStream_t stream, const double* X, int64_t rows, int64_t ld, int d, int Q, const double* omega, const double* g2, double* nrm,
                         double* ph) {
    if (rows <= 0) return int(hipSuccess);
    const int64_t nblk = (rows + 63) / 64;
    hipLaunchKernelGGL(wide_spx_side_kernel, dim3(unsigned(nblk < 65535 ? nblk : 65535)), dim3(WIDE_SPX_THREADS), 0, stream, X, rows, ld, d, Q, omega, g2, nrm,
                       ph);
    return int(hipGetLastError());
}

int wide_spx_launch(hipStream_t stream, const WideSpxArgs& A) {
    if (A.m <= 0 || A.n <= 0 || A.batch <= 0) return int(hipSuccess);
    const int64_t cb = (A.n + WIDE_SPX_TILE - 1) / WIDE_SPX_TILE, rb = (A.m + WIDE_SPX_TILE - 1) / WIDE_SPX_TILE;
    hipLaunchKernelGGL(wide_spx_kernel, dim3(unsigned(cb), unsigned(rb < 65535 ? rb : 65535), unsigned(A.batch < 65535 ? A.batch : 65535)),
                       dim3(WIDE_SPX_THREADS), 0, stream, A);
    return int(hipGetLastError());
}

}  // namespace gpsig
