// Host driver of gpsig_amd/csrc/spectral_pair.hpp for tests/test_spectral_grad_host.py: the value and the gradient of SignatureSpectral's
// state-space kernel for one pair of points, parameters with row stride d, g = 1.
#include "spectral_pair.hpp"

extern "C" {

double sp_value(const double* alpha, const double* omega, const double* gamma, int Q, int family, int d, const double* x, const double* y) {
    return gpsig::spectral_pair(alpha, omega, gamma, d, Q, family, d, [&](int f) { return x[f]; }, [&](int f) { return y[f]; });
}

// dx, dy, dalpha, domega, dgamma are overwritten
double sp_grad(const double* alpha, const double* omega, const double* gamma, int Q, int family, int d, const double* x, const double* y,
               double* dx, double* dy, double* dalpha, double* domega, double* dgamma) {
    for (int f = 0; f < d; ++f) dx[f] = dy[f] = 0.0;
    for (int k = 0; k < Q; ++k) dalpha[k] = 0.0;
    for (int k = 0; k < Q * d; ++k) domega[k] = dgamma[k] = 0.0;
    return gpsig::spectral_pair_grad(alpha, omega, gamma, d, Q, family, d, [&](int f) { return x[f]; }, [&](int f) { return y[f]; }, 1.0,
                                     [&](int f, double v) { dx[f] += v; dy[f] -= v; }, dalpha, domega, dgamma);
}

}
