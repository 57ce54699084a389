// spectral_pair.hpp -- SignatureSpectral's state-space kernel for one pair of points, its value and its gradient
// (gpsig/kernels.py:921-942; seq_core.hpp: spectral_eval is the same value from the packed table).
//
//     kappa(x, y) = sum_q alpha_q * E_q * cos(2 pi w2_q),   w1_q = |gamma_q (x - y)|^2,   w2_q = <omega_q, x - y>,
//     E_q = exp(-w1_q / 2) (Gaussian component) or exp(-sqrt(w1_q) / 2) (exponential component).
//
// The parameters come as three arrays with row stride `ld` (alpha[Q], omega[Q][ld], gamma[Q][ld]): the packed table of spectral_table()
// (ld = SPECTRAL_STRIDE) or the trainable tensors themselves (ld = d).  The pointer type is a template argument, so that the device can
// pass constant-address-space pointers (lr_as_const) and the host plain ones.  Plain C++ apart from that: the CPU suite checks the
// gradient against central differences (tests/emu/spectral_grad_host.cpp).
//
// Zero distance: an exponential component's sqrt has derivative 0 at w1 = 0 (landmarks are drawn from the points, so x == S_i occurs in
// every evaluation) -- the convention of autodiff._SqrtZeroGrad and of the torch checker; the reference's TensorFlow gives NaN there.
#pragma once

#include "seq_core.hpp"

namespace gpsig {

GPSIG_HD bool spectral_gauss(int family, int q, int Q) { return family == SPECTRAL_RBF || (family == SPECTRAL_MIXED && q < Q / 2); }

// one component: value alpha * E * cos, and its derivatives by alpha, w1, w2
struct SpectralTerm { double val, d_alpha, d_w1, d_w2; };

GPSIG_HD SpectralTerm spectral_term(double alpha, double w1, double w2, bool gauss) {
    const double two_pi = 6.283185307179586476925;
    const double ph = two_pi * w2;
    const double cs = cos(ph), sn = sin(ph);
    double env, denv;
    if (gauss) {
        env = kexp(-w1 / 2);
        denv = -env / 2;
    } else {
        const double s = sqrt(w1);
        env = kexp(-s / 2);
        denv = s > 0 ? -env / (4 * s) : 0.0;
    }
    const double ae = alpha * env;
    return SpectralTerm{ae * cs, env * cs, alpha * cs * denv, -ae * two_pi * sn};
}

// kappa(x, y); xf(f), yf(f) give the coordinates
template <typename TP, class FX, class FY>
GPSIG_HD double spectral_pair(TP alpha, TP omega, TP gamma, int ld, int Q, int family, int d, FX&& xf, FY&& yf) {
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) {
        double w1 = 0.0, w2 = 0.0;
        for (int f = 0; f < d; ++f) {
            const double diff = xf(f) - yf(f);
            const double gd = gamma[q * ld + f] * diff;
            w1 = fma(gd, gd, w1);
            w2 = fma(omega[q * ld + f], diff, w2);
        }
        acc += spectral_term(alpha[q], w1, w2, spectral_gauss(family, q, Q)).val;
    }
    return acc;
}

// kappa(x, y), and g * its gradient: gdiff(f, v) receives v = g * d kappa / d (x - y)_f once per component (the caller adds it to x's
// gradient and subtracts it from y's); dalpha[q], domega[q * ld + f], dgamma[q * ld + f] are ADDED to (any of them may be null)
template <typename TP, class FX, class FY, class GD>
GPSIG_HD double spectral_pair_grad(TP alpha, TP omega, TP gamma, int ld, int Q, int family, int d, FX&& xf, FY&& yf, double g, GD&& gdiff,
                                   double* dalpha, double* domega, double* dgamma) {
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) {
        double w1 = 0.0, w2 = 0.0;
        for (int f = 0; f < d; ++f) {
            const double diff = xf(f) - yf(f);
            const double gd = gamma[q * ld + f] * diff;
            w1 = fma(gd, gd, w1);
            w2 = fma(omega[q * ld + f], diff, w2);
        }
        const SpectralTerm t = spectral_term(alpha[q], w1, w2, spectral_gauss(family, q, Q));
        acc += t.val;
        if (dalpha) dalpha[q] += g * t.d_alpha;
        const double c1 = 2 * g * t.d_w1, c2 = g * t.d_w2;
        for (int f = 0; f < d; ++f) {
            const double diff = xf(f) - yf(f);
            const double ga = gamma[q * ld + f];
            if (domega) domega[q * ld + f] += c2 * diff;
            if (dgamma) dgamma[q * ld + f] += c1 * ga * diff * diff;
            gdiff(f, c1 * ga * ga * diff + c2 * omega[q * ld + f]);
        }
    }
    return acc;
}

}  // namespace gpsig
