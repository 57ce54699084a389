// spectral_cross_points_body.inc -- the body of spectral_cross_grad_points_kernel and of its lengths-aware twin (spectral_cross_api.hip), included
// between the braces of a __global__ function template <int DMAX> whose argument block is `A`: a text shared by inclusion, so that the existing
// instance stays the code it was.  A padded point's row (spec_cross_live) is zeros and nothing of it is read.
    const int d = A.d, Q = A.Q;
    const lr_const_ptr<double> al = lr_as_const(A.alpha), om = lr_as_const(A.omega), ga = lr_as_const(A.gamma);
    for (int64_t pt = blockIdx.x * int64_t(SC_THREADS) + threadIdx.x; pt < A.n; pt += int64_t(gridDim.x) * SC_THREADS) {
        if (!spec_cross_live(A, pt)) {
            for (int f = 0; f < d; ++f) A.dP[pt * d + f] = 0.0;
            continue;
        }
        double x[DMAX], gx[DMAX];
#pragma unroll
        for (int f = 0; f < DMAX; ++f) {
            x[f] = f < d ? A.P[pt * d + f] : 0.0;
            gx[f] = 0.0;
        }
        for (int i = 0; i < A.c; ++i) {
            const lr_const_ptr<double> y = lr_as_const(A.S) + size_t(i) * d;
            const double g = A.G[pt * A.c + i];
            for (int q = 0; q < Q; ++q) {
                double w1 = 0.0, w2 = 0.0;
#pragma unroll
                for (int f = 0; f < DMAX; ++f)
                    if (f < d) {
                        const double diff = x[f] - y[f];
                        const double gd = ga[q * d + f] * diff;
                        w1 = fma(gd, gd, w1);
                        w2 = fma(om[q * d + f], diff, w2);
                    }
                const SpectralTerm t = spectral_term(al[q], w1, w2, spectral_gauss(A.family, q, Q));
                const double c1 = 2 * g * t.d_w1, c2 = g * t.d_w2;
#pragma unroll
                for (int f = 0; f < DMAX; ++f)
                    if (f < d) {
                        const double diff = x[f] - y[f], gq = ga[q * d + f];
                        gx[f] += c1 * gq * gq * diff + c2 * om[q * d + f];
                    }
            }
        }
#pragma unroll
        for (int f = 0; f < DMAX; ++f)
            if (f < d) A.dP[pt * d + f] = gx[f];
    }
