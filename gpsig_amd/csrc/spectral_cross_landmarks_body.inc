// spectral_cross_landmarks_body.inc -- the body of spectral_cross_grad_landmarks_kernel and of its lengths-aware twin (spectral_cross_api.hip),
// included between the braces of a __global__ function template <int DMAX> whose argument block is `A`: a text shared by inclusion, so that the
// existing instance stays the code it was.  A padded point (spec_cross_live) is skipped, the others keep their threads and their order.
    constexpr int NW = SC_THREADS / 64;
    constexpr int W = 1 + 2 * DMAX;
    __shared__ double red[NW][W];
    const int d = A.d, Q = A.Q, i = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const lr_const_ptr<double> al = lr_as_const(A.alpha), om = lr_as_const(A.omega), ga = lr_as_const(A.gamma);
    const lr_const_ptr<double> y = lr_as_const(A.S) + size_t(i) * d;
    double* part = A.part + (size_t(i) * A.nchunk + blockIdx.x) * A.nv;
    const int64_t step = int64_t(A.nchunk) * SC_THREADS;
    double gs[DMAX];
#pragma unroll
    for (int f = 0; f < DMAX; ++f) gs[f] = 0.0;
    for (int q = 0; q < Q; ++q) {
        const bool gauss = spectral_gauss(A.family, q, Q);
        double va = 0.0, vo[DMAX], vg[DMAX];
#pragma unroll
        for (int f = 0; f < DMAX; ++f) vo[f] = vg[f] = 0.0;
        for (int64_t pt = int64_t(blockIdx.x) * SC_THREADS + threadIdx.x; pt < A.n; pt += step) {
            if (!spec_cross_live(A, pt)) continue;
            const double g = A.G[pt * A.c + i];
            double x[DMAX];
            double w1 = 0.0, w2 = 0.0;
#pragma unroll
            for (int f = 0; f < DMAX; ++f)
                if (f < d) {
                    x[f] = A.P[pt * d + f];
                    const double diff = x[f] - y[f];
                    const double gd = ga[q * d + f] * diff;
                    w1 = fma(gd, gd, w1);
                    w2 = fma(om[q * d + f], diff, w2);
                }
            const SpectralTerm t = spectral_term(al[q], w1, w2, gauss);
            const double c1 = 2 * g * t.d_w1, c2 = g * t.d_w2;
            va = fma(g, t.d_alpha, va);
#pragma unroll
            for (int f = 0; f < DMAX; ++f)
                if (f < d) {
                    const double diff = x[f] - y[f], gq = ga[q * d + f];
                    vo[f] = fma(c2, diff, vo[f]);
                    vg[f] = fma(c1 * gq, diff * diff, vg[f]);
                    gs[f] -= c1 * gq * gq * diff + c2 * om[q * d + f];
                }
        }
        va = wave_sum(va);
        if (lane == 0) red[wave][0] = va;
#pragma unroll
        for (int f = 0; f < DMAX; ++f)
            if (f < d) {
                const double so = wave_sum(vo[f]), sg = wave_sum(vg[f]);
                if (lane == 0) { red[wave][1 + f] = so; red[wave][1 + d + f] = sg; }
            }
        __syncthreads();
        if (threadIdx.x < 1 + 2 * d) {
            double s = 0.0;
            for (int w = 0; w < NW; ++w) s += red[w][threadIdx.x];
            part[d + q * (1 + 2 * d) + threadIdx.x] = s;
        }
        __syncthreads();
    }
#pragma unroll
    for (int f = 0; f < DMAX; ++f)
        if (f < d) {
            const double s = wave_sum(gs[f]);
            if (lane == 0) red[wave][f] = s;
        }
    __syncthreads();
    if (threadIdx.x < d) {
        double s = 0.0;
        for (int w = 0; w < NW; ++w) s += red[w][threadIdx.x];
        part[threadIdx.x] = s;
    }
