// The body of wide_lattice_fwd_kernel and of its ragged form wide_lattice_fwd_ragged_kernel (wide_kernels.hpp), included once in each with
// GPSIG_WIDE_RG 0 / 1: one text, and the dense kernel compiles to exactly what it was.  A: WideLatArgs / WideLatRaggedArgs.
    __shared__ double etab[EXP_TAB_N];
    __shared__ double xw[2][NW][LQ + 2];
    const double* const ktab = wide_tab<KD>(etab, threadIdx.x, 64 * NW);
    constexpr int GL = 64 * NW, PF = wide_lat_pf(C);
    const int lam = threadIdx.x, M = A.M, wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int dr = A.difference ? 1 : 0;
    int L1 = A.L1, L2 = A.L2, R1 = L1 - dr, R2 = L2 - dr, TF = R1 + GL - 1;
    for (int64_t pp = blockIdx.x; pp < A.P; pp += gridDim.x) {
        if constexpr (NW > 1) {
            __syncthreads();
            if (ln == 63) {
#pragma unroll
                for (int m = 0; m < LQ + 2; ++m) xw[0][wv][m] = xw[1][wv][m] = 0.0;
            }
            __syncthreads();
        }
        const int64_t pg = A.p0 + pp;
        WideLatDm<C, KD> dmg;
        dmg.lat = A.arg + (pg / A.N2) * A.si + (pg % A.N2) * A.sj;
        dmg.ld = A.ld;
#if GPSIG_WIDE_RG
        const int64_t i = pg / A.N2, j = A.ld ? pg % A.N2 : i;          // (the block diagonal: the sequence against itself)
        L1 = A.len1[i]; L2 = A.len2[j];
        R1 = L1 - dr; R2 = L2 - dr; TF = R1 + GL - 1;
        dmg.lat = A.arg + (A.rbase[i] - A.rbase[0]) * (A.ld ? A.ld : 1) + (A.cbase ? A.cbase[j] : 0);
        dmg.ld = A.ld ? A.ld : L2;
#endif
        dmg.b0 = C * lam; dmg.L2 = L2; dmg.K = wide_kap(A.kind, ktab, A.kp0, A.kp1); dmg.diff = dr;
        { const int nv = R2 - C * lam; dmg.nvalid = nv < 0 ? 0 : (nv > C ? C : nv); }
        dmg.mix_terms(A, pg);
        WaveFwd<C, LQ> fw;
        fw.reset();
        // the argument rows of the coming PF steps are in flight while a step computes (a launch of a few lattices is one wavefront per
        // SIMD: nothing else hides the latency of these strided loads)
        double raw[PF][C + 1];
        if (dr) { dmg.load(0, true, raw[0]); dmg.prime(raw[0]); }
#pragma unroll
        for (int u = 0; u < PF; ++u) { const int r = u - lam + dr; dmg.load(r, r >= 0 && r < L1, raw[u]); }
        double kM = 0.0;
        for (int t0 = 0; t0 < TF; t0 += PF) {
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                const int t = t0 + u;
                if (t >= TF) break;
                double cin[LQ + 2], cur[C + 1];
                cin[0] = 0.0;
#pragma unroll
                for (int m = 1; m < LQ + 2; ++m) {
                    cin[m] = wide_from_left(fw.sout[m]);
                    if constexpr (NW > 1) {
                        const double x = xw[t & 1][wv > 0 ? wv - 1 : 0][m];
                        cin[m] = (ln == 0 && wv > 0) ? x : cin[m];
                    }
                }
#pragma unroll
                for (int c = 0; c <= C; ++c) cur[c] = raw[u][c];
                const int a = t - lam;
                { const int r = a + PF + dr; dmg.load(r, r >= 0 && r < L1, raw[u]); }
                if (a >= 0 && a < R1) {
                    double dm[C];
                    dmg.row(cur, true, dm);
                    fw.step(dm, cin, M);
#pragma unroll
                    for (int m = 1; m <= LQ + 1; ++m)
                        if (m == M) kM += fw.sout[m];
                }
                if constexpr (NW > 1) {
                    if (ln == 63) {
#pragma unroll
                        for (int m = 1; m < LQ + 2; ++m) xw[(t + 1) & 1][wv][m] = fw.sout[m];
                    }
                    __syncthreads();
                }
            }
        }
        if (lam == GL - 1) {
            A.out[pg] = 1.0;                                                       // signature_algs.py:20
#pragma unroll
            for (int m = 1; m <= LQ; ++m)
                if (m < M) A.out[int64_t(m) * A.Ptot + pg] = fw.q[m - 1][C - 1];
            A.out[int64_t(M) * A.Ptot + pg] = kM;
        }
    }
