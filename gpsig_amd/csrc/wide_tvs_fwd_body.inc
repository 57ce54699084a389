// The body of wide_tvs_fwd_kernel and of its ragged form wide_tvs_fwd_ragged_kernel (wide_kernels.hpp), included once in each with GPSIG_WIDE_RG
// false / true: one text, and the dense kernel compiles to exactly what it was.  A: WideTvsArgs / WideTvsRaggedArgs.
    __shared__ double etab[EXP_TAB_N];
    const WideKap K = wide_kap(A.kind, wide_tab<KD>(etab, threadIdx.x, 64), A.kp0, A.kp1);
    const int64_t t = int64_t(blockIdx.x) * 64 + threadIdx.x;
    const int M = A.M, lt = M * (M + 1) / 2;
    const int i = blockIdx.z + 1, k0 = i * (i - 1) / 2;
    for (int64_t nl = blockIdx.y; nl < A.Nc; nl += gridDim.y) {
        const int64_t n = A.n0 + nl;
        const double* col = A.arg + nl * int64_t(A.L) * A.CW + t;
        int L = A.L;
#if GPSIG_WIDE_RG
        col = A.arg + (A.off[n] - A.off[A.n0]) * A.CW + t;
        L = A.len[n];
#endif
        double u[WIDE_MAX_LEVELS];
        wide_level_fwd<E, KD>(i, col, A, L, K, u, wide_mix_ctx<KD>(A, n, t));
        for (int j = 0; j < i; ++j) A.aux[(n * lt + k0 + j) * A.Tpad + t] = u[j];
    }
