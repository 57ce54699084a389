// lr_tiled_fwd_body.inc -- the body of lr_seq_features_tiled_kernel, included between the braces of a __global__ function template <int THREADS> whose
// argument block is `A`: LrTiledArgs in lr_tiled_kernel.hpp, LrTiledRaggedArgs (per-sequence lengths) in lr_ragged_inst.hip, LrTiledSpectralArgs
// (lr_tile_u evaluates spectral_pair) in lr_spectral_tiled_inst.hip, LrTiledKxArgs (lr_tile_u loads kxs) in lr_kx_inst.hip.  A text shared by inclusion, not a function: behind a reference or a
// by-value parameter the existing instance compiles to other code (more registers, or scratch).
    constexpr int NW = THREADS / 64, UNROLL = 8;
    constexpr bool RAGGED = lr_ragged<decltype(A)>::value;
    extern __shared__ double lrt_lds[];
    const int lp = A.lp, c = A.c, r = A.r, L = A.L, d = A.d, M = A.M, rows = A.rows_b, TL = A.TL;
    double* const U = lrt_lds;                                  // [c][lp]
    double* const bufA = U + size_t(c) * lp;                    // [rows][lp]
    double* const bufB = bufA + size_t(rows) * lp;              // [rows][lp]
    double* const cf = bufB + size_t(rows) * lp;                // [LR_TILE_LEVELS][rows]: level i at (i - 1) rows
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int halo = A.difference ? 1 : 0;
    const int l = L - halo;
    int ln = l, ntiles = A.ntiles;                              // the current sequence's steps and tiles: the ragged instances set them per sequence

    for (int64_t n = blockIdx.x; n < A.N; n += gridDim.x) {
        const double* Xn = A.X + n * int64_t(L) * d;
        double* phi = A.Phi + n * int64_t(A.F);
        if constexpr (RAGGED) {                                  // the sequence's own steps and tiles, from lengths[n] (wave-uniform)
            ln = lr_seq_points(A, n, L) - halo;
            ntiles = lr_tile_count(ln, TL);
        }
        __syncthreads();                                         // (the previous sequence's features were read from the carries)
        for (int q = threadIdx.x; q < M * rows; q += THREADS) cf[q] = 0.0;
        for (int k = 0; k < ntiles; ++k) {
            const int t0 = lr_tile_first(k, TL), tl = lr_tile_steps(ln, k, TL), np = tl + halo;
            const int nchunk = (tl + 63) / 64;
            lr_tile_u<THREADS>(A, Xn + int64_t(t0) * d, tl, np, bufB, bufA, bufB, U, lane, wave);
            lr_tile_excumsum<THREADS>(U, bufA, c, lp, tl, cf, M >= 2, nullptr, 0);                    // level 1; E_2 of the tile
            __syncthreads();
            double* cur = bufA;
            double* nxt = bufB;
            for (int lev = 2; lev <= M; ++lev) {
                lr_sketch_apply<NW, UNROLL>(A.sk[lev - 2].colptr, A.sk[lev - 2].ent, r, U, cur, nxt, false, lp, tl, nchunk, lane, wave);
                __syncthreads();
                lr_tile_excumsum<THREADS>(nxt, nxt, r, lp, tl, cf + size_t(lev - 1) * rows, lev < M, nullptr, 0);
                __syncthreads();
                double* tmp = cur; cur = nxt; nxt = tmp;
            }
        }
        if (threadIdx.x == 0) phi[0] = 1.0;
        for (int j = threadIdx.x; j < c; j += THREADS) phi[1 + j] = cf[j];
        for (int lev = 2; lev <= M; ++lev)
            for (int j = threadIdx.x; j < r; j += THREADS) phi[1 + c + (lev - 2) * r + j] = cf[size_t(lev - 1) * rows + j];
    }
