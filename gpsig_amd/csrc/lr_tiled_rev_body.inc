// lr_tiled_rev_body.inc -- the body of lr_seq_features_grad_tiled_kernel, included between the braces of a __global__ function template <int THREADS> whose
// argument block is `A`: LrTiledArgs in lr_tiled_kernel.hpp, LrTiledRaggedArgs (per-sequence lengths) in lr_ragged_inst.hip, LrTiledSpectralArgs in
// lr_spectral_tiled_inst.hip, LrTiledKxArgs (kxs from memory) in lr_kx_inst.hip.  A text shared by inclusion, not a function: behind a reference or a by-value parameter the existing instance compiles
// to other code (more registers, or scratch).  The phases that depend on the family are overloaded on the block (lr_tiled_kernel.hpp).
    constexpr int NW = THREADS / 64, UNROLL = 8;
    constexpr bool RAGGED = lr_ragged<decltype(A)>::value;
    extern __shared__ double lrt_lds[];
    const int lp = A.lp, c = A.c, r = A.r, L = A.L, d = A.d, M = A.M, rows = A.rows_b, TL = A.TL;
    double* const B0 = lrt_lds;                                 // U; later kxs; later per-wave partial sums
    double* const B1 = B0 + size_t(rows) * lp;                  // x; dU; x again
    double* const BX = B1 + size_t(rows) * lp;
    double* const BY = BX + size_t(rows) * lp;
    double* const cf = BY + size_t(rows) * lp;                  // [LR_TILE_LEVELS][rows]: forward carries, level i at (i - 1) rows
    double* const cb = cf + size_t(LR_TILE_LEVELS) * rows;      // [LR_TILE_LEVELS][rows]: reverse carries of dE_i at (i - 1) rows
    double* const dun = cb + size_t(LR_TILE_LEVELS) * rows;     // [rows]: the later tile's first dU
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int halo = A.difference ? 1 : 0;
    const int l = L - halo;
    int ln = l, ntiles = A.ntiles;                              // the current sequence's steps and tiles: the ragged instances set them per sequence
    double* const escr = A.escr + int64_t(blockIdx.x) * A.escr_stride;
    const lr_const_ptr<double> Sg = lr_as_const(A.S);
    const lr_const_ptr<double> Whg = lr_as_const(A.Wh);

    // this workgroup's sums over its tiles and sequences: the pairs per thread that c <= 64, c d <= 4096 need at this workgroup size
    constexpr int KW = LR_GRAD_KW * LR_GRAD_THREADS / THREADS, KS = LR_GRAD_KS * LR_GRAD_THREADS / THREADS;
    double accW[KW], accS[KS], accP = 0.0;
#pragma unroll
    for (int k = 0; k < KW; ++k) accW[k] = 0.0;
#pragma unroll
    for (int k = 0; k < KS; ++k) accS[k] = 0.0;

    for (int64_t n = blockIdx.x; n < A.N; n += gridDim.x) {
        const double* Xn = A.X + n * int64_t(L) * d;
        const double* g = A.dPhi + n * int64_t(A.F);
        if constexpr (RAGGED) {                                  // the sequence's own steps and tiles, from lengths[n] (wave-uniform); the gX rows
            ln = lr_seq_points(A, n, L) - halo;                  // of its padded points are zeros
            ntiles = lr_tile_count(ln, TL);
            lr_tile_zero_padded<THREADS>(A, n, ln + halo);
        }
        __syncthreads();
        // ---- the carries of this sequence: cf = 0;  cb_i = g_{i-1} (what the suffix sum of the last tile starts from);  dun = 0
        for (int q = threadIdx.x; q < LR_TILE_LEVELS * rows; q += THREADS) cf[q] = 0.0;
        for (int lev = 2; lev <= M; ++lev) {
            const double* gl = lev == 2 ? g + 1 : g + 1 + c + (lev - 3) * r;
            for (int j = threadIdx.x; j < (lev == 2 ? c : r); j += THREADS) cb[size_t(lev - 1) * rows + j] = gl[j];
        }
        for (int j = threadIdx.x; j < rows; j += THREADS) dun[j] = 0.0;
        // ---- pass A: E_2 = excumsum_t(U), E_{i+1} = excumsum_t(sketch_i(U, E_i)) of the whole sequence -> scratch, [column][l] per level
        for (int k = 0; (M >= 2 || lr_keeps_kxs<decltype(A)>::value) && k < ntiles; ++k) {
            const int t0 = lr_tile_first(k, TL), tl = lr_tile_steps(ln, k, TL), np = tl + halo;
            const int nchunk = (tl + 63) / 64;
            lr_tile_u<THREADS>(A, Xn + int64_t(t0) * d, tl, np, B1, BX, BY, B0, lane, wave);
            lr_tile_keep_kxs<THREADS>(A, BX, escr, ln + halo, t0, np);
            lr_tile_excumsum<THREADS>(B0, BX, c, lp, tl, cf, true, escr + t0, ln);
            __syncthreads();
            int64_t eo = int64_t(c) * ln;
            double* cur = BX;
            double* nxt = BY;
            for (int lev = 2; lev < M; ++lev) {
                lr_sketch_apply<NW, UNROLL>(A.sk[lev - 2].colptr, A.sk[lev - 2].ent, r, B0, cur, nxt, false, lp, tl, nchunk, lane, wave);
                __syncthreads();
                lr_tile_excumsum<THREADS>(nxt, nxt, r, lp, tl, cf + size_t(lev - 1) * rows, true, escr + eo + t0, ln);
                __syncthreads();
                eo += int64_t(r) * ln;
                double* tmp = cur; cur = nxt; nxt = tmp;
            }
        }
        // ---- pass B: tiles in decreasing time
        for (int k = ntiles - 1; k >= 0; --k) {
            const int t0 = lr_tile_first(k, TL), tl = lr_tile_steps(ln, k, TL), np = tl + halo;
            const int nchunk = (tl + 63) / 64, pchunk = (np + 63) / 64;
            const int q0 = halo && k > 0 ? 1 : 0;               // the tile's first point belongs to the tile before it
            __syncthreads();                                     // (the previous tile's dS sums read B1, BX and BY)
            lr_tile_u_again<THREADS>(A, Xn + int64_t(t0) * d, tl, np, B1, BX, BY, B0, lane, wave, escr, ln + halo, t0);
            for (int q = threadIdx.x; q < c * lp; q += THREADS) B1[q] = 0.0;                          // dU
            double* Y = BY;                                     // dP of the level being processed
            double* Xb = BX;                                    // E of that level, then dE
            if (M >= 2) {
                const double* gM = g + 1 + c + (M - 2) * r;
                for (int ch = 0; ch < nchunk; ++ch) {
                    const int t = ch * 64 + lane;
                    if (t < tl)
                        for (int j = wave; j < r; j += NW) Y[j * lp + t] = gM[j];
                }
            }
            __syncthreads();
            for (int lev = M; lev >= 2; --lev) {
                const int w = lev == 2 ? c : r;                 // width of E_lev
                int64_t eo = 0;
                for (int i = 2; i < lev; ++i) eo += int64_t(i == 2 ? c : r) * ln;
                for (int q = threadIdx.x; q < w * tl; q += THREADS) {
                    const int j = q / tl, t = q - j * tl;
                    Xb[j * lp + t] = escr[eo + int64_t(j) * ln + t0 + t];
                }
                __syncthreads();
                const LrGradSketch sk = A.sk[lev - 2];
                lr_sketch_apply<NW, UNROLL>(sk.ptr1, sk.ent1, c, Xb, Y, B1, true, lp, tl, nchunk, lane, wave);     // dU[i1] += val E[i2] dP[j]
                __syncthreads();
                lr_sketch_apply<NW, UNROLL>(sk.ptr2, sk.ent2, w, B0, Y, Xb, false, lp, tl, nchunk, lane, wave);    // dE[i2]  = val U[i1] dP[j]
                __syncthreads();
                // dP_{lev-1}[t] = g_{lev-1} + sum_{t' > t} dE[t'], in place: the later tiles' share comes in, this tile's goes out through cb
                double* const cbl = cb + size_t(lev - 1) * rows;
                for (int j = threadIdx.x; j < w; j += THREADS) {
                    double run = cbl[j];
                    double* e = Xb + size_t(j) * lp;
                    for (int t = tl - 1; t >= 0; --t) { const double v = e[t]; e[t] = run; run += v; }
                    cbl[j] = run;
                }
                __syncthreads();
                double* tmp = Xb; Xb = Y; Y = tmp;              // Y: dP_{lev-1}
            }
            // level 1: Phi_1 = sum_t U (M == 1: that is all there is)
            for (int ch = 0; ch < nchunk; ++ch) {
                const int t = ch * 64 + lane;
                if (t < tl)
                    for (int j = wave; j < c; j += NW) B1[j * lp + t] += M >= 2 ? Y[j * lp + t] : g[1 + j];
            }
            __syncthreads();
            // dfeat[j][q] -> Xb for the tile's own points q0 <= q < np: the adjoint of the time difference; dU beyond the tile from dun
            for (int ch = 0; ch < pchunk; ++ch) {
                const int t = ch * 64 + lane;
                if (t >= q0 && t < np)
                    for (int j = wave; j < c; j += NW)
                        Xb[j * lp + t] = halo ? (t >= 1 ? B1[j * lp + t - 1] : 0.0) - (t < tl ? B1[j * lp + t] : dun[j]) : B1[j * lp + t];
            }
            __syncthreads();
            if (tl > 0)
                for (int j = threadIdx.x; j < c; j += THREADS) dun[j] = B1[j * lp];
            __syncthreads();
            // x -> B1 and kxs -> B0 once more (U and dU are done with)
            lr_tile_kxs_again<THREADS>(A, Sg, Xn + int64_t(t0) * d, np, pchunk, B1, B0, escr, ln + halo, t0, lane, wave);
            lr_grad_whiten_adjoint<THREADS>(c, lp, q0, np, B0, Xb, Whg, Y, accW, lane, wave);
            __syncthreads();
            lr_grad_base_phase<THREADS>(A, Sg, n, t0, q0, np, B0, B1, Xb, Y, accS, accP, lane, wave);
        }
    }
    lr_grad_write_partials<THREADS>(A, accW, accS, accP, lrt_lds, lane, wave);
