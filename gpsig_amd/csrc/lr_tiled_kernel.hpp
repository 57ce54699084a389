// lr_tiled_kernel.hpp -- the low-rank feature map of a batch of sequences and its reverse pass for sequences whose (width, L) arrays do
// not fit the LDS: the whole-sequence kernels (lr_fused_kernel.hpp, lr_grad_kernel.hpp) walked in TILES of TL time steps (lr_tile_plan.hpp).
//
// Everything in the map is elementwise in time except the running sums, so a tile is self-contained given a few carried column vectors
// (rows of LDS behind the arrays, reset at every sequence a workgroup takes):
//   forward    tiles in increasing time.  cf[i][j] = sum of P_i[j] (P_1 = U) over the earlier tiles: what E_{i+1} = excumsum_t(P_i) starts
//              from in this tile, and Phi_i once the last tile is done.  The additions happen in the order of the whole-sequence kernel.
//              With `difference` a tile of tl steps reads tl + 1 points (U[t] = feat[t+1] - feat[t]).
//   reverse    pass A: the forward pass again, tiles in increasing time; the E_i of the WHOLE sequence go to the workgroup's scratch.
//              pass B: tiles in decreasing time.  A tile recomputes x, kxs, feat and U, walks the levels M .. 2 and level 1:
//                cb[i][j] = g_{i-1}[j] + the column sums of dE_i over the later tiles: what the suffix sum dP_{i-1}[t] starts from;
//                dun[j]   = the later tile's first dU: dfeat[p] = dU[p-1] - dU[p] of the tile's last point needs it.
//              With `difference` tile k completes the points (t0, t0 + tl] (tile 0 also point 0), without it [t0, t0 + tl): every gX row
//              is written exactly once, by one tile -- no atomics, bit-for-bit repeatable.  dWh, dS and the base parameter add up in the
//              per-thread registers over tiles and sequences and leave as one partial per workgroup (lr_grad_reduce_kernel).
// Layout, lane mappings and the loops themselves are the whole-sequence kernels' (lr_grad_kernel.hpp: lr_sketch_apply, lr_cross_base,
// lr_grad_whiten_adjoint, lr_grad_base_phase): arrays [column][time] with the row stride of a tile, lane = time, thread = column for the
// running sums, sketch entries through the scalar unit.  Float64; the kernels here serve the families of base_eval, SignatureSpectral's
// instances of the same bodies are in lr_spectral_tiled_inst.hip.
#pragma once

#include "lr_grad_kernel.hpp"
#include "lr_tile_plan.hpp"

namespace gpsig {

// lp: row stride of a tile's arrays; rows_b: rows of the work arrays (forward max(c, r, d), reverse lr_grad_rows); escr: reverse only
struct LrTiledArgs : LrGradArgs {
    double* Phi;            // forward: (N, F)
    int TL, ntiles;
};
// the ragged instances' (lr_fused_args.hpp: lr_ragged): sequence n has lengths[n] of its L points -- its own number of tiles, the last one
// short as any last tile; TL, lp and the LDS size are those of L; the reverse pass stores zeros in the gX rows beyond its points
struct LrTiledRaggedArgs : LrTiledArgs { const int32_t* lengths; };
template <> struct lr_ragged<LrTiledRaggedArgs> { static constexpr bool value = true; };

// a tile's feat -> ft and U -> u from its kxs in kx: `np` points, `tl` steps.  Ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void lr_tile_feat_u(const LrTiledArgs& A, int tl, int np, const double* kx, double* ft, double* u, int lane, int wave) {
    constexpr int NW = THREADS / 64;
    const int lp = A.lp, c = A.c;
    const int nchunk = (np + 63) / 64;
    const lr_const_ptr<double> Whg = lr_as_const(A.Wh);
    for (int ch = 0; ch < nchunk; ++ch) {
        const int t = ch * 64 + lane;
        if (t < np) {
            for (int j = wave; j < c; j += NW) {
                double acc = 0.0;
#pragma unroll 4
                for (int i = 0; i < c; ++i) acc = fma(kx[i * lp + t], Whg[size_t(i) * c + j], acc);
                ft[j * lp + t] = acc;
            }
        }
    }
    __syncthreads();
    for (int ch = 0; ch < nchunk; ++ch) {
        const int t = ch * 64 + lane;
        if (t < tl) {
            for (int j = wave; j < c; j += NW) {
                const double f0 = ft[j * lp + t];
                u[j * lp + t] = A.difference ? ft[j * lp + t + 1] - f0 : f0;
            }
        }
    }
    __syncthreads();
}

// a tile's x -> xb, kxs -> kx, feat -> ft (may be xb), U -> u: `np` points at Xt, `tl` steps.  Ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void lr_tile_u(const LrTiledArgs& A, const double* Xt, int tl, int np, double* xb, double* kx, double* ft, double* u,
                                          int lane, int wave) {
    constexpr int NW = THREADS / 64;
    const int nchunk = (np + 63) / 64;
    lr_load_points<THREADS>(Xt, np, A.d, A.lp, xb);
    __syncthreads();
    lr_cross_base<NW>(A.kind, A.p0, A.p1, lr_as_const(A.S), A.c, A.d, xb, kx, A.lp, np, nchunk, lane, wave);
    __syncthreads();
    lr_tile_feat_u<THREADS>(A, tl, np, kx, ft, u, lane, wave);
}

// ---- the phases of the reverse body that depend on the family, overloaded on the argument block: here the families of base_eval, which
// evaluate kappa again wherever kxs is needed; SignatureSpectral's (lr_spectral_tiled_inst.hip) keep kxs of the sequence in the workgroup's
// scratch (lr_keeps_kxs: pass A then runs for M = 1 as well) and write dkxs instead of the base-kernel phase.
template <typename Args> struct lr_keeps_kxs { static constexpr bool value = false; };
// the gX rows of a ragged sequence's padded points (it has Lp points) are zeros
template <int THREADS>
__device__ __forceinline__ void lr_tile_zero_padded(const LrTiledArgs& A, int64_t n, int Lp) {
    lr_zero_padded_rows<THREADS>(A.gX + n * int64_t(A.L) * A.d, Lp, A.L, A.d);
}
// pass A, after lr_tile_u: nothing to keep
template <int THREADS>
__device__ __forceinline__ void lr_tile_keep_kxs(const LrTiledArgs&, const double*, double*, int, int, int) {}
// pass B: lr_tile_u again
template <int THREADS>
__device__ __forceinline__ void lr_tile_u_again(const LrTiledArgs& A, const double* Xt, int tl, int np, double* xb, double* kx, double* ft, double* u,
                                                int lane, int wave, const double*, int, int) {
    lr_tile_u<THREADS>(A, Xt, tl, np, xb, kx, ft, u, lane, wave);
}
// ... and x -> xb, kxs -> kb once more for the tile's tail.  Ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void lr_tile_kxs_again(const LrTiledArgs& A, lr_const_ptr<double> Sg, const double* Xt, int np, int pchunk, double* xb,
                                                  double* kb, const double*, int, int, int lane, int wave) {
    lr_load_points<THREADS>(Xt, np, A.d, A.lp, xb);
    __syncthreads();
    lr_cross_base<THREADS / 64>(A.kind, A.p0, A.p1, Sg, A.c, A.d, xb, kb, A.lp, np, pchunk, lane, wave);
    __syncthreads();
}

// e[t] <- run, run += e[t] over a tile's steps for the columns j < w of `src` (thread = column), starting from and leaving the carry;
// the exclusive sums go to `dst` (may be src) and, with `es`, to the scratch row of the column at es + j * es_stride
template <int THREADS>
__device__ __forceinline__ void lr_tile_excumsum(const double* src, double* dst, int w, int lp, int tl, double* carry, bool store, double* es,
                                                 int es_stride) {
    for (int j = threadIdx.x; j < w; j += THREADS) {
        double run = carry[j];
        const double* u = src + size_t(j) * lp;
        double* e = dst + size_t(j) * lp;
        double* s = es ? es + size_t(j) * es_stride : nullptr;
#pragma unroll 8
        for (int t = 0; t < tl; ++t) {
            const double v = u[t];
            if (store) e[t] = run;
            if (s) s[t] = run;
            run += v;
        }
        carry[j] = run;
    }
}

// (the bodies of the two kernels are texts of their own, lr_tiled_fwd_body.inc and lr_tiled_rev_body.inc: lr_ragged_inst.hip includes them
// again between the braces of its instances, whose argument block carries the per-sequence lengths)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_tiled_kernel(LrTiledArgs A) {
#include "lr_tiled_fwd_body.inc"
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void lr_seq_features_grad_tiled_kernel(LrTiledArgs A) {
#include "lr_tiled_rev_body.inc"
}

// ---- lr_ragged_inst.hip: the ragged instances of the three reverse / tiled kernels and their launchers (declared here, once, for lr_grad_api.hip;
// the whole-sequence forward form's: lr_fused_args.hpp).  The whole-sequence reverse pass at 512 threads (at 1024 the ragged instance would keep
// scratch memory); the tiled forms at the workgroup sizes of the existing instances (forward 1024, reverse 512).  Return the hipError_t of the launch.
int lr_ragged_grad_launch(hipStream_t stream, const LrGradRaggedArgs& A, unsigned grid, size_t lds);
int lr_ragged_tiled_launch(hipStream_t stream, const LrTiledRaggedArgs& A, unsigned grid, size_t lds);
int lr_ragged_grad_tiled_launch(hipStream_t stream, const LrTiledRaggedArgs& A, unsigned grid, size_t lds);

}  // namespace gpsig
