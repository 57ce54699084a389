// wide_ragged_kernel.hpp -- the BLOCK-DIAGONAL argument lattices of a ragged batch on the wide route (wide_ragged_api.hip): for every sequence n of a
// chunk, with its own len[n] rows of the packed augmented tables XL (left form) and XR (right form) -- wide_kernels.hpp --,
//     arg_n = XL_n XR_n^T      len[n] x len[n], row-major with row stride len[n], at  arg + doff[n] - doff[n0]
// (off[n]: the sequence's first packed row, doff[n]: the cells of the lattices before it -- ragged_plan.hpp).  This is what the level diagonals (Kdiag,
// the normalisation factors, Kxx of the covariances) sweep; rocBLAS has no batched product of matrices of different sizes, and one product of all
// rows with all rows would compute N times the cells.
//
// The (d + 2)-deep contraction runs on the float64 matrix cores (v_mfma_f64_16x16x4_f64) in the tiling of wide_spectral_kernel.hpp: a workgroup of
// four wavefronts owns 64 rows x 64 columns of one sequence's lattice, a wavefront 16 rows against four 16-column accumulator tiles; both operand
// tiles are staged in LDS per 32 columns of the contraction, the row stride of 34 doubles keeps the operand reads of a half wavefront on distinct
// banks.  Rows and columns beyond len[n] and features beyond d + 2 are zeros in the operands and are never written.  Every entry is one accumulation
// chain over the features from column 0, in its own workgroup: no sum across workgroups, no atomics -- the same bits however the host chunks the batch.
#pragma once

#include <hip/hip_runtime.h>

namespace gpsig {

constexpr int WIDE_RG_KC = 32;                       // columns of the contraction per LDS tile
constexpr int WIDE_RG_LD = WIDE_RG_KC + 2;           // its row stride
constexpr int WIDE_RG_TILE = 64;                     // rows and columns of a lattice per workgroup
constexpr int WIDE_RG_THREADS = 256;

struct WideRaggedDiagArgs {
    const double* XL;       // packed left-form rows (all sequences), DA doubles each
    const double* XR;       // packed right-form rows
    double* arg;            // the chunk's lattices
    const int32_t* len;     // (N)
    const int64_t* off;     // (N + 1) packed rows before each sequence
    const int64_t* doff;    // (N + 1) lattice cells before each sequence
    int64_t n0, Nc;         // this launch: sequences n0 .. n0 + Nc - 1
    int32_t DA;
};

typedef double wide_rg_f64x4 __attribute__((ext_vector_type(4)));

// grid: (column blocks of the longest sequence, its row blocks, sequences of the chunk (grid-stride)); a workgroup whose tile lies beyond its sequence's
// extent has nothing to do (workgroup-uniform: the barriers below are reached by all four wavefronts or by none).
// The matrix core's operand layout: lane l gives row l & 15 at column 4 k + (l >> 4) of the step; its accumulator register g is the entry
// (row (l >> 4) + 4 g, column l & 15).
__global__ __launch_bounds__(WIDE_RG_THREADS) void wide_ragged_diag_args_kernel(const WideRaggedDiagArgs S) {
    __shared__ double at[WIDE_RG_TILE * WIDE_RG_LD];
    __shared__ double bt[WIDE_RG_TILE * WIDE_RG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = lane & 15, kq = lane >> 4;
    const int DA = S.DA;
    const int lk = tid & (WIDE_RG_KC - 1), lr = tid / WIDE_RG_KC;          // this thread's column and first row of a tile load (8 rows per pass)
    const int col0 = int(blockIdx.x) * WIDE_RG_TILE, row0 = int(blockIdx.y) * WIDE_RG_TILE;
    for (int64_t nl = blockIdx.z; nl < S.Nc; nl += gridDim.z) {
        const int64_t n = S.n0 + nl;
        const int ln = S.len[n];
        if (row0 >= ln || col0 >= ln) continue;
        const double* __restrict__ A = S.XL + S.off[n] * DA;
        const double* __restrict__ B = S.XR + S.off[n] * DA;
        double* __restrict__ Cn = S.arg + (S.doff[n] - S.doff[S.n0]);
        wide_rg_f64x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = wide_rg_f64x4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < DA; k0 += WIDE_RG_KC) {
            __syncthreads();                        // (the previous tiles' readers are done)
            const int f = k0 + lk;
#pragma unroll
            for (int rr = 0; rr < WIDE_RG_TILE; rr += WIDE_RG_THREADS / WIDE_RG_KC) {
                const int r = rr + lr;
                const int ar = row0 + r, bc = col0 + r;
                at[r * WIDE_RG_LD + lk] = (ar < ln && f < DA) ? A[int64_t(ar) * DA + f] : 0.0;
                bt[r * WIDE_RG_LD + lk] = (bc < ln && f < DA) ? B[int64_t(bc) * DA + f] : 0.0;
            }
            __syncthreads();
            const int steps = (DA - k0 < WIDE_RG_KC ? DA - k0 + 3 : WIDE_RG_KC) / 4;
            for (int kk = 0; kk < steps; ++kk) {
                const int k = kk * 4 + kq;
                const double a = at[(wave * 16 + m) * WIDE_RG_LD + k];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double bv = bt[(j * 16 + m) * WIDE_RG_LD + k];
                    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc[j], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = row0 + wave * 16 + kq + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = col0 + j * 16 + m;
                if (row < ln && col < ln) Cn[int64_t(row) * ln + col] = acc[j][g];
            }
        }
    }
}

}  // namespace gpsig
