"""The diagonal tiles of SignatureLinear's symmetric Gram as a feature contraction (csrc/sig_feat_kernel.hpp): sig_gram_diag_tile computes
only the 36 16 x 16 blocks (block row <= block column) of a 128 x 128 tile with bi == bj, from one slab, and sig_gram_reduce_sym_kernel
mirrors such a tile at 16-row granularity without reading a partial sum that was not written.

The GPU cases hold the one-call Gram bit for bit to the same Gram reassembled from owned row blocks: those go through whole, non-symmetric
tiles (sig_gram_dma_kernel's main loop) with the same depth pieces, so every entry of a diagonal tile and every mirrored entry is compared
with what the whole-tile loop computes.  The host-side tests restate the (wave, block) ownership and the reduce kernel's read rule in NumPy."""
import ctypes as C

import numpy as np
import pytest

BM, BK = 128, 16          # SG_BM == SG_BN, SG_BK
TOL = 1e-6                # test_gpu_parity.py: against the oracle; 1e-10 between the two GPU routes


def relerr(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all()
    scale = np.abs(want).max()
    return float((np.abs(got - want) / (np.abs(want) + 1e-6 * scale + 1e-300)).max())


# ---- host side: the mapping ---------------------------------------------------------------------------------------------------------------

def wave_blocks(w):
    """the (block row, block column) pairs wave w of sig_gram_diag_tile accumulates and stores"""
    return [(w, c) for c in range(w, 8)] + [(7 - w, c) for c in range(7 - w, 8)]


def planned_pieces(N, d, M):
    """sig_feat_api.hip, sig_features_K (the model: sig_piece_counts of sig_pieces.hpp): the depth pieces of a symmetric N x N Gram below the sizes where the graded tail applies (> 512 workgroups)"""
    F = sum(d ** m for m in range(1, M + 1))
    nslab = ((F + 1 + 15) // 16 * 16 + BK - 1) // BK
    nt = (N + BM - 1) // BM
    tiles, result_bytes = nt * (nt + 1) // 2, 8.0 * N * N * 0.5
    best, nsplit = 1e300, 1
    ns = 1
    while ns <= 128 and ns * 8 <= nslab + 7:
        wgs, per = float(tiles * ns), nslab / ns
        t = (per * 1.8e-6 + 10e-6 if wgs <= 256.0 else np.ceil(wgs / 512.0) * (per * 3.6e-6 + 10e-6)) + (2.0 * ns * result_bytes / 3e12 if ns > 1 else 0.0)
        if t < best * 0.999:
            best, nsplit = t, ns
        ns += 1
    assert tiles * nsplit <= 512          # (no graded tail: the count above is the number of pieces)
    return nslab, nsplit


def test_every_upper_block_has_one_owner():
    owners = {}
    for w in range(4):
        blocks = wave_blocks(w)
        assert len(blocks) == 9 and len(set(blocks)) == 9
        # the fragments the wave reads (block rows w .. 7) cover both operands of each of its blocks
        assert all(w <= r <= 7 and w <= c <= 7 for r, c in blocks)
        for b in blocks:
            assert b not in owners, (b, w, owners[b])
            owners[b] = w
    assert set(owners) == {(r, c) for r in range(8) for c in range(r, 8)} and len(owners) == 36


def tile_of(t, nt):
    """sig_tile_of for a symmetric product of nt tile rows: place t of the tile sequence -> (bi, bj)"""
    ntiles = nt * (nt + 1) // 2
    d = t * nt // ntiles
    if (t + 1) * nt // ntiles > d:
        return d, d
    t -= d
    nb = (nt + 7) // 8
    for Bi in range(nb):
        hi = min(8, nt - 8 * Bi)
        for Bj in range(Bi, nb):
            wj = min(8, nt - 8 * Bj)
            cnt = hi * (hi - 1) // 2 if Bj == Bi else hi * wj
            if t < cnt:
                if Bj == Bi:
                    li, rowlen = 0, hi - 1
                    while t >= rowlen:
                        t, li, rowlen = t - rowlen, li + 1, rowlen - 1
                    return 8 * Bi + li, 8 * Bj + li + 1 + t
                return 8 * Bi + t // wj, 8 * Bj + t % wj
            t -= cnt
    raise AssertionError("no tile")


@pytest.mark.parametrize("nt", [1, 2, 3, 8, 9, 17, 32, 40])
def test_tile_sequence_is_the_upper_triangle_with_the_diagonal_dealt_evenly(nt):
    ntiles = nt * (nt + 1) // 2
    tiles = [tile_of(t, nt) for t in range(ntiles)]
    assert sorted(tiles) == [(i, j) for i in range(nt) for j in range(i, nt)]
    # an XCD works on a contiguous eighth of the sequence: the diagonal (cheaper) tiles in it are an eighth of all, to within one
    for x in range(8):
        lo, hi = ntiles * x // 8, ntiles * (x + 1) // 8
        n = sum(i == j for i, j in tiles[lo:hi])
        assert abs(n - nt * (hi - lo) / ntiles) <= 1, (x, n)
    if nt == 32:
        assert all(sum(i == j for i, j in tiles[66 * x:66 * x + 66]) == 4 for x in range(8))


def _written(NA):
    """partial-sum entries the contraction stores for a symmetric NA x NA product: whole tiles above the diagonal, owned blocks on it"""
    nt = (NA + BM - 1) // BM
    W = np.zeros((NA, NA), dtype=bool)
    for bi in range(nt):
        for bj in range(bi, nt):
            if bi < bj:
                W[bi * BM:(bi + 1) * BM, bj * BM:(bj + 1) * BM] = True
            else:
                for w in range(4):
                    for r, c in wave_blocks(w):
                        W[bi * BM + 16 * r:bi * BM + 16 * r + 16, bi * BM + 16 * c:bi * BM + 16 * c + 16] = True      # (slices clip at NA)
    return W


def _reduce(NA):
    """sig_gram_reduce_sym_kernel thread by thread: which partial sums it reads, how often it writes each output entry"""
    nt = (NA + BM - 1) // BM
    reads, writes = np.zeros((NA, NA), dtype=bool), np.zeros((NA, NA), dtype=int)
    for bi in range(nt):
        for bj in range(bi, nt):
            for sbi in range(4):
                for sbj in range(4):
                    if bi == bj and sbi > sbj:
                        continue
                    dblock = bi == bj and sbi == sbj
                    i0, j0 = bi * BM + 32 * sbi, bj * BM + 32 * sbj
                    for r in range(32):               # the summing pass
                        for x in range(32):
                            i, j = i0 + r, j0 + x
                            if i < NA and j < NA and (not dblock or (r >> 4) <= (x >> 4)):
                                reads[i, j] = True
                                writes[i, j] += 1
                    for r in range(32):               # the mirror pass: out[j0 + r][i0 + x] = tile[x][r]
                        for x in range(32):
                            i, j = i0 + x, j0 + r
                            if i < NA and j < NA and (not dblock or (r >> 4) > (x >> 4)):
                                assert reads[i, j], "the mirror pass takes an entry that was not summed"
                                writes[j, i] += 1
    return reads, writes


@pytest.mark.parametrize("NA", [128, 129, 200])
def test_reduce_reads_only_what_was_written(NA):
    written = _written(NA)
    reads, writes = _reduce(NA)
    assert not (reads & ~written).any()
    assert (writes == 1).all()            # every entry of the Gram is written, by one thread


def test_a_listed_shape_has_more_than_one_depth_piece():
    assert planned_pieces(257, 3, 3) == (3, 1)
    for N in (128, 129, 200, 257):
        assert planned_pieces(N, 8, 3) == (37, 5)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------

def _ctx():
    import torch
    from gpsig_amd import _lib
    return _lib.context(0, torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)


def _inputs(seed, N, L, d, M):
    import torch
    from gpsig_amd import kernels
    rng = np.random.default_rng(seed)
    Xh = np.cumsum(0.4 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    kw = dict(lengthscales=0.7 + rng.random(d), variances=0.5 + rng.random(M + 1))
    kern = kernels.SignatureLinear(L * d, d, M, **kw)
    kern.sigma = 1.3
    kern.test_kw = kw
    return Xh, torch.as_tensor(Xh, device="cuda:0"), kern


def _gram_on(ctx, kern, X, N, L):
    """K(X) through the C ABI on a given context (device pointers)"""
    import torch
    from gpsig_amd import _lib
    ctx.set_pointer_mode(_lib.PTR_DEVICE)
    keep = []
    p = kern._params(keep)
    out = torch.full((N, N), float("nan"), dtype=torch.float64, device="cuda:0")
    ctx.call("gpsig_kernel_K", p, C.c_void_p(X.data_ptr()), None, N, N, L, L, 0, C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("d,M", [(3, 3), (8, 3)])
@pytest.mark.parametrize("N", [128, 129, 200, 257])
def test_one_call_gram_equals_the_row_blocks_bit_for_bit(N, d, M):
    """K(X) of the one-call symmetric route (diagonal tiles: upper blocks only, mirrored by the reduce) against the owned row blocks of a
    3-rank partition (whole non-symmetric tiles, the same depth pieces), symmetrised: torch.equal.  N = 128: one diagonal tile; 129: a
    second one a single row wide and one tile above the diagonal; 200: the edge inside a 16-block and a 32-block; 257: three tile rows.
    (d, M) = (3, 3) is 3 slabs in one piece; (8, 3) is 37 slabs, which the planner cuts into FIVE depth pieces at every one of these N
    (test_a_listed_shape_has_more_than_one_depth_piece restates its model; test_stale_partial_sums... observes the partial-sum buffer)."""
    import torch
    from gpsig_amd import _lib, parallel
    L = 12
    _, X, kern = _inputs(1000 * N + d, N, L, d, M)
    ctx = _ctx()
    try:
        ctx.set_option("sig_features", 1)
        ctx.set_option("sig_gemm_dma", 1)
        full = kern.K(X)
        ctx.set_pointer_mode(_lib.PTR_DEVICE)
        b = parallel.row_partition(N, 3)
        half = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
        keep = []
        p = kern._params(keep)
        for r in range(3):
            ctx.call("gpsig_kernel_K_symm_rows", p, C.c_void_p(X.data_ptr()), N, L, b[r], b[r + 1], C.c_void_p(half[b[r]:b[r + 1]].data_ptr()))
        out = torch.empty_like(half)
        ctx.check(ctx._lib.gpsig_symmetrize_owned_rows(ctx._h, _lib.F64, C.c_void_p(half.data_ptr()), N, C.c_void_p(out.data_ptr())))
        torch.cuda.synchronize()
    finally:
        ctx.set_option("sig_features", -1)
        ctx.set_option("sig_gemm_dma", 1)
    assert bool(torch.isfinite(full).all())
    assert torch.equal(out, full)


@pytest.mark.gpu
def test_stale_partial_sums_are_not_read():
    """N = 300 first, then N = 129 on the same context: the partial-sum buffer holds the larger Gram's values where the diagonal tiles of the
    smaller one store nothing.  Bit-identical to a fresh context's result, exactly symmetric, the normalised diagonal exactly
    sum_m sigma variances[m].  (d, M) = (8, 3): five depth pieces -- the fresh context's scratch is larger than features + ONE partial sum."""
    import torch
    from gpsig_amd import _lib
    L, d, M = 12, 8, 3
    _, Xbig, kern = _inputs(300, 300, L, d, M)
    N = 129
    X = Xbig[:N].contiguous()
    stream = torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream
    used, fresh = _lib.Context(0, stream), _lib.Context(0, stream)
    try:
        for c in (used, fresh):
            c.set_option("sig_features", 1)
        big = _gram_on(used, kern, Xbig, 300, L)
        assert bool(torch.isfinite(big).all())
        got = _gram_on(used, kern, X, N, L)
        want = _gram_on(fresh, kern, X, N, L)
        ld = (sum(d ** m for m in range(1, M + 1)) + 1 + 15) // 16 * 16
        one_piece = (9 * (8 * ld * N + 64)) // 8 + 256 + (9 * (8 * N * N + 64)) // 8 + 256 + 65536      # ctx.hpp: ensure() + the small buffers
        assert fresh.scratch_bytes() > one_piece, (fresh.scratch_bytes(), one_piece)
    finally:
        for c in (used, fresh):
            c.set_option("sig_features", -1)
            c.close()
    assert torch.equal(got, want)
    assert torch.equal(got, got.T)
    assert torch.equal(torch.diagonal(got).cpu(), torch.full((N,), float(np.sum(kern.sigma * kern.test_kw["variances"])), dtype=torch.float64))
    assert torch.equal(big, big.T)


@pytest.mark.gpu
def test_diagonal_tiles_against_the_pair_recursion_and_the_oracle():
    """N = 129 (a whole diagonal tile, a one-row one, one tile above the diagonal) against the pair recursion (sig_features 0) and the CPU
    oracle, at the tolerances of test_linear_gram_as_feature_contraction."""
    from oracle import sigkern_oracle as O
    N, L, d, M = 129, 12, 3, 3
    Xh, X, kern = _inputs(7, N, L, d, M)
    ko = O.SignatureKernelOracle(L * d, d, M, base="linear", **kern.test_kw)
    ko.sigma = kern.sigma
    ctx = _ctx()
    got = {}
    try:
        for route in (1, 0):
            ctx.set_option("sig_features", route)
            got[route] = kern.K(X).cpu().numpy()
    finally:
        ctx.set_option("sig_features", -1)
    want = ko.K(Xh)
    assert relerr(got[1], want) <= TOL and relerr(got[1], got[0]) <= 1e-10, (relerr(got[1], want), relerr(got[1], got[0]))
