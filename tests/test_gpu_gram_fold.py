"""The in-kernel fold of SignatureLinear's one-call symmetric Gram (csrc/sig_feat_kernel.hpp: sig_gram_fold): the workgroup of
sig_gram_dma_kernel that finishes the last depth piece of a tile adds the tile's pieces itself -- in index order, from zero, as
sig_gram_reduce_sym_kernel does -- and writes the tile and its mirror image.  The order of the launch (sig_tile_of: groups of consecutive tiles,
piece-major inside a group; one group as built) decides only who that is.

Every GPU case goes through the C ABI on contexts that have served nothing else and holds the default call
  * bit for bit to the same call under sig_gemm_dma = 0 (the staging kernel and the reduce kernel),
  * bit for bit to the Gram reassembled from the owned row blocks of a 3-rank partition (whole tiles, the reduce kernel),
  * to the float64 oracle on sampled sub-blocks, 1e-10.
The host-side tests restate sig_tile_of and the piece model (sig_pieces.hpp) in NumPy."""
import ctypes as C

import numpy as np
import pytest

BM, BK = 128, 16          # SG_BM == SG_BN, SG_BK
GROUPS = 1                # SG_FOLD_GROUPS: the groups of tiles a folding launch is issued in (the restatement below is checked for 2, 4, 8 too)


def relmax(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---- host side: the piece model and the order of the items ---------------------------------------------------------------------------------

def nslab_of(d, M):
    F = sum(d ** m for m in range(1, M + 1))
    return ((F + 1 + 15) // 16 * 16 + BK - 1) // BK


def piece_counts(N, nslab):
    """sig_piece_counts of sig_pieces.hpp for a symmetric N x N Gram, option sig_graded on: (equal pieces, graded)"""
    nt = (N + BM - 1) // BM
    tiles, result_bytes = nt * (nt + 1) // 2, 8.0 * N * N * 0.5
    best, nsplit, ns = 1e300, 1, 1
    while ns <= 128 and ns * 8 <= nslab + 7:
        wgs, per = float(tiles * ns), nslab / ns
        t = (per * 1.8e-6 + 10e-6 if wgs <= 256.0 else np.ceil(wgs / 512.0) * (per * 3.6e-6 + 10e-6)) + (2.0 * ns * result_bytes / 3e12 if ns > 1 else 0.0)
        if t < best * 0.999:
            best, nsplit = t, ns
        ns += 1
    if tiles > 1024 and nsplit < 4 and nslab >= 32:
        nsplit = 4
    graded = 1
    wgs, piece_t = float(tiles * nsplit), nslab / nsplit * 3.6e-6
    if wgs > 512.0 and nslab // nsplit >= 32:
        rounds = wgs / 512.0
        best_t = (np.ceil(rounds) - rounds) * piece_t
        for g in range(2, 6):
            t = piece_t / float(1 << (g - 1)) + (g - 1) * 2.0 * result_bytes / 3e12
            if t < best_t * 0.95 and (nslab // nsplit) >> (g - 1) >= 8:
                best_t, graded = t, g
    return nsplit, graded


def piece_bounds(nslab, equal, graded):
    """sig_piece_bounds: the slab ranges; their number is the launch's pieces"""
    equal = max(1, equal)
    if equal > nslab:
        equal = max(1, nslab)
    bound = [nslab * s // equal for s in range(equal - 1)]
    last0 = nslab * (equal - 1) // equal
    bound.append(last0)
    if graded > 1 and nslab - last0 >= 2 * graded:
        at, left = last0, nslab - last0
        for _ in range(1, graded):
            take = max(left // 2, 1)
            at, left = at + take, left - take
            bound.append(at)
    return bound + [nslab]


def pieces_of(N, d, M):
    ns, gr = piece_counts(N, nslab_of(d, M))
    return len(piece_bounds(nslab_of(d, M), ns, gr)) - 1


def place_to_tile(t, ntiles, nti, ntj, symmetric):
    """sig_tile_of, second half: place t of the tile sequence -> (bi, bj)"""
    if symmetric:
        d = t * ntj // ntiles
        if (t + 1) * ntj // ntiles > d:
            return d, d
        t -= d
    nbi, nbj = (nti + 7) // 8, (ntj + 7) // 8
    for Bi in range(nbi):
        hi = min(8, nti - 8 * Bi)
        for Bj in range(Bi if symmetric else 0, nbj):
            wj = min(8, ntj - 8 * Bj)
            cnt = hi * (hi - 1) // 2 if (symmetric and Bj == Bi) else hi * wj
            if t < cnt:
                if symmetric and Bj == Bi:
                    li, rowlen = 0, hi - 1
                    while t >= rowlen:
                        t, li, rowlen = t - rowlen, li + 1, rowlen - 1
                    return 8 * Bi + li, 8 * Bj + li + 1 + t
                return 8 * Bi + t // wj, 8 * Bj + t % wj
            t -= cnt
    raise AssertionError("no tile")


def item_of(b, ntiles, pieces, groups):
    """sig_tile_of, first half: workgroup b of the launch -> (piece, place in the tile sequence)"""
    t0, t1 = 0, ntiles
    if groups > 1:
        g = 0
        for gg in range(1, groups):
            if (ntiles * gg // groups) * pieces <= b:
                g = gg
        t0, t1 = ntiles * g // groups, ntiles * (g + 1) // groups
    ng, base = t1 - t0, t0 * pieces
    assert ng > 0
    split = (b - base) // ng
    j = b - base - split * ng
    off = (base + split * ng) & 7
    x = (off + j) & 7
    start = 0
    for xp in range(x):
        j0 = (xp - off + 8) & 7
        start += (ng - 1 - j0) // 8 + 1 if j0 < ng else 0
    return split, t0 + start + ((j - ((x - off + 8) & 7)) >> 3)


@pytest.mark.parametrize("pieces", [1, 3, 14])
@pytest.mark.parametrize("ntiles", [1, 6, 36, 528, 529])
@pytest.mark.parametrize("groups", [GROUPS, 2, 4, 8])
def test_every_item_is_issued_once(ntiles, pieces, groups):
    """Triangular counts are symmetric launches (1, 3, 8 and 32 tile rows); 529 is a general 23 x 23 grid."""
    nt = int((np.sqrt(8 * ntiles + 1) - 1) / 2)
    symmetric = nt * (nt + 1) // 2 == ntiles
    nti = ntj = nt if symmetric else 23
    assert ntiles == (nt * (nt + 1) // 2 if symmetric else nti * ntj)
    items, last_of_group = [], []
    for b in range(ntiles * pieces):
        split, t = item_of(b, ntiles, pieces, groups)
        assert 0 <= split < pieces and 0 <= t < ntiles
        bi, bj = place_to_tile(t, ntiles, nti, ntj, symmetric)
        assert 0 <= bi < nti and 0 <= bj < ntj and (not symmetric or bi <= bj)
        items.append((split, bi, bj))
        if split == pieces - 1:
            last_of_group.append(b)
    want = [(s, i, j) for s in range(pieces) for i in range(nti) for j in range(i if symmetric else 0, ntj)]
    assert sorted(items) == want
    # the tiles finish group after group: the last pieces of all but the last group are issued before that group begins
    if groups > 1 and ntiles >= groups:
        before = sum(1 for b in last_of_group if b < (ntiles * (groups - 1) // groups) * pieces)
        assert before == ntiles * (groups - 1) // groups


def test_the_listed_shapes_have_the_pieces_they_are_listed_for():
    """What sig_piece_counts gives the shapes of the GPU cases below.  (The model cuts even a single tile of 22 slabs into 3 pieces -- few
    workgroups, most of the chip idle -- and leaves 528 tiles of 22 slabs whole: the one-piece path is met at d = 3, M = 3 and at N = 4,096.)"""
    assert nslab_of(3, 3) == 3 and nslab_of(4, 4) == 22 and nslab_of(5, 4) == 49 and nslab_of(8, 3) == 37 and nslab_of(4, 5) == 86
    assert [pieces_of(N, 3, 3) for N in (1, 17, 128, 129)] == [1, 1, 1, 1]      # one piece: the workgroup is the last by construction, no counter
    assert [pieces_of(N, 4, 4) for N in (1, 17, 128, 129, 300)] == [3, 3, 3, 3, 3]
    assert pieces_of(300, 5, 4) == 7 and pieces_of(300, 8, 3) == 5              # deeper splits
    assert pieces_of(4096, 4, 4) == 1                                           # 528 tiles on 512 workgroup slots, one piece each
    assert piece_counts(4096, nslab_of(4, 5)) == (2, 2) and pieces_of(4096, 4, 5) == 3      # 528 tiles x 3 pieces, the last two graded
    assert piece_bounds(86, 2, 2) == [0, 43, 64, 86]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------

def _fresh(**options):
    """a context that has served nothing else, on the current stream"""
    import torch
    from gpsig_amd import _lib
    ctx = _lib.Context(0, torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
    ctx.set_option("sig_features", 1)
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.set_pointer_mode(_lib.PTR_DEVICE)
    return ctx


def _case(seed, N, L, d, M, cls="SignatureLinear", normalization=True):
    from gpsig_amd import kernels
    rng = np.random.default_rng(seed)
    Xh = np.cumsum(0.4 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    kw = dict(lengthscales=0.7 + rng.random(d), variances=0.5 + rng.random(M + 1), normalization=normalization)
    kern = getattr(kernels, cls)(L * d, d, M, **kw)
    kern.sigma = 1.3
    return Xh, kern, kw


def _oracle(kern, kw, L, d, M, cls):
    from oracle import sigkern_oracle as O
    ko = O.SignatureKernelOracle(L * d, d, M, base="cosine" if cls == "SignatureCosine" else "linear", **kw)
    ko.sigma = kern.sigma
    return ko


def _gram(ctx, kern, X, N, L):
    """K(X) through the C ABI (device pointers); float32 sequences give a float32 Gram"""
    import torch
    from gpsig_amd import _lib
    keep = []
    p = kern._params(keep, _lib.F32 if X.dtype == torch.float32 else _lib.F64)
    out = torch.full((N, N), float("nan"), dtype=X.dtype, device="cuda:0")
    ctx.call("gpsig_kernel_K", p, C.c_void_p(X.data_ptr()), None, N, N, L, L, 0, C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    return out


def _from_row_blocks(ctx, kern, X, N, L):
    """the owned row blocks of a 3-rank partition, symmetrised"""
    import torch
    from gpsig_amd import _lib, parallel
    b = parallel.row_partition(N, 3)
    half = torch.zeros((N, N), dtype=torch.float64, device="cuda:0")
    keep = []
    p = kern._params(keep)
    for r in range(3):
        if b[r + 1] > b[r]:
            ctx.call("gpsig_kernel_K_symm_rows", p, C.c_void_p(X.data_ptr()), N, L, b[r], b[r + 1], C.c_void_p(half[b[r]:b[r + 1]].data_ptr()))
    out = torch.empty_like(half)
    ctx.check(ctx._lib.gpsig_symmetrize_owned_rows(ctx._h, _lib.F64, C.c_void_p(half.data_ptr()), N, C.c_void_p(out.data_ptr())))
    torch.cuda.synchronize()
    return out


def _sampled_against_the_oracle(got, ko, Xh, N, seed, tol=1e-10):
    """A cross block of the oracle is a cross Gram: where a sequence meets itself there it holds K / (K + jitter), the symmetric Gram's diagonal
    the level weights exactly (kernels.py:430-433) -- such entries are left to the symmetric block, which is the oracle's symmetric Gram."""
    rng = np.random.default_rng(seed)
    k = min(6, N)
    for I, J in ((np.arange(k), np.arange(N - k, N)), (rng.choice(N, min(5, N), replace=False), rng.choice(N, min(7, N), replace=False)),
                 (np.arange(k), np.arange(k))):
        same = len(I) == len(J) and bool((I == J).all())
        want = ko.K(Xh[I]) if same else ko.K(Xh[I], Xh[J])
        sub = got[np.ix_(I, J)]
        if not same:
            sub = np.where(I[:, None] == J[None, :], want, sub)
        err = relmax(sub, want)
        assert err < tol, (err, I, J)


def _three_ways(N, L, d, M, cls="SignatureLinear", normalization=True, rows=True):
    import torch
    Xh, kern, kw = _case(7000 + 31 * N + d, N, L, d, M, cls, normalization)
    X = torch.as_tensor(Xh, device="cuda:0")
    ctxs = [_fresh(), _fresh(sig_gemm_dma=0), _fresh()]
    try:
        got = _gram(ctxs[0], kern, X, N, L)
        staged = _gram(ctxs[1], kern, X, N, L)
        blocks = _from_row_blocks(ctxs[2], kern, X, N, L) if rows else None
    finally:
        for c in ctxs:
            c.close()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, staged)
    if rows:
        assert torch.equal(got, blocks)
    assert torch.equal(got, got.T)
    if normalization:
        assert torch.equal(torch.diagonal(got).cpu(), torch.full((N,), float(np.sum(kern.sigma * kw["variances"])), dtype=torch.float64))
    _sampled_against_the_oracle(got.cpu().numpy(), _oracle(kern, kw, L, d, M, cls), Xh, N, N)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 17, 128, 129, 300])
def test_fold_three_ways(N):
    """d = 4, M = 4, L = 6 (22 slabs, 3 pieces at each N).  N = 1, 17, 128: one diagonal tile; 129: 2 x 2 tiles, the second tile row one row
    high; 300: 6 upper tiles, 3 of them diagonal, the last tile row 44 rows high."""
    _three_ways(N, 6, 4, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 17, 128, 129])
def test_fold_of_a_single_piece(N):
    """d = 3, M = 3 (3 slabs): one piece, no counter -- the workgroup adds its own partial tile to zero and writes the tile and its mirror"""
    _three_ways(N, 6, 3, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("d,M", [(5, 4), (8, 3)])
def test_fold_deeper_splits(d, M):
    """49 and 37 slabs at N = 300: more pieces per tile than the 22-slab cases have"""
    _three_ways(300, 6, d, M)


@pytest.mark.gpu
def test_fold_raw_diagonal():
    """normalization off: the diagonal is summed like every other entry (diag_set 0)"""
    _three_ways(300, 6, 4, 4, normalization=False)


@pytest.mark.gpu
def test_fold_cosine():
    _three_ways(300, 6, 4, 4, cls="SignatureCosine")


@pytest.mark.gpu
def test_fold_float32_call():
    """float32 sequences: widened, contracted and folded in float64, narrowed.  Row blocks are float64 only on this route; the oracle gets
    the same float32 values widened, and the result is its float64 Gram rounded once (2^-24 relative) on top of the 1e-10 of the others."""
    import torch
    N, L, d, M = 300, 6, 4, 4
    Xh, kern, kw = _case(32, N, L, d, M)
    X = torch.as_tensor(Xh.astype(np.float32), device="cuda:0")
    ctxs = [_fresh(), _fresh(sig_gemm_dma=0)]
    try:
        got = _gram(ctxs[0], kern, X, N, L)
        staged = _gram(ctxs[1], kern, X, N, L)
    finally:
        for c in ctxs:
            c.close()
    assert got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert torch.equal(got, staged) and torch.equal(got, got.T)
    _sampled_against_the_oracle(got.cpu().numpy(), _oracle(kern, kw, L, d, M, "SignatureLinear"), Xh.astype(np.float32).astype(np.float64), N, 32,
                                tol=1e-10 + 2.0 ** -24)


@pytest.mark.gpu
@pytest.mark.parametrize("d,M", [(4, 4), (4, 5)])
def test_fold_more_items_than_workgroup_slots(d, M):
    """N = 4096, L = 6.  d = 4, M = 5: 528 tiles x 3 pieces (the last two graded) = 1,584 workgroups on 512 slots -- every group of the order, a
    tile's pieces on different XCDs, folds under other workgroups' multiplies.  d = 4, M = 4: 528 tiles of one piece.  The whole matrix
    against the staging and reduce kernels."""
    import torch
    N, L = 4096, 6
    Xh, kern, kw = _case(4096 + M, N, L, d, M)
    X = torch.as_tensor(Xh, device="cuda:0")
    ctxs = [_fresh(), _fresh(sig_gemm_dma=0), _fresh()]
    try:
        got = _gram(ctxs[0], kern, X, N, L)
        again = _gram(ctxs[0], kern, X, N, L)
        staged = _gram(ctxs[1], kern, X, N, L)
        blocks = _from_row_blocks(ctxs[2], kern, X, N, L)
    finally:
        for c in ctxs:
            c.close()
    assert torch.equal(got, staged) and torch.equal(again, staged)
    assert torch.equal(got, blocks)
    assert torch.equal(got, got.T)
    _sampled_against_the_oracle(got.cpu().numpy(), _oracle(kern, kw, L, d, M, "SignatureLinear"), Xh, N, 4096)


@pytest.mark.gpu
def test_fold_with_a_warm_consumer():
    """K(X1), K(X2), K(X1) back to back on one context: the partial sums of the three calls live at the same addresses, so a workgroup that
    folds without an acquire (or with too narrow a one) can find the previous call's lines in its CU's cache."""
    import torch
    N, L, d, M = 300, 6, 4, 4
    Xh1, kern, _ = _case(1, N, L, d, M)
    Xh2 = _case(2, N, L, d, M)[0]
    X1, X2 = torch.as_tensor(Xh1, device="cuda:0"), torch.as_tensor(Xh2, device="cuda:0")
    fold, staged = _fresh(), _fresh(sig_gemm_dma=0)
    try:
        want = [_gram(staged, kern, X, N, L) for X in (X1, X2)]
        import gpsig_amd._lib as _lib
        keep = []
        p = kern._params(keep)
        outs = [torch.full((N, N), float("nan"), dtype=torch.float64, device="cuda:0") for _ in range(3)]
        for out, X in zip(outs, (X1, X2, X1)):                      # no synchronisation in between
            fold.call("gpsig_kernel_K", p, C.c_void_p(X.data_ptr()), None, N, N, L, L, 0, C.c_void_p(out.data_ptr()))
        torch.cuda.synchronize()
    finally:
        fold.close()
        staged.close()
    assert not torch.equal(want[0], want[1])
    assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1]) and torch.equal(outs[2], want[0])


@pytest.mark.gpu
@pytest.mark.parametrize("N,L,d,M", [(300, 6, 4, 4), (400, 64, 8, 3)])
def test_fold_in_a_recorded_graph(N, L, d, M):
    """kern.graphed("K", X): the recording holds no memset of the counters -- every tile's last arriver leaves its counter zero, and the
    warm-up call has run.  6 tiles x 3 pieces and 10 tiles x 5 pieces (the shape of test_gpu_graph.py's replay test, where a recorded
    memset node left the replays without a last arriver).  Two replays on new contents, each equal to the eager call on a fresh context."""
    import torch
    Xh, kern, _ = _case(11, N, L, d, M)
    X = torch.as_tensor(Xh, device="cuda:0")
    g = kern.graphed("K", X)
    eager = _fresh()
    try:
        for seed in (12, 13):
            Xn = torch.as_tensor(_case(seed, N, L, d, M)[0], device="cuda:0")
            X.copy_(Xn)
            got = g.replay().clone()
            torch.cuda.synchronize()
            want = _gram(eager, kern, Xn, N, L)
            assert torch.equal(got, want), seed
    finally:
        g.close()
        eager.close()
