"""The device-side draw of the low-rank random objects (gpsig_lr_draw, csrc/lr_draw_kernels.hpp) against the host restatement of
tests/draw_reference.py: which landmarks, which jitter and which projection entries a 64-bit seed must produce -- exactly --, and the
eigendecomposition behind the whitening as a backward error.  gpsig_lr_draw is called through the library context with a fixed seed whose two
key words are both non-zero; what was drawn is read back with DeviceLowRankState.export().

(a) indices, gather and jitter: the landmarks are the scaled candidates at draw_reference.landmark_indices, in that order (1e-15 relative; whether
    they are bit-equal is printed), the jitter diagonal is bit-equal.  (b) 'sqrt' / 'log' projections: colptr, i1, i2 exact, |val - ref| <=
    1e-13 scale (the device's log, cos and sqrt are a few ulp, the cosine's argument is at most 2 pi and rounded once, the radius is below 8.7).
(c) 'lin' projections: everything exact.  (d) the eigendecomposition, with every point a landmark (N = 1, L = c) so that the test chooses W:
    R = max|W U - U diag(ev)| / max|ev|, O = max|U^T U - I| and E = max|ev - ev_ref| / max|ev_ref| (mpmath.eigsy at 40 digits), each at most
    B(n) = (30 (n - 1) + 16) 2^-52 -- one rounding per rotation step at the kernel's cap of 30 sweeps; 4.2e-13 at n = 64.  The bound comes from
    the algorithm.  Eigenvectors are not compared with LAPACK's: clustered eigenvalues make that meaningless.  (e) a NaN coordinate never gives
    a finite whitening.

What a run on an MI355X printed.  c = 63 and c = 64 -- 65,536 and 67,584 bytes of dynamic LDS plus the kernel's static arrays, asked for without
raising the kernel's dynamic-LDS attribute -- are launched and pass like every other size: the runtime accepts the launch, nothing had to change.
Landmarks: bit-equal in all eight draws.  Projection values: max|val - ref| / scale between 1.4e-16 and 6.4e-16 over the sixteen sparse projections.
The NaN case: no error, all 64 entries of the whitening NaN, 2 sweeps.  The one product change these tests asked for: the exported sweep count was
the index of the last sweep (0 for a matrix that is diagonal already, which is also rocSOLVER's 0); it now counts the sweeps taken.

The eigendecomposition, "device R O E sweeps | LAPACK (numpy.linalg.eigh on the same matrices) R O E"; B(n) is 3.6e-15, 1.0e-14, 1.7e-14 at
n = 1, 2, 3, 2.0e-13 .. 2.2e-13 at 31 .. 33 and 4.1e-13 .. 4.3e-13 at 62 .. 65.  The Jacobi kernel is at most 63 times LAPACK's figure (E at
rbf_walk, n = 64), mostly 3 to 10 times; rocSOLVER is level with LAPACK.
  rbf_walk   1  2.7e-17 2.3e-16 2.7e-17  1 | 2.7e-17 2.3e-16 2.7e-17      linear3    1  3.1e-17 1.7e-17 3.1e-17  1 | 3.1e-17 1.7e-17 3.1e-17
             2  9.5e-17 2.6e-16 5.9e-17  2 | 9.5e-17 2.6e-16 5.9e-17                 2  1.9e-16 3.1e-16 2.5e-16  2 | 4.8e-17 2.6e-16 4.4e-17
             3  1.3e-16 3.2e-16 7.5e-17  4 | 2.2e-16 2.5e-16 2.5e-16                 3  1.5e-16 2.2e-16 1.3e-16  5 | 1.7e-16 6.1e-16 1.3e-16
            31  8.5e-16 7.3e-15 2.3e-15 11 | 2.1e-16 2.0e-15 3.8e-16                31  7.6e-16 7.4e-15 1.9e-15  9 | 2.1e-16 1.4e-15 3.0e-16
            32  9.3e-16 7.1e-15 3.5e-15 11 | 2.0e-16 1.6e-15 9.6e-17                32  9.0e-16 7.8e-15 1.7e-15  9 | 3.1e-16 2.1e-15 1.5e-16
            33  6.2e-16 6.7e-15 2.2e-15 12 | 2.7e-16 1.6e-15 2.3e-16                33  1.0e-15 8.7e-15 2.2e-15 10 | 5.5e-16 3.2e-15 6.9e-16
            62  1.7e-15 1.6e-14 7.9e-15 14 | 2.3e-16 1.7e-15 3.3e-16                62  8.0e-16 1.3e-14 1.8e-15  9 | 7.7e-16 2.0e-15 6.2e-16
            63  2.0e-15 1.7e-14 9.8e-15 14 | 1.0e-16 2.8e-15 2.0e-16                63  1.5e-15 1.3e-14 3.0e-15  9 | 5.3e-16 1.3e-15 4.4e-16
            64  1.6e-15 1.4e-14 6.9e-15 12 | 1.4e-16 2.0e-15 1.1e-16                64  1.0e-15 1.3e-14 2.6e-15  9 | 3.4e-16 1.8e-15 2.7e-16
   rocSOLVER 65 2.2e-16 2.0e-15 2.2e-16  0 | 3.2e-16 1.8e-15 5.3e-16      rocSOLVER 65  4.1e-16 1.3e-15 2.2e-16  0 | 2.6e-16 1.8e-15 1.4e-16
   rocSOLVER 33 2.1e-16 1.4e-15 3.5e-16  0 | (as 33 above)                rocSOLVER 33  1.6e-16 1.7e-15 1.9e-16  0 | (as 33 above)
  rbf_twice  1  2.7e-17 2.3e-16 2.7e-17  1 | 2.7e-17 2.3e-16 2.7e-17      rbf_far: 2.7e-17 2.3e-16 2.7e-17 at n = 1, 3.7e-17 2.6e-16 3.7e-17 at 2 and 3,
             2  1.0e-16 1.9e-16 1.3e-16  2 | 1.0e-16 4.3e-16 1.3e-16      1.0e-16 .. 1.1e-16 3.5e-16 1.1e-16 from 31 on (the distance of the longdouble
             3  3.5e-16 3.2e-16 3.6e-16  4 | 1.5e-16 3.7e-16 1.6e-16      reference's 1 + jd from the double's), one sweep; the same figures on the
            31  7.6e-16 7.5e-15 2.5e-15 13 | 4.2e-16 2.6e-15 3.4e-16      rocSOLVER route and from LAPACK; eigenvalues bit-equal to sort(1 + jd) on all
            32  6.4e-16 8.3e-15 1.8e-15 13 | 2.5e-16 2.5e-15 4.9e-16      three.
            33  5.7e-16 8.3e-15 1.6e-15 12 | 1.8e-16 3.2e-15 2.3e-16
            62  1.3e-15 1.7e-14 5.9e-15 15 | 4.7e-16 2.1e-15 5.7e-16
            63  1.4e-15 1.7e-14 6.9e-15 14 | 4.6e-16 1.8e-15 4.0e-16
            64  9.4e-16 1.6e-14 4.4e-15 14 | 1.4e-16 1.7e-15 1.3e-16
   rocSOLVER 65 5.1e-16 2.1e-15 3.3e-16  0 | 1.7e-16 2.1e-15 1.9e-16
   rocSOLVER 33 1.7e-16 2.1e-15 2.5e-16  0 | (as 33 above)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import draw_reference as D

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SEED = 0x9E3779B97F4A7C15          # both key words non-zero (the public draw_low_rank seeds from 63 bits: the top bit is set here)
JITTER = 1e-6                      # gpsig_amd.kernels.JITTER
JACOBI_MAX = 64                    # LR_JACOBI_MAX: the one-workgroup Jacobi kernel up to here, rocSOLVER beyond


def context():
    from gpsig_amd import _lib
    return _lib.context(0, torch.cuda.current_stream(DEV).cuda_stream)


def make(base, d, M, c, r, sparsity, lengthscales=None):
    from gpsig_amd import kernels as K
    cls = {"rbf": K.SignatureRBF, "linear": K.SignatureLinear}[base]
    return cls(d, d, M, lengthscales=lengthscales, low_rank=True, num_components=c, rank_bound=r, sparsity=sparsity)


def draw(kern, X=None, X2=None, Z=None, increments=False, seed=SEED):
    """gpsig_lr_draw with a given seed (kernels.SignatureKernel._draw_low_rank_on_device takes its seed from the kernel object's generator):
    X (N, L, d), X2 (N2, L2, d), Z (lt, T, [2,] d) NumPy arrays -> the exported host state, with .jacobi_sweeps"""
    from gpsig_amd import kernels as K
    dev = [None if a is None else torch.tensor(a, device=DEV) for a in (X, X2, Z)]
    L_ = K._launch_lr(kern, *dev)
    p = kern._params(L_.keep, L_.dtype_id)
    n1, l1 = X.shape[:2] if X is not None else (0, 1)
    n2, l2 = X2.shape[:2] if X2 is not None else (0, 1)
    st = K.DeviceLowRankState(L_.ctx, kern.num_components, kern.rank_bound, kern.num_levels - 1)
    L_.ctx.call("gpsig_lr_draw", p, int(kern.num_components), int(kern.rank_bound), K.DeviceLowRankState.SPARSITY[kern.sparsity], C.c_uint64(seed),
                L_.inp(dev[0]), n1, l1, L_.inp(dev[1]), n2, l2, L_.inp(dev[2]), Z.shape[1] if Z is not None else 0, int(bool(increments)),
                C.byref(st._h))
    try:
        h = st.export()
        h.jacobi_sweeps = st.jacobi_sweeps
    finally:
        st.close()
    return h


# ---- (a) indices, gather and jitter ---------------------------------------------------------------------------------------------------------------
def check_landmarks(h, cand, c, tag):
    idx = D.landmark_indices(cand.shape[0], c, SEED)
    want = cand[idx]
    assert h.landmarks.shape == want.shape
    print("draw-edges landmarks", *tag, "bit-equal" if np.array_equal(h.landmarks, want) else "max rel %.1e" % np.abs(h.landmarks / want - 1).max())
    assert (np.abs(h.landmarks - want) <= 1e-15 * np.abs(want)).all()
    assert np.array_equal(h.jitter_diag, D.jitter_diag(c, SEED, JITTER))
    return idx


@pytest.mark.parametrize("total,c", [("c", 5), ("c+1", 5), (200, 7), (200, 64), (200, 65), (200, 130)])
def test_landmarks_and_jitter(total, c):
    """distinct random points; (c, c): every point in order; 130 of 200: the membership loop goes beyond one lane stride (and the
    eigendecomposition to rocSOLVER)"""
    rng = np.random.default_rng(300 + c)
    d = 3
    N, L = (1, c) if total == "c" else (1, c + 1) if total == "c+1" else (8, 25)
    X = rng.standard_normal((N, L, d))
    ls = 0.6 + rng.random(d)
    h = draw(make("rbf", d, 2, c, 3, "sqrt", lengthscales=ls), X=X)
    idx = check_landmarks(h, X.reshape(-1, d) / ls, c, (total, c))
    if total == "c":
        assert idx == list(range(c))
    assert np.isfinite(h.whitening).all() and h.whitening.shape == (c, c)
    assert (h.jacobi_sweeps >= 1) == (c <= JACOBI_MAX)


def test_landmarks_from_tensors_and_both_tables():
    """Z (with increments), X and X2 all present and every candidate a landmark: the order is Z, X, X2 (the boundaries ztot and n1 l1)"""
    rng = np.random.default_rng(31)
    d, M, T = 3, 2, 2
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d))
    X, X2 = rng.standard_normal((2, 3, d)), rng.standard_normal((1, 4, d))
    ls = 0.6 + rng.random(d)
    cand = np.concatenate([Z.reshape(-1, d), X.reshape(-1, d), X2.reshape(-1, d)]) / ls
    c = cand.shape[0]
    assert c == 12 + 6 + 4
    h = draw(make("rbf", d, M, c, 3, "sqrt", lengthscales=ls), X=X, X2=X2, Z=Z, increments=True)
    assert check_landmarks(h, cand, c, ("Z+X+X2", c)) == list(range(c))
    # ... and one short of all of them: a boundary inside each of the three ranges may be the one left out
    h = draw(make("rbf", d, M, c - 1, 3, "sqrt", lengthscales=ls), X=X, X2=X2, Z=Z, increments=True)
    check_landmarks(h, cand, c - 1, ("Z+X+X2", c - 1))


# ---- (b), (c) projections -------------------------------------------------------------------------------------------------------------------------
def projections(c, r, M, sparsity):
    X = np.random.default_rng(c + r).standard_normal((1, c + 2, 2))
    h = draw(make("rbf", 2, M, c, r, sparsity), X=X)
    assert len(h.sketches) == M - 1
    k2 = c
    for i, sk in enumerate(h.sketches):
        assert (sk.k1, sk.k2, sk.r) == (c, k2, r)
        yield i, sk, c * k2
        k2 = r


@pytest.mark.parametrize("sparsity", ["sqrt", "log"])
@pytest.mark.parametrize("c,r,M", [(5, 3, 2), (8, 8, 3), (9, 70, 3), (12, 130, 2)])
def test_sparse_projections(sparsity, c, r, M):
    """(5, 3, 2): D = 25, one short pass.  (8, 8, 3): D = 64, exactly one pass, twice.  (9, 70, 3): D = 81, a short second pass, and D = 630;
    r > 64 is a second pass of lr_colptr_kernel carrying its base.  (12, 130, 2): three colptr passes, the last with two columns.
    'log': 1 / s comes from the host's log on both sides; an entry could differ only if a 53-bit uniform fell into an ulp of it."""
    for i, sk, Dk in projections(c, r, M, sparsity):
        colptr, i1, i2, val, scale = D.sparse_projection(Dk, r, c, i, sparsity, SEED)
        assert np.array_equal(sk.colptr, colptr), (i, "colptr")
        assert np.array_equal(sk.i1, i1) and np.array_equal(sk.i2, i2), (i, "rows")
        err = float(np.abs(sk.val - val).max() / scale) if len(val) else 0.0
        print("draw-edges sparse", sparsity, (c, r, M), "projection", i, "entries", len(val), "max|val - ref| / scale %.1e" % err)
        assert len(val) > 0 and err <= 1e-13, (i, err)


@pytest.mark.parametrize("c,r,M", [(3, 9, 3), (9, 70, 2), (70, 100, 2)])
def test_lin_projections(c, r, M):
    """(3, 9, 3): r == D at level 2 -- every coordinate pair, Floyd from j = 0.  r > 64: the membership loop beyond one lane stride."""
    for i, sk, Dk in projections(c, r, M, "lin"):
        colptr, i1, i2, val = D.lin_projection(Dk, r, c, i, SEED)
        assert np.array_equal(sk.colptr, colptr) and np.array_equal(sk.i1, i1) and np.array_equal(sk.i2, i2) and np.array_equal(sk.val, val), i
        if r == Dk:
            assert sorted(sk.i1 + c * sk.i2) == list(range(Dk))


# ---- (d) the eigendecomposition -------------------------------------------------------------------------------------------------------------------
def eigen_case(family, n, route):
    base, X = D.eigen_family(family, n)
    ctx = context()
    ctx.set_option("lr_jacobi", 1 if route == "jacobi" else 0)
    try:
        h = draw(make(base, 3, 2, n, 1, "sqrt"), X=X[None])
    finally:
        ctx.set_option("lr_jacobi", 1)
    assert np.array_equal(h.landmarks, X)                                 # no lengthscales: the points themselves, in order
    jd = D.jitter_diag(n, SEED, JITTER)
    assert np.array_equal(h.jitter_diag, jd)
    got = D.whitening_checks(X, jd, h.whitening, h.eigenvalues, JITTER, base)
    print("draw-edges eigen", family, n, route, "R %.1e O %.1e E %.1e sweeps %d" % (got["R"], got["O"], got["E"], h.jacobi_sweeps))
    assert got["finite"] and got["ascending"] and got["signs"], got
    assert max(got["R"], got["O"], got["E"]) <= D.bound(n), (got, D.bound(n))
    if route == "jacobi" and n <= JACOBI_MAX:
        assert 1 <= h.jacobi_sweeps < 30
    else:
        assert h.jacobi_sweeps == 0
    return h, jd


ROUTES = [(n, "jacobi") for n in D.EIGEN_SIZES if n <= JACOBI_MAX] + [(65, "rocsolver"), (33, "rocsolver")]


@pytest.mark.parametrize("n,route", ROUTES)
@pytest.mark.parametrize("family", ["rbf_walk", "linear3", "rbf_twice"])
def test_eigendecomposition_backward_error(family, n, route):
    """n in 1, 2, 3, 31 .. 33, 62 .. 64 through the Jacobi kernel (odd n: a bye in every step; 64: every item slot of the kernel taken, and
    with 63 the launches of more than 64 KB of LDS); 65, and 33 under lr_jacobi = 0, through rocSOLVER"""
    eigen_case(family, n, route)


@pytest.mark.parametrize("n,route", ROUTES)
def test_eigendecomposition_of_a_diagonal_gram(n, route):
    """points 60 lengthscales apart: W = diag(1 + jd) exactly, so the eigenvalues are those numbers sorted and the eigenvectors a permutation;
    the Jacobi kernel sees it in its first sweep"""
    h, jd = eigen_case("rbf_far", n, route)
    assert np.array_equal(h.eigenvalues, np.sort(1.0 + jd))
    P = h.whitening * np.sqrt(h.eigenvalues + JITTER)[None, :]
    assert ((h.whitening != 0).sum(0) == 1).all() and ((h.whitening != 0).sum(1) == 1).all() and (h.whitening >= 0).all()
    assert np.abs(P[h.whitening != 0] - 1).max() <= 4 * 2.0 ** -52
    assert np.array_equal(np.argmax(h.whitening, axis=0), np.argsort(1.0 + jd, kind="stable"))
    if route == "jacobi":
        assert h.jacobi_sweeps == 1


# ---- (e) a non-finite landmark --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["rbf", "linear"])
def test_a_nan_coordinate_never_gives_a_finite_whitening(base):
    """n = 8, one NaN coordinate: an error from gpsig_lr_state_sizes or a non-finite whitening.  (The convergence test of the Jacobi kernel
    takes its maxima with fmax, which drops NaNs: the iteration 'converges', and the NaNs must arrive through the eigenvalues.)"""
    X = np.random.default_rng(8).standard_normal((1, 8, 3))
    X[0, 5, 1] = np.nan
    try:
        h = draw(make(base, 3, 2, 8, 1, "sqrt"), X=X)
    except RuntimeError as e:
        print("draw-edges nan", base, "refused:", e)
        return
    print("draw-edges nan", base, "finite entries of the whitening:", int(np.isfinite(h.whitening).sum()), "of 64; sweeps", h.jacobi_sweeps)
    assert not np.isfinite(h.whitening).all()
