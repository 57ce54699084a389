"""tests/draw_reference.py on its own, without the product: the generator against the published known-answer vectors of Philox-4x32-10
(Random123's kat_vectors), the properties every draw must have, and the condition under which tests/test_gpu_draw_edges.py may hold the
device's eigendecomposition to draw_reference.bound(n): LAPACK's own decomposition of the same matrices, put through the same
whitening_checks, stays under it."""
import numpy as np
import pytest

import draw_reference as D

SEED = 0x9E3779B97F4A7C15          # both key words non-zero
JITTER = 1e-6


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    assert tuple(int(w) for w in D.philox4x32_words(counter, key)) == want
    # ... vectorised: the same words at every position of an array of counters
    got = D.philox4x32_words(tuple(np.full(5, c, dtype=np.uint64) for c in counter), key)
    assert all((g == w).all() and g.shape == (5,) for g, w in zip(got, want))


def test_counter_and_key_layout():
    """philox4x32(index, stream, seed) is the round above on counter {index lo, index hi, stream, 0} and key {seed lo, seed hi}"""
    index, stream = 0x85a308d3243f6a88, 0x13198a2e
    got = D.philox4x32(index, stream, 0x299f31d0a4093822)
    want = D.philox4x32_words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0), (0xa4093822, 0x299f31d0))
    assert all(int(g) == int(w) for g, w in zip(got, want))
    a = D.philox4x32(np.array([index, 7], dtype=np.uint64), stream, 0x299f31d0a4093822)
    assert all(int(x[0]) == int(w) for x, w in zip(a, want)) and int(a[0][1]) != int(a[0][0])


def test_uniforms():
    w = D.philox4x32(np.arange(20000, dtype=np.uint64), 2, SEED)
    u = D.u01(w[0], w[1])
    assert u.dtype == np.float64 and (u > 0).all() and (u < 1).all()
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * u.size)
    assert D.u01(0, 0) == 2.0 ** -54                                    # the smallest value
    assert D.u01(0xffffffff, 0xffffffbf) == 1.0 - 2.0 ** -52            # the largest below 1: 2^53 - 2 and a half, rounded to even
    assert D.u01(0xffffffff, 0xffffffff) == 1.0                         # all 53 bits set: the one pair in 2^53 that reaches the end point
    assert D.u01(1 << 31, 0) == 0.5                                     # 2^52 + 0.5 rounds to 2^52: the half is gone from here on
    assert D.below(0xffffffff, 0xffffffff, 10) == 9 and D.below(0, 0, 10) == 0 and D.below(1 << 31, 0, 7) == 3
    assert D.below(0xffffffff, 0xffffffff, 2 ** 63 - 1) == 2 ** 63 - 2


@pytest.mark.parametrize("total,c", [(1, 1), (7, 7), (8, 7), (200, 7), (200, 64), (200, 65), (200, 130), (2 ** 40, 50)])
def test_floyd_subsets(total, c):
    idx = D.landmark_indices(total, c, SEED)
    assert len(idx) == c and len(set(idx)) == c and idx == sorted(idx) and 0 <= idx[0] and idx[-1] < total
    if total == c:
        assert idx == list(range(c))
    assert idx == D.landmark_indices(total, c, SEED)
    if total > c + 1:
        assert idx != D.landmark_indices(total, c, SEED + 1) and idx != D.landmark_indices(total, c, SEED + (1 << 32))


def test_floyd_is_uniform():
    """every 2-subset of 5 equally often: 10 cells, 4,000 seeds, chi-square with 9 degrees of freedom (below 33.7 with probability 1 - 1e-4)"""
    counts = {}
    for seed in range(4000):
        key = tuple(D.landmark_indices(5, 2, seed))
        counts[key] = counts.get(key, 0) + 1
    assert len(counts) == 10
    assert sum((v - 400) ** 2 / 400 for v in counts.values()) < 33.7


def test_jitter_diagonal():
    jd = D.jitter_diag(130, SEED, JITTER)
    assert jd.shape == (130,) and (jd > 0).all() and (jd < JITTER).all() and len(set(jd)) == 130
    assert np.array_equal(jd[:9], D.jitter_diag(9, SEED, JITTER))


@pytest.mark.parametrize("sparsity", ["sqrt", "log"])
@pytest.mark.parametrize("D_,r,k1", [(25, 3, 5), (64, 8, 8), (81, 70, 9), (630, 70, 9), (144, 130, 12), (1, 1, 1)])
def test_sparse_projection_is_well_formed(sparsity, D_, r, k1):
    colptr, i1, i2, val, scale = D.sparse_projection(D_, r, k1, 1, sparsity, SEED)
    assert colptr.shape == (r + 1,) and colptr[0] == 0 and (np.diff(colptr) >= 0).all() and colptr[-1] == len(val) == len(i1) == len(i2)
    rows = i1.astype(np.int64) + k1 * i2
    assert (i1 >= 0).all() and (i1 < k1).all() and (rows < D_).all()
    for j in range(r):
        assert (np.diff(rows[colptr[j]:colptr[j + 1]]) > 0).all()
    inv_s, scale2 = D.sparse_scales(D_, r, sparsity)
    assert scale == scale2 and np.isfinite(val).all()
    if D_ == 1 and sparsity == "sqrt":
        assert len(val) == r                                             # s = 1: every entry present
    elif D_ > 1:
        n, p = D_ * r, inv_s
        assert abs(len(val) - n * p) <= 6 * np.sqrt(n * p * (1 - p)) and (np.abs(val) <= 8.7 * scale).all()
    # another projection number is another stream
    other = D.sparse_projection(D_, r, k1, 0, sparsity, SEED)
    assert D_ * r < 1000 or not np.array_equal(other[0], colptr)


def test_sparse_values_are_standard_normal():
    colptr, i1, i2, val, scale = D.sparse_projection(630, 70, 9, 0, "sqrt", SEED)
    v = val / scale
    assert len(v) > 1500 and abs(v.mean()) < 5 / np.sqrt(len(v)) and abs(v.var() - 1) < 0.15 and abs((np.abs(v) < 1).mean() - 0.6827) < 0.05


@pytest.mark.parametrize("D_,r,k1", [(9, 9, 3), (81, 70, 9), (4900, 100, 70), (7000, 100, 70)])
def test_lin_projection_is_well_formed(D_, r, k1):
    colptr, i1, i2, val = D.lin_projection(D_, r, k1, 0, SEED)
    assert np.array_equal(colptr, np.arange(r + 1)) and set(val) == {1.0, -1.0} and len(val) == r
    rows = i1.astype(np.int64) + k1 * i2
    assert len(set(rows)) == r and rows.min() >= 0 and rows.max() < D_ and (i1 < k1).all()
    if r == D_:
        assert sorted(rows) == list(range(D_))


def lapack_whitening(W):
    """numpy.linalg.eigh's decomposition of W (float64), with the sign convention and the whitening of the product"""
    ev, U = np.linalg.eigh(W)
    first = np.argmax(np.abs(U), axis=0)                                # (the first of the largest)
    U = U * np.where(U[first, np.arange(U.shape[0])] < 0, -1.0, 1.0)[None, :]
    return U / np.sqrt(ev + JITTER)[None, :], ev


@pytest.mark.parametrize("n", D.EIGEN_SIZES)
@pytest.mark.parametrize("family", D.EIGEN_FAMILIES)
def test_reference_solver_stays_under_the_bound(family, n):
    """whitening_checks on LAPACK's decomposition: R, O and E under B(n) on every matrix the device is judged on"""
    base, X = D.eigen_family(family, n)
    jd = D.jitter_diag(n, SEED, JITTER)
    Wh, ev = lapack_whitening(np.asarray(D.landmark_gram(X, jd, base), dtype=np.float64))
    got = D.whitening_checks(X, jd, Wh, ev, JITTER, base)
    print("draw-reference lapack", family, n, "R %.1e O %.1e E %.1e" % (got["R"], got["O"], got["E"]))
    assert got["ascending"] and got["signs"] and got["finite"]
    assert max(got["R"], got["O"], got["E"]) <= D.bound(n), got
    if family == "rbf_far":
        assert np.array_equal(ev, np.sort(1.0 + jd))


def test_whitening_checks_notice_a_poor_decomposition():
    """a decomposition that lost half its digits, a swapped pair of eigenvalues and a flipped column are each reported"""
    n = 33
    base, X = D.eigen_family("rbf_walk", n)
    jd = D.jitter_diag(n, SEED, JITTER)
    Wh, ev = lapack_whitening(np.asarray(D.landmark_gram(X, jd, base), dtype=np.float64))
    rot = np.eye(n)
    c, s = np.cos(1e-8), np.sin(1e-8)
    rot[np.ix_([n - 2, n - 1], [n - 2, n - 1])] = [[c, -s], [s, c]]
    U = (Wh * np.sqrt(ev + JITTER)) @ rot
    got = D.whitening_checks(X, jd, U / np.sqrt(ev + JITTER), ev, JITTER, base)
    assert got["R"] > D.bound(n) and got["O"] <= D.bound(n)
    got = D.whitening_checks(X, jd, Wh * (1 + 1e-9), ev, JITTER, base)
    assert got["O"] > D.bound(n)
    ev2 = ev.copy()
    ev2[-1] *= 1 + 1e-10
    got = D.whitening_checks(X, jd, Wh, ev2, JITTER, base)
    assert got["E"] > D.bound(n)
    got = D.whitening_checks(X, jd, Wh[:, ::-1], ev[::-1], JITTER, base)
    assert not got["ascending"] and got["R"] <= D.bound(n)
    flipped = Wh.copy()
    flipped[:, 5] *= -1
    got = D.whitening_checks(X, jd, flipped, ev, JITTER, base)
    assert not got["signs"] and got["R"] <= D.bound(n)
