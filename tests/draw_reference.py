"""A host restatement of the device-side low-rank draw (gpsig_lr_draw, csrc/lr_draw_kernels.hpp), plain NumPy and Python integers: which
landmarks, which jitter and which projection entries a seed must produce, and how good an eigendecomposition the whitening came from.  No HIP
and nothing from the library; the landmark Gram's closed forms are those of tests/cross_reference.py.  tests/test_draw_reference.py pins it on
the CPU (the published known-answer vectors of Philox-4x32-10 among them); tests/test_gpu_draw_edges.py holds the device to it.

The generator is Philox-4x32-10 (Salmon et al., SC11) with counter {index lo, index hi, stream, 0} and key {seed lo, seed hi}: the value of
stream s at index i is a function of (seed, s, i) alone.  Streams: 1 landmark indices, 2 the jitter diagonal, 16 + k presence and radius of
projection k's entries, 32 + k their angle, 48 + k the coordinate pairs of a 'lin' projection."""
import functools
import math

import numpy as np

import cross_reference as R

LD = np.longdouble
U64 = np.uint64
MASK = U64(0xFFFFFFFF)
MUL0, MUL1 = U64(0xD2511F53), U64(0xCD9E8D57)
BUMP0, BUMP1 = 0x9E3779B9, 0xBB67AE85
S32 = U64(32)
STREAM_LANDMARKS, STREAM_JITTER, STREAM_PRESENT, STREAM_VALUE, STREAM_LIN = 1, 2, 16, 32, 48


def philox4x32_words(counter, key):
    """Philox-4x32-10 on counter words (c0, c1, c2, c3) -- integers or integer arrays of one shape -- and key words (k0, k1): four uint64 arrays
    holding the 32-bit output words"""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=U64) & MASK for c in counter))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = MUL0 * c0, MUL1 * c2                       # 32 x 32 -> 64 bits: no wrap
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ U64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ U64(k1), p0 & MASK
        k0, k1 = (k0 + BUMP0) & 0xFFFFFFFF, (k1 + BUMP1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox4x32(index, stream, seed):
    """the four words of stream ``stream`` at ``index`` (an integer or an array of them, below 2^64) under the 64-bit ``seed``"""
    index = np.asarray(index, dtype=U64)
    seed = int(seed)
    return philox4x32_words((index & MASK, index >> S32, U64(stream), U64(0)), (seed & 0xFFFFFFFF, seed >> 32))


def u01(a, b):
    """53 random bits -> a double in (0, 1): ((a >> 5) << 26 | b >> 6) + 0.5, times 2^-53.  Both steps in float64, as on the device; beyond
    2^52 the half is rounded away, to even (so the one word pair with all 53 bits set gives 1.0 itself)."""
    m = ((np.asarray(a, dtype=U64) >> U64(5)) << U64(26)) | (np.asarray(b, dtype=U64) >> U64(6))
    return (m.astype(np.float64) + 0.5) * 2.0 ** -53


def below(a, b, n):
    """a uniform integer in [0, n): the high 64 bits of (a << 32 | b) n, in Python integers"""
    return (((int(a) << 32) | int(b)) * int(n)) >> 64


def _floyd(lo, hi, stream, seed):
    """Floyd's subset algorithm for j = lo .. hi - 1: t = below(j + 1), j itself where t was drawn before.  Draw order, and the words."""
    js = np.arange(lo, hi, dtype=U64)
    w = philox4x32(js, stream, seed)
    out = []
    for i, j in enumerate(range(lo, hi)):
        t = below(w[0][i], w[1][i], j + 1)
        out.append(j if t in out else t)
    return out, w


def landmark_indices(total, c, seed):
    """c distinct indices out of ``total``, ascending"""
    return sorted(_floyd(total - c, total, STREAM_LANDMARKS, seed)[0])


def jitter_diag(c, seed, jitter):
    w = philox4x32(np.arange(c, dtype=U64), STREAM_JITTER, seed)
    return jitter * u01(w[0], w[1])


def sparse_scales(D, r, sparsity):
    """(inv_s, scale) of a 'sqrt' / 'log' projection of D rows and r columns"""
    if sparsity == "sqrt":
        s = math.sqrt(float(D))
    elif sparsity == "log":
        s = float(D) / math.log(float(D)) if D > 1 else math.inf
    else:
        raise ValueError(sparsity)
    return (1.0, math.sqrt(1.0 / r)) if s < 1.0 else (1.0 / s, math.sqrt(s / r))


def sparse_projection(D, r, k1, sk, sparsity, seed):
    """projection ``sk`` (0 for level 2) of D = k1 k2 rows and r columns -> (colptr, i1, i2, val, scale): by column, rows ascending"""
    inv_s, scale = sparse_scales(D, r, sparsity)
    ctr = (np.arange(r, dtype=U64)[:, None] * U64(D) + np.arange(D, dtype=U64)[None, :]).reshape(-1)      # col * D + row
    w = philox4x32(ctr, STREAM_PRESENT + sk, seed)
    present = u01(w[0], w[1]) < inv_s
    counts = present.reshape(r, D).sum(1)
    colptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    at = np.flatnonzero(present)                                                                          # column-major, rows ascending
    row = at % D
    v = philox4x32(ctr[at], STREAM_VALUE + sk, seed)
    u1, u2 = u01(w[2][at], w[3][at]).astype(LD), u01(v[0], v[1])
    angle = (2.0 * math.pi * u2).astype(LD)                                                               # rounded once, as the kernel's
    val = np.sqrt(-2 * np.log(u1)) * np.cos(angle) * LD(scale)
    return colptr, (row % k1).astype(np.int32), (row // k1).astype(np.int32), val.astype(np.float64), scale


def lin_projection(D, r, k1, sk, seed):
    """'lin': r distinct coordinate pairs out of D in draw order, one per column, with Rademacher signs -> (colptr, i1, i2, val)"""
    rows, w = _floyd(D - r, D, STREAM_LIN + sk, seed)
    rows = np.asarray(rows, dtype=np.int64)
    val = np.where((w[2] & U64(1)) != 0, 1.0, -1.0)
    return np.arange(r + 1, dtype=np.int32), (rows % k1).astype(np.int32), (rows // k1).astype(np.int32), val


def bound(n):
    """B(n) = (30 (n - 1) + 16) 2^-52: one rounding per rotation step of a cyclic Jacobi iteration at its cap of 30 sweeps of n - 1 steps, and
    16 for what surrounds it (the Gram's entries, the root and the division of the whitening)"""
    return (30 * (n - 1) + 16) * 2.0 ** -52


def landmark_gram(S, jd, base):
    """W = kappa(S, S) + diag(jd) in longdouble"""
    W = R.cross(base, S, S)
    return W + np.diag(np.asarray(jd, dtype=LD))


@functools.lru_cache(maxsize=None)
def _eigsy_cached(n, raw):
    import mpmath
    W = np.frombuffer(raw, dtype=LD).reshape(n, n)
    hi = W.astype(np.float64)
    lo = (W - hi.astype(LD)).astype(np.float64)
    with mpmath.workdps(40):
        A = mpmath.matrix(n, n)
        for i in range(n):
            for j in range(n):
                A[i, j] = mpmath.mpf(float(hi[i, j])) + mpmath.mpf(float(lo[i, j]))
        ev = mpmath.eigsy(A, eigvals_only=True)
        ev = sorted(ev[i] for i in range(n))
        return tuple(LD(float(e)) + LD(float(e - mpmath.mpf(float(e)))) for e in ev)


def reference_eigenvalues(W):
    """the eigenvalues of a symmetric longdouble matrix by mpmath.eigsy at 40 digits, ascending, as longdouble (one computation per matrix)"""
    W = np.ascontiguousarray(W, dtype=LD)
    return np.array(_eigsy_cached(W.shape[0], W.tobytes()), dtype=LD)


EIGEN_FAMILIES = ("rbf_walk", "linear3", "rbf_far", "rbf_twice")
EIGEN_SIZES = (1, 2, 3, 31, 32, 33, 62, 63, 64, 65)


def eigen_family(family, n):
    """(base, points (n, 3)) of the landmark Grams the eigendecomposition is judged on.  rbf_walk: a random walk, the spectrum decays to the
    jitter.  linear3: rank 3 plus the jitter, n - 3 eigenvalues cluster below 1e-6, off-diagonal entries of both signs.  rbf_far: points 60
    lengthscales apart on integer coordinates -- every off-diagonal entry underflows to 0, every diagonal entry is exp(0).  rbf_twice: a
    random walk with every point stored twice (the last once when n is odd)."""
    rng = np.random.default_rng(1000 + n)
    if family == "rbf_walk":
        return "rbf", np.cumsum(0.3 * rng.standard_normal((n, 3)), axis=0)
    if family == "linear3":
        return "linear", rng.standard_normal((n, 3))
    if family == "rbf_far":
        X = np.zeros((n, 3))
        X[:, 0] = 60.0 * rng.permutation(n)
        return "rbf", X
    if family == "rbf_twice":
        return "rbf", np.repeat(np.cumsum(0.3 * rng.standard_normal(((n + 1) // 2, 3)), axis=0), 2, axis=0)[:n]
    raise ValueError(family)


SIGN_TIE = 8 * 2.0 ** -52


def whitening_checks(S, jd, Wh, ev, jitter, base):
    """How good an eigendecomposition of W = kappa(S, S) + diag(jd) the whitening Wh[i][j] = U[i][j] / sqrt(ev[j] + jitter) came from:
        R = max|W U - U diag(ev)| / max|ev|, O = max|U^T U - I|, E = max|ev - ev_ref| / max|ev_ref| (mpmath at 40 digits),
    whether ev ascends, and whether every column of U has its largest component positive.  Where several components of a column lie within
    8 ulp of the largest (the 45 degree vectors of a repeated point), which of them is 'the first largest' is decided by roundings the
    whitening's root and division have covered: one of them being positive is what can be asked."""
    W = landmark_gram(S, jd, base)
    ev = np.asarray(ev, dtype=np.float64)
    evl = ev.astype(LD)
    U = np.asarray(Wh, dtype=LD) * np.sqrt(evl + LD(jitter))[None, :]
    n = W.shape[0]
    ref = reference_eigenvalues(W)
    A = np.abs(U)
    near = A >= A.max(0)[None, :] * (1 - LD(SIGN_TIE))
    return dict(R=float(np.abs(W @ U - U * evl[None, :]).max() / np.abs(evl).max()),
                O=float(np.abs(U.T @ U - np.eye(n, dtype=LD)).max()),
                E=float(np.abs(evl - ref).max() / np.abs(ref).max()),
                ascending=bool((np.diff(ev) >= 0).all()),
                signs=bool((near & (U > 0)).any(0).all()),
                finite=bool(np.isfinite(np.asarray(Wh, dtype=np.float64)).all() and np.isfinite(ev).all()))
