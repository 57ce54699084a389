"""Ragged batches in exact mode (``kern.exact_ragged``; csrc/wide_ragged_api.hip) on the GPU: ``lengths=`` / ``lengths2=`` on K, Kdiag, K_tens_vs_seq,
K_tens_n_seq_covs and K_seq_n_seq_covs of an exact kernel object, inducing_variables.Kuu_Kuf_Kff and models.SVGP.predict_f through them.

Sequence n is X[n, :len_n], evaluated as that truncated sequence would be on its own.  `want` is
  * oracle/sigkern_oracle.py on the truncated sequences, one sequence or one pair at a time, and separately
  * the dense entry point on X[n:n+1, :len_n] under context option wide = 1.
Error: max|got - want| / max|want|, level by level where levels are returned.  Bounds: tests/test_gpu_wide.py's for values -- 1e-10 against the oracle,
1e-7 for Matern-1/2 wherever a sequence meets itself (its line 156: kappa(x, x) is 1e-8 from one in the reference's own arithmetic); the same two bounds
against the dense entry point.  SVGP.predict_f: 1e-6, the bound of tests/test_gpu_parity.py::test_svgp_predict_and_kl (a Cholesky solve amplifies the
covariances' error).  Every case runs with NaN in all padded rows and again with zeros there: identical bits.  Host- and device-pointer calls return
identical bits.  With difference=True and no lags the ragged result agrees with the dense call on the table padded by repetition, to the same bounds.

Measured maxima (MI355X, one run of this module with -s): against the oracle Kzx 2.3e-14, Kdiag 8.9e-15, normalised Kzx on the diagonals' tables
2.4e-14, K symmetric 2.8e-15, K cross 1.2e-14, the surface with lags 9.1e-15 (K) ... 8.8e-14 (K_seq_n_seq_covs), Kuu_Kuf_Kff 1.6e-15; Matern-1/2 where a
sequence meets itself 3.8e-8 (Kzx normalised), 4.2e-8 (Kdiag), 4.1e-8 (K symmetric) -- the oracle's own error there: against the dense entry point the same
cases are at 2.7e-15 or below.  Against the dense entry point one sequence / pair at a time: 1.5e-14 at most (0 in most cases); against the dense call
on the table padded by repetition 9.8e-15 at most.  predict_f: mean 4.5e-15, variance 1.3e-15.  One point with lags: Kdiag 0, Kzx 1.3e-16."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sigkern_oracle as O

pytestmark = pytest.mark.gpu

CLASS = {"rbf": "SignatureRBF", "matern12": "SignatureMatern12", "matern32": "SignatureMatern32", "matern52": "SignatureMatern52"}


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def rel(got, want):
    got, want = host(got), host(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def rel_levels(got, want):
    """levels first: the largest error of any level, each relative to its own largest entry (a level that is exactly zero -- more levels than
    steps -- must come out exactly zero)"""
    got, want = host(got), host(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    worst = 0.0
    for g, w in zip(got, want):
        if w.size and np.abs(w).max() == 0.0:
            assert np.array_equal(g, w), "a level of exact zeros came out non-zero"
        else:
            worst = max(worst, rel(g, w))
    return worst


def tol_for(base, meets_itself):
    return 1e-7 if (base == "matern12" and meets_itself) else 1e-10


def make(base, L, d, M, seed=0, **kw):
    """the kernel object (exact_ragged on), a dense twin (off) and the oracle, with the same random hyper-parameters"""
    from gpsig_amd import kernels
    rng = np.random.default_rng(1000 + seed)
    ls = rng.uniform(0.8, 1.6, d) * np.sqrt(d)
    var = rng.uniform(0.5, 1.5, M + 1)
    objs = []
    for _ in range(2):
        k = getattr(kernels, CLASS[base])(L * d, d, M, lengthscales=ls, variances=var, **kw)
        objs.append(k)
    ko = O.SignatureKernelOracle(d, d, M, base=base, lengthscales=ls, variances=var, **kw)
    if kw.get("num_lags"):
        for o in objs + [ko]:
            o.lags, o.gamma = np.array([0.23]), np.array([0.6, 0.45])
            if hasattr(o, "lag_axis"):
                o.lag_axis = "sequence"
    objs[0].exact_ragged = True
    return objs[0], objs[1], ko


def table(rng, N, L, d, lengths, fill):
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.4, axis=1)
    for n, l in enumerate(lengths):
        X[n, l:] = fill
    return X.reshape(N, L * d)


def refill(X, L, d, lengths, fill):
    Y = X.reshape(len(lengths), L, d).copy()
    for n, l in enumerate(lengths):
        Y[n, l:] = fill
    return Y.reshape(len(lengths), L * d)


def by_repetition(X, L, d, lengths):
    Y = X.reshape(len(lengths), L, d).copy()
    for n, l in enumerate(lengths):
        Y[n, l:] = Y[n, l - 1]
    return Y.reshape(len(lengths), L * d)


def cuts(X, L, d, lengths):
    return [X.reshape(len(lengths), L, d)[n:n + 1, :l].reshape(1, l * d) for n, l in enumerate(lengths)]


def tensors(rng, M, T, de, increments):
    lt = M * (M + 1) // 2
    return rng.standard_normal((lt, T, 2, de) if increments else (lt, T, de)) * 0.7


class options:
    """context options of the default-stream context (host- and device-pointer calls of the kernel objects share it), put back afterwards"""

    def __init__(self, **opts):
        self.opts = opts

    def __enter__(self):
        from gpsig_amd import _lib
        self.ctx = _lib.context(0, 0)
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)
        return self.ctx

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, {"wide": -1, "wide_chunk_mb": 0}[k])
        return False


def dev(a):
    return torch.as_tensor(a, device="cuda:0")


def both_modes(fn, *arrays):
    """fn on host arrays and on CUDA tensors: identical bits; returns the host result (tuples element by element)"""
    a = fn(*arrays)
    b = fn(*[dev(x) for x in arrays])
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert np.array_equal(host(x), host(y)), "host- and device-pointer calls differ"
    return a


def nan_and_zeros(fn, X, L, d, lengths):
    """fn(X) with NaN in all padded rows and with zeros there: identical bits, nothing of them is read"""
    a = fn(refill(X, L, d, lengths, np.nan))
    b = fn(refill(X, L, d, lengths, 0.0))
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert np.isfinite(host(x)).all()
        assert np.array_equal(host(x), host(y)), "the padded rows changed bits"
    return a


def note(name, e):
    print("%-64s %.2e" % (name, e))
    return e


# ---- Kzx ---------------------------------------------------------------------------------------------------------------------------------------------
KZX = [("rbf", 4, 70, 13, 12, [13, 12, 2, 1, 7]),                # two lane blocks of tensors, the second short
       ("matern12", 4, 70, 13, 12, [13, 12, 2, 1, 7]),
       ("rbf", 4, 70, 13, 12, [13, 12, 2, 1, 7] * 5),            # 175 rows: four uneven chunks at wide_chunk_mb = 1 with increments
       ("rbf", 3, 33, 9, 126, [9, 1, 5, 8]),
       ("matern52", 3, 33, 9, 126, [9, 1, 5, 8]),
       ("rbf", 8, 9, 7, 10, [7, 3, 1, 6, 2]),
       ("matern32", 8, 9, 7, 10, [7, 3, 1, 6, 2])]


@pytest.mark.parametrize("base,M,T,L,d,lengths", KZX)
def test_kzx(base, M, T, L, d, lengths):
    rng = np.random.default_rng(7 * M + T + d)
    N = len(lengths)
    for difference in (True, False):
        for increments in (True, False):
            for normalization in ((True, False) if (difference and increments) else (False,)):
                k, kd, ko = make(base, L, d, M, difference=difference, normalization=normalization)
                Z = tensors(rng, M, T, d, increments)
                X = table(rng, N, L, d, lengths, np.nan)
                tol = tol_for(base, normalization)
                call = lambda A, **kw: both_modes(lambda z, x: k.K_tens_vs_seq(z, x, increments=increments, lengths=lengths, **kw), Z, A)      # noqa: E731
                got = nan_and_zeros(lambda A: call(A, return_levels=True), X, L, d, lengths)
                want = np.concatenate([ko.K_tens_vs_seq(Z, c, increments=increments, return_levels=True) for c in cuts(X, L, d, lengths)], axis=2)
                tag = (difference, increments, normalization)
                e = note("Kzx levels vs oracle %s %s" % (base, tag), rel_levels(got, want))
                assert e < tol, (tag, e)
                assert rel(call(X), want.sum(0)) < tol
                with options(wide_chunk_mb=1):
                    e = note("  ... under wide_chunk_mb = 1", rel_levels(call(X, return_levels=True), want))
                    assert e < tol, (tag, e)
                with options(wide=1):
                    one = np.concatenate([host(kd.K_tens_vs_seq(Z, c, increments=increments, return_levels=True)) for c in cuts(X, L, d, lengths)], axis=2)
                e = note("  ... vs the dense entry point, one sequence at a time", rel_levels(got, one))
                assert e < tol, (tag, e)
                if difference:
                    pad = kd.K_tens_vs_seq(Z, by_repetition(X, L, d, lengths), increments=increments, return_levels=True)
                    e = note("  ... vs the dense call on the table padded by repetition", rel_levels(got, pad))
                    assert e < tol, (tag, e)


# ---- level diagonals ---------------------------------------------------------------------------------------------------------------------------------
DIAG = [("rbf", 4, 70, 46, [70, 66, 65, 64, 2, 1], True),        # two columns per lane; lengths around the 64-column tile edge
        ("matern32", 4, 70, 46, [70, 66, 65, 64, 2, 1], True),
        # (Matern-1/2 at test_gpu_wide.py's own lengths: the reference's value at a self-pair is exp(-sqrt(rounding noise of |x|^2)), off by
        # 1e-8 |x|, and the 1e-7 of that file's line 156 was set for paths of about ten steps -- at 70 steps the ORACLE is 1.5e-7 from the truth)
        ("matern12", 4, 13, 12, [13, 12, 2, 1, 7], True),
        ("rbf", 4, 131, 12, [131, 130, 129, 65, 3], True),       # four columns per lane, three tiles
        ("rbf", 5, 260, 28, [260, 257, 70], True),               # eight wavefronts per lattice (N = 3), five tiles
        ("rbf", 1, 9, 5, [9, 4, 1], True),                       # M = 1
        ("matern32", 1, 9, 5, [9, 4, 1], False),
        ("rbf", 4, 65, 10, [65, 64, 33, 1], False),              # difference=False: 65 columns
        ("matern52", 4, 65, 10, [65, 64, 33, 1], False)]


@pytest.mark.parametrize("base,M,L,d,lengths,difference", DIAG)
def test_level_diagonals(base, M, L, d, lengths, difference):
    rng = np.random.default_rng(11 * M + L + d)
    N = len(lengths)
    k, kd, ko = make(base, L, d, M, difference=difference, normalization=False)
    X = table(rng, N, L, d, lengths, np.nan)
    tol = tol_for(base, True)
    call = lambda A: both_modes(lambda x: k.Kdiag(x, return_levels=True, lengths=lengths), A)      # noqa: E731
    got = nan_and_zeros(call, X, L, d, lengths)
    want = np.concatenate([ko.Kdiag(c, return_levels=True) for c in cuts(X, L, d, lengths)], axis=1)
    e = note("Kdiag levels vs oracle %s M=%d L=%d d=%d" % (base, M, L, d), rel_levels(got, want))
    assert e < tol, e
    assert rel(k.Kdiag(X, lengths=lengths), want.sum(0)) < tol
    for mb in (1, 2):                                            # (L = 260: one sequence alone is half a megabyte of cells)
        with options(wide_chunk_mb=mb):
            assert np.array_equal(host(call(X)), host(got)), "Kdiag depends on the chunking"
    with options(wide=1):
        one = np.concatenate([host(kd.Kdiag(c, return_levels=True)) for c in cuts(X, L, d, lengths)], axis=1)
    e = note("  ... vs the dense entry point, one sequence at a time", rel_levels(got, one))
    assert e < tol, e
    if difference:
        with options(wide=1):
            pad = kd.Kdiag(by_repetition(X, L, d, lengths), return_levels=True)
        e = note("  ... vs the dense call on the table padded by repetition", rel_levels(got, pad))
        assert e < tol, e
    # the normalised diagonal reads no features: sigma * variances, the lengths checked and ignored
    k.normalization = True
    assert np.array_equal(host(k.Kdiag(X, return_levels=True, lengths=lengths)), np.tile((k.sigma * np.asarray(k.variances))[:, None], [1, N]))
    # the factors of a normalised Kzx are these diagonals: one inducing tensor block against the same table
    Z = tensors(rng, M, 5, d, True)
    gz = nan_and_zeros(lambda A: k.K_tens_vs_seq(Z, A, increments=True, return_levels=True, lengths=lengths), X, L, d, lengths)
    ko.normalization = True
    wz = np.concatenate([ko.K_tens_vs_seq(Z, c, increments=True, return_levels=True) for c in cuts(X, L, d, lengths)], axis=2)
    e = note("  ... normalised Kzx on the same table", rel_levels(gz, wz))
    assert e < tol, e


# ---- K ---------------------------------------------------------------------------------------------------------------------------------------------------
def oracle_K(ko, A, B=None):
    """levels (M+1, N1, N2) from one pair at a time; B None: symmetric (a sequence against itself is the symmetric call of that sequence)"""
    rows = []
    for i, a in enumerate(A):
        row = []
        for j, b in enumerate(A if B is None else B):
            row.append(ko.K(a, return_levels=True) if (B is None and i == j) else ko.K(a, b, return_levels=True))
        rows.append(np.concatenate(row, axis=2))
    return np.concatenate(rows, axis=1)


def dense_K(kd, A, B=None):
    rows = []
    for i, a in enumerate(A):
        row = []
        for j, b in enumerate(A if B is None else B):
            row.append(host(kd.K(a, return_levels=True) if (B is None and i == j) else kd.K(a, b, return_levels=True)))
        rows.append(np.concatenate(row, axis=2))
    return np.concatenate(rows, axis=1)


@pytest.mark.parametrize("base", ["rbf", "matern12"])
@pytest.mark.parametrize("normalization", [True, False])
def test_K_symmetric(base, normalization):
    M, L, d, lengths = 4, 33, 12, [33, 17, 2, 9]
    rng = np.random.default_rng(3)
    for difference in (True, False):
        k, kd, ko = make(base, L, d, M, difference=difference, normalization=normalization)
        X = table(rng, len(lengths), L, d, lengths, np.nan)
        tol = tol_for(base, True)
        call = lambda A, **kw: both_modes(lambda x: k.K(x, lengths=lengths, **kw), A)      # noqa: E731
        got = nan_and_zeros(lambda A: call(A, return_levels=True), X, L, d, lengths)
        cs = cuts(X, L, d, lengths)
        e = note("K symmetric levels vs oracle %s %s" % (base, (normalization, difference)), rel_levels(got, oracle_K(ko, cs)))
        assert e < tol, e
        assert rel(call(X), oracle_K(ko, cs).sum(0)) < tol
        with options(wide=1):
            one = dense_K(kd, cs)
        e = note("  ... vs the dense entry point, one pair at a time", rel_levels(got, one))
        assert e < tol, e
        with options(wide_chunk_mb=1):
            assert rel_levels(call(X, return_levels=True), oracle_K(ko, cs)) < tol
        if difference:
            with options(wide=1):
                pad = kd.K(by_repetition(X, L, d, lengths), return_levels=True)
            e = note("  ... vs the dense call on the table padded by repetition", rel_levels(got, pad))
            assert e < tol, e


@pytest.mark.parametrize("base", ["rbf", "matern32"])
@pytest.mark.parametrize("sides", ["both ragged", "left dense", "right dense"])
def test_K_cross(base, sides):
    M, d, L1, L2 = 4, 12, 20, 70
    len1 = [20, 1, 7] if sides != "left dense" else [20, 20, 20]
    len2 = [70, 66, 3, 64] if sides != "right dense" else [70, 70, 70, 70]
    rng = np.random.default_rng(5)
    for normalization in (True, False):
        k, kd, ko = make(base, max(L1, L2), d, M, normalization=normalization)          # (input_dim: the wider table's columns)
        X, X2 = table(rng, len(len1), L1, d, len1, np.nan), table(rng, len(len2), L2, d, len2, np.nan)
        kw = dict(lengths=None if sides == "left dense" else len1, lengths2=None if sides == "right dense" else len2)
        call = lambda A, B: both_modes(lambda a, b: k.K(a, b, return_levels=True, **kw), A, B)      # noqa: E731
        got = call(X, X2)
        again = call(refill(X, L1, d, len1, 0.0), refill(X2, L2, d, len2, 0.0))
        assert np.isfinite(host(got)).all() and np.array_equal(host(got), host(again)), "the padded rows changed bits"
        c1, c2 = cuts(X, L1, d, len1), cuts(X2, L2, d, len2)
        tol = tol_for(base, normalization)
        e = note("K cross levels vs oracle %s %s %s" % (base, sides, normalization), rel_levels(got, oracle_K(ko, c1, c2)))
        assert e < tol, e
        with options(wide=1):
            one = dense_K(kd, c1, c2)
        e = note("  ... vs the dense entry point, one pair at a time", rel_levels(got, one))
        assert e < tol, e
        with options(wide_chunk_mb=1):
            assert rel_levels(call(X, X2), oracle_K(ko, c1, c2)) < tol
        pad = kd.K(by_repetition(X, L1, d, len1), by_repetition(X2, L2, d, len2), return_levels=True)
        e = note("  ... vs the dense call on the tables padded by repetition", rel_levels(got, pad))
        assert e < tol, e


# ---- the public surface with lags ----------------------------------------------------------------------------------------------------------------------
SURF = dict(M=3, L=12, d=6, T=7, lengths=[12, 7, 2, 5, 9])


def _surface(base="rbf"):
    s = SURF
    rng = np.random.default_rng(17)
    k, kd, ko = make(base, s["L"], s["d"], s["M"], num_lags=1, normalization=True)
    X = table(rng, len(s["lengths"]), s["L"], s["d"], s["lengths"], np.nan)
    Z = tensors(rng, s["M"], s["T"], 2 * s["d"], True)
    return k, kd, ko, X, Z, cuts(X, s["L"], s["d"], s["lengths"])


@pytest.mark.parametrize("method", ["K", "K_X2", "Kdiag", "K_tens_vs_seq", "K_tens_n_seq_covs", "K_tens_n_seq_covs_full", "K_seq_n_seq_covs",
                                    "K_seq_n_seq_covs_full"])
def test_public_surface_with_lags(method):
    """num_lags = 1 with lag_axis = "sequence", normalisation on: every sequence's lag interpolation runs on its own axis i / (len_n - 1) -- what the
    oracle and the dense entry point give for the truncated sequence on its own.  Fails on a commit where exact mode refuses lengths=."""
    s = SURF
    k, kd, ko, X, Z, cs = _surface()
    L, d, lengths, N = s["L"], s["d"], s["lengths"], len(s["lengths"])
    tol = 1e-10
    rngi = np.random.default_rng(23)
    Xi = np.cumsum(rngi.standard_normal((3, 5, d)) * 0.3, axis=1)          # inducing sequences: dense
    if method == "K":
        got = nan_and_zeros(lambda A: both_modes(lambda x: k.K(x, return_levels=True, lengths=lengths), A), X, L, d, lengths)
        want = oracle_K(ko, cs)
        with options(wide=1):
            one = dense_K(kd, cs)
        pairs = [(got, want), (got, one)]
    elif method == "K_X2":
        got = nan_and_zeros(lambda A: both_modes(lambda a, x: k.K(a, x, return_levels=True, lengths2=lengths), Xi.reshape(3, -1), A), X, L, d, lengths)
        pairs = [(got, oracle_K(ko, [Xi[i:i + 1].reshape(1, -1) for i in range(3)], cs))]
    elif method == "Kdiag":
        k.normalization = kd.normalization = ko.normalization = False
        got = nan_and_zeros(lambda A: both_modes(lambda x: k.Kdiag(x, return_levels=True, lengths=lengths), A), X, L, d, lengths)
        with options(wide=1):
            one = np.concatenate([host(kd.Kdiag(c, return_levels=True)) for c in cs], axis=1)
        pairs = [(got, np.concatenate([ko.Kdiag(c, return_levels=True) for c in cs], axis=1)), (got, one)]
    elif method == "K_tens_vs_seq":
        got = nan_and_zeros(lambda A: both_modes(lambda z, x: k.K_tens_vs_seq(z, x, increments=True, return_levels=True, lengths=lengths), Z, A), X, L, d, lengths)
        with options(wide=1):
            one = np.concatenate([host(kd.K_tens_vs_seq(Z, c, increments=True, return_levels=True)) for c in cs], axis=2)
        pairs = [(got, np.concatenate([ko.K_tens_vs_seq(Z, c, increments=True, return_levels=True) for c in cs], axis=2)), (got, one)]
    elif method.startswith("K_tens_n_seq_covs"):
        full = method.endswith("full")
        got = nan_and_zeros(lambda A: both_modes(lambda z, x: k.K_tens_n_seq_covs(z, x, full_X_cov=full, increments=True, return_levels=True, lengths=lengths),
                                                 Z, A), X, L, d, lengths)
        per = [ko.K_tens_n_seq_covs(Z, c, full_X_cov=False, increments=True, return_levels=True) for c in cs]
        Kxx = oracle_K(ko, cs) if full else np.concatenate([p[2] for p in per], axis=1)
        pairs = [(got[0], per[0][0]), (got[1], np.concatenate([p[1] for p in per], axis=2)), (got[2], Kxx)]
        assert np.array_equal(host(got[0]), host(kd.K_tens(Z, increments=True, return_levels=True))), "Kzz is the dense call's"
    else:
        full = method.endswith("full")
        A = Xi.reshape(3, -1)
        got = nan_and_zeros(lambda B: both_modes(lambda a, x: k.K_seq_n_seq_covs(a, x, full_X2_cov=full, return_levels=True, lengths2=lengths), A, B),
                            X, L, d, lengths)
        per = [ko.K_seq_n_seq_covs(A, c, full_X2_cov=full, return_levels=True) for c in cs]
        K22 = oracle_K(ko, cs) if full else np.concatenate([p[2] for p in per], axis=1)
        pairs = [(got[0], per[0][0]), (got[1], np.concatenate([p[1] for p in per], axis=2)), (got[2], K22)]
    for g, w in pairs:
        e = note("surface with lags: %s" % method, rel_levels(g, w))
        assert e < tol, (method, e)


@pytest.mark.parametrize("full_cov", [False, True])
def test_predict_f_with_lags(full_cov):
    from gpsig_amd import inducing_variables as IV, models
    from oracle import svgp_oracle as SO
    s = SURF
    k, kd, ko, X, Z, cs = _surface()
    T, N, R = s["T"], len(s["lengths"]), 2
    rng = np.random.default_rng(29)
    q_mu = rng.standard_normal((T, R))
    q_sqrt = np.tril(0.3 * rng.standard_normal((R, T, T))) + np.eye(T)[None]
    feat = IV.InducingTensors(Z, s["M"], increments=True)
    m = models.SVGP(k, feat, q_diag=False, whiten=True, q_mu=q_mu, q_sqrt=q_sqrt)
    per = [O.inducing_tensors_Kuu_Kuf_Kff(ko, Z, c, increments=True, jitter=1e-6, full_f_cov=False) for c in cs]
    Kzz, Kzx = per[0][0], np.concatenate([p[1] for p in per], axis=1)
    if full_cov:
        Kxx = oracle_K(ko, cs).sum(0) + 1e-6 * np.eye(N)
    else:
        Kxx = np.concatenate([p[2] for p in per])
    for g, w in zip(IV.Kuu_Kuf_Kff(feat, k, X, jitter=1e-6, full_f_cov=full_cov, lengths=s["lengths"]), (Kzz, Kzx, Kxx)):
        e = note("Kuu_Kuf_Kff with lags, full_f_cov=%s" % full_cov, rel(g, w))
        assert e < 1e-10, e
    want_mean, want_var = SO.base_conditional(Kzx, Kzz, Kxx, q_mu, full_cov=full_cov, q_sqrt=q_sqrt, white=True)
    mean, var = m.predict_f(X, full_cov=full_cov, lengths=s["lengths"])
    e = (note("predict_f mean", rel(mean, want_mean)), note("predict_f variance", rel(var, want_var)))
    assert max(e) < 1e-6, e


def test_one_point_sequence_with_lags():
    """A sequence of one point has no time axis: its lagged copies are the point itself.  So its values are those of the lag-free kernel on twice the
    columns at the point repeated, with the lag weights folded into the lengthscales."""
    from gpsig_amd import kernels
    M, L, d, T = 3, 6, 4, 5
    rng = np.random.default_rng(31)
    lengths = [1, 6, 1, 3]
    for base, difference in (("rbf", False), ("matern32", False), ("rbf", True)):
        k, kd, ko = make(base, L, d, M, num_lags=1, normalization=False, difference=difference)
        X = table(rng, len(lengths), L, d, lengths, np.nan)
        Z = tensors(rng, M, T, 2 * d, True)
        ls2 = np.concatenate([np.asarray(k.lengthscales) / g for g in k.gamma])
        k0 = getattr(kernels, CLASS[base])(2 * d, 2 * d, M, lengthscales=ls2, variances=np.asarray(k.variances), normalization=False, difference=difference)
        gd = host(k.Kdiag(X, return_levels=True, lengths=lengths))
        gz = host(k.K_tens_vs_seq(Z, X, increments=True, return_levels=True, lengths=lengths))
        assert np.isfinite(gd).all() and np.isfinite(gz).all()
        for n in (0, 2):
            x = X.reshape(len(lengths), L, d)[n, 0]
            xx = np.concatenate([x, x])[None, :]
            with options(wide=1):
                wd, wz = host(k0.Kdiag(xx, return_levels=True)), host(k0.K_tens_vs_seq(Z, xx, increments=True, return_levels=True))
            e = max(note("one point with lags: Kdiag %s" % base, rel_levels(gd[:, n:n + 1], wd)) if not difference else 0.0,
                    note("one point with lags: Kzx %s" % base, rel(gz[:, :, n:n + 1], wz)))
            assert e < 1e-10, (base, difference, n, e)
            if difference:                                       # no increments: every level above the zeroth is exactly zero
                assert np.array_equal(gd[1:, n], np.zeros(M)) and np.array_equal(gz[1:, :, n], np.zeros((M, T)))


def test_float32_inputs_are_computed_in_float64_and_rounded():
    M, L, d, lengths = 3, 9, 5, [9, 4, 1, 6]
    rng = np.random.default_rng(37)
    k, kd, ko = make("rbf", L, d, M)
    X = table(rng, len(lengths), L, d, lengths, np.nan).astype(np.float32)
    Z = tensors(rng, M, 4, d, True).astype(np.float32)
    for fn in (lambda x, z: k.K(x, lengths=lengths), lambda x, z: k.Kdiag(x, lengths=lengths), lambda x, z: k.K_tens_vs_seq(z, x, increments=True, lengths=lengths)):
        got = fn(X, Z)
        assert host(got).dtype == np.float32
        assert np.array_equal(host(got), host(fn(X.astype(np.float64), Z.astype(np.float64))).astype(np.float32))
        gt = fn(dev(X), dev(Z))
        assert gt.dtype == torch.float32 and np.array_equal(host(gt), host(got))


# ---- refusals: typed, and each names its bound -----------------------------------------------------------------------------------------------------------
def test_refusals_name_their_bounds():
    from gpsig_amd import kernels, _lib
    L, d, M, lengths = 9, 3, 3, [9, 4, 1, 6]
    rng = np.random.default_rng(41)
    X = table(rng, len(lengths), L, d, lengths, np.nan)
    for cls in (kernels.SignatureLinear, kernels.SignatureCosine, kernels.SignaturePoly, kernels.SignatureMix, kernels.SignatureSpectral):
        k = cls(L * d, d, M)
        k.exact_ragged = True
        with pytest.raises(NotImplementedError, match="SignatureRBF and the Matern families only"):
            k.K(X, lengths=lengths)
        with pytest.raises(NotImplementedError, match="SignatureRBF and the Matern families only"):
            k.Kdiag(X, lengths=lengths)
    k = kernels.SignatureRBF(L * d, d, M, order=2)
    k.exact_ragged = True
    with pytest.raises(NotImplementedError, match=r"first order only \(order = 2\)"):
        k.K(X, lengths=lengths)
    k = kernels.SignatureRBF(L * d, d, M)
    k.exact_ragged = True
    with options(wide=0):
        with pytest.raises(NotImplementedError, match="context option wide = 0 refuses it"):
            k.K_tens_vs_seq(np.zeros((6, 2, d)), X, lengths=lengths)
    # sequence lattices beyond 512 columns: 514 observations with differences are 513 columns; 513 are served
    kl = kernels.SignatureRBF(514, 1, 2, normalization=False)
    kl.exact_ragged = True
    long = np.cumsum(rng.standard_normal((2, 514)) * 0.1, axis=1)
    with pytest.raises(NotImplementedError, match=r"at most 512 columns \(got 513\)"):
        kl.Kdiag(long, lengths=[514, 3])
    assert np.isfinite(host(kl.Kdiag(long, lengths=[513, 3]))).all()
    # inside the library: float32, a NULL lengths pointer, a length out of range, graph capture
    ctx = _lib.context(0, 0)
    ctx.set_pointer_mode(_lib.PTR_HOST)
    keep = []
    lens = np.asarray(lengths, dtype=np.int32)
    out = np.empty(len(lengths))
    vp = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    with pytest.raises(NotImplementedError, match="float64 only"):
        ctx.call("gpsig_kernel_Kdiag_ragged", k._params(keep, _lib.F32), vp(np.zeros(X.shape, dtype=np.float32)), len(lengths), L, vp(lens), 0, vp(np.zeros(len(lengths), dtype=np.float32)))
    p = k._params(keep)
    with pytest.raises(ValueError, match="null lengths pointer"):
        ctx.call("gpsig_kernel_Kdiag_ragged", p, vp(X), len(lengths), L, None, 0, vp(out))
    with pytest.raises(ValueError, match="null lengths pointer"):
        ctx.call("gpsig_kernel_K_tens_vs_seq_ragged", p, vp(np.zeros((6, 2, d))), vp(X), 2, len(lengths), L, None, 0, 0, vp(np.empty((2, len(lengths)))))
    for bad in ([9, 4, 0, 6], [9, 10, 1, 6]):
        with pytest.raises(ValueError, match=r"outside \[1, 9\]"):
            ctx.call("gpsig_kernel_Kdiag_ragged", p, vp(X), len(lengths), L, vp(np.asarray(bad, dtype=np.int32)), 0, vp(out))
    s = torch.cuda.Stream("cuda:0")
    with torch.cuda.stream(s):
        sctx = _lib.context(0, s.cuda_stream)
        sctx.set_pointer_mode(_lib.PTR_DEVICE)
        Xd, ld, od = dev(refill(X, L, d, lengths, 0.0)), dev(lens), torch.empty(len(lengths), dtype=torch.float64, device="cuda:0")
        ptr = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        sctx.call("gpsig_kernel_Kdiag_ragged", p, ptr(Xd), len(lengths), L, ptr(ld), 0, ptr(od))
        s.synchronize()
        want = od.clone()
        with pytest.raises(NotImplementedError, match="not served during library graph capture"):
            with sctx.graph():
                sctx.call("gpsig_kernel_Kdiag_ragged", p, ptr(Xd), len(lengths), L, ptr(ld), 0, ptr(od))
        sctx.call("gpsig_kernel_Kdiag_ragged", p, ptr(Xd), len(lengths), L, ptr(ld), 0, ptr(od))      # the context works as before
        s.synchronize()
        assert torch.equal(od, want)
