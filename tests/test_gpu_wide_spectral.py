"""Exact-mode SignatureSpectral beyond 32 columns (kernel object opt-in ``spectral_wide``): the wide route's argument array filled by the spectral
argument kernel (csrc/wide_spectral_kernel.hpp, wide_spectral_inst.hip) instead of the dgemm, the chain / lattice / tensor kernels in their identity kind.

Oracle: oracle.sigkern_oracle.SignatureKernelOracle(base="spectral", lengthscales=None), which takes explicit coordinate differences (exact at
coinciding points).  Data as tests/test_gpu_wide.py::_data (scale 1 / sqrt(d)), alpha in U(0.3, 1.2), omega = 0.3 / sqrt(d) N(0, 1), gamma in U(0.4, 1.3).
Tolerance: 1e-10 relative to the largest entry, the bound tests/test_gpu_wide.py holds the distance kernels to.  A NumPy restatement of the expanded
form (xs + ss - 2 ip, phases as differences of one-sided sums) reaches 7e-15 with coinciding rows at exactly 0 and misses by up to 8e-8 ('exp', 'mixed':
the square root of rounding noise on self-pairs) without that property -- so the bound also fails a kernel that lacks it.

Errors measured on the GPU (MI355X), the largest over the shapes, flags and families of each test:
    against the oracle, every quantity and flag: 'gauss' 5.9e-16 .. 2.9e-15 over the ten shapes, 2.1e-14 at Q = 64; 'exp' 1.7e-15 .. 6.8e-15;
        'mixed' 1.7e-15 .. 5.2e-15 (the Q = 64 shape is the largest of each family)
    K_tens_vs_seq at order 2: 6.0e-16 (points), 1.1e-15 (increments)
    coinciding points, 'exp': K_tens 6.0e-16, K_tens_vs_seq 5.7e-16 (increments), 2.6e-16 / 9.2e-16 (points), Kdiag level 1 2.1e-16
    SVGP.predict_f at 65 columns: mean 1.5e-15, variance 1.9e-16
    K_seq_n_seq_covs against inducing sequences of another length: passes at 1e-10 (its figures were not written down)
    chunks (wide_chunk_mb = 1 against 0), host against device pointers, float32 against rounded float64, 32 / 16 columns with and without the
        flag: the same bits
The test at Q = 64 and 130 tensors takes 6 s, nearly all of it the NumPy oracle's 64 passes over (260, 260, 40) differences per component.
SVGP.predict_f is held to 1e-6, the bound of tests/test_gpu_parity.py::test_svgp_predict_and_kl (a Cholesky solve amplifies the covariances' error)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sigkern_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-10
# (M, T, N, L, d, Q)
SHAPES = [(4, 70, 9, 13, 33, 5), (3, 20, 5, 11, 63, 5), (3, 20, 5, 11, 64, 1), (4, 65, 4, 17, 65, 3), (4, 65, 4, 17, 126, 3), (2, 7, 66, 5, 300, 2),
          (4, 130, 6, 9, 40, 64), (8, 9, 3, 10, 34, 2), (1, 5, 3, 4, 65, 1), (2, 5, 3, 4, 4096, 2)]
SAMPLE = {(4, 70, 9, 13, 33, 5), (4, 65, 4, 17, 65, 3), (4, 65, 4, 17, 126, 3), (4, 130, 6, 9, 40, 64)}       # 'exp' and 'mixed'
FAMILIES = ["gauss", "exp", "mixed"]


def rel(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _data(rng, M, T, N, L, d, increments):
    lt = M * (M + 1) // 2
    s = 1.0 / np.sqrt(d)                  # distances of order one whatever the width
    Z = rng.standard_normal((lt, T, 2, d) if increments else (lt, T, d)) * s
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.5 * s, axis=1)
    return Z, X.reshape(N, L * d)


def shared_base(ko, cache):
    """The oracle's base-kernel matrices are what its evaluations cost (Q passes over a (P, P2, d) array of differences: 22 s for K_tens at 130
    tensors with increments and Q = 64), and they do not depend on the flags the tests vary.  So an oracle instance evaluates its own base kernel
    in blocks of 16 rows -- it is elementwise: the same bits, half the time -- and a test's instances share the matrices by content."""
    inner = ko._base_kern

    def base(X, X2=None):
        Y = X if X2 is None else X2
        key = (X.shape, X.tobytes(), Y.shape, Y.tobytes())
        if key not in cache:
            cache[key] = np.concatenate([inner(X[..., i:i + 16, :], Y) for i in range(0, X.shape[-2], 16)], axis=-2)
        return cache[key]
    ko._base_kern = base
    return ko


def make(family, M, L, d, Q, seed=3, wide=True, cache=None, **kw):
    """the kernel object (flag set) and the oracle with the same parameters"""
    from gpsig_amd import kernels
    rng = np.random.default_rng(seed)
    alpha, omega, gamma = rng.uniform(0.3, 1.2, Q), 0.3 / np.sqrt(d) * rng.standard_normal((Q, d)), rng.uniform(0.4, 1.3, (Q, d))
    variances = rng.uniform(0.5, 1.5, M + 1)
    k = kernels.SignatureSpectral(L * d, d, M, family=family, Q=Q, variances=variances, **kw)
    k.alpha, k.omega, k.gamma = alpha, omega, gamma
    k.spectral_wide = wide
    ko = O.SignatureKernelOracle(L * d, d, M, base="spectral", lengthscales=None, variances=variances,
                                 base_params=dict(alpha=alpha, omega=omega, gamma=gamma, family=k.family), **kw)
    return k, shared_base(ko, {} if cache is None else cache)


def levels(out):
    return np.stack([host(o) for o in out]) if isinstance(out, (list, tuple)) else host(out)


def with_options(opts, fn):
    """gpsig_set_option on the host-pointer context and on the device-pointer one of the current stream; defaults restored"""
    from gpsig_amd import _lib
    ctxs = [_lib.context(0, 0), _lib.context(0, torch.cuda.current_stream(DEV).cuda_stream)]
    defaults = {"wide_chunk_mb": 0, "wide": -1}
    try:
        for ctx in ctxs:
            for n, v in opts.items():
                ctx.set_option(n, v)
        return fn()
    finally:
        for ctx in ctxs:
            for n in opts:
                ctx.set_option(n, defaults[n])


def quantities(k, X, X2, Zs, tens=True):
    """every quantity of the feature as one list of arrays (Zs: {increments: Z}); K_tens does not depend on the sequences' flags (tens: include it)"""
    out = [levels(k.K(X, return_levels=True)), host(k.K(X)), levels(k.K(X, X2, return_levels=True)), levels(k.Kdiag(X, return_levels=True)), host(k.Kdiag(X))]
    for inc, Z in Zs.items():
        if tens:
            out += [levels(k.K_tens(Z, return_levels=True, increments=inc)), host(k.K_tens(Z, increments=inc))]
        out += [levels(k.K_tens_vs_seq(Z, X, return_levels=True, increments=inc)), host(k.K_tens_vs_seq(Z, X, increments=inc))]
        out += [host(o) for o in k.K_tens_n_seq_covs(Z, X, increments=inc)]
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_oracle(shape, family):
    """K(X), K(X, X2) levels, Kdiag, K_tens, K_tens_vs_seq, K_tens_n_seq_covs; increments, differences and normalisation on / off"""
    if family != "gauss" and shape not in SAMPLE:
        pytest.skip("a sample of the shapes is enough for the 'exp' and 'mixed' families")
    M, T, N, L, d, Q = shape
    rng = np.random.default_rng(1000 * M + T + d)
    Zs = {inc: _data(rng, M, T, N, L, d, inc)[0] for inc in (False, True)}
    X = _data(rng, M, T, N, L, d, False)[1]
    X2 = _data(rng, M, T, 3, L, d, False)[1]
    worst, cache = 0.0, {}
    for ti, (difference, normalization) in enumerate(((True, True), (True, False), (False, True), (False, False))):
        k, ko = make(family, M, L, d, Q, cache=cache, difference=difference, normalization=normalization)
        got = quantities(k, X, X2, Zs, tens=ti == 0)
        want = quantities(ko, X, X2, Zs, tens=ti == 0)
        assert len(got) == len(want)
        for qi, (g, w) in enumerate(zip(got, want)):
            e = rel(g, w)
            worst = max(worst, e)
            assert np.isfinite(g).all() and e < TOL, (difference, normalization, qi, e)
    print("against the oracle", shape, family, "worst relative error", worst)


def test_tensors_vs_sequences_at_order_two():
    """(not normalised: the factors would be order-2 sequence lattices, which this route refuses)"""
    M, T, N, L, d, Q = 4, 70, 9, 13, 33, 5
    rng = np.random.default_rng(11)
    for inc in (False, True):
        Z, X = _data(rng, M, T, N, L, d, inc)
        k, ko = make("mixed", M, L, d, Q, order=2, normalization=False)
        e = rel(levels(k.K_tens_vs_seq(Z, X, return_levels=True, increments=inc)), levels(ko.K_tens_vs_seq(Z, X, return_levels=True, increments=inc)))
        print("K_tens_vs_seq at order 2, increments", inc, ":", e)
        assert e < TOL, (inc, e)


def test_chunks_and_pointer_modes_give_the_same_bits():
    """wide_chunk_mb = 1: 150 sequences of 30 observations give argument lattices of 1.08 MB per left sequence (K: one per chunk) and 7.2 kB per diagonal
    lattice (Kdiag: 145 per chunk); Kzx at 10 components x 2 endpoints x 128 padded tensors takes 614 kB per sequence (one per chunk)"""
    M, T, N, L, d, Q = 4, 70, 150, 30, 33, 2
    rng = np.random.default_rng(91)
    Zs = {inc: _data(rng, M, T, N, L, d, inc)[0] for inc in (False, True)}
    X = _data(rng, M, T, N, L, d, False)[1]
    X2 = X[:7] * 1.01
    k, _ = make("exp", M, L, d, Q)
    whole = quantities(k, X, X2, Zs)
    parts = with_options({"wide_chunk_mb": 1}, lambda: quantities(k, X, X2, Zs))
    dwhole = quantities(k, dev(X), dev(X2), {i: dev(z) for i, z in Zs.items()})
    dparts = with_options({"wide_chunk_mb": 1}, lambda: quantities(k, dev(X), dev(X2), {i: dev(z) for i, z in Zs.items()}))
    for qi, (a, b, c_, e_) in enumerate(zip(whole, parts, dwhole, dparts)):
        assert np.isfinite(a).all(), qi
        assert np.array_equal(a, b), ("chunks, host pointers", qi)
        assert np.array_equal(a, c_), ("host against device pointers", qi)
        assert np.array_equal(a, e_), ("chunks, device pointers", qi)


def test_coinciding_points():
    """family 'exp': inducing-tensor points gathered from the sequences' own observations (the reference initialises Z that way) -- K_tens has tensor
    points that coincide with one another, K_tens_vs_seq tensor points that coincide with observations; and the self-pairs of Kdiag.  The square
    root of a squared distance of 1e-16 in place of 0 would cost 1e-8 here."""
    M, T, N, L, d, Q = 4, 70, 9, 13, 65, 3
    rng = np.random.default_rng(5)
    lt = M * (M + 1) // 2
    X = _data(rng, M, T, N, L, d, False)[1]
    pts = X.reshape(N * L, d)
    Z = pts[rng.integers(0, N * L, size=(lt, T, 2))]
    assert Z.shape == (lt, T, 2, d)
    k, ko = make("exp", M, L, d, Q, normalization=False)
    for name, g, w in (("K_tens", k.K_tens(Z, return_levels=True, increments=True), ko.K_tens(Z, return_levels=True, increments=True)),
                       ("K_tens_vs_seq", k.K_tens_vs_seq(Z, X, return_levels=True, increments=True), ko.K_tens_vs_seq(Z, X, return_levels=True, increments=True)),
                       ("K_tens, no increments", k.K_tens(Z[:, :, 0], return_levels=True), ko.K_tens(Z[:, :, 0], return_levels=True)),
                       ("K_tens_vs_seq, no increments", k.K_tens_vs_seq(Z[:, :, 0], X, return_levels=True), ko.K_tens_vs_seq(Z[:, :, 0], X, return_levels=True))):
        e = rel(levels(g), levels(w))
        print("coinciding points,", name, ":", e)
        assert e < TOL, (name, e)
    k, ko = make("exp", M, L, d, Q, normalization=False, difference=False)
    g, w = levels(k.Kdiag(X, return_levels=True)), levels(ko.Kdiag(X, return_levels=True))
    e = rel(g[1], w[1])
    print("coinciding points, Kdiag level 1 without differences:", e)
    assert e < TOL, e
    # one observation per sequence: level 1 is kappa(x, x) = sum_q alpha_q times the level's variance, whatever x
    k1, _ = make("exp", M, 1, d, Q, normalization=False, difference=False)
    g1 = levels(k1.Kdiag(X[:, :d], return_levels=True))
    want = np.sum(k1.alpha) * np.asarray(k1.variances).reshape(-1)[1] * float(k1.sigma)
    assert np.abs(g1[1] - want).max() <= (Q + 4) * 2.3e-16 * want, np.abs(g1[1] - want).max()      # (Q additions, the two factors: a rounding each)


def test_svgp_predict_f():
    from gpsig_amd import inducing_variables as IV, models
    from oracle import svgp_oracle as SO
    rng = np.random.default_rng(61)
    N, L, d, M, T, R, Q = 11, 9, 65, 3, 9, 2, 3
    Z, X = _data(rng, M, T, N, L, d, True)
    k, ko = make("mixed", M, L, d, Q)
    q_mu = rng.standard_normal((T, R))
    q_sqrt = np.tril(0.3 * rng.standard_normal((R, T, T))) + np.eye(T)[None]
    feat = IV.InducingTensors(Z, M, increments=True)
    m = models.SVGP(k, feat, q_diag=False, whiten=True, q_mu=q_mu, q_sqrt=q_sqrt)
    Kzz, Kzx, Kxx = O.inducing_tensors_Kuu_Kuf_Kff(ko, Z, X, increments=True, jitter=1e-6)
    want_mean, want_var = SO.base_conditional(Kzx, Kzz, Kxx, q_mu, full_cov=False, q_sqrt=q_sqrt, white=True)
    mean, var = m.predict_f(X)
    e = (rel(mean, want_mean), rel(var, want_var))
    print("SVGP.predict_f at 65 columns:", e)
    assert max(e) <= 1e-6, e
    for g, w in zip(IV.Kuu_Kuf_Kff(feat, k, X, jitter=1e-6), (Kzz, Kzx, Kxx)):
        assert rel(g, w) < TOL
    assert rel(IV.Kuu(feat, k, jitter=1e-6), Kzz) < TOL and rel(IV.Kuf(feat, k, X), Kzx) < TOL


def test_sequences_against_inducing_sequences():
    """K_seq_n_seq_covs and inducing_variables.Kuu_Kuf_Kff with InducingSequences (sequences of another length on the other side)"""
    M, N, L, d, Q = 3, 5, 11, 63, 5
    rng = np.random.default_rng(29)
    X = _data(rng, M, 1, N, L, d, False)[1]
    Zs = _data(rng, M, 1, 4, 7, d, False)[1].reshape(4, 7, d)
    for normalization in (True, False):
        k, ko = make("mixed", M, L, d, Q, normalization=normalization)
        got, want = k.K_seq_n_seq_covs(Zs, X, return_levels=True), ko.K_seq_n_seq_covs(Zs, X, return_levels=True)
        for g, w in zip(got, want):
            e = rel(levels(g), levels(w))
            print("K_seq_n_seq_covs, normalization", normalization, ":", e)
            assert e < TOL, (normalization, e)


def test_float32_is_the_rounded_float64_evaluation():
    M, T, N, L, d, Q = 3, 20, 5, 11, 63, 5
    rng = np.random.default_rng(41)
    Z, X = _data(rng, M, T, N, L, d, True)
    X32, Z32 = X.astype(np.float32), Z.astype(np.float32)
    k, _ = make("gauss", M, L, d, Q)
    K64, K32 = k.K(X32.astype(np.float64)), k.K(X32)
    assert K32.dtype == np.float32 and np.isfinite(K64).all() and np.array_equal(K32, K64.astype(np.float32))
    T64, T32 = k.K_tens_vs_seq(Z32.astype(np.float64), X32.astype(np.float64), increments=True), k.K_tens_vs_seq(Z32, X32, increments=True)
    assert T32.dtype == np.float32 and np.array_equal(T32, T64.astype(np.float32))


# ---- refusals and unchanged ground -----------------------------------------------------------------------------------------------------
def test_without_the_flag_refused_as_before():
    rng = np.random.default_rng(96)
    M, T, N, L, d, Q = 3, 5, 4, 10, 40, 2
    Z, X = _data(rng, M, T, N, L, d, False)
    k, _ = make("gauss", M, L, d, Q, wide=False)
    assert not k.spectral_wide
    for call in (lambda: k.K(X), lambda: k.Kdiag(X), lambda: k.K_tens(Z), lambda: k.K_tens_vs_seq(Z, X)):
        with pytest.raises(NotImplementedError, match="at most 32 features"):
            call()
    k.lr_spectral_wide = True                   # the low-rank switch alone does not unlock exact mode
    with pytest.raises(NotImplementedError, match="at most 32 features"):
        k.K(X)


def test_refusals_name_their_bound():
    from gpsig_amd import _lib
    rng = np.random.default_rng(97)
    M, T, N, L, d, Q = 3, 5, 4, 10, 40, 2
    Z, X = _data(rng, M, T, N, L, d, False)
    k, _ = make("gauss", M, L, d, Q, order=2)
    with pytest.raises(NotImplementedError, match="first-order sequence lattices"):
        k.K(X)
    k, _ = make("gauss", M, L, d, Q)
    assert np.isfinite(k.K(X)).all()
    with pytest.raises(NotImplementedError, match="wide = 0"):
        with_options({"wide": 0}, lambda: k.K(X))
    with pytest.raises(NotImplementedError, match="wide = 0"):
        with_options({"wide": 0}, lambda: k.K_tens_vs_seq(Z, X))
    with pytest.raises(NotImplementedError, match="wide = 0"):
        with_options({"wide": 0}, lambda: k.K_tens(Z))
    k9, _ = make("gauss", 9, L, d, Q)
    with pytest.raises(NotImplementedError, match="num_levels <= 8"):
        k9.K_tens(rng.standard_normal((45, T, d)))
    # a gradient entry point still refuses the family
    ctx = _lib.context(0, 0)
    ctx.set_pointer_mode(_lib.PTR_HOST)
    keep = []
    p = k._params(keep)
    lt = M * (M + 1) // 2
    G = np.ones((M + 1, T, N))
    gZ, gX, gb = np.zeros((lt, T, d)), np.zeros((N, L, d)), np.zeros(2)
    vp = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    with pytest.raises(ValueError, match="unknown base kernel"):        # (GPSIG_ERR_INVALID, as at every width)
        ctx.call("gpsig_tens_vs_seq_levels_grad", p, vp(Z), vp(np.ascontiguousarray(X)), T, N, L, 0, vp(G), vp(gZ), vp(gX), gb.ctypes.data_as(C.POINTER(C.c_double)))
    assert not gZ.any() and not gX.any()


@pytest.mark.parametrize("d", [32, 16])
def test_up_to_32_columns_the_flag_changes_no_bit(d):
    M, T, N, L, Q = 3, 20, 5, 11, 3
    rng = np.random.default_rng(98)
    Zs = {inc: _data(rng, M, T, N, L, d, inc)[0] for inc in (False, True)}
    X = _data(rng, M, T, N, L, d, False)[1]
    X2 = X[:3] * 1.01
    k, _ = make("mixed", M, L, d, Q, wide=False)
    without = quantities(k, X, X2, Zs)
    k.spectral_wide = True
    for qi, (a, b) in enumerate(zip(without, quantities(k, X, X2, Zs))):
        assert np.isfinite(a).all() and np.array_equal(a, b), qi
