"""SignatureSpectral in low-rank mode (gpsig/kernels.py:239-311 with _spectral, :921-942, as the base kernel of Nystrom_map): the spectral
instances of the low-rank feature kernels, the spectral cross op of the training path (gpsig_spectral_cross / _grad) and the module /
SVGP gradients through it, against the checkers given the same random objects."""
import numpy as np
import pytest
import torch

from oracle import sigkern_oracle as O
from oracle import sigkern_oracle_torch as OT

pytestmark = pytest.mark.gpu

FAMILIES = ("rbf", "exp", "mixed")
# Given the same random objects the two sides differ by rounding only, amplified by the whitening of a landmark Gram whose small
# eigenvalues sit at the jitter (1e-6): the bound tests/test_gpu_parity.py gives the RBF kernel there, for the same reason.
LR_TOL = 1e-7


def relerr(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def _spectral_params(rng, Q, d):
    return rng.uniform(0.3, 1.2, Q), 0.3 * rng.standard_normal((Q, d)), rng.uniform(0.4, 1.3, (Q, d))


def make_kernel(L, d, M, family, Q, rng, **kw):
    from gpsig_amd import kernels
    k = kernels.SignatureSpectral(L * d, d, M, family=family, Q=Q, low_rank=True, variances=rng.uniform(0.5, 1.5, M + 1), **kw)
    k.alpha, k.omega, k.gamma = _spectral_params(rng, Q, d)
    return k


def make_oracle(k, st):
    ko = O.SignatureKernelOracle(k.input_dim, k.num_features, k.num_levels, base="spectral",
                                 normalization=k.normalization, difference=k.difference, lengthscales=None, variances=k.variances,
                                 base_params=dict(alpha=k.alpha, omega=k.omega, gamma=k.gamma, family=k.family))
    return O.LowRankOracle(ko, st.landmarks, st.jitter_diag, st.sketches)


def _seqs(rng, N, L, d):
    return np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)


def _features(k, st, A, tensors=False, increments=False):
    from gpsig_amd import kernels
    L_ = kernels._launch_f64(A)
    p = k._params(L_.keep)
    lr = st.as_c(L_.keep)
    Phi, _, _ = k._lr_features(L_, p, lr, A, tensors=tensors, increments=increments)
    return np.array(Phi)


def _with_option(name, value, fn, default):
    from gpsig_amd import _lib
    ctx = _lib.context(0, 0)
    try:
        ctx.set_option(name, value)
        return fn()
    finally:
        ctx.set_option(name, default)


def test_constructor_and_limits():
    from gpsig_amd import kernels
    rng = np.random.default_rng(1)
    L, d, M = 8, 3, 3
    k = kernels.SignatureSpectral(L * d, d, M, low_rank=True, num_components=6, rank_bound=5)
    assert k.low_rank
    with pytest.raises(NotImplementedError):
        kernels.SignatureSpectral(L * d, d, M, low_rank=True, num_lags=1)
    with pytest.raises(NotImplementedError):
        kernels.SignatureSpectral(L * d, d, M, low_rank=True, order=2)
    dbig = 33
    kb = kernels.SignatureSpectral(L * dbig, dbig, M, low_rank=True, num_components=6, rank_bound=5)
    with pytest.raises(NotImplementedError):
        kb.K(rng.standard_normal((4, L * dbig)))
    # float32: computed by the float64 kernels and rounded, as for every other family in low-rank mode
    k = make_kernel(L, d, M, "rbf", 4, rng, num_components=8, rank_bound=6)
    X = _seqs(rng, 7, L, d)
    k.rng = np.random.default_rng(2)
    st = k.draw_low_rank(X=X)
    g64 = k.K(X.astype(np.float32).astype(np.float64), lr_state=st)
    g32 = k.K(X.astype(np.float32), lr_state=st)
    assert g32.dtype == np.float32
    assert relerr(g32, g64) <= 1e-6


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("sparsity", ["sqrt", "log", "lin"])
def test_parity_given_the_same_randomness(family, sparsity):
    rng = np.random.default_rng(41 + len(family) + len(sparsity))
    N, N2, L, d, M, T, Q = 13, 7, 12, 3, 4, 5, 5
    X, Y = _seqs(rng, N, L, d), _seqs(rng, N2, L, d)
    for norm in (True, False):
        for incr in (False, True):
            Z = 0.5 * rng.standard_normal((M * (M + 1) // 2, T, 2, d) if incr else (M * (M + 1) // 2, T, d))
            k = make_kernel(L, d, M, family, Q, rng, normalization=norm, num_components=11, rank_bound=9, sparsity=sparsity)
            k.rng = np.random.default_rng(7)
            st = k.draw_low_rank(X=X, X2=Y, Z=Z, increments=incr)
            lo = make_oracle(k, st)
            assert relerr(k.K(X, lr_state=st), lo.K(X)) <= LR_TOL
            assert relerr(k.K(X, Y, lr_state=st, return_levels=True), lo.K(X, Y, return_levels=True)) <= LR_TOL
            assert relerr(k.Kdiag(X, lr_state=st), lo.Kdiag(X)) <= LR_TOL
            assert relerr(k.K_tens(Z, increments=incr, lr_state=st), lo.K_tens(Z, increments=incr)) <= LR_TOL
            assert relerr(k.K_tens_vs_seq(Z, X, increments=incr, lr_state=st, return_levels=True),
                          lo.K_tens_vs_seq(Z, X, increments=incr, return_levels=True)) <= LR_TOL
            if not incr:
                for full in (False, True):
                    got = k.K_seq_n_seq_covs(Y.reshape(N2, L, d), X, full_X2_cov=full, return_levels=True, lr_state=st)
                    want = lo.K_seq_n_seq_covs(Y, X, full_X2_cov=full, return_levels=True)
                    for g, w in zip(got, want):
                        assert relerr(g, w) <= LR_TOL, (full, norm)
    # K_tens_n_seq_covs draws its own state (as the reference draws inside the graph): the state of the same seed gives the oracle's
    k.rng = np.random.default_rng(9)
    got = k.K_tens_n_seq_covs(Z, X, increments=incr)
    k.rng = np.random.default_rng(9)
    st = k.draw_low_rank(X=X, Z=Z, increments=incr)
    lo = make_oracle(k, st)
    want = (lo.K_tens(Z, increments=incr), lo.K_tens_vs_seq(Z, X, increments=incr), lo.Kdiag(X))      # kernels.py:560-574
    for g, w in zip(got, want):
        assert relerr(g, w) <= LR_TOL


@pytest.mark.parametrize("family", FAMILIES)
def test_parity_device_draw(family):
    rng = np.random.default_rng(51)
    N, L, d, M, T, Q = 11, 10, 4, 3, 6, 4
    X = _seqs(rng, N, L, d)
    Z = 0.5 * rng.standard_normal((M * (M + 1) // 2, T, d))
    k = make_kernel(L, d, M, family, Q, rng, num_components=10, rank_bound=8)
    k.rng = np.random.default_rng(3)
    dev = torch.device("cuda:0")
    Xt, Zt = torch.tensor(X, device=dev), torch.tensor(Z, device=dev)
    st = k.draw_low_rank(X=Xt, Z=Zt)
    lo = make_oracle(k, st.export())
    assert relerr(k.K(Xt, lr_state=st), lo.K(X)) <= LR_TOL
    assert relerr(k.Kdiag(Xt, lr_state=st), lo.Kdiag(X)) <= LR_TOL
    assert relerr(k.K_tens(Zt, lr_state=st), lo.K_tens(Z)) <= LR_TOL
    assert relerr(k.K_tens_vs_seq(Zt, Xt, lr_state=st), lo.K_tens_vs_seq(Z, X)) <= LR_TOL


def _columns_agree(a, b, tol=1e-9):
    scale = np.maximum(np.abs(b).max(axis=0), 1e-300)
    return float((np.abs(a - b).max(axis=0) / scale).max()) <= tol


@pytest.mark.parametrize("L,d,c,r", [(20, 3, 12, 9), (50, 6, 50, 50), (90, 5, 20, 16), (30, 32, 16, 12)])
def test_sequence_feature_routes(L, d, c, r):
    """lr_fused = 1 (two LDS arrays where L, c, r <= 64), 2 (three arrays), 0 (one kernel per op) give the same features."""
    rng = np.random.default_rng(L + d)
    k = make_kernel(L, d, 3, "mixed", 5, rng, num_components=c, rank_bound=r)
    X = _seqs(rng, 9, L, d)
    k.rng = np.random.default_rng(4)
    st = k.draw_low_rank(X=X)
    got = {v: _with_option("lr_fused", v, lambda: _features(k, st, X), 1) for v in (1, 2, 0)}
    assert np.isfinite(got[0]).all()
    assert _columns_agree(got[1], got[0]) and _columns_agree(got[2], got[0])
    assert relerr(k.K(X, lr_state=st), make_oracle(k, st).K(X)) <= LR_TOL


@pytest.mark.parametrize("incr", [False, True])
def test_tensor_feature_routes(incr):
    rng = np.random.default_rng(61)
    M, T, d = 4, 9, 5
    k = make_kernel(10, d, M, "exp", 6, rng, num_components=14, rank_bound=10)
    Z = 0.5 * rng.standard_normal((M * (M + 1) // 2, T, 2, d) if incr else (M * (M + 1) // 2, T, d))
    k.rng = np.random.default_rng(5)
    st = k.draw_low_rank(Z=Z, increments=incr)
    fused = _with_option("lr_fused", 1, lambda: _features(k, st, Z, tensors=True, increments=incr), 1)
    multi = _with_option("lr_fused", 0, lambda: _features(k, st, Z, tensors=True, increments=incr), 1)
    assert np.isfinite(fused).all() and _columns_agree(fused, multi)


def test_parameter_update_with_one_state():
    """The parameter table is uploaded per call: a changed alpha with the same low-rank state gives the oracle's new numbers."""
    rng = np.random.default_rng(71)
    L, d, M = 12, 3, 3
    k = make_kernel(L, d, M, "rbf", 4, rng, num_components=10, rank_bound=8)
    X = _seqs(rng, 8, L, d)
    k.rng = np.random.default_rng(6)
    st = k.draw_low_rank(X=X)
    a = k.K(X, lr_state=st)
    assert relerr(a, make_oracle(k, st).K(X)) <= LR_TOL
    k.alpha = k.alpha * np.linspace(0.5, 2.0, k.Q)
    b = k.K(X, lr_state=st)
    # the state keeps the whitening it was drawn with; the features take the new alpha: the oracle of the new parameters given that whitening
    lo = make_oracle(k, st)
    lo.Wh = st.whitening
    assert relerr(b, lo.K(X)) <= LR_TOL
    assert relerr(b, a) > 1e-3
    # and a state whitened for the new parameters gives the new oracle outright
    st2 = k.low_rank_state(st.landmarks, st.jitter_diag, st.sketches)
    assert relerr(k.K(X, lr_state=st2), make_oracle(k, st2).K(X)) <= LR_TOL


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,c,d,Q", [(300, 17, 3, 5), (1000, 40, 6, 4), (70, 9, 12, 3), (257, 5, 32, 2)])
def test_spectral_cross_op(family, n, c, d, Q):
    from gpsig_amd import autodiff
    rng = np.random.default_rng(n + d)
    dev = torch.device("cuda:0")
    P = torch.tensor(0.7 * rng.standard_normal((n, d)), device=dev, requires_grad=True)
    Sn = 0.7 * rng.standard_normal((c, d))
    Sn[: c // 2] = P.detach().cpu().numpy()[rng.choice(n, c // 2, replace=False)]      # points paired with themselves
    S = torch.tensor(Sn, device=dev, requires_grad=True)
    al, om, ga = (torch.tensor(v, device=dev, requires_grad=True) for v in (rng.uniform(0.3, 1.2, Q), 0.3 * rng.standard_normal((Q, d)),
                                                                              rng.uniform(0.4, 1.3, (Q, d)) / np.sqrt(d)))
    K = autodiff._SpectralCross.apply(P, S, al, om, ga, family)
    leaves = [t.detach().cpu().clone().requires_grad_(True) for t in (P, S, al, om, ga)]
    Kw = OT.base_spectral(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], family)
    assert relerr(K, Kw) <= 1e-12
    G = rng.standard_normal((n, c))
    (K * torch.tensor(G, device=dev)).sum().backward()
    (Kw * torch.tensor(G)).sum().backward()
    for t, w in zip((P, S, al, om, ga), leaves):
        assert torch.isfinite(t.grad).all()
        assert relerr(t.grad, w.grad) <= 1e-10
    # deterministic: a second reverse pass gives the same bits
    grads = [t.grad.clone() for t in (P, S, al, om, ga)]
    for t in (P, S, al, om, ga):
        t.grad = None
    (autodiff._SpectralCross.apply(P, S, al, om, ga, family) * torch.tensor(G, device=dev)).sum().backward()
    for g, t in zip(grads, (P, S, al, om, ga)):
        assert torch.equal(g, t.grad)


def rel(a, b):
    return relerr(a, b)


@pytest.mark.parametrize("family,sparsity,normalization,difference,lr_hip", [
    ("rbf", "sqrt", True, True, True), ("exp", "lin", True, True, True), ("mixed", "log", False, True, True),
    ("rbf", "sqrt", True, False, True), ("exp", "sqrt", True, True, False), ("mixed", "sqrt", True, True, False)])
def test_low_rank_spectral_module_gradients(family, sparsity, normalization, difference, lr_hip):
    from gpsig_amd import kernels, autodiff
    d, M, L, N, N2, T, c, r, Q = 3, 3, 9, 8, 5, 4, 7, 6, 4
    rng = np.random.default_rng(77)
    kern = kernels.SignatureSpectral(L * d, d, M, family=family, Q=Q, normalization=normalization, difference=difference,
                                     variances=rng.uniform(0.5, 1.5, M + 1), low_rank=True, num_components=c, rank_bound=r, sparsity=sparsity)
    kern.alpha, kern.omega, kern.gamma = np.exp(0.3 * rng.standard_normal(Q)), 0.3 * np.exp(0.3 * rng.standard_normal((Q, d))), np.exp(0.3 * rng.standard_normal((Q, d)))
    kern.sigma = 1.2
    kern.rng = np.random.default_rng(5)
    mod = autodiff.SignatureKernelModule(kern, device="cuda:0")
    mod.lr_hip = lr_hip
    leaf = lambda t: t.detach().cpu().clone().requires_grad_(True)
    al, om, ga = leaf(autodiff.positive(mod.raw_alpha)), leaf(autodiff.positive(mod.raw_omega)), leaf(autodiff.positive(mod.raw_sgamma))
    orc = OT.LowRankTorchOracle(d, M, "spectral", variances=leaf(mod.variances), sigma=leaf(mod.sigma), lengthscales=None,
                                normalization=normalization, difference=difference, spectral=(al, om, ga, kern.family))
    lt = M * (M + 1) // 2
    X, X2 = rng.standard_normal((N, L * d)) * 0.5, rng.standard_normal((N2, L * d)) * 0.5
    dev = torch.device("cuda:0")
    cu = lambda a: torch.tensor(a, device=dev)
    for increments in (False, True):
        Z = rng.standard_normal((lt, T, 2, d) if increments else (lt, T, d)) * 0.5
        nz = lt * T * (2 if increments else 1)
        dr_c, dr_k, dr_x = mod.draw_low_rank(nz + N * L), mod.draw_low_rank(N * L), mod.draw_low_rank(N * L + N2 * L)
        W1, W2, W3 = rng.standard_normal((T, T)), rng.standard_normal((T, N)), rng.standard_normal(N)
        Wk, Wc = rng.standard_normal((N, N)), rng.standard_normal((N, N2))
        Zg, Xg = torch.tensor(Z, device=dev, requires_grad=True), torch.tensor(X, device=dev, requires_grad=True)
        Kzz, Kzx, Kxx = mod.K_tens_n_seq_covs(Zg, Xg, increments=increments, lr=dr_c)
        Kk, Kc = mod.K(Xg, lr=dr_k), mod.K(Xg, cu(X2), lr=dr_x)
        loss = (Kzz * cu(W1)).sum() + (Kzx * cu(W2)).sum() + (Kxx * cu(W3)).sum() + (Kk * cu(Wk)).sum() + (Kc * cu(Wc)).sum()
        mod.zero_grad()
        loss.backward()
        Zc, Xc = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
        for t in (orc.variances, orc.sigma, al, om, ga):
            t.grad = None
        oKzz, oKzx, oKxx = orc.set_draw(dr_c.idx, dr_c.jitter_diag, dr_c.sketches).K_tens_n_seq_covs(Zc, Xc, increments=increments)
        oKk = orc.set_draw(dr_k.idx, dr_k.jitter_diag, dr_k.sketches).K(Xc)
        oKc = orc.set_draw(dr_x.idx, dr_x.jitter_diag, dr_x.sketches).K(Xc, torch.tensor(X2))
        oloss = (oKzz * torch.tensor(W1)).sum() + (oKzx * torch.tensor(W2)).sum() + (oKxx * torch.tensor(W3)).sum() + \
                (oKk * torch.tensor(Wk)).sum() + (oKc * torch.tensor(Wc)).sum()
        oloss.backward()
        for a, b in ((Kzz, oKzz), (Kzx, oKzx), (Kxx, oKxx), (Kk, oKk), (Kc, oKc)):
            assert rel(a, b) < 1e-8, (increments, rel(a, b))
        assert rel(Zg.grad, Zc.grad) < 1e-6 and rel(Xg.grad, Xc.grad) < 1e-6, (rel(Zg.grad, Zc.grad), rel(Xg.grad, Xc.grad))
        for raw, con in ((mod.raw_variances, orc.variances), (mod.raw_sigma, orc.sigma), (mod.raw_alpha, al), (mod.raw_omega, om),
                         (mod.raw_sgamma, ga)):
            jac = torch.sigmoid(raw.detach().cpu())
            assert rel(raw.grad, con.grad * jac) < 1e-6, (raw.shape, rel(raw.grad, con.grad * jac))


def test_low_rank_spectral_svgp_trains():
    from gpsig_amd import kernels, models, inducing_variables, likelihoods
    rng = np.random.default_rng(8)
    N, L, d, M, T = 40, 12, 2, 3, 6
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.3, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    kern = kernels.SignatureSpectral(L * d, d, M, family="mixed", Q=4, low_rank=True, num_components=10, rank_bound=8)
    kern.alpha, kern.omega, kern.gamma = np.ones(4), 0.2 * np.ones((4, d)), np.ones((4, d))
    kern.rng = np.random.default_rng(3)
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    feat = inducing_variables.InducingTensors(Z, M, increments=True)
    m = models.SVGPModule(kern, feat, likelihoods.Bernoulli(), num_data=N, device="cuda:0")
    Xt = torch.tensor(X.reshape(N, -1), device="cuda:0")
    Yt = torch.tensor(lab[:, None].astype(np.float64), device="cuda:0")
    loss = -m.elbo(Xt, Yt)
    loss.backward()
    names = []
    for n_, p_ in m.named_parameters():
        if p_.requires_grad:
            assert p_.grad is not None and bool(torch.isfinite(p_.grad).all()), n_
            names.append(n_)
    assert any("raw_alpha" in n_ for n_ in names) and any("raw_omega" in n_ for n_ in names) and any("raw_sgamma" in n_ for n_ in names)
    trace = m.fit(Xt, Yt, iterations=30, lr=5e-2)
    assert np.isfinite(trace).all() and np.mean(trace[-5:]) > np.mean(trace[:5])
