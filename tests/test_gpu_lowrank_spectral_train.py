"""Low-rank SignatureSpectral trained through the fused feature kernels: gpsig_lr_seq_features_spectral_dev / _grad (csrc/lr_grad_api.hip,
the spectral instance of lr_seq_features_grad_kernel + the spectral cross op's reverse kernels) against the torch route of the same feature
map (autodiff._LowRankScope._seq_torch, lr_hip = False) given the same landmarks, whitening, parameters and projections."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def relerr(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    if got.size == 0:
        return 0.0
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def _set_threads(value):
    from gpsig_amd import _lib
    _lib.context(0, torch.cuda.current_stream(DEV).cuda_stream).set_option("lr_grad_threads", value)


class Setup:
    """A low-rank SignatureSpectral module (lr_hip = False), one draw, sequences, landmarks (half of them points of the sequences),
    a random whitening and the parameters as leaves."""

    def __init__(self, N, L, d, M, c, Q, family, difference=True, seed=0, r=None):
        from gpsig_amd import kernels, autodiff
        rng = np.random.default_rng(seed)
        r = c if r is None else r
        k = kernels.SignatureSpectral(L * d, d, M, family=family, Q=Q, difference=difference, low_rank=True, num_components=c,
                                      rank_bound=r)
        k.rng = np.random.default_rng(seed + 1)
        self.mod = autodiff.SignatureKernelModule(k, device=DEV)
        self.mod.lr_hip = False
        self.family, self.M, self.c = family, M, c
        X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1)
        pool = 0.7 * rng.standard_normal((2 * c + 4, d))
        self.draw = self.mod.draw_low_rank(pool.shape[0])
        self.scope = autodiff._LowRankScope(self.mod, torch.tensor(pool, device=DEV), self.draw)
        self.r = int(self.draw.sketches[0].r) if self.draw.sketches else r
        Sn = 0.7 * rng.standard_normal((c, d))
        if N * L:
            pts = X.reshape(-1, d)
            take = rng.choice(pts.shape[0], min(c // 2 + 1, pts.shape[0]), replace=False)
            Sn[: len(take)] = pts[take]                     # landmarks equal to points: zero distances
        leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
        self.X, self.S = leaf(X), leaf(Sn)
        self.Wh = leaf(rng.standard_normal((c, c)) / np.sqrt(c))
        self.al, self.om = leaf(rng.uniform(0.3, 1.2, Q)), leaf(0.3 * rng.standard_normal((Q, d)))
        self.ga = leaf(rng.uniform(0.4, 1.3, (Q, d)) / np.sqrt(d))
        self.leaves = (self.X, self.S, self.Wh, self.al, self.om, self.ga)

    def hip(self, X=None):
        from gpsig_amd import autodiff
        return autodiff._LrSeqFeaturesSpectral.apply(self.X if X is None else X, self.S, self.Wh, self.al, self.om, self.ga, self.mod._spec,
                                                     self.family, self.draw.sketches, self.r)

    def torch_route(self):
        from gpsig_amd import autodiff
        sc = self.scope
        sc.S, sc.Wh = self.S, self.Wh
        sc.mod._kappa = lambda A, B: autodiff.base_kernel_matrix("spectral", A, B, spectral=(self.family, self.al, self.om, self.ga))
        return torch.cat(sc._seq_torch(self.X), dim=1)

    def grads(self, Phi, G):
        return torch.autograd.grad(Phi, self.leaves, G, allow_unused=True)


@pytest.mark.parametrize("family", ["rbf", "exp", "mixed"])
@pytest.mark.parametrize("difference", [True, False])
def test_forward_matches_torch_route(family, difference):
    s = Setup(N=37, L=20, d=4, M=4, c=12, Q=5, family=family, difference=difference, seed=3)
    Phi = s.hip()
    want = s.torch_route()
    assert Phi.shape == want.shape == (37, 1 + 12 + 3 * s.r)
    assert relerr(Phi, want) <= 1e-11


# (M, c, d, Q, L, N, difference, family, lr_grad_threads)
REVERSE_CASES = [
    (2, 64, 32, 5, 2, 600, True, "rbf", 1024),
    (3, 7, 3, 1, 63, 600, True, "exp", 512),
    (5, 16, 4, 64, 64, 3, False, "mixed", 1024),
    (8, 16, 4, 5, 65, 37, True, "mixed", 512),
    (3, 7, 3, 2, 129, 20, True, "exp", 1024),
    (2, 7, 3, 3, 1, 9, False, "rbf", 512),
    (3, 9, 2, 4, 12, 1, True, "exp", 1024),
    (3, 7, 3, 2, 10, 0, True, "rbf", 512),
    (2, 64, 32, 5, 2, 600, True, "mixed", 512),
    (3, 7, 3, 1, 63, 600, True, "exp", 1024),
]


@pytest.mark.parametrize("M,c,d,Q,L,N,difference,family,threads", REVERSE_CASES)
def test_reverse_matches_torch_autograd(M, c, d, Q, L, N, difference, family, threads):
    s = Setup(N=N, L=L, d=d, M=M, c=c, Q=Q, family=family, difference=difference, seed=M + c + L)
    G = torch.tensor(np.random.default_rng(5).standard_normal((N, 1 + c + (M - 1) * s.r)), device=DEV)
    _set_threads(threads)
    try:
        got = s.grads(s.hip(), G)
    finally:
        _set_threads(1024)
    # (no sequences: the torch route has nothing to run on, every gradient is zero)
    want = s.grads(s.torch_route(), G) if N else [torch.zeros_like(g) for g in got]
    for name, g, w in zip(("X", "S", "Wh", "alpha", "omega", "gamma"), got, want):
        w = torch.zeros_like(g) if w is None else w
        assert relerr(g, w) <= 1e-9, (name, relerr(g, w))


def test_reverse_is_deterministic():
    s = Setup(N=700, L=30, d=5, M=4, c=20, Q=6, family="mixed", seed=11)
    G = torch.tensor(np.random.default_rng(2).standard_normal((700, 1 + 20 + 3 * s.r)), device=DEV)
    a = s.grads(s.hip(), G)
    b = s.grads(s.hip(), G)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_chunked_dkxs_matches_two_half_batches():
    # dkxs = N L c doubles: 8,400 x 63 x 64 x 8 bytes = 271 MB, above the 256 MB budget of one chunk; each half stays below it
    N, L = 8400, 63
    s = Setup(N=N, L=L, d=2, M=2, c=64, Q=2, family="exp", seed=4)
    G = torch.tensor(np.random.default_rng(6).standard_normal((N, 1 + 64 + s.r)), device=DEV)
    full = s.grads(s.hip(), G)
    h = N // 2
    X1, X2 = s.X[:h].detach().clone().requires_grad_(True), s.X[h:].detach().clone().requires_grad_(True)
    g1 = torch.autograd.grad(s.hip(X1), (X1,) + s.leaves[1:], G[:h])
    g2 = torch.autograd.grad(s.hip(X2), (X2,) + s.leaves[1:], G[h:])
    assert relerr(full[0], torch.cat([g1[0], g2[0]])) <= 1e-12
    for k in range(1, 6):
        assert relerr(full[k], g1[k] + g2[k]) <= 1e-12, k


def _module_setup(c, lr_hip, seed=77):
    from gpsig_amd import kernels, autodiff
    d, M, L, Q = 3, 3, 9, 4
    rng = np.random.default_rng(seed)
    kern = kernels.SignatureSpectral(L * d, d, M, family="mixed", Q=Q, low_rank=True, num_components=c, rank_bound=6,
                                     variances=rng.uniform(0.5, 1.5, M + 1))
    kern.alpha, kern.omega, kern.gamma = np.exp(0.3 * rng.standard_normal(Q)), 0.3 * np.exp(0.3 * rng.standard_normal((Q, d))), \
        np.exp(0.3 * rng.standard_normal((Q, d)))
    kern.rng = np.random.default_rng(5)
    mod = autodiff.SignatureKernelModule(kern, device=DEV)
    mod.lr_hip = lr_hip
    return mod, rng


def _module_loss(mod, rng, N, L=9, d=3, M=3, T=4):
    lt = M * (M + 1) // 2
    X = torch.tensor(rng.standard_normal((N, L * d)) * 0.5, device=DEV, requires_grad=True)
    Z = torch.tensor(rng.standard_normal((lt, T, 2, d)) * 0.5, device=DEV, requires_grad=True)
    dr_c, dr_k = mod.draw_low_rank(lt * T * 2 + N * L), mod.draw_low_rank(N * L)
    W1, W2, W3, Wk = (torch.tensor(rng.standard_normal(sh), device=DEV) for sh in ((T, T), (T, N), (N,), (N, N)))
    Kzz, Kzx, Kxx = mod.K_tens_n_seq_covs(Z, X, increments=True, lr=dr_c)
    Kk = mod.K(X, lr=dr_k)
    loss = (Kzz * W1).sum() + (Kzx * W2).sum() + (Kxx * W3).sum() + (Kk * Wk).sum()
    mod.zero_grad()
    loss.backward()
    return [X.grad, Z.grad] + [p.grad for p in (mod.raw_variances, mod.raw_sigma, mod.raw_alpha, mod.raw_omega, mod.raw_sgamma)]


def test_module_takes_the_new_route(monkeypatch):
    from gpsig_amd import _lib, autodiff
    names = []
    orig_call = _lib.Context.call

    def spy(self, name, params, *args):
        names.append(name)
        return orig_call(self, name, params, *args)

    def no_torch(self, Xs):
        raise AssertionError("sequence features took the torch route")

    with monkeypatch.context() as mp:
        mp.setattr(_lib.Context, "call", spy)
        mp.setattr(autodiff._LowRankScope, "_seq_torch", no_torch)
        mod, rng = _module_setup(7, True)
        got = _module_loss(mod, rng, N=8)
    assert "gpsig_lr_seq_features_spectral_dev" in names and "gpsig_lr_seq_features_spectral_grad" in names
    ref, rng2 = _module_setup(7, False)
    want = _module_loss(ref, rng2, N=8)
    for g, w in zip(got, want):
        assert relerr(g, w) <= 1e-9, relerr(g, w)
    # beyond the library's limits (65 components) the module still trains, through the torch route
    big, rng3 = _module_setup(65, True)
    grads = _module_loss(big, rng3, N=10)
    assert all(bool(torch.isfinite(g).all()) for g in grads)


def _svgp_peak_mb(base, lr_hip, N=1024, L=50, d=6, M=4, T=64, c=50, Q=5):
    from gpsig_amd import kernels, models, inducing_variables, likelihoods
    rng = np.random.default_rng(0)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    if base == "spectral":
        kern = kernels.SignatureSpectral(L * d, d, M, family="rbf", Q=Q, low_rank=True, num_components=c, rank_bound=c)
        kern.alpha, kern.omega, kern.gamma = np.ones(Q), np.full((Q, d), 0.1), np.full((Q, d), 1 / np.sqrt(d))
    else:
        kern = kernels.SignatureRBF(L * d, d, M, low_rank=True, num_components=c, rank_bound=c)
    kern.rng = np.random.default_rng(3)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=DEV)
    m.kernel.lr_hip = lr_hip
    Xt = torch.tensor(X.reshape(N, -1), device=DEV)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=DEV)

    def step():
        m.zero_grad()
        (-m.elbo(Xt, Yt)).backward()

    step()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(DEV)
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) / 2 ** 20
    del m
    torch.cuda.empty_cache()
    return peak


def test_svgp_step_memory():
    rbf = _svgp_peak_mb("rbf", True)
    spectral = _svgp_peak_mb("spectral", True)
    bound = 2 * rbf + 256
    assert spectral <= bound, (spectral, rbf)
    # the torch route of the same step does not meet the bound
    assert _svgp_peak_mb("spectral", False) > bound


def test_old_entry_point_still_refuses_spectral():
    from gpsig_amd import autodiff, _lib
    s = Setup(N=4, L=6, d=3, M=2, c=5, Q=2, family="rbf", seed=1)
    keep = []
    p = s.mod._spec.params(3, 2.0, keep)
    arr = autodiff._sketch_array(s.draw.sketches, keep)
    X, S, Wh = (autodiff._c(t) for t in (s.X, s.S, s.Wh))
    out = torch.empty((4, 1 + 5 + s.r), dtype=torch.float64, device=DEV)
    ctx = autodiff._ctx_for(X)
    with pytest.raises(NotImplementedError):
        ctx.call("gpsig_lr_seq_features_dev", p, 5, s.r, len(s.draw.sketches), arr, autodiff._ptr(X), 4, 6, autodiff._ptr(S), autodiff._ptr(Wh),
                 autodiff._ptr(out))
    assert _lib.BASE["spectral"] == p.base_kernel
