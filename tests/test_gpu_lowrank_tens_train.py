"""The low-rank feature map of inducing tensors trained through the fused HIP kernels: gpsig_lr_tens_features_dev / _grad and the spectral pair
(csrc/lr_grad_api.hip, lr_tens_grad_kernel.hpp; the spectral instance + the spectral cross op's reverse kernels) against the torch route of
the same feature map (autodiff._LowRankScope._tens_torch) given the same landmarks, whitening, parameters and projections.

Tensors and landmarks are drawn on a grid of 1/256 (|value| < 8): every product and sum of the torch route's squared distance
(-2 <z, s> + |z|^2 + |s|^2 by a GEMM and two reductions) is then exact in float64, so a landmark copied from a tensor's point is at distance
exactly zero in BOTH routes.  With unrestricted values the torch route's distance there is rounding noise of 1e-16, its square root 1e-8:
the Matern families of the reference route itself would be off by that much, in the values and far more in the gradients."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SPECTRAL = ("rbf", "exp", "mixed")                       # SignatureSpectral's families (as `base`: "spectral:<family>")
BASES = ("linear", "rbf", "cosine", "poly", "mix", "matern12", "matern32", "matern52")
DKX_BUDGET = 256 << 20                                   # LR_SPECTRAL_DKXS_BUDGET of csrc/lr_grad_api.hip: bytes of dkx per chunk of tensors


def relerr(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    if got.size == 0:
        return 0.0
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def grid(a):
    return np.clip(np.round(np.asarray(a) * 256.0) / 256.0, -7.0, 7.0)


class Setup:
    """A low-rank module (lr_hip = False), one draw, inducing tensors, landmarks (half of them points of the tensors), a random whitening
    and the parameters as leaves."""

    def __init__(self, T, d, M, c, base="rbf", Q=5, increments=True, seed=0, r=None):
        from gpsig_amd import kernels, autodiff
        rng = np.random.default_rng(seed)
        r = c if r is None else r
        kw = dict(low_rank=True, num_components=c, rank_bound=r)
        self.family = base.split(":")[1] if base.startswith("spectral") else None
        if self.family:
            k = kernels.SignatureSpectral(2 * d, d, M, family=self.family, Q=Q, **kw)
        else:
            cls = {"linear": kernels.SignatureLinear, "rbf": kernels.SignatureRBF, "cosine": kernels.SignatureCosine, "poly": kernels.SignaturePoly,
                   "mix": kernels.SignatureMix, "matern12": kernels.SignatureMatern12, "matern32": kernels.SignatureMatern32,
                   "matern52": kernels.SignatureMatern52}[base]
            k = cls(2 * d, d, M, lengthscales=None, **kw)
        k.rng = np.random.default_rng(seed + 1)
        self.mod = autodiff.SignatureKernelModule(k, device=DEV)
        self.mod.lr_hip = False
        self.M, self.c, self.increments = M, c, increments
        lt, E = M * (M + 1) // 2, 2 if increments else 1
        Z = grid(0.6 * rng.standard_normal((lt, T, E, d) if increments else (lt, T, d)))
        pool = 0.7 * rng.standard_normal((2 * c + 4, d))
        self.draw = self.mod.draw_low_rank(pool.shape[0])
        self.scope = autodiff._LowRankScope(self.mod, torch.tensor(pool, device=DEV), self.draw)
        self.r = int(self.draw.sketches[0].r) if self.draw.sketches else r
        Sn = grid(0.7 * rng.standard_normal((c, d)))
        if T:
            pts = Z.reshape(-1, d)
            take = rng.choice(pts.shape[0], min(c // 2 + 1, pts.shape[0]), replace=False)
            Sn[: len(take)] = pts[take]                     # landmarks equal to points: zero distances
        leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
        self.Z, self.S = leaf(Z), leaf(Sn)
        self.Wh = leaf(rng.standard_normal((c, c)) / np.sqrt(c))
        self.leaves = (self.Z, self.S, self.Wh)
        if self.family:
            self.al, self.om = leaf(rng.uniform(0.3, 1.2, Q)), leaf(0.3 * rng.standard_normal((Q, d)))
            self.ga = leaf(rng.uniform(0.4, 1.3, (Q, d)) / np.sqrt(d))
            self.leaves += (self.al, self.om, self.ga)
        elif self.mod.raw_p0 is not None:
            self.leaves += (self.mod.raw_p0,)
        self.F = 1 + c + (M - 1) * self.r

    def hip(self, Z=None):
        from gpsig_amd import autodiff
        Z = self.Z if Z is None else Z
        if self.family:
            return autodiff._LrTensFeaturesSpectral.apply(Z, self.S, self.Wh, self.al, self.om, self.ga, self.mod._spec, self.family,
                                                          self.draw.sketches, self.r, self.increments)
        return autodiff._LrTensFeatures.apply(Z, self.S, self.Wh, self.mod.p0, self.mod._spec, self.draw.sketches, self.r, self.increments)

    def torch_route(self):
        from gpsig_amd import autodiff
        sc = self.scope
        sc.S, sc.Wh = self.S, self.Wh
        if self.family:
            sc.mod._kappa = lambda A, B: autodiff.base_kernel_matrix("spectral", A, B, spectral=(self.family, self.al, self.om, self.ga))
        return torch.cat(sc._tens_torch(self.Z, self.increments), dim=1)

    def grads(self, Phi, G, leaves=None):
        return torch.autograd.grad(Phi, self.leaves if leaves is None else leaves, G, allow_unused=True)


@pytest.mark.parametrize("base", BASES + tuple("spectral:" + f for f in SPECTRAL))
@pytest.mark.parametrize("increments", [True, False])
def test_forward_matches_torch_route(base, increments):
    s = Setup(T=37, d=4, M=4, c=12, base=base, increments=increments, seed=3)
    Phi = s.hip()
    want = s.torch_route()
    assert Phi.shape == want.shape == (37, 1 + 12 + 3 * s.r)
    err = relerr(Phi, want)
    print("forward", base, increments, err)
    assert err <= 1e-11


# (M, c, r, d, Q, T, increments, base)
REVERSE_CASES = [
    (1, 7, 7, 3, 0, 37, True, "rbf"),                       # no projection, one component
    (2, 64, 64, 32, 0, 600, True, "rbf"),                   # the widest tables; more tensors than workgroups: the stride loop, the partial reduce
    (8, 64, 64, 32, 0, 3, True, "rbf"),                     # 36 components of 2 x 64 x 32: the largest footprint the kernel is built for
    (8, 16, 12, 4, 0, 5, False, "matern12"),                # r < c; 28 chained projections
    (3, 7, 20, 3, 0, 1, True, "linear"),                    # r > c; one tensor
    (3, 7, 6, 3, 0, 0, True, "rbf"),                        # no tensors
    (2, 7, 7, 3, 0, 600, False, "matern12"),
    (4, 12, 9, 4, 0, 37, False, "linear"),
    (3, 7, 20, 3, 1, 600, True, "spectral:exp"),
    (5, 16, 12, 4, 64, 3, False, "spectral:mixed"),
    (2, 64, 64, 32, 1, 37, True, "spectral:mixed"),
    (8, 16, 16, 4, 64, 1, True, "spectral:exp"),
    (3, 7, 6, 3, 1, 0, False, "spectral:exp"),
]


@pytest.mark.parametrize("M,c,r,d,Q,T,increments,base", REVERSE_CASES)
def test_reverse_matches_torch_autograd(M, c, r, d, Q, T, increments, base):
    s = Setup(T=T, d=d, M=M, c=c, r=r, base=base, Q=Q, increments=increments, seed=M + c + T)
    G = torch.tensor(np.random.default_rng(5).standard_normal((T, s.F)), device=DEV)
    got = s.grads(s.hip(), G)
    # (no tensors: the torch route has nothing to run on, every gradient is zero)
    want = s.grads(s.torch_route(), G) if T else [torch.zeros_like(g) if g is not None else None for g in got]
    assert len(got) == len(s.leaves)
    for k, (g, w) in enumerate(zip(got, want)):
        if g is None and w is None:                      # (the base parameter of a family whose kappa does not depend on it)
            continue
        g = torch.zeros_like(s.leaves[k]) if g is None else g
        w = torch.zeros_like(g) if w is None else w
        err = relerr(g, w)
        print("reverse", base, M, c, r, d, T, "leaf", k, err)
        assert err <= 1e-9, (k, err)


@pytest.mark.parametrize("base,Q", [("poly", 0), ("mix", 0)])
def test_reverse_reaches_the_base_parameter(base, Q):
    s = Setup(T=37, d=4, M=3, c=12, r=9, base=base, increments=True, seed=9)
    G = torch.tensor(np.random.default_rng(5).standard_normal((37, s.F)), device=DEV)
    got, want = s.grads(s.hip(), G), s.grads(s.torch_route(), G)
    assert len(got) == 4 and got[3] is not None and float(got[3].abs()) > 0
    for g, w in zip(got, want):
        assert relerr(g, w) <= 1e-9, relerr(g, w)


@pytest.mark.parametrize("base", ["matern12", "spectral:mixed"])
def test_reverse_is_deterministic(base):
    s = Setup(T=700, d=5, M=4, c=20, base=base, Q=6, seed=11)
    G = torch.tensor(np.random.default_rng(2).standard_normal((700, s.F)), device=DEV)
    a = s.grads(s.hip(), G)
    b = s.grads(s.hip(), G)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_chunked_dkx_matches_two_half_batches():
    # dkx = lt T E c doubles; M = 8 (lt = 36), increments, c = 64: 36,864 bytes per tensor, so 7,282 tensors are the first count above the
    # 256 MB budget of one chunk (the smallest lt T E c above it at the widest tensor the kernel is built for); each half stays below it
    M, c, E = 8, 64, 2
    per_tensor = (M * (M + 1) // 2) * E * c * 8
    T = DKX_BUDGET // per_tensor + 1
    T += T % 2
    assert (T - 2) * per_tensor <= DKX_BUDGET < T * per_tensor and T // 2 * per_tensor <= DKX_BUDGET
    s = Setup(T=T, d=2, M=M, c=c, r=8, base="spectral:exp", Q=2, seed=4)
    G = torch.tensor(np.random.default_rng(6).standard_normal((T, s.F)), device=DEV)
    full = s.grads(s.hip(), G)
    h = T // 2
    Z1, Z2 = s.Z[:, :h].detach().clone().requires_grad_(True), s.Z[:, h:].detach().clone().requires_grad_(True)
    g1 = torch.autograd.grad(s.hip(Z1), (Z1,) + s.leaves[1:], G[:h])
    g2 = torch.autograd.grad(s.hip(Z2), (Z2,) + s.leaves[1:], G[h:])
    assert relerr(full[0], torch.cat([g1[0], g2[0]], dim=1)) <= 1e-12
    for k in range(1, 6):
        assert relerr(full[k], g1[k] + g2[k]) <= 1e-12, k


def _module_setup(base, c, lr_hip, seed=77):
    from gpsig_amd import kernels, autodiff
    d, M, L, Q = 3, 3, 9, 4
    rng = np.random.default_rng(seed)
    kw = dict(low_rank=True, num_components=c, rank_bound=6, variances=rng.uniform(0.5, 1.5, M + 1))
    if base == "spectral":
        kern = kernels.SignatureSpectral(L * d, d, M, family="mixed", Q=Q, **kw)
        kern.alpha, kern.omega, kern.gamma = np.exp(0.3 * rng.standard_normal(Q)), 0.3 * np.exp(0.3 * rng.standard_normal((Q, d))), \
            np.exp(0.3 * rng.standard_normal((Q, d)))
    else:
        kern = kernels.SignatureRBF(L * d, d, M, lengthscales=rng.uniform(0.8, 1.5, d), **kw)
    kern.rng = np.random.default_rng(5)
    mod = autodiff.SignatureKernelModule(kern, device=DEV)
    mod.lr_hip = lr_hip
    return mod, rng


def _module_loss(mod, rng, N, L=9, d=3, M=3, T=4):
    lt = M * (M + 1) // 2
    X = torch.tensor(rng.standard_normal((N, L * d)) * 0.5, device=DEV, requires_grad=True)
    Z = torch.tensor(rng.standard_normal((lt, T, 2, d)) * 0.5, device=DEV, requires_grad=True)
    dr_c, dr_z = mod.draw_low_rank(lt * T * 2 + N * L), mod.draw_low_rank(lt * T * 2)
    W1, W2, W3, Wz = (torch.tensor(rng.standard_normal(sh), device=DEV) for sh in ((T, T), (T, N), (N,), (T, T)))
    Kzz, Kzx, Kxx = mod.K_tens_n_seq_covs(Z, X, increments=True, lr=dr_c)
    Kz = mod.K_tens(Z, increments=True, lr=dr_z)
    loss = (Kzz * W1).sum() + (Kzx * W2).sum() + (Kxx * W3).sum() + (Kz * Wz).sum()
    mod.zero_grad()
    loss.backward()
    return [X.grad, Z.grad] + [p.grad for p in mod.parameters() if p.grad is not None]


@pytest.mark.parametrize("base", ["rbf", "spectral"])
def test_module_takes_the_new_route(base, monkeypatch):
    from gpsig_amd import _lib, autodiff
    names = []
    orig_call = _lib.Context.call

    def spy(self, name, params, *args):
        names.append(name)
        return orig_call(self, name, params, *args)

    def no_torch(self, Zs, increments):
        raise AssertionError("tensor features took the torch route")

    with monkeypatch.context() as mp:
        mp.setattr(_lib.Context, "call", spy)
        mp.setattr(autodiff._LowRankScope, "_tens_torch", no_torch)
        mod, rng = _module_setup(base, 7, True)
        got = _module_loss(mod, rng, N=8)
    sfx = "_spectral" if base == "spectral" else ""
    assert "gpsig_lr_tens_features%s_dev" % sfx in names and "gpsig_lr_tens_features%s_grad" % sfx in names
    ref, rng2 = _module_setup(base, 7, False)
    want = _module_loss(ref, rng2, N=8)
    assert len(got) == len(want) >= 4
    for g, w in zip(got, want):
        assert relerr(g, w) <= 1e-9, relerr(g, w)
    # beyond the library's limits (65 components) the module still trains, through the torch route
    big, rng3 = _module_setup(base, 65, True)
    grads = _module_loss(big, rng3, N=10, T=8)
    assert all(bool(torch.isfinite(g).all()) for g in grads)


def _raw_call(s, c, ctx=None):
    """gpsig_lr_tens_features_dev on the arrays of `s` claiming `c` components"""
    from gpsig_amd import autodiff
    keep = []
    p = s.mod._spec.params(3, 0.0, keep)
    arr = autodiff._sketch_array(s.draw.sketches, keep)
    Z, S, Wh = (autodiff._c(t) for t in (s.Z, s.S, s.Wh))
    out = torch.empty((4, 1 + c + s.r), dtype=torch.float64, device=DEV)
    ctx = autodiff._ctx_for(Z) if ctx is None else ctx
    ctx.call("gpsig_lr_tens_features_dev", p, c, s.r, len(s.draw.sketches), arr, autodiff._ptr(Z), 4, 1, autodiff._ptr(S), autodiff._ptr(Wh),
             autodiff._ptr(out))
    return out


def test_refusals():
    from gpsig_amd import _lib
    s = Setup(T=4, d=3, M=2, c=5, base="rbf", seed=1)
    assert bool(torch.isfinite(_raw_call(s, 5)).all())
    # a context in host-pointer mode (a context of its own: the shared ones stay in device-pointer mode)
    host = _lib.Context(0, 0)
    try:
        host.set_pointer_mode(_lib.PTR_HOST)
        with pytest.raises(ValueError):
            _raw_call(s, 5, host)
    finally:
        host.close()
    # 65 components: beyond the reverse pass's tables (the arrays are never read)
    big = Setup(T=4, d=3, M=2, c=65, base="rbf", seed=1)
    with pytest.raises(NotImplementedError):
        _raw_call(big, 65)
