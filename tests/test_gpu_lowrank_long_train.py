"""Low-rank training on sequences whose (width, L) arrays exceed the LDS: the time-tiled feature kernels (csrc/lr_tiled_kernel.hpp, planned
by csrc/lr_tile_plan.hpp) behind gpsig_lr_seq_features_dev / _grad, against the torch route of the same feature map
(autodiff._LowRankScope._seq_torch, lr_hip = False) given the same landmarks, whitening, parameters and projections.

Tolerances are those of tests/test_gpu_lowrank_tens_train.py: relerr = max|got - want| / max|want|, 1e-11 for features, 1e-9 for gradients
against torch autograd, 1e-12 for the batch-split identity.  As there, sequences and landmarks lie on a grid of 1/256 (|value| < 8): the torch
route's squared distance is then exact, so that a landmark copied from a point is at distance zero in both routes (the Matern families).

The tile length at 64 rows (c = r = 64) is 64 steps of U, at 16 rows 256.  With the time difference a sequence of L points has L - 1 steps:
L = 65 is one tile, 66 a second tile of one step, 129 exactly two tiles, 130 a third tile of one step, 193 exactly three, and without the
difference 65, 129 and 193 are the lengths with a last tile of one step, 128 the exact multiple: three to four tiles at the upper end."""
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


def grid(a):
    return np.clip(np.round(np.asarray(a) * 256.0) / 256.0, -7.0, 7.0)


class Setup:
    """A low-rank module (lr_hip = False), one draw, sequences, landmarks (half of them points of the sequences), a random whitening and the
    parameters as leaves."""

    def __init__(self, N, L, d, M, c, base="rbf", difference=True, seed=0):
        from gpsig_amd import kernels, autodiff
        rng = np.random.default_rng(seed)
        cls = {"linear": kernels.SignatureLinear, "rbf": kernels.SignatureRBF, "poly": kernels.SignaturePoly,
               "matern32": kernels.SignatureMatern32}[base]
        k = cls(L * d, d, M, lengthscales=None, difference=difference, low_rank=True, num_components=c, rank_bound=c)
        k.rng = np.random.default_rng(seed + 1)
        self.mod = autodiff.SignatureKernelModule(k, device=DEV)
        self.mod.lr_hip = False
        self.M, self.c = M, c
        X = grid(np.cumsum(0.1 * rng.standard_normal((N, L, d)), axis=1))
        pool = 0.7 * rng.standard_normal((2 * c + 4, d))
        self.draw = self.mod.draw_low_rank(pool.shape[0])
        self.scope = autodiff._LowRankScope(self.mod, torch.tensor(pool, device=DEV), self.draw)
        self.r = int(self.draw.sketches[0].r) if self.draw.sketches else c
        Sn = grid(0.7 * rng.standard_normal((c, d)))
        pts = X.reshape(-1, d)
        take = rng.choice(pts.shape[0], min(c // 2 + 1, pts.shape[0]), replace=False)
        Sn[: len(take)] = pts[take]                         # landmarks equal to points: zero distances
        leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
        self.X, self.S = leaf(X), leaf(Sn)
        self.Wh = leaf(rng.standard_normal((c, c)) / np.sqrt(c))
        self.leaves = (self.X, self.S, self.Wh)
        self.names = ("X", "S", "Wh")
        if self.mod.raw_p0 is not None:
            self.leaves += (self.mod.raw_p0,)
            self.names += ("base parameter",)
        self.F = 1 + c + (M - 1) * self.r

    def hip(self, X=None):
        from gpsig_amd import autodiff
        return autodiff._LrSeqFeatures.apply(self.X if X is None else X, self.S, self.Wh, self.mod.p0, self.mod._spec, self.draw.sketches, self.r)

    def torch_route(self):
        sc = self.scope
        sc.S, sc.Wh = self.S, self.Wh
        return torch.cat(sc._seq_torch(self.X), dim=1)

    def grads(self, Phi, G, leaves=None):
        return torch.autograd.grad(Phi, self.leaves if leaves is None else leaves, G, allow_unused=True)


# (c = r, L, M, difference, base)
CASES = [(64, L, 4, diff, "rbf") for L in (65, 66, 128, 129, 130, 193) for diff in (True, False)] + [
    (64, 130, 2, True, "rbf"),
    (64, 129, 2, False, "rbf"),
    (16, 330, 4, True, "rbf"),                              # 16 rows: tiles of 256 steps, the second one of 73
    (16, 330, 2, False, "rbf"),
    (50, 100, 4, True, "rbf"),                              # the whole-sequence forward kernel with the tiled reverse pass
    (64, 130, 4, True, "matern32"),
    (64, 130, 4, True, "linear"),
    (64, 130, 4, True, "poly"),
]


@pytest.mark.parametrize("c,L,M,difference,base", CASES)
def test_values_and_gradients_match_the_torch_route(c, L, M, difference, base):
    s = Setup(N=3, L=L, d=3, M=M, c=c, base=base, difference=difference, seed=c + L + M)
    G = torch.tensor(np.random.default_rng(5).standard_normal((3, s.F)), device=DEV)
    Phi, want = s.hip(), s.torch_route()
    assert Phi.shape == want.shape == (3, s.F)
    err = relerr(Phi, want)
    print("features", base, c, L, M, difference, err)
    got_g, want_g = s.grads(Phi, G), s.grads(want, G)
    errs = {}
    for name, g, w in zip(s.names, got_g, want_g):
        assert g is not None and w is not None, name
        errs[name] = relerr(g, w)
        print("gradient", base, c, L, M, difference, name, errs[name])
    assert err <= 1e-11, err
    for name, e in errs.items():
        assert e <= 1e-9, (name, e)
    if base == "poly":
        assert len(got_g) == 4 and float(got_g[3].abs()) > 0


def _raw_calls(s, c, N, L):
    """gpsig_lr_seq_features_dev and _grad on the arrays of `s` claiming `c` components"""
    from gpsig_amd import autodiff
    import ctypes as C
    keep = []
    p = s.mod._spec.params(3, 0.0, keep)
    arr = autodiff._sketch_array(s.draw.sketches, keep)
    X, S, Wh = (autodiff._c(t.detach()) for t in (s.X, s.S, s.Wh))
    F = 1 + c + (s.M - 1) * s.r
    out = torch.empty((N, F), dtype=torch.float64, device=DEV)
    ctx = autodiff._ctx_for(X)
    ctx.call("gpsig_lr_seq_features_dev", p, c, s.r, len(s.draw.sketches), arr, autodiff._ptr(X), N, L, autodiff._ptr(S), autodiff._ptr(Wh),
             autodiff._ptr(out))
    G = torch.ones((N, F), dtype=torch.float64, device=DEV)
    gX, gS, gWh = torch.empty_like(X), torch.empty_like(S), torch.empty_like(Wh)
    gb = torch.zeros(2, dtype=torch.float64, device=DEV)
    ctx.call("gpsig_lr_seq_features_grad", p, c, s.r, len(s.draw.sketches), arr, autodiff._ptr(X), N, L, autodiff._ptr(S), autodiff._ptr(Wh),
             autodiff._ptr(G), autodiff._ptr(gX), autodiff._ptr(gS), autodiff._ptr(gWh), C.cast(gb.data_ptr(), C.POINTER(C.c_double)))
    return out, gX, gS, gWh


def test_library_serves_a_long_sequence():
    s = Setup(N=3, L=130, d=3, M=4, c=64, seed=2)
    out, gX, gS, gWh = _raw_calls(s, 64, 3, 130)             # (Context.call raises unless the library returns 0)
    assert all(bool(torch.isfinite(t).all()) for t in (out, gX, gS, gWh))
    assert bool((out[:, 0] == 1).all()) and float(gX.abs().max()) > 0


def _module_setup(base, c, lr_hip, L, seed=77):
    from gpsig_amd import kernels, autodiff
    d, M, Q = 3, 3, 4
    rng = np.random.default_rng(seed)
    kw = dict(low_rank=True, num_components=c, rank_bound=c, variances=rng.uniform(0.5, 1.5, M + 1))
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


def _module_loss(mod, rng, N, L, d=3):
    X = torch.tensor(np.cumsum(rng.standard_normal((N, L, d)) * 0.1, axis=1).reshape(N, L * d), device=DEV, requires_grad=True)
    draw = mod.draw_low_rank(N * L)
    W = torch.tensor(rng.standard_normal((N, N)), device=DEV)
    mod.zero_grad()
    (mod.K(X, lr=draw) * W).sum().backward()
    return [X.grad] + [p.grad for p in mod.parameters() if p.grad is not None]


def test_module_takes_the_tiled_route(monkeypatch):
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
        mod, rng = _module_setup("rbf", 64, True, L=130)
        got = _module_loss(mod, rng, N=4, L=130)
    assert "gpsig_lr_seq_features_dev" in names and "gpsig_lr_seq_features_grad" in names
    ref, rng2 = _module_setup("rbf", 64, False, L=130)
    want = _module_loss(ref, rng2, N=4, L=130)
    assert len(got) == len(want) >= 3
    for g, w in zip(got, want):
        assert relerr(g, w) <= 1e-9, relerr(g, w)


def test_carries_reset_between_sequences_and_batches_split():
    # 600 sequences on at most 512 workgroups: some take two, each of two tiles (65 steps)
    N, L, c = 600, 66, 64
    s = Setup(N=N, L=L, d=3, M=3, c=c, seed=4)
    G = torch.tensor(np.random.default_rng(6).standard_normal((N, s.F)), device=DEV)
    Phi = s.hip()
    full = s.grads(Phi, G)
    again = s.grads(s.hip(), G)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    h = N // 2
    X1, X2 = s.X[:h].detach().clone().requires_grad_(True), s.X[h:].detach().clone().requires_grad_(True)
    P1, P2 = s.hip(X1), s.hip(X2)
    assert torch.equal(Phi, torch.cat([P1, P2]))
    g1 = torch.autograd.grad(P1, (X1,) + s.leaves[1:], G[:h])
    g2 = torch.autograd.grad(P2, (X2,) + s.leaves[1:], G[h:])
    assert torch.equal(full[0], torch.cat([g1[0], g2[0]]))
    for k in (1, 2):
        err = relerr(full[k], g1[k] + g2[k])
        print("split", s.names[k], err)
        assert err <= 1e-12, (k, err)


def test_refusals_stay_typed(monkeypatch):
    from gpsig_amd import autodiff
    # 65 components: beyond the reverse pass's tables, whatever the length
    big = Setup(N=3, L=130, d=3, M=2, c=65, seed=1)
    with pytest.raises(NotImplementedError):
        _raw_calls(big, 65, 3, 130)
    # SignatureSpectral keeps its whole-sequence limit: at L = 130 and 64 components it trains through the torch route
    calls = []
    orig = autodiff._LowRankScope._seq_torch

    def spy(self, Xs):
        calls.append(tuple(Xs.shape))
        return orig(self, Xs)

    monkeypatch.setattr(autodiff._LowRankScope, "_seq_torch", spy)
    mod, rng = _module_setup("spectral", 64, True, L=130)
    grads = _module_loss(mod, rng, N=4, L=130)
    assert calls and calls[0][1] == 130
    assert all(bool(torch.isfinite(g).all()) for g in grads)
