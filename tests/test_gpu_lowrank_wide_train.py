"""Low-rank training on wide state spaces: the Nystrom cross matrix as an op on the matrix cores (autodiff._LrCross, csrc/lr_cross_kernel.hpp)
followed by the feature kernels that take it from memory (autodiff._LrSeqFeaturesKx / _LrTensFeaturesKx, csrc/lr_kx_inst.hip), against the torch
route of the same maps (autodiff._LowRankScope._seq_torch / _seq_torch_ragged / _tens_torch) given the same landmarks, whitening, parameters
and projections; against the ops that take the points where both serve; and through the module and an SVGP step.

Tolerances and fixtures are those of tests/test_gpu_lowrank_long_train.py (copied, not imported): relerr = max|got - want| / max|want|, 1e-11 for
features, 1e-9 for gradients against torch autograd, 1e-12 for identities between two HIP routes; sequences and landmarks lie on a grid of 1/256
(|value| < 8) with half the landmarks copied from points, so that both routes see distance zero there (the Matern families).

The tile length at 64 rows (c = r = 64) is 64 steps of U whatever the number of columns, at 16 rows 256: L = 65 with the time difference is
one tile, 66 without it a second tile of two steps, 130 a third tile of one step; 330 at 16 rows tiles of 256 and 73 steps."""
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


def kernel_class(base):
    from gpsig_amd import kernels
    return {"linear": kernels.SignatureLinear, "rbf": kernels.SignatureRBF, "poly": kernels.SignaturePoly, "mix": kernels.SignatureMix,
            "matern32": kernels.SignatureMatern32}[base]


class Setup:
    """A low-rank module (lr_hip = False), one draw, sequences of d columns (``lengths``: the rows beyond each are NaN), landmarks (half of them
    valid points of the sequences), a random whitening and the parameters as leaves."""

    def __init__(self, N, L, d, M, c, base="rbf", difference=True, seed=0, lengths=None):
        from gpsig_amd import autodiff
        rng = np.random.default_rng(seed)
        k = kernel_class(base)(L * d, d, M, lengthscales=None, difference=difference, low_rank=True, num_components=c, rank_bound=c)
        k.rng = np.random.default_rng(seed + 1)
        self.mod = autodiff.SignatureKernelModule(k, device=DEV)
        self.mod.lr_hip = False
        self.M, self.c, self.N, self.L, self.d = M, c, N, L, d
        self.lengths = [L] * N if lengths is None else [int(l) for l in lengths]
        X = grid(np.cumsum(0.1 * rng.standard_normal((N, L, d)), axis=1))
        pool = 0.7 * rng.standard_normal((2 * c + 4, d))
        self.draw = self.mod.draw_low_rank(pool.shape[0])
        self.scope = autodiff._LowRankScope(self.mod, torch.tensor(pool, device=DEV), self.draw)
        self.r = int(self.draw.sketches[0].r) if self.draw.sketches else c
        Sn = grid(0.7 * rng.standard_normal((c, d)))
        pts = np.concatenate([X[n, :l] for n, l in enumerate(self.lengths)], axis=0)
        take = rng.choice(pts.shape[0], min(c // 2 + 1, pts.shape[0]), replace=False)
        Sn[: len(take)] = pts[take]                         # landmarks equal to valid points: zero distances
        for n, l in enumerate(self.lengths):
            X[n, l:] = np.nan
        leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
        self.X, self.S = leaf(X), leaf(Sn)
        self.Wh = leaf(rng.standard_normal((c, c)) / np.sqrt(c))
        self.lens = None if lengths is None else torch.tensor(self.lengths, dtype=torch.int32, device=DEV)
        self.leaves = (self.X, self.S, self.Wh)
        self.names = ("X", "S", "Wh")
        if self.mod.raw_p0 is not None:
            self.leaves += (self.mod.raw_p0,)
            self.names += ("base parameter",)
        self.F = 1 + c + (M - 1) * self.r

    def kx(self, X=None):
        from gpsig_amd import autodiff
        X = self.X if X is None else X
        kxs = autodiff._LrCross.apply(X.reshape(-1, self.d), self.S, self.mod.p0, self.mod._spec).reshape(X.shape[0], self.L, self.c)
        lens = None if self.lens is None else self.lens[: X.shape[0]]
        return autodiff._LrSeqFeaturesKx.apply(kxs, lens, self.Wh, self.mod._spec, self.draw.sketches, self.r)

    def fused(self):
        from gpsig_amd import autodiff
        return autodiff._LrSeqFeatures.apply(self.X, self.S, self.Wh, self.mod.p0, self.mod._spec, self.draw.sketches, self.r)

    def torch_route(self):
        sc = self.scope
        sc.S, sc.Wh = self.S, self.Wh
        return torch.cat(sc._seq_torch(self.X) if self.lens is None else sc._seq_torch_ragged(self.X, self.lens), dim=1)

    def grads(self, Phi, G, leaves=None):
        return torch.autograd.grad(Phi, self.leaves if leaves is None else leaves, G, allow_unused=True)


def check_against_torch(s, tag, Phi=None):
    G = torch.tensor(np.random.default_rng(5).standard_normal((s.N, s.F)), device=DEV)
    Phi, want = s.kx() if Phi is None else Phi, s.torch_route()
    assert Phi.shape == want.shape == (s.N, s.F)
    err = relerr(Phi, want)
    print("features", tag, err)
    got_g, want_g = s.grads(Phi, G), s.grads(want, G)
    errs = {}
    for name, g, w in zip(s.names, got_g, want_g):
        assert g is not None and w is not None, name
        errs[name] = relerr(g, w)
        print("gradient", tag, name, errs[name])
    assert err <= 1e-11, err
    for name, e in errs.items():
        assert e <= 1e-9, (name, e)
    if "base parameter" in s.names:
        assert len(got_g) == 4 and float(got_g[3].abs()) > 0
    return got_g


# (c = r, d, L, M, difference, base)
CASES = [
    (64, 130, 5, 4, True, "rbf"),
    (64, 130, 65, 4, True, "rbf"),
    (64, 130, 66, 4, False, "rbf"),
    (64, 130, 130, 2, True, "matern32"),
    (16, 300, 330, 4, True, "linear"),                      # 16 rows: tiles of 256 and 73 steps
    (50, 126, 100, 4, True, "poly"),
    (64, 65, 129, 4, False, "mix"),
]


@pytest.mark.parametrize("c,d,L,M,difference,base", CASES)
def test_values_and_gradients_match_the_torch_route(c, d, L, M, difference, base):
    s = Setup(N=3, L=L, d=d, M=M, c=c, base=base, difference=difference, seed=c + L + M)
    check_against_torch(s, (base, c, d, L, M, difference))


def test_ragged_batch():
    lengths = (130, 66, 1)
    s = Setup(N=3, L=130, d=130, M=4, c=64, seed=9, lengths=lengths)
    assert bool(torch.isnan(s.X[1, 66:]).all()) and bool(torch.isnan(s.X[2, 1:]).all())
    got_g = check_against_torch(s, ("ragged",) + lengths)
    for n, l in enumerate(lengths):
        assert bool((got_g[0][n, l:] == 0).all()), (n, l)  # padded rows: written, exactly zero
    assert float(got_g[0].abs().max()) > 0


@pytest.mark.parametrize("base", ["rbf", "matern32"])
def test_identity_with_the_ops_that_take_the_points(base):
    s = Setup(N=3, L=70, d=24, M=4, c=16, base=base, seed=21)
    a, b = s.kx(), s.fused()
    e = relerr(a, b)
    print("kx against fused", base, e)
    assert e <= 1e-12, e
    check_against_torch(s, (base, "kx"), Phi=a)
    check_against_torch(s, (base, "fused"), Phi=b)


def test_batches_split_and_the_reverse_pass_repeats():
    s = Setup(N=5, L=66, d=130, M=3, c=64, seed=4)
    G = torch.tensor(np.random.default_rng(6).standard_normal((5, s.F)), device=DEV)
    Phi = s.kx()
    full, again = s.grads(Phi, G), s.grads(s.kx(), G)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    X1, X2 = s.X[:2].detach().clone().requires_grad_(True), s.X[2:].detach().clone().requires_grad_(True)
    e = relerr(Phi, torch.cat([s.kx(X1), s.kx(X2)]))
    print("split", e)
    assert e <= 1e-12, e


class TensSetup:
    """The twin of Setup for inducing tensors (lt, T[, 2], d).  The tensors' points and the landmarks that are not copies have norm ~2 at every d:
    at the 0.6 per coordinate of tests/test_gpu_lowrank_tens_train.py (d = 3 there) two points of 130 columns are at squared distance ~94, every
    kernel value but the coincident pairs' is e^-47, and the gradient of either route is the rounding residue of the terms that cancel at those
    pairs -- nothing to compare."""

    def __init__(self, T, d, M, c, increments, base="rbf", seed=0):
        from gpsig_amd import autodiff
        rng = np.random.default_rng(seed)
        k = kernel_class(base)(10 * d, d, M, lengthscales=None, low_rank=True, num_components=c, rank_bound=c)
        k.rng = np.random.default_rng(seed + 1)
        self.mod = autodiff.SignatureKernelModule(k, device=DEV)
        self.mod.lr_hip = False
        self.M, self.c, self.d, self.T, self.increments = M, c, d, T, increments
        lt = M * (M + 1) // 2
        Z = grid(2.0 / np.sqrt(d) * rng.standard_normal((lt, T, 2, d) if increments else (lt, T, d)))
        pool = 0.7 * rng.standard_normal((2 * c + 4, d))
        self.draw = self.mod.draw_low_rank(pool.shape[0])
        self.scope = autodiff._LowRankScope(self.mod, torch.tensor(pool, device=DEV), self.draw)
        self.r = int(self.draw.sketches[0].r) if self.draw.sketches else c
        Sn = grid(2.0 / np.sqrt(d) * rng.standard_normal((c, d)))
        pts = Z.reshape(-1, d)
        take = rng.choice(pts.shape[0], min(c // 2 + 1, pts.shape[0]), replace=False)
        Sn[: len(take)] = pts[take]
        leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
        self.Z, self.S = leaf(Z), leaf(Sn)
        self.Wh = leaf(rng.standard_normal((c, c)) / np.sqrt(c))
        self.leaves, self.names = (self.Z, self.S, self.Wh), ("Z", "S", "Wh")
        self.F = 1 + c + (M - 1) * self.r

    def kx(self):
        from gpsig_amd import autodiff
        kzs = autodiff._LrCross.apply(self.Z.reshape(-1, self.d), self.S, self.mod.p0, self.mod._spec).reshape(*self.Z.shape[:-1], self.c)
        return autodiff._LrTensFeaturesKx.apply(kzs, self.Wh, self.mod._spec, self.draw.sketches, self.r, self.increments)

    def torch_route(self):
        sc = self.scope
        sc.S, sc.Wh = self.S, self.Wh
        return torch.cat(sc._tens_torch(self.Z, self.increments), dim=1)


@pytest.mark.parametrize("M,c,d,T,increments", [(4, 64, 130, 70, True), (2, 16, 300, 1, False), (4, 50, 126, 600, True)])
def test_tensor_features_match_the_torch_route(M, c, d, T, increments):
    s = TensSetup(T, d, M, c, increments, seed=M + c + T)
    G = torch.tensor(np.random.default_rng(7).standard_normal((T, s.F)), device=DEV)
    Phi, want = s.kx(), s.torch_route()
    assert Phi.shape == want.shape == (T, s.F)
    err = relerr(Phi, want)
    print("tensor features", M, c, d, T, increments, err)
    got_g, want_g = torch.autograd.grad(Phi, s.leaves, G), torch.autograd.grad(want, s.leaves, G)
    errs = {name: relerr(g, w) for name, g, w in zip(s.names, got_g, want_g)}
    print("tensor gradients", errs, "max |gradient|", [float(w.abs().max()) for w in want_g])
    assert err <= 1e-11, err
    for name, e in errs.items():
        assert e <= 1e-9, (name, e)


def _module(d, lr_hip, L=9, M=4, c=50):
    from gpsig_amd import autodiff, kernels
    kern = kernels.SignatureRBF(L * d, d, M, lengthscales=np.full(d, np.sqrt(d)), low_rank=True, num_components=c)
    kern.rng = np.random.default_rng(5)
    mod = autodiff.SignatureKernelModule(kern, device=DEV)
    mod.lr_hip = lr_hip
    return mod


def _covs(mod, d, N=7, L=9, T=40):
    rng = np.random.default_rng(31)
    M = mod.kern.num_levels
    X = torch.tensor(np.cumsum(rng.standard_normal((N, L, d)) * 0.4, axis=1).reshape(N, -1), device=DEV, requires_grad=True)
    Z = torch.tensor(rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.7, device=DEV, requires_grad=True)
    mod.kern.rng = np.random.default_rng(11)
    outs = mod.K_tens_n_seq_covs(Z, X, increments=True)
    sum(o.sum() for o in outs).backward()
    assert all(bool(torch.isfinite(t.grad).all()) for t in (X, Z))


NEW = ("gpsig_lr_cross", "gpsig_lr_seq_features_kx_dev", "gpsig_lr_tens_features_kx_dev")


def test_module_routes(monkeypatch):
    from gpsig_amd import _lib, autodiff
    names = []
    orig_call = _lib.Context.call

    def spy(self, name, params, *args):
        names.append(name)
        return orig_call(self, name, params, *args)

    def no_torch(self, *a, **kw):
        raise AssertionError("the feature map took the torch route")

    with monkeypatch.context() as mp:
        mp.setattr(_lib.Context, "call", spy)
        for f in ("_seq_torch", "_seq_torch_ragged", "_tens_torch"):
            mp.setattr(autodiff._LowRankScope, f, no_torch)
        _covs(_module(130, True), 130)
        wide = list(names)
        del names[:]
        _covs(_module(3, True), 3)
        narrow = list(names)
    for n in NEW + ("gpsig_lr_cross_grad", "gpsig_lr_seq_features_kx_grad", "gpsig_lr_tens_features_kx_grad"):
        assert n in wide, (n, wide)
    assert "gpsig_lr_seq_features_dev" in narrow and not any(n in narrow for n in NEW), narrow
    with monkeypatch.context() as mp:
        del names[:]
        mp.setattr(_lib.Context, "call", spy)
        _covs(_module(130, False), 130)
        assert not names, names


def _svgp(d, lr_hip, N=12, L=9, M=4, T=8, c=50):
    from gpsig_amd import inducing_variables, kernels, likelihoods, models
    rng = np.random.default_rng(8)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.3, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    kern = kernels.SignatureRBF(L * d, d, M, lengthscales=np.full(d, np.sqrt(d)), low_rank=True, num_components=c)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=DEV)
    m.kernel.lr_hip = lr_hip
    m.q_mu.data = torch.tensor(0.3 * rng.standard_normal((T, 1)), device=DEV)
    kern.rng = np.random.default_rng(3)                     # (the draw of the evaluation: the same in both models)
    elbo = m.elbo(torch.tensor(X.reshape(N, -1), device=DEV), torch.tensor(lab[:, None].astype(np.float64), device=DEV))
    elbo.backward()
    return elbo.detach(), {n: p.grad for n, p in m.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("d", [130, 300])
def test_svgp_step_matches_the_torch_route(d, monkeypatch):
    from gpsig_amd import _lib
    names = []
    orig_call = _lib.Context.call

    def spy(self, name, params, *args):
        names.append(name)
        return orig_call(self, name, params, *args)

    with monkeypatch.context() as mp:
        mp.setattr(_lib.Context, "call", spy)
        got, got_g = _svgp(d, True)
    assert all(n in names for n in NEW), names
    want, want_g = _svgp(d, False)
    e = abs(float(got) - float(want)) / max(1.0, abs(float(want)))
    print("elbo", d, float(got), float(want), e)
    assert e <= 1e-10, e
    assert set(got_g) == set(want_g) and len(got_g) >= 4
    for n in want_g:
        assert (got_g[n] is None) == (want_g[n] is None), n
        if want_g[n] is None:
            continue
        eg = relerr(got_g[n], want_g[n])
        print("gradient", d, n, eg)
        assert eg <= 1e-8, (n, eg)


def _raw(s, entry, c=None, nsk=None, levels=None, dtype=None, kxs_null=False):
    """a raw call of a forward kx entry point on the arrays of `s`, claiming c components / nsk sketches / `levels` levels"""
    from gpsig_amd import autodiff
    keep = []
    p = s.mod._spec.params(s.d, 0.0, keep)
    if levels is not None:
        p.num_levels = levels
    if dtype is not None:
        p.dtype = dtype
    sk = list(s.draw.sketches)
    if nsk is not None:
        sk = (sk * nsk)[:nsk]
    arr = autodiff._sketch_array(sk, keep)
    c = s.c if c is None else c
    kxs = torch.zeros((s.N, s.L, s.c), dtype=torch.float64, device=DEV)
    Wh = autodiff._c(s.Wh)
    out = torch.empty((s.N, 1 + c + len(sk) * s.r), dtype=torch.float64, device=DEV)
    ctx = autodiff._ctx_for(kxs)
    if entry == "seq":
        ctx.call("gpsig_lr_seq_features_kx_dev", p, c, s.r, len(sk), arr, None if kxs_null else autodiff._ptr(kxs), s.N, s.L, None, autodiff._ptr(Wh),
                 autodiff._ptr(out))
    else:
        ctx.call("gpsig_lr_tens_features_kx_dev", p, c, s.r, len(sk), arr, None if kxs_null else autodiff._ptr(kxs), 1, 0, autodiff._ptr(Wh),
                 autodiff._ptr(out))
    return out


@pytest.mark.parametrize("entry", ["seq", "tens"])
def test_refusals_stay_typed(entry):
    from gpsig_amd import _lib
    s = Setup(N=10, L=5, d=130, M=4, c=64, seed=1)          # (as tensors: 10 components of one point, one tensor)
    assert bool(torch.isfinite(_raw(s, entry)).all())
    with pytest.raises(NotImplementedError):
        _raw(s, entry, c=65)
    with pytest.raises(NotImplementedError):
        _raw(s, entry, nsk=9, levels=10)
    with pytest.raises(NotImplementedError):
        _raw(s, entry, dtype=_lib.F32)
    with pytest.raises(ValueError):
        _raw(s, entry, kxs_null=True)
