"""Low-rank SignatureSpectral on long and ragged batches: gpsig_lr_seq_features_spectral_ragged_dev / _ragged_grad (csrc/lr_grad_api.hip: the
lengths-aware spectral instances of the whole-sequence and the time-tiled feature kernels, csrc/lr_spectral_tiled_inst.hip, and the lengths-aware
reverse kernels of the spectral cross op) against the torch route of the same feature map (autodiff._LowRankScope._seq_torch / _seq_torch_ragged,
lr_hip = False) given the same landmarks, whitening, parameters and projections.

relerr = max|got - want| / max|want|.  Tolerances, the project's own for these comparisons (test_gpu_lowrank_long_train.py,
test_gpu_lowrank_ragged.py): 1e-11 for features against the torch route, 1e-9 for gradients against torch autograd, 1e-12 between two runs of
the library that sum the same terms in another grouping; torch.equal where the library promises the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = ("X", "S", "Wh", "alpha", "omega", "gamma")
ENTRY = ("gpsig_lr_seq_features_spectral_ragged_dev", "gpsig_lr_seq_features_spectral_ragged_grad")


def relerr(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    if got.size == 0:
        return 0.0
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


class Setup:
    """A low-rank SignatureSpectral module (lr_hip = False: the torch checker), one draw, sequences, landmarks (half of them valid points of the
    sequences: zero distances, which the "exp" envelope's derivative has to survive), a random whitening and the parameters as leaves.  With
    `lengths` the rows beyond each sequence's length are NaN."""

    def __init__(self, N, L, d, M, c, Q, family, difference=True, seed=0, lengths=None):
        from gpsig_amd import kernels, autodiff
        rng = np.random.default_rng(seed)
        k = kernels.SignatureSpectral(L * d, d, M, family=family, Q=Q, difference=difference, low_rank=True, num_components=c, rank_bound=c)
        k.rng = np.random.default_rng(seed + 1)
        self.mod = autodiff.SignatureKernelModule(k, device=DEV)
        self.mod.lr_hip = False
        self.family, self.M, self.c, self.N, self.L, self.d = family, M, c, N, L, d
        self.lengths = [L] * N if lengths is None else [int(l) for l in lengths]
        X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1)
        pool = 0.7 * rng.standard_normal((2 * c + 4, d))
        self.draw = self.mod.draw_low_rank(pool.shape[0])
        self.scope = autodiff._LowRankScope(self.mod, torch.tensor(pool, device=DEV), self.draw)
        self.r = int(self.draw.sketches[0].r) if self.draw.sketches else c
        Sn = 0.7 * rng.standard_normal((c, d))
        pts = np.concatenate([X[n, :l] for n, l in enumerate(self.lengths)], axis=0)
        take = rng.choice(pts.shape[0], min(c // 2 + 1, pts.shape[0]), replace=False)
        Sn[: len(take)] = pts[take]                         # landmarks equal to valid points: zero distances
        if lengths is not None:
            for n, l in enumerate(self.lengths):
                X[n, l:] = np.nan
        leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
        self.X, self.S = leaf(X), leaf(Sn)
        self.Wh = leaf(rng.standard_normal((c, c)) / np.sqrt(c))
        self.al, self.om = leaf(rng.uniform(0.3, 1.2, Q)), leaf(0.3 * rng.standard_normal((Q, d)))
        self.ga = leaf(rng.uniform(0.4, 1.3, (Q, d)) / np.sqrt(d))
        self.leaves = (self.X, self.S, self.Wh, self.al, self.om, self.ga)
        self.lens = None if lengths is None else torch.tensor(self.lengths, dtype=torch.int32, device=DEV)
        self.F = 1 + c + (M - 1) * self.r

    def G(self, seed=5, N=None):
        return torch.tensor(np.random.default_rng(seed).standard_normal((self.N if N is None else N, self.F)), device=DEV)

    def new(self, X=None, lens="own"):
        """the new entry points (lens: the setup's lengths, a tensor of one's own, or None: the NULL pointer)"""
        from gpsig_amd import autodiff
        return autodiff._LrSeqFeaturesSpectralRagged.apply(self.X if X is None else X, self.lens if isinstance(lens, str) else lens, self.S, self.Wh,
                                                           self.al, self.om, self.ga, self.mod._spec, self.family, self.draw.sketches, self.r)

    def whole(self, X):
        """the existing whole-sequence spectral pair"""
        from gpsig_amd import autodiff
        return autodiff._LrSeqFeaturesSpectral.apply(X, self.S, self.Wh, self.al, self.om, self.ga, self.mod._spec, self.family,
                                                     self.draw.sketches, self.r)

    def torch_route(self):
        from gpsig_amd import autodiff
        sc = self.scope
        sc.S, sc.Wh = self.S, self.Wh
        sc.mod._kappa = lambda A, B: autodiff.base_kernel_matrix("spectral", A, B, spectral=(self.family, self.al, self.om, self.ga))
        return torch.cat(sc._seq_torch(self.X) if self.lens is None else sc._seq_torch_ragged(self.X, self.lens), dim=1)

    def grads(self, Phi, G, leaves=None):
        return torch.autograd.grad(Phi, self.leaves if leaves is None else leaves, G, allow_unused=True)


def fits_lds(c, d, L):
    """the four (width, L) arrays of a whole sequence fit the LDS in the reverse pass: the limit of the existing spectral pair"""
    return 8 * ((L + 63) // 64 * 64 + 1) * 4 * max(c, d, 16) <= 156 * 1024


# ---- 1. values and all six gradients against _seq_torch.  (c = r, L, M, difference, family, d, Q)
DENSE = [(64, L, 4, diff, "mixed", 3, 4) for L in (65, 66, 129, 130) for diff in (True, False)]      # one tile; + 1 step; two tiles; + 1 step
DENSE += [(64, 130, 2, True, "mixed", 3, 4), (64, 130, 2, False, "mixed", 3, 4)]
DENSE += [(16, 330, 4, True, "mixed", 3, 4)]                                                         # tiles of 256 steps
DENSE += [(50, 100, 4, True, "mixed", 3, 4)]                                                         # whole-sequence forward, tiled reverse
DENSE += [(64, 130, 4, True, "rbf", 3, 4), (64, 130, 4, True, "exp", 3, 4)]
DENSE += [(64, 130, 3, True, "mixed", 32, 2)]                                                        # the widest table row


@pytest.mark.parametrize("c,L,M,difference,family,d,Q", DENSE)
def test_dense_matches_torch_route(c, L, M, difference, family, d, Q):
    assert not fits_lds(c, d, L)                            # beyond the existing pair: every case runs a tiled kernel
    s = Setup(N=3, L=L, d=d, M=M, c=c, Q=Q, family=family, difference=difference, seed=c + L + M)
    G = s.G()
    Phi, want = s.new(lens=None), s.torch_route()
    assert Phi.shape == want.shape == (3, s.F)
    err = relerr(Phi, want)
    print("features", err)
    got_g, want_g = s.grads(Phi, G), s.grads(want, G)
    errs = {}
    for name, g, w in zip(NAMES, got_g, want_g):
        assert g is not None and w is not None, name
        errs[name] = relerr(g, w)
        print("gradient", name, errs[name])
    assert err <= 1e-11, err
    assert all(e <= 1e-9 for e in errs.values()), errs


# ---- 2. ragged against the truncated sequences and the torch route
RAGGED = [(64, 130, 4, True, (130, 66, 65, 3, 1)), (64, 130, 4, False, (130, 66, 65, 3, 1)),
          (8, 20, 4, True, (20, 7, 2, 1, 13)), (8, 20, 4, False, (20, 7, 2, 1, 13))]          # (the whole-sequence ragged instances)


@pytest.mark.parametrize("c,L,M,difference,lengths", RAGGED)
def test_ragged_matches_truncated_sequences(c, L, M, difference, lengths):
    s = Setup(N=len(lengths), L=L, d=3, M=M, c=c, Q=4, family="mixed", difference=difference, seed=L + c, lengths=lengths)
    G = s.G()
    Phi = s.new()
    assert Phi.shape == (s.N, s.F) and bool(torch.isfinite(Phi).all())
    for n, l in enumerate(lengths):
        cut = s.X[n:n + 1, :l]
        e = relerr(Phi[n:n + 1], s.new(cut, lens=None))
        print("truncated", n, l, e)
        assert e <= 1e-12, (n, l, e)
        if fits_lds(c, 3, l):
            e = relerr(Phi[n:n + 1], s.whole(cut))
            print("truncated, existing pair", n, l, e)
            assert e <= 1e-12, (n, l, e)
    got_g = s.grads(Phi, G)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in got_g)
    for n, l in enumerate(lengths):
        assert torch.equal(got_g[0][n, l:], torch.zeros_like(got_g[0][n, l:])), (n, l)       # padded rows: written, exactly zero
    want = s.torch_route()
    assert relerr(Phi, want) <= 1e-11, relerr(Phi, want)
    for name, g, w in zip(NAMES, got_g, s.grads(want, G)):
        e = relerr(g, w)
        print("gradient", name, e)
        assert e <= 1e-9, (name, e)


# ---- 3. a NULL lengths pointer is lengths all L, bit for bit
@pytest.mark.parametrize("c,L", [(64, 130), (8, 20)])
def test_null_lengths_equals_full_lengths(c, L):
    s = Setup(N=3, L=L, d=3, M=4, c=c, Q=4, family="mixed", seed=2)
    G = s.G()
    full = torch.full((3,), L, dtype=torch.int32, device=DEV)
    a, b = s.new(lens=None), s.new(lens=full)
    assert torch.equal(a, b)
    for x, y in zip(s.grads(a, G), s.grads(b, G)):
        assert torch.equal(x, y)


# ---- 4. carries and partial sums: more sequences than workgroups
def test_many_sequences_repeat_and_split():
    N, h = 600, 300
    s = Setup(N=N, L=66, d=3, M=3, c=64, Q=4, family="mixed", seed=9)
    G = s.G()
    Phi = s.new(lens=None)
    full = s.grads(Phi, G)
    again = s.grads(s.new(lens=None), G)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    X1, X2 = s.X[:h].detach().clone().requires_grad_(True), s.X[h:].detach().clone().requires_grad_(True)
    P1, P2 = s.new(X1, lens=None), s.new(X2, lens=None)
    assert torch.equal(Phi, torch.cat([P1, P2]))
    g1 = torch.autograd.grad(P1, (X1,) + s.leaves[1:], G[:h])
    g2 = torch.autograd.grad(P2, (X2,) + s.leaves[1:], G[h:])
    assert torch.equal(full[0], torch.cat([g1[0], g2[0]]))
    for k in range(1, 6):
        e = relerr(full[k], g1[k] + g2[k])
        print("split", NAMES[k], e)
        assert e <= 1e-12, (k, e)


# ---- 5. dkxs in chunks on the tiled path
def test_chunked_dkxs_matches_two_half_batches():
    # dkxs = N L c doubles: 4,100 x 130 x 64 x 8 bytes = 273 MB, above the 256 MB budget of one chunk; each half stays below it
    N, L = 4100, 130
    s = Setup(N=N, L=L, d=2, M=2, c=64, Q=2, family="exp", seed=4)
    G = s.G(6)
    full = s.grads(s.new(lens=None), G)
    h = N // 2
    X1, X2 = s.X[:h].detach().clone().requires_grad_(True), s.X[h:].detach().clone().requires_grad_(True)
    g1 = torch.autograd.grad(s.new(X1, lens=None), (X1,) + s.leaves[1:], G[:h])
    g2 = torch.autograd.grad(s.new(X2, lens=None), (X2,) + s.leaves[1:], G[h:])
    assert relerr(full[0], torch.cat([g1[0], g2[0]])) <= 1e-12
    for k in range(1, 6):
        assert relerr(full[k], g1[k] + g2[k]) <= 1e-12, k


# ---- 6. the module route
MOD_LENGTHS = [130, 66, 65, 2]


def _module_setup(lr_hip, tiled, c=64, L=130, seed=77):
    from gpsig_amd import kernels, autodiff
    d, M, Q = 3, 3, 4
    rng = np.random.default_rng(seed)
    kern = kernels.SignatureSpectral(L * d, d, M, family="mixed", Q=Q, low_rank=True, num_components=c, rank_bound=c,
                                     variances=rng.uniform(0.5, 1.5, M + 1))
    kern.alpha, kern.omega, kern.gamma = np.exp(0.3 * rng.standard_normal(Q)), 0.3 * np.exp(0.3 * rng.standard_normal((Q, d))), \
        np.exp(0.3 * rng.standard_normal((Q, d)))
    kern.rng = np.random.default_rng(5)
    mod = autodiff.SignatureKernelModule(kern, device=DEV)
    mod.lr_hip = lr_hip
    if tiled is not None:
        mod.lr_spectral_tiled = tiled
    return mod, rng


def _module_loss(mod, rng, lengths, N=4, L=130, d=3):
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.1, axis=1)
    for n, l in enumerate(lengths or ()):
        X[n, l:] = np.nan
    X = torch.tensor(X.reshape(N, L * d), device=DEV, requires_grad=True)
    draw = mod.draw_low_rank(N * L)
    W = torch.tensor(rng.standard_normal((N, N)), device=DEV)
    mod.zero_grad()
    (mod.K(X, lr=draw, lengths=lengths) * W).sum().backward()
    return [X.grad] + [p.grad for p in mod.parameters() if p.grad is not None]


@pytest.mark.parametrize("lengths", [None, MOD_LENGTHS], ids=["dense", "ragged"])
def test_module_takes_the_tiled_route(monkeypatch, lengths):
    from gpsig_amd import _lib, autodiff
    names = []
    orig_call = _lib.Context.call

    def spy(self, name, params, *args):
        names.append(name)
        return orig_call(self, name, params, *args)

    def no_torch(self, Xs, *a):
        raise AssertionError("sequence features took the torch route")

    with monkeypatch.context() as mp:
        mp.setattr(_lib.Context, "call", spy)
        mp.setattr(autodiff._LowRankScope, "_seq_torch", no_torch)
        mp.setattr(autodiff._LowRankScope, "_seq_torch_ragged", no_torch)
        mod, rng = _module_setup(True, True)
        got = _module_loss(mod, rng, lengths)
    assert ENTRY[0] in names and ENTRY[1] in names
    ref, rng2 = _module_setup(False, True)
    want = _module_loss(ref, rng2, lengths)
    assert len(got) == len(want) >= 6
    for n, l in enumerate(lengths or ()):
        assert bool((got[0].reshape(4, 130, 3)[n, l:] == 0).all())
    for g, w in zip(got, want):
        assert relerr(g, w) <= 1e-9, relerr(g, w)


@pytest.mark.parametrize("lengths", [None, MOD_LENGTHS], ids=["dense", "ragged"])
def test_module_default_keeps_the_torch_route(monkeypatch, lengths):
    from gpsig_amd import _lib, autodiff
    names, calls = [], []
    orig_call, orig = _lib.Context.call, {k: getattr(autodiff._LowRankScope, k) for k in ("_seq_torch", "_seq_torch_ragged")}

    def spy(self, name, params, *args):
        names.append(name)
        return orig_call(self, name, params, *args)

    def count(key):
        def f(self, Xs, *a):
            calls.append(key)
            return orig[key](self, Xs, *a)
        return f

    monkeypatch.setattr(_lib.Context, "call", spy)
    for key in orig:
        monkeypatch.setattr(autodiff._LowRankScope, key, count(key))
    mod, rng = _module_setup(True, None)
    assert mod.lr_spectral_tiled is False
    grads = _module_loss(mod, rng, lengths)
    assert ("_seq_torch" if lengths is None else "_seq_torch_ragged") in calls
    assert ENTRY[0] not in names and ENTRY[1] not in names
    assert all(bool(torch.isfinite(g).all()) for g in grads)


# ---- 7. typed refusals
def _raw_calls(s, c, d):
    """both new entry points on the arrays of `s`, claiming `c` components and `d` features"""
    from gpsig_amd import autodiff
    keep = []
    p = s.mod._spec.params(d, float(s.al.shape[0]), keep)
    p.base_params[1] = float(autodiff._SPECTRAL_FAMILY[s.family])
    arr = autodiff._sketch_array(s.draw.sketches, keep)
    X, S, Wh, a, o, g = (autodiff._c(t.detach()) for t in s.leaves)
    ptr = autodiff._ptr
    out = torch.empty((s.N, s.F), dtype=torch.float64, device=DEV)
    ctx = autodiff._ctx_for(X)
    errs = []
    try:
        ctx.call(ENTRY[0], p, c, s.r, len(s.draw.sketches), arr, ptr(X), s.N, s.L, None, ptr(S), ptr(Wh), ptr(a), ptr(o), ptr(g), ptr(out))
    except Exception as e:  # noqa: BLE001
        errs.append(e)
    G = torch.ones((s.N, s.F), dtype=torch.float64, device=DEV)
    outs = [torch.empty_like(t) for t in (X, S, Wh, a, o, g)]
    try:
        ctx.call(ENTRY[1], p, c, s.r, len(s.draw.sketches), arr, ptr(X), s.N, s.L, None, ptr(S), ptr(Wh), ptr(a), ptr(o), ptr(g), ptr(G),
                 *(ptr(t) for t in outs))
    except Exception as e:  # noqa: BLE001
        errs.append(e)
    return errs


def test_refusals_are_typed():
    big = Setup(N=3, L=130, d=3, M=2, c=65, Q=2, family="rbf", seed=1)
    errs = _raw_calls(big, 65, 3)
    assert len(errs) == 2 and all(isinstance(e, NotImplementedError) for e in errs), errs
    wide = Setup(N=3, L=130, d=33, M=2, c=8, Q=2, family="rbf", seed=1)
    errs = _raw_calls(wide, 8, 33)
    assert len(errs) == 2 and all(isinstance(e, NotImplementedError) for e in errs), errs
    ok = Setup(N=3, L=130, d=3, M=2, c=8, Q=2, family="rbf", seed=1)
    assert _raw_calls(ok, 8, 3) == []
    for bad in (torch.full((3,), 130, dtype=torch.int64, device=DEV), torch.full((4,), 130, dtype=torch.int32, device=DEV),
                torch.full((3, 1), 130, dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError):
            ok.new(lens=bad)


# ---- the memory of an SVGP step just past the whole-sequence limit (c = r = 50: L = 64 fits the reverse pass, L = 65 does not)
def _svgp_peak_mb(base, lr_hip, tiled, N=1024, L=65, d=6, M=4, T=64, c=50, Q=5):
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
    m.kernel.lr_spectral_tiled = tiled
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
    assert not fits_lds(50, 6, 65) and fits_lds(50, 6, 64)
    rbf = _svgp_peak_mb("rbf", True, False)
    tiled = _svgp_peak_mb("spectral", True, True)
    torch_route = _svgp_peak_mb("spectral", True, False)
    bound = 2 * rbf + 256
    print("peak MB: rbf", rbf, "spectral tiled", tiled, "spectral torch route", torch_route, "bound", bound)
    assert tiled <= bound, (tiled, rbf)
    # the torch route of the same step (the default of lr_spectral_tiled) does not meet the bound
    assert torch_route > bound, (torch_route, bound)
