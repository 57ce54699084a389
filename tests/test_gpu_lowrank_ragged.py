"""Ragged batches in low-rank mode: gpsig_lr_seq_features_ragged_dev / _ragged_grad (the ragged instances of the whole-sequence and the
time-tiled feature kernels, csrc/lr_ragged_inst.hip) behind autodiff._LrSeqFeaturesRagged, against
  * the torch route of the same map (autodiff._LowRankScope._seq_torch_ragged) given the same landmarks, whitening, parameters and projections;
  * the existing op (autodiff._LrSeqFeatures) on each sequence truncated to its length and evaluated alone.
The contract: the features of sequence n are those of X[n, :lengths[n]] alone; the rows beyond are never read (they are NaN in every case
here); their gX rows are written, as exact zeros; with the time difference a one-point sequence has no step: Phi = [1, 0, .., 0].

Tolerances and fixtures are those of tests/test_gpu_lowrank_long_train.py (copied, not imported): relerr = max|got - want| / max|want|, 1e-11 for
features and 1e-9 for gradients against torch autograd, 1e-12 for identities between runs of the library's own kernels; sequences and
landmarks lie on a grid of 1/256 (|value| < 8), so that a landmark copied from a point is at distance zero in both routes (the Matern families).

The tile length at 64 rows (c = r = 64) is 64 steps of U, at 16 rows 256.  In a table of L = 130 with the time difference the lengths
130, 66, 65, 2, 1 have 3, 2, 1, 1 tiles and no step at all; without it 130, 129, 128, 65, 1 have 3, 3, 2, 2 and 1 tiles."""
import ctypes as C

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
    """A low-rank module (lr_hip = False), one draw, a table of sequences whose rows beyond each length are NaN, landmarks (half of them valid
    points of the sequences), a random whitening and the parameters as leaves."""

    def __init__(self, lengths, L, d, M, c, base="rbf", difference=True, seed=0, pad_nan=True):
        from gpsig_amd import kernels, autodiff
        rng = np.random.default_rng(seed)
        N = len(lengths)
        cls = {"linear": kernels.SignatureLinear, "rbf": kernels.SignatureRBF, "poly": kernels.SignaturePoly,
               "matern32": kernels.SignatureMatern32}[base]
        k = cls(L * d, d, M, lengthscales=None, difference=difference, low_rank=True, num_components=c, rank_bound=c)
        k.rng = np.random.default_rng(seed + 1)
        self.mod = autodiff.SignatureKernelModule(k, device=DEV)
        self.mod.lr_hip = False
        self.M, self.c, self.N, self.L = M, c, N, L
        self.lengths = [int(l) for l in lengths]
        X = grid(np.cumsum(0.1 * rng.standard_normal((N, L, d)), axis=1))
        pool = 0.7 * rng.standard_normal((2 * c + 4, d))
        self.draw = self.mod.draw_low_rank(pool.shape[0])
        self.scope = autodiff._LowRankScope(self.mod, torch.tensor(pool, device=DEV), self.draw)
        self.r = int(self.draw.sketches[0].r) if self.draw.sketches else c
        Sn = grid(0.7 * rng.standard_normal((c, d)))
        pts = np.concatenate([X[n, :l] for n, l in enumerate(self.lengths)], axis=0)
        take = rng.choice(pts.shape[0], min(c // 2 + 1, pts.shape[0]), replace=False)
        Sn[: len(take)] = pts[take]                         # landmarks equal to valid points: zero distances
        if pad_nan:
            for n, l in enumerate(self.lengths):
                X[n, l:] = np.nan
        leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
        self.X, self.S = leaf(X), leaf(Sn)
        self.Wh = leaf(rng.standard_normal((c, c)) / np.sqrt(c))
        self.lens = torch.tensor(self.lengths, dtype=torch.int32, device=DEV)
        self.leaves = (self.X, self.S, self.Wh)
        self.names = ("X", "S", "Wh")
        if self.mod.raw_p0 is not None:
            self.leaves += (self.mod.raw_p0,)
            self.names += ("base parameter",)
        self.F = 1 + c + (M - 1) * self.r

    def ragged(self, X=None, lens=None):
        from gpsig_amd import autodiff
        return autodiff._LrSeqFeaturesRagged.apply(self.X if X is None else X, self.lens if lens is None else lens, self.S, self.Wh, self.mod.p0,
                                                   self.mod._spec, self.draw.sketches, self.r)

    def hip(self, X=None):
        from gpsig_amd import autodiff
        return autodiff._LrSeqFeatures.apply(self.X if X is None else X, self.S, self.Wh, self.mod.p0, self.mod._spec, self.draw.sketches, self.r)

    def truncated(self):
        """every sequence cut to its length, through the existing op, alone"""
        return torch.cat([self.hip(self.X[n:n + 1, :l]) for n, l in enumerate(self.lengths)], dim=0)

    def torch_route(self):
        sc = self.scope
        sc.S, sc.Wh = self.S, self.Wh
        return torch.cat(sc._seq_torch_ragged(self.X, self.lens), dim=1)

    def grads(self, Phi, G, leaves=None):
        return torch.autograd.grad(Phi, self.leaves if leaves is None else leaves, G, allow_unused=True)


def check_contract(s, tag):
    """Case 1's checks: against the torch route, against the truncated sequences, the padded rows, finiteness."""
    G = torch.tensor(np.random.default_rng(5).standard_normal((s.N, s.F)), device=DEV)
    Phi, want, cut = s.ragged(), s.torch_route(), s.truncated()
    assert Phi.shape == want.shape == cut.shape == (s.N, s.F)
    got_g, want_g, cut_g = s.grads(Phi, G), s.grads(want, G), s.grads(cut, G)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in got_g) and bool(torch.isfinite(Phi).all())
    errs = {"features": relerr(Phi, want), "features/truncated": relerr(Phi, cut)}
    for name, g, w, t in zip(s.names, got_g, want_g, cut_g):
        assert w is not None and t is not None, name
        errs[name] = relerr(g, w)
        errs[name + "/truncated"] = relerr(g, t)
    for k, v in errs.items():
        print(tag, k, v)
    for n, l in enumerate(s.lengths):
        assert bool((got_g[0][n, l:] == 0).all()), (n, l)                        # padded rows: written, exactly zero
        if s.mod.kern.difference and l == 1:                                     # no step: [1, 0, .., 0] and a zero gradient row
            assert bool((Phi[n, 0] == 1).all()) and bool((Phi[n, 1:] == 0).all()) and bool((got_g[0][n] == 0).all())
    assert float(got_g[0].abs().max()) > 0
    assert errs["features"] <= 1e-11, errs
    for name in s.names:
        assert errs[name] <= 1e-9, (name, errs)
    for k, v in errs.items():
        if k.endswith("/truncated"):
            assert v <= 1e-12, (k, errs)
    if "base parameter" in s.names:
        assert len(got_g) == 4 and float(got_g[3].abs()) > 0


# (c = r, L, M, difference, base, lengths)
CASES = [
    (8, 20, 4, True, "rbf", [20, 7, 2, 1, 13]),                     # 1: the whole-sequence kernels
    (8, 20, 4, False, "rbf", [20, 7, 2, 1, 13]),
    (64, 130, 4, True, "rbf", [130, 66, 65, 2, 1]),                 # 2: the tiled kernels, TL = 64
    (64, 130, 2, True, "rbf", [130, 66, 65, 2, 1]),
    (64, 130, 4, False, "rbf", [130, 129, 128, 65, 1]),
    (64, 130, 2, False, "rbf", [130, 129, 128, 65, 1]),
    (16, 330, 4, True, "rbf", [330, 258, 257, 40]),                 # 2b: 16 rows, TL = 256
    (50, 100, 4, True, "rbf", [100, 64, 3]),                        # 3: the whole-sequence forward kernel with the tiled reverse pass
    (64, 130, 4, True, "matern32", [130, 66, 65, 2, 1]),            # 4: the families
    (64, 130, 4, True, "linear", [130, 66, 65, 2, 1]),
    (64, 130, 4, True, "poly", [130, 66, 65, 2, 1]),
]


@pytest.mark.parametrize("c,L,M,difference,base,lengths", CASES)
def test_ragged_features_and_gradients(c, L, M, difference, base, lengths):
    s = Setup(lengths, L=L, d=3, M=M, c=c, base=base, difference=difference, seed=c + L + M)
    check_contract(s, "%s c=%d L=%d M=%d diff=%s" % (base, c, L, M, difference))


@pytest.mark.parametrize("c,L", [(8, 20), (64, 130)])
def test_full_lengths_equal_the_existing_ops(c, L):
    s = Setup([L] * 4, L=L, d=3, M=4, c=c, seed=3)
    G = torch.tensor(np.random.default_rng(7).standard_normal((4, s.F)), device=DEV)
    a, b = s.ragged(), s.hip()
    assert relerr(a, b) <= 1e-12, relerr(a, b)
    for name, g, w in zip(s.names, s.grads(a, G), s.grads(b, G)):
        e = relerr(g, w)
        print("full lengths", c, L, name, e)
        assert e <= 1e-12, (name, e)


def test_carries_and_scratch_reset_between_sequences_of_different_length():
    # 600 sequences on at most 512 workgroups: some take two, of different tile counts (2, none, 1, 1, 1)
    N, L, c = 600, 66, 64
    lengths = [(66, 1, 65, 2, 30)[n % 5] for n in range(N)]
    s = Setup(lengths, L=L, d=3, M=3, c=c, seed=4)
    G = torch.tensor(np.random.default_rng(6).standard_normal((N, s.F)), device=DEV)
    Phi = s.ragged()
    full = s.grads(Phi, G)
    Phi2 = s.ragged()
    again = s.grads(Phi2, G)
    assert torch.equal(Phi, Phi2) and bool(torch.isfinite(Phi).all())
    for x, y in zip(full, again):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    for n in (0, 1, 2, 3, 4, 512, 513, 599):
        assert bool((full[0][n, lengths[n]:] == 0).all())
    h = N // 2
    X1, X2 = s.X[:h].detach().clone().requires_grad_(True), s.X[h:].detach().clone().requires_grad_(True)
    P1, P2 = s.ragged(X1, s.lens[:h].clone()), s.ragged(X2, s.lens[h:].clone())
    assert torch.equal(Phi, torch.cat([P1, P2]))
    g1 = torch.autograd.grad(P1, (X1,) + s.leaves[1:], G[:h])
    g2 = torch.autograd.grad(P2, (X2,) + s.leaves[1:], G[h:])
    assert torch.equal(full[0], torch.cat([g1[0], g2[0]]))
    for k in (1, 2):
        err = relerr(full[k], g1[k] + g2[k])
        print("split", s.names[k], err)
        assert err <= 1e-12, (k, err)


# ---- the module route
MOD_LENGTHS = [130, 66, 65, 2]


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


def _ragged_table(rng, N, L, d, lengths):
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.1, axis=1)
    for n, l in enumerate(lengths):
        X[n, l:] = np.nan
    return torch.tensor(X.reshape(N, L * d), device=DEV, requires_grad=True)


def _module_loss(mod, rng, N, L, d=3):
    X = _ragged_table(rng, N, L, d, MOD_LENGTHS)
    draw = mod.draw_low_rank(N * L)
    W = torch.tensor(rng.standard_normal((N, N)), device=DEV)
    mod.zero_grad()
    (mod.K(X, lr=draw, lengths=MOD_LENGTHS) * W).sum().backward()
    return [X.grad] + [p.grad for p in mod.parameters() if p.grad is not None]


def _svgp_loss(mod, rng, N, L, d=3):
    from gpsig_amd import inducing_variables as iv, likelihoods, models
    M = mod.kern.num_levels
    Z = 0.5 * rng.standard_normal((M * (M + 1) // 2, 6, d))
    svgp = models.SVGPModule(mod, iv.InducingTensors(Z, M), likelihoods.Gaussian(), device=DEV)
    X = _ragged_table(rng, N, L, d, MOD_LENGTHS)
    Y = torch.tensor(rng.standard_normal((N, 1)), device=DEV)
    svgp.zero_grad()
    mod.kern.rng = np.random.default_rng(11)                # (the draw of the evaluation: the same in both modules)
    svgp.elbo(X, Y, lengths=np.asarray(MOD_LENGTHS)).backward()
    return [X.grad] + [p.grad for p in svgp.parameters() if p.grad is not None]


@pytest.mark.parametrize("loss", [_module_loss, _svgp_loss], ids=["K", "elbo"])
def test_module_takes_the_ragged_route(monkeypatch, loss):
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
        mod, rng = _module_setup("rbf", 64, True, L=130)
        got = loss(mod, rng, N=4, L=130)
    assert "gpsig_lr_seq_features_ragged_dev" in names and "gpsig_lr_seq_features_ragged_grad" in names
    assert "gpsig_lr_seq_features_dev" not in names
    ref, rng2 = _module_setup("rbf", 64, False, L=130)
    want = loss(ref, rng2, N=4, L=130)
    assert len(got) == len(want) >= 3
    for n, l in enumerate(MOD_LENGTHS):
        assert bool((got[0].reshape(4, 130, 3)[n, l:] == 0).all())
    for g, w in zip(got, want):
        assert relerr(g, w) <= 1e-9, relerr(g, w)


# ---- refusals
def _raw_calls(s, c, N, L, lens):
    """gpsig_lr_seq_features_ragged_dev and _ragged_grad on the arrays of `s` claiming `c` components"""
    from gpsig_amd import autodiff
    keep = []
    p = s.mod._spec.params(3, 0.0, keep)
    arr = autodiff._sketch_array(s.draw.sketches, keep)
    X, S, Wh = (autodiff._c(t.detach()) for t in (s.X, s.S, s.Wh))
    F = 1 + c + (s.M - 1) * s.r
    out = torch.empty((N, F), dtype=torch.float64, device=DEV)
    ctx = autodiff._ctx_for(X)
    lp = None if lens is None else autodiff._ptr(lens)
    calls = []
    try:
        ctx.call("gpsig_lr_seq_features_ragged_dev", p, c, s.r, len(s.draw.sketches), arr, autodiff._ptr(X), N, L, lp, autodiff._ptr(S),
                 autodiff._ptr(Wh), autodiff._ptr(out))
    except Exception as e:  # noqa: BLE001
        calls.append(e)
    G = torch.ones((N, F), dtype=torch.float64, device=DEV)
    gX, gS, gWh = torch.empty_like(X), torch.empty_like(S), torch.empty_like(Wh)
    gb = torch.zeros(2, dtype=torch.float64, device=DEV)
    try:
        ctx.call("gpsig_lr_seq_features_ragged_grad", p, c, s.r, len(s.draw.sketches), arr, autodiff._ptr(X), N, L, lp, autodiff._ptr(S),
                 autodiff._ptr(Wh), autodiff._ptr(G), autodiff._ptr(gX), autodiff._ptr(gS), autodiff._ptr(gWh),
                 C.cast(gb.data_ptr(), C.POINTER(C.c_double)))
    except Exception as e:  # noqa: BLE001
        calls.append(e)
    return calls


def test_refusals_stay_typed(monkeypatch):
    from gpsig_amd import autodiff
    # 65 components: beyond the reverse pass's tables, whatever the lengths (the forward direction has no such table, as in the existing pair)
    big = Setup([130, 66, 3], L=130, d=3, M=2, c=65, seed=1)
    errs = _raw_calls(big, 65, 3, 130, big.lens)
    assert len(errs) == 1 and isinstance(errs[0], NotImplementedError), errs
    # a NULL lengths pointer: the library's invalid-argument error, from both entry points
    ok = Setup([20, 7, 2], L=20, d=3, M=2, c=8, seed=1)
    errs = _raw_calls(ok, 8, 3, 20, None)
    assert len(errs) == 2 and all(isinstance(e, ValueError) for e in errs), errs
    assert _raw_calls(ok, 8, 3, 20, ok.lens) == []
    # SignatureSpectral with lengths: the torch route of the ragged map, finite gradients
    calls = []
    orig = autodiff._LowRankScope._seq_torch_ragged

    def spy(self, Xs, lengths):
        calls.append(tuple(Xs.shape))
        return orig(self, Xs, lengths)

    monkeypatch.setattr(autodiff._LowRankScope, "_seq_torch_ragged", spy)
    mod, rng = _module_setup("spectral", 64, True, L=130)
    grads = _module_loss(mod, rng, N=4, L=130)
    assert calls and calls[0][1] == 130
    assert all(bool(torch.isfinite(g).all()) for g in grads)
