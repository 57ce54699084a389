"""Low-rank SignatureSpectral on wide state spaces: the spectral cross op beyond 32 columns on the float64 matrix cores (gpsig_spectral_cross /
gpsig_spectral_cross_grad at 33 .. 4096 columns, csrc/lr_cross_spectral_kernel.hpp; autodiff._SpectralCross) alone -- values and gradients
against autodiff.base_kernel_matrix("spectral", ...) under torch autograd, repeatability, the ragged guarantee, dispatch and refusals -- and
through the module and an SVGP step against the torch route (lr_hip = False).

Data follow tests/test_gpu_lowrank_cross.py: points and landmarks are randn 1.5 / sqrt(d) on a grid of 1/256 clipped to +-7, half the landmarks
copied from points; gamma in [0.5, 1.5] and omega in [-1, 1] on a grid of 1/8.  Every product and partial sum of the three contractions is exact
in float64 in any order there, so both sides see distance and phase 0 at the coincident pairs; what remains is exp / cos / sqrt rounding.
relerr = max|got - want| / max|want|: 1e-11 for values, 1e-9 for each gradient."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FAMILIES = ("rbf", "exp", "mixed")


def relerr(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def grid(a, step=256.0):
    return np.clip(np.round(np.asarray(a) * step) / step, -7.0, 7.0)


def data(n, c, d, Q, seed):
    rng = np.random.default_rng(seed)
    P = grid(rng.standard_normal((n, d)) * 1.5 / np.sqrt(d))
    S = grid(rng.standard_normal((c, d)) * 1.5 / np.sqrt(d))
    take = rng.choice(n, min((c + 1) // 2, n), replace=False)
    S[: len(take)] = P[take]                                # landmarks equal to points: zero distances and phases
    alpha = rng.uniform(0.3, 1.2, Q)
    omega = np.round(rng.uniform(-1.0, 1.0, (Q, d)) * 8.0) / 8.0
    gamma = np.round(rng.uniform(0.5, 1.5, (Q, d)) * 8.0) / 8.0
    return P, S, alpha, omega, gamma


def on_device(arrays, requires_grad=False):
    return [torch.tensor(a, device=DEV, requires_grad=requires_grad) for a in arrays]


NAMES = ("dP", "dS", "dalpha", "domega", "dgamma")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,c,d,Q", [(15, 1, 33, 1), (16, 17, 65, 3), (65, 64, 130, 5), (33, 50, 1928, 2)])
def test_values_and_gradients_match_torch(family, n, c, d, Q):
    from gpsig_amd import autodiff
    leaves = on_device(data(n, c, d, Q, seed=n + c + d + Q), requires_grad=True)
    P, S, al, om, ga = leaves
    G = torch.tensor(np.random.default_rng(3).standard_normal((n, c)), device=DEV)
    got = autodiff._SpectralCross.apply(P, S, al, om, ga, family)
    want = autodiff.base_kernel_matrix("spectral", P, S, spectral=(family, al, om, ga))
    err = relerr(got, want)
    print("values", family, n, c, d, Q, err)
    gg, gw = torch.autograd.grad(got, leaves, G), torch.autograd.grad(want, leaves, G)
    errs = []
    for name, a, b in zip(NAMES, gg, gw):
        assert bool(torch.isfinite(a).all()), name          # (the coincident pairs of the exponential envelope)
        errs.append((name, relerr(a, b)))
        print("gradient", family, n, c, d, Q, *errs[-1])
    assert err <= 1e-11, err
    for name, e in errs:
        assert e <= 1e-9, (name, e)


def raw_grad(P, S, al, om, ga, G, family="mixed", c=None, d=None):
    """gpsig_spectral_cross_grad on the arrays as they are, claiming c landmarks and d columns"""
    from gpsig_amd import autodiff
    n, Q = P.shape[0], al.shape[0]
    c = S.shape[0] if c is None else c
    d = S.shape[1] if d is None else d
    dP = torch.full_like(P, 7.0)
    dS, dal, dom, dga = (torch.full_like(t, 7.0) for t in (S, al, om, ga))
    ptr = lambda t: autodiff._ptr(t) if t.numel() else None
    lc = autodiff._ctx_for(S)
    lc.check(lc._lib.gpsig_spectral_cross_grad(lc._h, Q, autodiff._SPECTRAL_FAMILY[family], d, ptr(P), n, ptr(S), c, ptr(al), ptr(om), ptr(ga), ptr(G),
                                               ptr(dP), ptr(dS), ptr(dal), ptr(dom), ptr(dga)))
    return dP, dS, dal, dom, dga


def test_reverse_pass_repeats_bit_for_bit():
    # 9,001 points are nine shares of the landmark sums in one chunk; a budget of 1 MB has room for 165 points' weights and one share a chunk
    from gpsig_amd import autodiff
    n, c, d, Q = 9001, 64, 256, 3
    ten = on_device(data(n, c, d, Q, seed=11))
    G = torch.tensor(np.random.default_rng(12).standard_normal((n, c)), device=DEV)
    first = raw_grad(*ten, G)
    again = raw_grad(*ten, G)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    ctx = autodiff._ctx_for(G)
    try:
        ctx.set_option("wide_chunk_mb", 1)
        capped = raw_grad(*ten, G)
        capped2 = raw_grad(*ten, G)
    finally:
        ctx.set_option("wide_chunk_mb", 0)
    for a, b in zip(capped, capped2):
        assert torch.equal(a, b)
    assert torch.equal(first[0], capped[0])                 # (dP does not go through the partials)
    for name, a, b in zip(NAMES[1:], capped[1:], first[1:]):
        e = relerr(a, b)
        print(name, "chunks of a 1 MB budget against one chunk of nine shares", e)
        assert e <= 1e-12, (name, e)


def test_padded_rows_take_no_part():
    n, c, d, Q = 40, 9, 40, 2
    Pn, Sn, al, om, ga = data(n, c, d, Q, seed=5)
    rng = np.random.default_rng(6)
    dead = np.sort(rng.choice(n, 13, replace=False))
    live = np.setdiff1d(np.arange(n), dead)
    Sn[: (c + 1) // 2] = Pn[live[: (c + 1) // 2]]           # the copied landmarks are live points
    Gn = rng.standard_normal((n, c))
    Pn[dead] = np.nan
    Gn[dead] = 0.0
    P, S, al, om, ga, G = on_device((Pn, Sn, al, om, ga, Gn))
    for family in FAMILIES:
        full = raw_grad(P, S, al, om, ga, G, family)
        assert bool((full[0][dead] == 0).all())              # written, exactly zero
        assert bool(torch.isfinite(full[0]).all()) and float(full[0].abs().max()) > 0
        alone = raw_grad(P[live].contiguous(), S, al, om, ga, G[live].contiguous(), family)
        assert torch.equal(full[0][live], alone[0])
        for name, a, b in zip(NAMES[1:], full[1:], alone[1:]):
            assert bool(torch.isfinite(a).all()), (family, name)
            assert torch.equal(a, b), (family, name, relerr(a, b))


def test_dispatch_and_refusals():
    from gpsig_amd import autodiff
    from oracle import sigkern_oracle_torch as OT
    # 32 columns: the kernels of before, bit for bit (two calls: nothing of the wide path is left behind either), within 1e-12 of the oracle
    n, c, Q = 70, 9, 3
    P, S, al, om, ga = on_device(data(n, c, 32, Q, seed=2))
    wide = on_device(data(n, c, 40, Q, seed=2))
    before = autodiff._SpectralCross.apply(P, S, al, om, ga, "mixed")
    autodiff._SpectralCross.apply(*wide, "mixed")
    after = autodiff._SpectralCross.apply(P, S, al, om, ga, "mixed")
    assert torch.equal(before, after)
    assert relerr(before, OT.base_spectral(*(t.cpu() for t in (P, S, al, om, ga)), "mixed")) <= 1e-12
    G = torch.ones((n, c), dtype=torch.float64, device=DEV)
    for a, b in zip(raw_grad(P, S, al, om, ga, G), raw_grad(P, S, al, om, ga, G)):
        assert torch.equal(a, b)
    # refusals, typed: more than 64 landmarks beyond 32 columns, more than 4096 columns
    with pytest.raises(NotImplementedError):
        raw_grad(*wide, G, c=65, d=33)
    with pytest.raises(NotImplementedError):
        raw_grad(*wide, G, d=4097)
    with pytest.raises(NotImplementedError):
        autodiff._SpectralCross.apply(wide[0], torch.zeros((65, 40), dtype=torch.float64, device=DEV), *wide[2:], "mixed")
    # an empty batch zeroes the sums
    _, dS, dal, dom, dga = raw_grad(wide[0][:0], *wide[1:], G[:0])
    for t in (dS, dal, dom, dga):
        assert bool((t == 0).all())
    assert autodiff._SpectralCross.apply(wide[0][:0], *wide[1:], "mixed").shape == (0, c)


def _module(family, lr_hip, d=40, L=9, M=3, c=9, r=8, Q=3):
    from gpsig_amd import autodiff, kernels
    rng = np.random.default_rng(77)
    kern = kernels.SignatureSpectral(L * d, d, M, family=family, Q=Q, variances=rng.uniform(0.5, 1.5, M + 1), low_rank=True, num_components=c,
                                     rank_bound=r)
    kern.alpha = np.exp(0.3 * rng.standard_normal(Q))
    kern.omega = 0.3 * np.exp(0.3 * rng.standard_normal((Q, d))) / np.sqrt(d)
    kern.gamma = np.exp(0.3 * rng.standard_normal((Q, d))) / np.sqrt(d)
    mod = autodiff.SignatureKernelModule(kern, device=DEV)
    mod.lr_hip = lr_hip
    return mod


def _covs(mod, lengths, d=40, N=6, L=9, T=5):
    """K_tens_n_seq_covs and K(X) of one module, forward and backward: the values, and the gradients of the inputs and of every parameter"""
    rng = np.random.default_rng(31)
    M = mod.kern.num_levels
    Xn = np.cumsum(rng.standard_normal((N, L, d)) * 0.4, axis=1)
    if lengths is not None:
        for n, l in enumerate(lengths):
            Xn[n, l:] = np.nan
    X = torch.tensor(Xn.reshape(N, -1), device=DEV, requires_grad=True)
    Z = torch.tensor(rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.7, device=DEV, requires_grad=True)
    W = [torch.tensor(rng.standard_normal(s), device=DEV) for s in ((T, T), (T, N), (N,), (N, N))]
    mod.kern.rng = np.random.default_rng(11)                # (the draws of the evaluations: the same in both modules)
    outs = list(mod.K_tens_n_seq_covs(Z, X, increments=True, lengths=lengths)) + [mod.K(X, lengths=lengths)]
    mod.zero_grad()
    sum((o * w).sum() for o, w in zip(outs, W)).backward()
    grads = {"X": X.grad, "Z": Z.grad}
    grads.update({n: p.grad for n, p in mod.named_parameters() if p.requires_grad and p.grad is not None})
    return outs, grads


@pytest.mark.parametrize("family", ["mixed", "exp"])
@pytest.mark.parametrize("lengths", [None, (9, 4, 1, 9, 7, 2)])
def test_module_takes_the_cross_op_and_matches_the_torch_route(family, lengths, monkeypatch):
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
        got, got_g = _covs(_module(family, True), lengths)
    for n in ("gpsig_lr_seq_features_kx_dev", "gpsig_lr_tens_features_kx_dev", "gpsig_lr_seq_features_kx_grad", "gpsig_lr_tens_features_kx_grad"):
        assert n in names, (n, names)
    want, want_g = _covs(_module(family, False), lengths)
    for name, a, b in zip(("Kzz", "Kzx", "Kxx", "K"), got, want):
        e = relerr(a, b)
        print("values", family, lengths, name, e)
        assert e < 1e-8, (name, e)
    assert set(got_g) == set(want_g) and {"raw_alpha", "raw_omega", "raw_sgamma"} <= set(got_g)
    for name in want_g:
        e = relerr(got_g[name], want_g[name])
        print("gradient", family, lengths, name, e)
        assert e < 1e-6, (name, e)
    if lengths is not None:
        Xg = got_g["X"].reshape(len(lengths), 9, -1)
        for n, l in enumerate(lengths):
            assert bool((Xg[n, l:] == 0).all()), (n, l)


def _svgp(d, family, lr_hip, N=12, L=9, M=4, T=8, c=50, Q=3):
    from gpsig_amd import inducing_variables, kernels, likelihoods, models
    rng = np.random.default_rng(8)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.3, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    kern = kernels.SignatureSpectral(L * d, d, M, family=family, Q=Q, low_rank=True, num_components=c)
    kern.alpha, kern.omega, kern.gamma = np.ones(Q), np.full((Q, d), 0.1), np.full((Q, d), 1.0 / np.sqrt(d))
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=DEV)
    m.kernel.lr_hip = lr_hip
    m.q_mu.data = torch.tensor(0.3 * rng.standard_normal((T, 1)), device=DEV)
    kern.rng = np.random.default_rng(3)                     # (the draw of the evaluation: the same in both models)
    elbo = m.elbo(torch.tensor(X.reshape(N, -1), device=DEV), torch.tensor(lab[:, None].astype(np.float64), device=DEV))
    elbo.backward()
    return elbo.detach(), {n: p.grad for n, p in m.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("d,family", [(130, "rbf"), (63, "exp")])
def test_svgp_step_matches_the_torch_route(d, family, monkeypatch):
    from gpsig_amd import _lib
    names = []
    orig_call = _lib.Context.call

    def spy(self, name, params, *args):
        names.append(name)
        return orig_call(self, name, params, *args)

    with monkeypatch.context() as mp:
        mp.setattr(_lib.Context, "call", spy)
        got, got_g = _svgp(d, family, True)
    assert "gpsig_lr_seq_features_kx_dev" in names and "gpsig_lr_tens_features_kx_dev" in names, names
    want, want_g = _svgp(d, family, False)
    e = abs(float(got) - float(want)) / max(1.0, abs(float(want)))
    print("elbo", d, family, float(got), float(want), e)
    assert e <= 1e-10, e
    assert set(got_g) == set(want_g) and len(got_g) >= 4
    for n in want_g:
        assert (got_g[n] is None) == (want_g[n] is None), n
        if want_g[n] is None:
            continue
        eg = relerr(got_g[n], want_g[n])
        print("gradient", d, family, n, eg)
        assert eg <= 1e-8, (n, eg)
