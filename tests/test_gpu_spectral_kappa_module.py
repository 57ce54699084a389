"""Exact-mode SignatureSpectral training through the batched kappa op: SignatureKernelModule.spectral_kappa = "hip" (autodiff._SpectralKappa on every
kappa of the matrix route) against "torch" (base_kernel_matrix's difference form, today's route), and the default "auto".

The module: 33 columns, L = 9, 5 sequences, 6 inducing tensors with increments, 3 levels, Q = 3, each family.  (SignatureSpectral takes neither lags nor
lengthscales -- the reference overwrites the lag weights, kernels.py:82 against :913 --, so the 33 columns are 33 features, and the parameters compared
are all the module has: alpha, omega, gamma, variances, sigma, and the inducing tensors Z.)  Bounds: 1e-10 for values, 1e-9 for gradients, relative to
the largest entry of the torch route's array.

Errors measured on the GPU (MI355X), the largest over the families:
    K_tens_n_seq_covs (both full_X_cov), Kdiag, K: values 0 .. 7.6e-16; gradients <= 2.7e-15 (raw_omega through K, 'mixed'), Z <= 9.5e-16
    SVGP step: loss equal to the last bit in all three families; gradients <= 1.3e-15 (kernel.raw_omega, 'exp')
    "auto": the torch route's bits in every quantity and gradient
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL_VALUE, TOL_GRAD = 1e-10, 1e-9
FAMILIES = ["rbf", "exp", "mixed"]
N, L, D, M, T, Q = 5, 9, 33, 3, 6, 3


def rel(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max() / (want.abs().max() + 1e-300))


def build(family):
    from gpsig_amd import kernels
    rng = np.random.default_rng(5)
    k = kernels.SignatureSpectral(L * D, D, M, family=family, Q=Q, variances=rng.uniform(0.5, 1.5, M + 1))
    k.alpha, k.omega, k.gamma = rng.uniform(0.3, 1.2, Q), 0.3 / np.sqrt(D) * np.abs(rng.standard_normal((Q, D))) + 0.01, rng.uniform(0.4, 1.3, (Q, D)) / np.sqrt(D)
    X = np.cumsum(rng.standard_normal((N, L, D)) * 0.5, axis=1).reshape(N, L * D)
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, D)) * 0.7
    return k, torch.as_tensor(X, device=DEV), Z


def evaluate(mod, Z, X, route, fn):
    """fn(mod, Z, X) -> tuple of arrays; then a backward of one random linear functional of them -> (arrays, {parameter: gradient})"""
    mod.spectral_kappa = route
    mod.zero_grad(set_to_none=True)
    Zp = Z.detach().clone().requires_grad_(True)
    outs = fn(mod, Zp, X)
    g = torch.Generator(device="cpu").manual_seed(7)
    loss = sum((o * torch.randn(o.shape, generator=g, dtype=torch.float64).to(DEV)).sum() for o in outs)
    loss.backward()
    grads = {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}
    grads["Z"] = Zp.grad.clone()
    return [o.detach() for o in outs], grads


def compare(tag, got, want):
    (og, gg), (ow, gw) = got, want
    ev = max(rel(a, b) for a, b in zip(og, ow))
    assert set(gg) == set(gw), (set(gg), set(gw))
    eg = {n: rel(gg[n], gw[n]) for n in gw}
    print(tag, "values %.1e" % ev, "gradients", " ".join("%s %.1e" % (n, e) for n, e in sorted(eg.items())))
    assert ev < TOL_VALUE, (tag, ev)
    assert max(eg.values()) < TOL_GRAD, (tag, eg)
    return set(gw)


@pytest.mark.parametrize("family", FAMILIES)
def test_covariances_on_both_routes(family):
    from gpsig_amd import autodiff
    k, X, Z = build(family)
    mod = autodiff.SignatureKernelModule(k, device=DEV)
    Zt = torch.as_tensor(Z, device=DEV)
    fns = {
        "K_tens_n_seq_covs, diagonal": lambda m, z, x: m.K_tens_n_seq_covs(z, x, full_X_cov=False, increments=True),
        "K_tens_n_seq_covs, full": lambda m, z, x: m.K_tens_n_seq_covs(z, x, full_X_cov=True, increments=True),
        "Kdiag": lambda m, z, x: (m.Kdiag(x), z.sum()[None]),
        "K": lambda m, z, x: (m.K(x), z.sum()[None]),
    }
    for name, fn in fns.items():
        want = evaluate(mod, Zt, X, "torch", fn)
        got = evaluate(mod, Zt, X, "hip", fn)
        names = compare("%s %s:" % (family, name), got, want)
        if name.startswith("K_tens"):
            assert {"raw_alpha", "raw_omega", "raw_sgamma", "raw_variances", "Z"} <= names, names
        # the default: this module's difference tensors are far below SPECTRAL_KAPPA_MIN_BYTES, so "auto" is the torch route bit for bit
        auto = evaluate(mod, Zt, X, "auto", fn)
        assert all(torch.equal(a, b) for a, b in zip(auto[0], want[0]))
        assert all(torch.equal(auto[1][n], want[1][n]) for n in want[1])


@pytest.mark.parametrize("family", FAMILIES)
def test_one_svgp_step_on_both_routes(family):
    from gpsig_amd import inducing_variables, likelihoods, models
    k, X, Z = build(family)
    Y = torch.as_tensor((np.arange(N) % 2)[:, None].astype(np.float64), device=DEV)
    m = models.SVGPModule(k, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=DEV)
    with torch.no_grad():
        g = torch.Generator(device="cpu").manual_seed(9)
        m.q_mu.copy_(0.3 * torch.randn(m.q_mu.shape, generator=g, dtype=torch.float64))
    res = {}
    for route in ("torch", "hip"):
        m.kernel.spectral_kappa = route
        m.zero_grad(set_to_none=True)
        loss = -m.elbo(X, Y)
        loss.backward()
        res[route] = (loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    el = float((res["hip"][0] - res["torch"][0]).abs() / res["torch"][0].abs())
    eg = {n: rel(res["hip"][1][n], res["torch"][1][n]) for n in res["torch"][1]}
    print(family, "SVGP step: loss %.1e" % el, "gradients", " ".join("%s %.1e" % (n, e) for n, e in sorted(eg.items())))
    assert set(res["hip"][1]) == set(res["torch"][1])
    assert {"Z", "q_mu", "q_sqrt", "kernel.raw_alpha", "kernel.raw_omega", "kernel.raw_sgamma", "kernel.raw_variances"} <= set(eg), set(eg)
    assert el < TOL_VALUE, el
    assert max(eg.values()) < TOL_GRAD, eg


def test_low_rank_mode_keeps_its_torch_fallback(monkeypatch):
    """the attribute belongs to exact mode: a low-rank module on its torch route (lr_hip = False: _LowRankScope._cross -> _kappa) never asks the route
    function, whatever the attribute says and however low the byte rule is set -- K and its gradients are the same bits under both values of it"""
    from gpsig_amd import autodiff, kernels

    def never(*a, **k):
        raise AssertionError("spectral_kappa_route asked in low-rank mode")
    monkeypatch.setattr(autodiff, "spectral_kappa_route", never)
    monkeypatch.setattr(autodiff, "SPECTRAL_KAPPA_MIN_BYTES", 0)
    rng = np.random.default_rng(6)
    k = kernels.SignatureSpectral(L * D, D, M, family="exp", Q=Q, low_rank=True, num_components=8, rank_bound=8)
    k.alpha, k.omega, k.gamma = rng.uniform(0.3, 1.2, Q), rng.uniform(0.01, 0.1, (Q, D)), rng.uniform(0.4, 1.3, (Q, D)) / np.sqrt(D)
    k.rng = np.random.default_rng(2)
    mod = autodiff.SignatureKernelModule(k, device=DEV)
    mod.lr_hip = False
    X = torch.as_tensor(np.cumsum(rng.standard_normal((N, L, D)) * 0.5, axis=1).reshape(N, L * D), device=DEV)
    draw = mod.draw_low_rank(N * L)
    res = {}
    for route in ("torch", "hip"):
        mod.spectral_kappa = route
        mod.zero_grad(set_to_none=True)
        K = mod.K(X, lr=draw)
        K.sum().backward()
        res[route] = (K.detach(), {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None})
    assert torch.equal(res["hip"][0], res["torch"][0])
    assert "raw_alpha" in res["torch"][1]
    assert all(torch.equal(res["hip"][1][n], res["torch"][1][n]) for n in res["torch"][1])
