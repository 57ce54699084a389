"""The Nystrom cross op of the families of base_eval on the float64 matrix cores (csrc/lr_cross_kernel.hpp: gpsig_lr_cross / gpsig_lr_cross_grad,
autodiff._LrCross) alone: the operand and result layout on exact integers, values and gradients against autodiff.base_kernel_matrix under
torch autograd, repeatability, and the typed refusals.

relerr = max|got - want| / max|want|; 1e-11 for values, 1e-9 for gradients against torch autograd.  Points and landmarks lie on a grid of 1/256
with half the landmarks copied from points: every product and partial sum is exact in float64 in any order there, so both sides see distance 0
at the coincident pairs (the Matern families)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
FAMILIES = ("linear", "cosine", "poly", "rbf", "mix", "matern12", "matern32", "matern52")
P0 = {"poly": 0.75, "mix": 0.375}
P1 = {"poly": 3.0}


def relerr(got, want):
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def grid(a):
    return np.clip(np.round(np.asarray(a) * 256.0) / 256.0, -7.0, 7.0)


def spec_of(base):
    from gpsig_amd import autodiff
    return autodiff._Spec(base, 2, True, p1=P1.get(base, 0.0))


def data(n, c, d, seed):
    rng = np.random.default_rng(seed)
    P = grid(rng.standard_normal((n, d)) * 1.5 / np.sqrt(d))
    S = grid(rng.standard_normal((c, d)) * 1.5 / np.sqrt(d))
    take = rng.choice(n, min((c + 1) // 2, n), replace=False)
    S[: len(take)] = P[take]                                # landmarks equal to points: zero distances
    return P, S


@pytest.mark.parametrize("n,c,d", [(16, 16, 4), (17, 17, 5), (33, 64, 130), (1, 1, 1)])
def test_layout_on_exact_integers(n, c, d):
    from gpsig_amd import autodiff
    rng = np.random.default_rng(n + c + d)
    P = torch.tensor(rng.integers(-3, 4, (n, d)).astype(np.float64), device=DEV)
    S = torch.tensor(rng.integers(-3, 4, (c, d)).astype(np.float64), device=DEV)
    K = autodiff._LrCross.apply(P, S, None, spec_of("linear"))
    assert K.shape == (n, c)
    assert torch.equal(K, P @ S.T)


@pytest.mark.parametrize("base", FAMILIES)
@pytest.mark.parametrize("n,c,d", [(15, 1, 3), (16, 17, 65), (65, 64, 130)])
def test_values_and_gradients_match_torch(base, n, c, d):
    from gpsig_amd import autodiff
    Pn, Sn = data(n, c, d, seed=n + c + d)
    leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
    P, S = leaf(Pn), leaf(Sn)
    p0 = leaf(np.float64(P0[base])) if base in P0 else None
    leaves = (P, S) + ((p0,) if p0 is not None else ())
    G = torch.tensor(np.random.default_rng(3).standard_normal((n, c)), device=DEV)
    got = autodiff._LrCross.apply(P, S, p0, spec_of(base))
    want = autodiff.base_kernel_matrix(base, P, S, p0=p0, p1=P1.get(base, 0.0))
    err = relerr(got, want)
    print("values", base, n, c, d, err)
    gg, gw = torch.autograd.grad(got, leaves, G), torch.autograd.grad(want, leaves, G)
    errs = []
    for name, a, b in zip(("dP", "dS", "g_base"), gg, gw):
        errs.append((name, relerr(a, b)))
        print("gradient", base, n, c, d, *errs[-1])
    assert err <= 1e-11, err
    for name, e in errs:
        assert e <= 1e-9, (name, e)
    if base in P0:
        assert len(gg) == 3 and float(gg[2].abs()) > 0


def raw_grad(P, S, G, base="rbf", c=None, d=None, dtype=None):
    """gpsig_lr_cross_grad on the arrays as they are, claiming c landmarks and d columns"""
    from gpsig_amd import _lib, autodiff
    n = P.shape[0]
    c = S.shape[0] if c is None else c
    p = spec_of(base).params(P.shape[1] if d is None else d, P0.get(base, 0.0), [])
    if dtype is not None:
        p.dtype = dtype
    dP, dS = torch.empty_like(P), torch.full_like(S, 7.0)
    gb = torch.full((2,), 7.0, dtype=torch.float64, device=DEV)
    ptr = lambda t: autodiff._ptr(t) if t.numel() else None
    autodiff._ctx_for(S).call("gpsig_lr_cross_grad", p, ptr(P), n, ptr(S), c, ptr(G), ptr(dP), ptr(dS), C.cast(gb.data_ptr(), C.POINTER(C.c_double)))
    return dP, dS, gb


def test_reverse_pass_repeats_bit_for_bit():
    # 9,001 points are nine shares of the landmark sums; a budget of 1 MB has room for eight partials of 64 x 256 doubles: the cap bites
    from gpsig_amd import autodiff
    n, c, d = 9001, 64, 256
    Pn, Sn = data(n, c, d, seed=11)
    P, S = torch.tensor(Pn, device=DEV), torch.tensor(Sn, device=DEV)
    G = torch.tensor(np.random.default_rng(12).standard_normal((n, c)), device=DEV)
    first = raw_grad(P, S, G, "mix")
    again = raw_grad(P, S, G, "mix")
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    ctx = autodiff._ctx_for(P)
    try:
        ctx.set_option("wide_chunk_mb", 1)
        capped = raw_grad(P, S, G, "mix")
        capped2 = raw_grad(P, S, G, "mix")
    finally:
        ctx.set_option("wide_chunk_mb", 0)
    for a, b in zip(capped, capped2):
        assert torch.equal(a, b)
    assert torch.equal(first[0], capped[0])                 # (dP does not go through the partials)
    e = relerr(capped[1], first[1])
    print("dS, eight shares against nine", e)
    assert e <= 1e-12, e
    # and against something independent: the host reference of tests/cross_reference.py (np.longdouble closed forms)
    import cross_reference
    want = cross_reference.cross_grad("mix", Pn, Sn, G.cpu().numpy(), P0["mix"], 0.0)
    for tag, got in (("nine shares", first), ("eight shares", capped)):
        for name, a, b in zip(("dP", "dS", "g_base"), (got[0], got[1], got[2][0]), want):
            a, b = a.cpu().numpy().astype(np.longdouble), np.asarray(b)
            e = float(np.abs(a - b).max() / np.abs(b).max())
            print("gradient against the host reference,", tag, name, e)
            assert np.isfinite(a).all() and e <= 1e-9, (tag, name, e)


def test_empty_batch_and_refusals():
    from gpsig_amd import _lib
    Pn, Sn = data(16, 16, 8, seed=1)
    P, S = torch.tensor(Pn, device=DEV), torch.tensor(Sn, device=DEV)
    G = torch.ones((16, 16), dtype=torch.float64, device=DEV)
    _, dS, gb = raw_grad(P[:0], S, G[:0], "poly")
    assert bool((dS == 0).all()) and float(gb[0]) == 0.0
    with pytest.raises(NotImplementedError):
        raw_grad(P, S, G, c=65)
    with pytest.raises(NotImplementedError):
        raw_grad(P, S, G, d=4097)
    with pytest.raises(NotImplementedError):
        raw_grad(P, S, G, dtype=_lib.F32)
