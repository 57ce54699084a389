"""The host reference of the cross ops (tests/cross_reference.py) against autodiff.base_kernel_matrix under torch autograd in float64 on the CPU:
what lets the GPU tests of tests/test_gpu_cross_edges.py trust it.  Three small shapes per family on the data of tests/test_gpu_lowrank_cross.py
and tests/test_gpu_lowrank_spectral_wide.py -- the grid of 1/256, half the landmarks copied from points, so every shape has coincident pairs
(asserted) and both sides see distance exactly 0 there.  relerr = max|got - want| / max|want|: 1e-11 for values, 1e-9 for each gradient."""
import numpy as np
import pytest
import torch

import cross_reference as R
from test_gpu_lowrank_cross import P0, P1, data
from test_gpu_lowrank_spectral_wide import NAMES, data as spectral_data

SHAPES = [(7, 1, 2), (16, 17, 5), (33, 40, 67)]             # (d = 1 has no cosine gradient to compare: the value is +-1)
SPECTRAL_SHAPES = [(7, 1, 3, 1), (16, 17, 33, 3), (21, 40, 67, 4)]


def relerr(got, want):
    got, want = np.asarray(got, dtype=np.float64), want.detach().numpy()
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def coincident(P, S):
    return int((np.abs(P[:, None, :] - S[None, :, :]).max(-1) == 0).sum())


@pytest.mark.parametrize("base", R.FAMILIES)
@pytest.mark.parametrize("n,c,d", SHAPES)
def test_closed_forms_match_torch_autograd(base, n, c, d):
    from gpsig_amd import autodiff
    Pn, Sn = data(n, c, d, seed=n + c + d)
    assert coincident(Pn, Sn) >= (c + 1) // 2
    Gn = np.random.default_rng(3).standard_normal((n, c))
    p0, p1 = P0.get(base, 0.0), P1.get(base, 0.0)
    leaf = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    P, S, tp0 = leaf(Pn), leaf(Sn), leaf(p0)
    leaves = (P, S) + ((tp0,) if base in P0 else ())
    want = autodiff.base_kernel_matrix(base, P, S, p0=tp0 if base in P0 else None, p1=p1)
    gw = torch.autograd.grad(want, leaves, torch.tensor(Gn))
    err = relerr(R.cross(base, Pn, Sn, p0, p1), want)
    print("values", base, n, c, d, err)
    assert err <= 1e-11, err
    got = R.cross_grad(base, Pn, Sn, Gn, p0, p1)
    for name, a, b in zip(("dP", "dS", "g_base"), got, gw):
        e = relerr(a, b)
        print("gradient", base, n, c, d, name, e)
        assert e <= 1e-9, (name, e)
    if base not in P0:
        assert float(got[2]) == 0.0


@pytest.mark.parametrize("family", R.SPECTRAL_FAMILIES)
@pytest.mark.parametrize("n,c,d,Q", SPECTRAL_SHAPES)
def test_spectral_matches_torch_autograd(family, n, c, d, Q, monkeypatch):
    from gpsig_amd import autodiff
    monkeypatch.setattr(R, "BLOCK_ELEMS", 5 * c * d)         # several blocks of rows, a short last one
    arrays = spectral_data(n, c, d, Q, seed=n + c + d + Q)
    assert coincident(arrays[0], arrays[1]) >= (c + 1) // 2
    Gn = np.random.default_rng(3).standard_normal((n, c))
    leaves = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in arrays]
    P, S, al, om, ga = leaves
    want = autodiff.base_kernel_matrix("spectral", P, S, spectral=(family, al, om, ga))
    gw = torch.autograd.grad(want, leaves, torch.tensor(Gn))
    err = relerr(R.spectral_cross(family, *arrays), want)
    print("values", family, n, c, d, Q, err)
    assert err <= 1e-11, err
    for name, a, b in zip(NAMES, R.spectral_cross_grad(family, *arrays, Gn), gw):
        e = relerr(a, b)
        print("gradient", family, n, c, d, Q, name, e)
        assert e <= 1e-9, (name, e)


def test_nothing_flows_through_a_zero_distance():
    """one point, one landmark, the same: the Matern families and the exponential envelope give a zero gradient, not NaN"""
    P = np.array([[0.5, -1.25, 2.0]])
    G = np.ones((1, 1))
    for base in ("matern12", "matern32", "matern52"):
        assert float(R.cross(base, P, P)[0, 0]) == pytest.approx(1.0, abs=1e-19)
        dP, dS, gb = R.cross_grad(base, P, P, G)
        assert (dP == 0).all() and (dS == 0).all() and gb == 0
    al, om, ga = np.array([0.7]), np.array([[0.25, 0.5, -1.0]]), np.array([[1.0, 0.5, 1.5]])
    out = R.spectral_cross_grad("exp", P, P, al, om, ga, G)
    assert all(np.isfinite(np.asarray(o, dtype=np.float64)).all() for o in out)
    assert (out[0] == 0).all() and (out[1] == 0).all() and float(out[2][0]) == 1.0 and (out[3] == 0).all() and (out[4] == 0).all()
