"""SignatureMix on the wide-state-space route (csrc/wide_kernels.hpp: WIDE_KD_MIX), the identity it rests on, on the CPU against oracle/sigkern_oracle.py.

With a = <z, x> - |z|^2/2 - |x|^2/2 (what the route's one dgemm of augmented rows yields), hz = |z|^2/2, hx = |x|^2/2, q = 1 - p0 and
psi(a) = p0 exp(a) + q a:      kappa_mix(z, x) = psi(a) + q (hz + hx).
A one-sided term is the same number at both ends of a difference taken along the other side, so it cancels there; which terms a primitive's kernels
must add is decided in ONE host function (csrc/wide_api.hip: mix_sides), and this file pins its table:

    Kzx                 the x term stays without increments, the z term stays without the time difference
    sequence lattices   both stay without differences, none with
    Kzz                 both stay without increments, none with

Each case: psi plus the terms the table keeps, pushed through the oracle's recursions, matches base_mix to 1e-13 (relative to the largest entry), and
dropping a term the table keeps is off by more than 1e-3."""
import numpy as np
import pytest

from oracle import sigkern_oracle as O

P0 = 0.4


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))


def _parts(Z, X, p0=P0):
    """(psi(a), q hz as a column, q hx as a row) of the points Z (n, d) against X (m, d)"""
    hz, hx = 0.5 * (Z * Z).sum(-1), 0.5 * (X * X).sum(-1)
    a = Z @ X.T - hz[:, None] - hx[None, :]
    q = 1.0 - p0
    return p0 * np.exp(a) + q * a, q * hz[:, None] * np.ones_like(a), q * hx[None, :] * np.ones_like(a)


def _check(levels, psi, tz, tx, keep_z, keep_x, want):
    got = levels(psi + (tz if keep_z else 0.0) + (tx if keep_x else 0.0))
    assert rel(got, want) < 1e-13, rel(got, want)
    # the terms the table drops really are dead weight ...
    assert rel(levels(psi + tz + tx), want) < 1e-13
    # ... and the ones it keeps are not
    if keep_z:
        assert rel(levels(psi + (tx if keep_x else 0.0)), want) > 1e-3
    if keep_x:
        assert rel(levels(psi + (tz if keep_z else 0.0)), want) > 1e-3


@pytest.mark.parametrize("d", [28, 126])
@pytest.mark.parametrize("difference", [True, False])
@pytest.mark.parametrize("increments", [True, False])
def test_tensor_vs_sequence_terms(d, difference, increments):
    rng = np.random.default_rng(d + 2 * difference + increments)
    M, T, N, L = 3, 5, 4, 7
    lt = M * (M + 1) // 2
    Z = rng.standard_normal((lt, T, 2, d) if increments else (lt, T, d)) / np.sqrt(d)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.5 / np.sqrt(d), axis=1)
    Zf, Xf = Z.reshape(-1, d), X.reshape(N * L, d)

    def levels(Mf):
        if increments:
            Mf = Mf.reshape(lt, T, 2, N, L)
            Mf = Mf[:, :, 1] - Mf[:, :, 0]
        else:
            Mf = Mf.reshape(lt, T, N, L)
        return O.signature_kern_tens_vs_seq_first_order(Mf, M, difference=difference)

    want = levels(O.base_mix(Zf, Xf, mixing=P0))
    psi, tz, tx = _parts(Zf, Xf)
    _check(levels, psi, tz, tx, keep_z=not difference, keep_x=not increments, want=want)


@pytest.mark.parametrize("d", [28, 126])
@pytest.mark.parametrize("difference", [True, False])
def test_sequence_lattice_terms(d, difference):
    rng = np.random.default_rng(10 + d + difference)
    M, N1, N2, L1, L2 = 3, 3, 2, 6, 5
    X = np.cumsum(rng.standard_normal((N1, L1, d)) * 0.5 / np.sqrt(d), axis=1)
    Y = np.cumsum(rng.standard_normal((N2, L2, d)) * 0.5 / np.sqrt(d), axis=1)
    Xf, Yf = X.reshape(-1, d), Y.reshape(-1, d)

    def levels(Mf):
        return O.signature_kern_first_order(Mf.reshape(N1, L1, N2, L2), M, difference=difference)

    want = levels(O.base_mix(Xf, Yf, mixing=P0))
    psi, tz, tx = _parts(Xf, Yf)
    _check(levels, psi, tz, tx, keep_z=not difference, keep_x=not difference, want=want)


@pytest.mark.parametrize("d", [28, 126])
@pytest.mark.parametrize("increments", [True, False])
def test_tensor_gram_terms(d, increments):
    rng = np.random.default_rng(20 + d + increments)
    M, T = 3, 6
    lt = M * (M + 1) // 2
    Z = rng.standard_normal((lt, T, 2, d) if increments else (lt, T, d)) / np.sqrt(d)
    E = 2 if increments else 1

    def blocks(fn):          # per component: its points against themselves
        return np.stack([fn(Z[k].reshape(T * E, d)) for k in range(lt)])

    def levels(Mb):
        if increments:
            Mb = Mb.reshape(lt, T, 2, T, 2)
            Mb = Mb[:, :, 1, :, 1] + Mb[:, :, 0, :, 0] - Mb[:, :, 1, :, 0] - Mb[:, :, 0, :, 1]
        return O.tensor_kern(Mb, M)

    want = levels(blocks(lambda z: O.base_mix(z, None, mixing=P0)))
    psi, tz, tx = (blocks(lambda z, i=i: _parts(z, z)[i]) for i in range(3))
    _check(levels, psi, tz, tx, keep_z=not increments, keep_x=not increments, want=want)
