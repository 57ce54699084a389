"""The training path's lag op for ragged batches (csrc/seq_lags_kernel.hpp: gpsig_seq_lags_ragged_dev / _grad through
autodiff._SeqLagsRagged) against its torch restatement autodiff._add_lags_ragged on the GPU.

relerr = max|got - want| / max|want|; 1e-12, the project's identity bound: both sides evaluate gpsig/lags.py:33 in float64 on the same
points; the reverse pass adds at most p + 1 products per element of dX in another order, dlags N L d terms in another order."""
import numpy as np
import pytest
import torch

from lags_ragged_inputs import LAGS, check_inputs

pytestmark = pytest.mark.gpu

# (N, L, d, lengths, lags): more than one wavefront of time steps with lengths at and around the 64-lane edge; more columns than a wavefront
CASES = {
    "long": (7, 130, 3, (130, 129, 65, 64, 3, 2, 1), LAGS[:2]),
    "wide": (4, 20, 70, (20, 19, 2, 1), LAGS[2:]),
}
for _N, _L, _d, _lengths, _lags in CASES.values():
    check_inputs(_lengths, _lags)


def relerr(got, want):
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def _inputs(case, nan=False, seed=0):
    N, L, d, lengths, lags = CASES[case]
    rng = np.random.default_rng(seed)
    X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1)
    G = rng.standard_normal((N, L, len(lags) + 1, d))
    if nan:
        for n, l in enumerate(lengths):
            X[n, l:] = np.nan
    dev = torch.device("cuda:0")
    return (torch.tensor(X, device=dev, requires_grad=True), torch.tensor(lags, dtype=torch.float64, device=dev, requires_grad=True),
            torch.tensor(lengths, dtype=torch.int32, device=dev), torch.tensor(G, device=dev))


@pytest.mark.parametrize("case", sorted(CASES))
def test_op_against_the_torch_restatement(case):
    from gpsig_amd import autodiff
    X, lags, lens, G = _inputs(case, nan=True)
    got = autodiff._SeqLagsRagged.apply(X, lags, lens)
    want = autodiff._add_lags_ragged(X, lags, lens)
    err = relerr(got, want)
    print(case, "forward", err)
    assert err <= 1e-12, err
    lengths = CASES[case][3]
    for n, l in enumerate(lengths):
        assert bool((got[n, l:] == got[n, l - 1]).all()), n
    one = lengths.index(1)
    assert bool((got[one, :, 1:] == X[one, 0]).all())                   # one point: the lagged copies are the point itself
    gX, gl = torch.autograd.grad(got, (X, lags), G)
    wX, wl = torch.autograd.grad(want, (X, lags), G)
    for n, l in enumerate(lengths):
        assert bool((gX[n, l:] == 0).all()), n
    for name, g, w in (("dX", gX, wX), ("dlags", gl, wl)):
        err = relerr(g, w)
        print(case, name, err)
        assert err <= 1e-12, (name, err)


def test_two_backward_calls_are_bit_equal():
    from gpsig_amd import autodiff
    X, lags, lens, G = _inputs("long")
    grads = [torch.autograd.grad(autodiff._SeqLagsRagged.apply(X, lags, lens), (X, lags), G) for _ in range(2)]
    assert bool((grads[0][0] == grads[1][0]).all()) and bool((grads[0][1] == grads[1][1]).all())


def test_padded_rows_get_exact_zeros_whatever_they_and_their_upstream_hold():
    from gpsig_amd import autodiff
    X, lags, lens, G = _inputs("long", nan=True)
    for n, l in enumerate(CASES["long"][3]):
        G[n, l:] = float("nan")
    gX, _ = torch.autograd.grad(autodiff._SeqLagsRagged.apply(X, lags, lens), (X, lags), G)
    for n, l in enumerate(CASES["long"][3]):
        assert bool((gX[n, l:] == 0).all()), n                          # (row len - 1 and its lag brackets collect the padded upstream rows)


def test_zero_upstream_gives_zero_dlags():
    from gpsig_amd import autodiff
    X, lags, lens, G = _inputs("long", nan=True)
    gX, gl = torch.autograd.grad(autodiff._SeqLagsRagged.apply(X, lags, lens), (X, lags), torch.zeros_like(G))
    assert bool((gl == 0).all()) and bool((gX == 0).all())
