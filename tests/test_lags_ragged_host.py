"""Ragged batches with lags on per-sequence time axes (``lag_axis = "sequence"``), the part that needs no GPU: the torch restatement
autodiff._add_lags_ragged against autodiff._add_lags of each truncated sequence, values and autograd, and the switch on the kernel object.

relerr = max|got - want| / max|want|; 1e-12, the project's identity bound: both sides evaluate the formula of gpsig/lags.py:33 in float64 on
the same points -- a handful of roundings, the bracket found by search on one side and arithmetically on the other."""
import numpy as np
import pytest
import torch

from lags_ragged_inputs import LAGS, check_inputs

CPU = torch.device("cpu")
N, L, d = 4, 9, 2
LENGTHS = (9, 4, 2, 1)
LAG_SETS = (LAGS[:2], LAGS[2:])

check_inputs(LENGTHS, LAGS)
check_inputs((L,), LAGS)


def relerr(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def _table(nan=True, seed=0):
    X = np.cumsum(0.3 * np.random.default_rng(seed).standard_normal((N, L, d)), axis=1)
    if nan:
        for n, l in enumerate(LENGTHS):
            X[n, l:] = np.nan
    return X


def _truncated(X, lags):
    """Row blocks of _add_lags on each truncated sequence; a sequence of one point by the rule: its lagged copies are the point itself."""
    from gpsig_amd import autodiff
    rows = []
    for n, l in enumerate(LENGTHS):
        if l == 1:
            rows.append(X[n:n + 1, :1, None, :].expand(1, 1, lags.shape[0] + 1, d))
        else:
            rows.append(autodiff._add_lags(X[n:n + 1, :l], lags))
    return rows


@pytest.mark.parametrize("lagset", LAG_SETS, ids=["odd", "clamped-and-tiny"])
def test_add_lags_ragged_is_add_lags_of_each_truncated_sequence(lagset):
    from gpsig_amd import autodiff
    X, lags = torch.tensor(_table()), torch.tensor(lagset, dtype=torch.float64)
    lens = torch.tensor(LENGTHS, dtype=torch.int32)
    got = autodiff._add_lags_ragged(X, lags, lens)
    assert got.shape == (N, L, len(lagset) + 1, d)
    assert bool(torch.isfinite(got).all())                              # NaN in the padded input rows never reaches the output
    for n, (l, want) in enumerate(zip(LENGTHS, _truncated(X, lags))):
        err = relerr(got[n:n + 1, :l], want)
        print("sequence", n, "length", l, err)
        assert err <= 1e-12, (n, err)
        assert bool((got[n, l:] == got[n, l - 1]).all()), n             # rows >= len repeat row len - 1
    assert bool((got[3, :, 1:] == X[3, 0]).all())                       # one point: the lagged copies are the point itself


@pytest.mark.parametrize("lagset", LAG_SETS, ids=["odd", "clamped-and-tiny"])
def test_full_lengths_equal_add_lags(lagset):
    from gpsig_amd import autodiff
    X, lags = torch.tensor(_table(nan=False)), torch.tensor(lagset, dtype=torch.float64)
    got = autodiff._add_lags_ragged(X, lags, torch.full((N,), L, dtype=torch.int32))
    err = relerr(got, autodiff._add_lags(X, lags))
    print("full lengths", err)
    assert err <= 1e-12, err


@pytest.mark.parametrize("lagset", LAG_SETS, ids=["odd", "clamped-and-tiny"])
def test_autograd_is_that_of_the_truncated_sequences(lagset):
    from gpsig_amd import autodiff
    p = len(lagset)
    G = torch.tensor(np.random.default_rng(5).standard_normal((N, L, p + 1, d)))
    for n, l in enumerate(LENGTHS):
        G[n, l:] = 0.0                                                  # the repeated rows are checked on their own below
    X = torch.tensor(_table(), requires_grad=True)
    lags = torch.tensor(lagset, dtype=torch.float64, requires_grad=True)
    got = autodiff._add_lags_ragged(X, lags, torch.tensor(LENGTHS, dtype=torch.int32))
    gX, gl = torch.autograd.grad(got, (X, lags), G, retain_graph=True)
    Xw = torch.tensor(np.nan_to_num(_table()), requires_grad=True)
    lw = torch.tensor(lagset, dtype=torch.float64, requires_grad=True)
    want = _truncated(Xw, lw)
    wX, wl = torch.autograd.grad(want, (Xw, lw), [G[n:n + 1, :l] for n, l in enumerate(LENGTHS)], allow_unused=True)
    for n, l in enumerate(LENGTHS):
        assert bool((gX[n, l:] == 0).all()), n                          # the padded rows: exact zeros
        assert bool((wX[n, l:] == 0).all()), n
    for name, g, w in (("dX", gX, wX), ("dlags", gl, wl)):
        err = relerr(g, w)
        print(name, err)
        assert err <= 1e-12, (name, err)
    # the gradients of the output rows >= len go to the sources of row len - 1
    H = torch.zeros_like(G)
    H[1, 6] = 1.0
    H2 = torch.zeros_like(G)
    H2[1, LENGTHS[1] - 1] = 1.0
    a = torch.autograd.grad(got, (X, lags), H, retain_graph=True)
    b = torch.autograd.grad(got, (X, lags), H2)
    assert all(bool((u == v).all()) for u, v in zip(a, b))


def test_one_point_adds_exact_zero_to_the_lags_gradient():
    from gpsig_amd import autodiff
    X = torch.tensor(_table()[3:4], requires_grad=True)
    lags = torch.tensor(LAGS[:2], dtype=torch.float64, requires_grad=True)
    out = autodiff._add_lags_ragged(X, lags, torch.tensor([1], dtype=torch.int32))
    gX, gl = torch.autograd.grad(out, (X, lags), torch.ones_like(out))
    assert bool((gl == 0).all())
    assert bool((gX[0, 0] == L * 3).all()) and bool((gX[0, 1:] == 0).all())


def test_header_declares_and_lib_binds_the_entry_points():
    import os
    import re
    from gpsig_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpsig_hip.h")).read()

    def args(name):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
        assert m, "%s is not declared in include/gpsig_hip.h" % name
        return [a.strip().split()[-1].lstrip("*") for a in m.group(1).split(",")]

    # the evaluation entry point: the arguments of gpsig_lr_seq_features_ragged
    assert args("gpsig_lr_seq_features_ragged_lagged") == args("gpsig_lr_seq_features_ragged")
    assert _lib._KERNEL_FUNCS["gpsig_lr_seq_features_ragged_lagged"] == _lib._KERNEL_FUNCS["gpsig_lr_seq_features_ragged"]
    assert args("gpsig_seq_lags_ragged_dev") == ["ctx", "X", "lengths", "lags", "N", "L", "d", "p", "out"]
    assert args("gpsig_seq_lags_ragged_grad") == ["ctx", "X", "lengths", "lags", "G", "N", "L", "d", "p", "dX", "dlags"]
    for name in ("gpsig_seq_lags_ragged_dev", "gpsig_seq_lags_ragged_grad"):
        assert len(_lib._PLAIN[name][0]) == len(args(name))
    assert _lib.load().gpsig_abi_version() == 1


def _module(num_lags=1):
    from gpsig_amd import kernels, autodiff
    M = 3
    k = kernels.SignatureRBF(L * d, d, M, low_rank=True, num_components=4, rank_bound=4, num_lags=num_lags)
    k.rng = np.random.default_rng(0)
    return autodiff.SignatureKernelModule(k, device=CPU), torch.tensor(_table().reshape(N, L * d))


def test_module_takes_lengths_with_lags_on_the_sequence_axis():
    """The module's evaluations refuse CPU tensors where they open the low-rank scope (the product has no CPU path); everything before and
    behind that gate is torch ops under lr_hip = False.  With the gate stood in, K of a ragged table with lags runs on the CPU."""
    from gpsig_amd import autodiff
    mod, X = _module()
    mod.kern.lag_axis = "sequence"
    mod.lr_hip = False
    X.requires_grad_(True)
    with pytest.raises(RuntimeError, match="no CPU path"):             # past the scaling: no longer the refusal of lengths with lags
        mod.K(X, lengths=list(LENGTHS))

    def open_on_cpu(lr, *points):
        pool = torch.cat([p_.reshape(-1, p_.shape[-1]) for p_ in points], dim=0)
        mod._lr = autodiff._LowRankScope(mod, pool, lr if lr is not None else mod.draw_low_rank(pool.shape[0]))

    mod._lr_open = open_on_cpu
    K = mod.K(X, lengths=list(LENGTHS))
    assert K.shape == (N, N) and bool(torch.isfinite(K).all())
    K.sum().backward()
    g = X.grad.reshape(N, L, d)
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(mod.raw_lags.grad).all())
    for n, l in enumerate(LENGTHS):
        assert bool((g[n, l:] == 0).all()), n
    # the scaled sequences are the restatement's lagged copies under the module's lengthscales and lag weights
    Xs = mod._scaled(X.detach(), lengths=list(LENGTHS))
    mod._ragged = None
    want = autodiff._add_lags_ragged(X.detach().reshape(N, L, d), mod.lags, torch.tensor(LENGTHS)) / mod.lengthscales * mod.gamma[:, None]
    assert relerr(Xs, want.reshape(N, L, -1)) <= 1e-12


def test_lag_axis_other_values_are_value_errors():
    mod, X = _module()
    mod.kern.lag_axis = "nonsense"
    with pytest.raises(ValueError, match="lag_axis"):
        mod.K(X, lengths=list(LENGTHS))
    from gpsig_amd import kernels
    k = kernels.SignatureRBF(L * d, d, 3, low_rank=True, num_components=4, rank_bound=4, num_lags=1)
    k.lag_axis = "nonsense"
    with pytest.raises(ValueError, match="lag_axis"):
        k._ragged_lengths(list(LENGTHS), np.zeros((N, L * d)))


def test_the_default_still_refuses():
    mod, X = _module()
    assert mod.kern.lag_axis == "table"
    with pytest.raises(NotImplementedError, match="time axis"):
        mod.K(X, lengths=list(LENGTHS))
