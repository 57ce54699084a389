"""Ragged batches in low-rank mode, the part that needs no GPU: the C ABI's two entry points as the header declares and gpsig_amd._lib binds
them, the torch route of the ragged feature map (autodiff._LowRankScope._seq_torch_ragged) on CPU tensors against the per-sequence evaluation
of the truncated sequences, and the checks of ``lengths=`` in SignatureKernelModule.

relerr = max|got - want| / max|want|; 1e-12: both sides are the same torch ops in float64 on the same points, summed over the same steps
(the ragged route adds exact zeros for the steps beyond a sequence's length)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
NAMES = ("gpsig_lr_seq_features_ragged_dev", "gpsig_lr_seq_features_ragged_grad")


def relerr(got, want):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    if got.size == 0:
        return 0.0
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "gpsig_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert m, "%s is not declared in include/gpsig_hip.h" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_and_lib_binds_the_entry_points():
    from gpsig_amd import _lib
    plain = {"gpsig_lr_seq_features_dev": _header_args("gpsig_lr_seq_features_dev"), "gpsig_lr_seq_features_grad": _header_args("gpsig_lr_seq_features_grad")}
    for name, base in zip(NAMES, ("gpsig_lr_seq_features_dev", "gpsig_lr_seq_features_grad")):
        args = _header_args(name)
        # the arguments of the existing entry point plus `lengths`, directly after L
        assert len(args) == len(plain[base]) + 1
        at = [i for i, a in enumerate(args) if re.search(r"\bL$", a)][0]
        assert re.fullmatch(r"const\s+int32_t\s*\*\s*lengths", args[at + 1]), args[at + 1]
        assert [a.split()[-1] for a in args[:at + 1] + args[at + 2:]] == [a.split()[-1] for a in plain[base]]
        assert name in _lib._KERNEL_FUNCS, name
        assert len(_lib._KERNEL_FUNCS[name]) + 2 == len(args)               # (ctx, params) + the bound argument types
        assert len(_lib._KERNEL_FUNCS[name]) == len(_lib._KERNEL_FUNCS[base]) + 1


class Setup:
    """A low-rank module on the CPU, one draw, a table of N = 4 sequences of room L = 9 whose rows beyond each length are NaN, landmarks and a
    random whitening as leaves."""
    N, L, d, M, c = 4, 9, 2, 3, 4
    lengths = (9, 4, 2, 1)

    def __init__(self, difference, seed=0):
        from gpsig_amd import kernels, autodiff
        N, L, d, M, c = self.N, self.L, self.d, self.M, self.c
        rng = np.random.default_rng(seed)
        k = kernels.SignatureRBF(L * d, d, M, lengthscales=None, difference=difference, low_rank=True, num_components=c, rank_bound=c)
        k.rng = np.random.default_rng(seed + 1)
        self.mod = autodiff.SignatureKernelModule(k, device=CPU)
        self.mod.lr_hip = False
        pool = 0.7 * rng.standard_normal((2 * c + 4, d))
        self.draw = self.mod.draw_low_rank(pool.shape[0])
        self.scope = autodiff._LowRankScope(self.mod, torch.tensor(pool), self.draw)
        X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1)
        for n, l in enumerate(self.lengths):
            X[n, l:] = np.nan
        leaf = lambda a: torch.tensor(a, requires_grad=True)
        self.X, self.S, self.Wh = leaf(X), leaf(0.7 * rng.standard_normal((c, d))), leaf(rng.standard_normal((c, c)) / np.sqrt(c))
        self.scope.S, self.scope.Wh = self.S, self.Wh
        self.lens = torch.tensor(self.lengths, dtype=torch.int32)


@pytest.mark.parametrize("difference", [True, False])
def test_seq_torch_ragged_equals_the_truncated_sequences(difference):
    s = Setup(difference)
    F = 1 + s.c + (s.M - 1) * int(s.draw.sketches[0].r)
    G = torch.tensor(np.random.default_rng(3).standard_normal((s.N, F)))
    got = torch.cat(s.scope._seq_torch_ragged(s.X, s.lens), dim=1)
    assert got.shape == (s.N, F) and bool(torch.isfinite(got).all())
    rows = [torch.cat(s.scope._seq_torch(s.X[n:n + 1, :l]), dim=1) for n, l in enumerate(s.lengths)]
    want = torch.cat(rows, dim=0)
    err = relerr(got, want)
    print("features", difference, err)
    assert err <= 1e-12, err
    if difference:                                              # one point, no step: [1, 0, .., 0]
        assert bool((got[3, 0] == 1).all()) and bool((got[3, 1:] == 0).all())
    leaves = (s.X, s.S, s.Wh)
    gg = torch.autograd.grad(got, leaves, G)
    gw = torch.autograd.grad(want, leaves, G)
    assert all(bool(torch.isfinite(g).all()) for g in gg)
    for n, l in enumerate(s.lengths):
        assert bool((gg[0][n, l:] == 0).all()), n              # the padded points' rows: exact zeros
    for name, g, w in zip(("X", "S", "Wh"), gg, gw):
        e = relerr(g, w)
        print("gradient", difference, name, e)
        assert e <= 1e-12, (name, e)


def _module(low_rank=True, num_lags=0):
    from gpsig_amd import kernels, autodiff
    L, d, M = 9, 2, 3
    k = kernels.SignatureRBF(L * d, d, M, low_rank=low_rank, num_components=4, rank_bound=4, num_lags=num_lags)
    k.rng = np.random.default_rng(0)
    return autodiff.SignatureKernelModule(k, device=CPU), torch.zeros((4, L * d), dtype=torch.float64)


@pytest.mark.parametrize("bad", [[9, 4, 0, 1], [9, 4, 10, 1], [9, 4, 2], [[9, 4, 2, 1]], np.array([9.0, 4.0, 2.0, 1.0]),
                                 torch.tensor([9.0, 4.0, 2.0, 1.0])],
                         ids=["zero", "L+1", "short", "2-d", "float-numpy", "float-torch"])
def test_bad_lengths_are_value_errors(bad):
    mod, X = _module()
    with pytest.raises(ValueError):
        mod.K(X, lengths=bad)
    with pytest.raises(ValueError):
        mod.K(X, X, lengths2=bad)
    with pytest.raises(ValueError):
        mod.Kdiag(X, lengths=bad)


def test_exact_mode_and_lags_are_not_implemented():
    mod, X = _module(low_rank=False)
    with pytest.raises(NotImplementedError, match="repeating its last"):
        mod.K(X, lengths=[9, 4, 2, 1])
    mod, X = _module(num_lags=1)
    with pytest.raises(NotImplementedError, match="time axis"):
        mod.K(X, lengths=[9, 4, 2, 1])
