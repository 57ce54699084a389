"""Ragged batches WITH LAGS in low-rank mode, each sequence on its own time axis (``lag_axis = "sequence"``): the C entry point
gpsig_lr_seq_features_ragged_lagged on the time-tiled kernels and on the wide route, in float64 and float32, the ``lengths=`` keywords of
gpsig_amd.kernels.SignatureKernel / models.SVGP.predict_f, and the training path (autodiff.SignatureKernelModule, models.SVGPModule) through
the library's lag op.

The reference for every value is the truncated sequence X[n, :len_n] evaluated on its own by the dense entry points, given the same state.

Tolerances are the project's own (the docstring of tests/test_gpu_lowrank_eval_long.py): identities between the library's own fused kernels
relerr = max|got - want| / max|want| <= 1e-12; K against oracle.LowRankOracle on the same random objects 1e-7 of the largest entry (1e-5 for the
linear kernel); float32 against float64 on the same state <= 1e-4 of the largest entry; the Python surface <= 1e-9; the training path against the
torch-op route: values <= 1e-11, gradients <= 1e-9.

Shapes.  Tiled route: c = 4, r = 3, d = 3 with two lags (9 staging rows) -- a tile is 896 steps, L = 900: lengths at the table's end, one past a
tile, at a tile, mid-tile, past a wavefront and two points; with the difference the halo point of the first tile sits on a shortened axis.
Wide route (footprints of csrc/lr_tile_plan.hpp in doubles, 19,968 fit the LDS): c = r = 8, one lag, L = 80; d = 80 gives d' = 160 and
65 c + 138 d' = 22,600, the wide route; d = 70 (d' = 140: 19,840) still fits a tile and runs on the tiled kernels at a wide block.  float32
reaches the wide route at d' = 320 (44,680 > 39,936): d = 160."""
import numpy as np
import pytest
import torch

from oracle import sigkern_oracle as O
from lags_ragged_inputs import LAGS, check_inputs
from test_gpu_lowrank_eval_long import features, host, make_kernel, oracle_for, relerr, seqs

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
T_L, T_D, T_M, T_C, T_R = 900, 3, 3, 4, 3
T_LEN = [900, 897, 896, 450, 65, 2, 1]
W_L, W_C = 80, 8
W_LEN = [80, 79, 17, 2]
S_L, S_D, S_M = 20, 3, 3
S_LEN = [20, 19, 7, 2]
R_L = 66
R_LEN = [66, 65, 33, 4, 2, 1]

check_inputs(T_LEN, LAGS[:2])
check_inputs(W_LEN, LAGS[:1])
check_inputs(S_LEN, LAGS[:1])
check_inputs(R_LEN, LAGS[:1])


def ragged(rng, lengths, L, d):
    """(the table with NaN beyond each length, the same table whole)"""
    full = seqs(rng, len(lengths), L, d).reshape(len(lengths), L, d)
    nan = full.copy()
    for n, l in enumerate(lengths):
        nan[n, l:] = np.nan
    return nan.reshape(len(lengths), L * d), full.reshape(len(lengths), L * d)


def cut(X, n, l, L, d):
    return np.ascontiguousarray(X.reshape(-1, L, d)[n:n + 1, :l].reshape(1, l * d))


def set_lags(k, lags):
    k.lags = np.asarray(lags, dtype=np.float64)
    k.lag_axis = "sequence"
    return k


def one_point_features(k, st, x, base, kw):
    """the features of a sequence of one point whose lagged copies are the point itself, by hand: the same kernel without lags on the
    d (p + 1) columns [x, x, ..], its lengthscales ls / gamma_j per block"""
    p1, d = k.num_lags + 1, k.num_features
    ls = np.concatenate([np.asarray(k.lengthscales) / g for g in np.asarray(k.gamma)])
    kw = {n: v for n, v in kw.items() if n not in ("num_lags", "lengthscales", "base")}
    k0 = make_kernel(base, 1, d * p1, k.num_levels, k.num_components, k.rank_bound, "lin", lengthscales=ls, **kw)
    return features(k0, st, np.tile(x.reshape(1, d), (1, p1)))[0]


# ---- 1. the tiled route ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("difference", [True, False])
@pytest.mark.parametrize("base", ["rbf", "linear", "matern32"])
def test_tiled_route_float64(base, difference):
    L, d, lengths = T_L, T_D, T_LEN
    rng = np.random.default_rng(31)
    X, full = ragged(rng, lengths, L, d)
    kw = dict(normalization=False, lengthscales=0.6 + rng.random(d), difference=difference, num_lags=2)
    k = set_lags(make_kernel(base, L, d, T_M, T_C, T_R, "lin", **kw), LAGS[:2])
    st = k.draw_low_rank(X=full)                                # (table-axis landmarks: any point of the state space is a valid landmark)
    F = 1 + T_C + (T_M - 1) * T_R
    hst = features(k, st, X, lengths)
    dev = features(k, st, torch.as_tensor(X, device=DEV), lengths)
    assert np.isfinite(hst).all() and (hst[:, 0] == 1.0).all()
    assert np.array_equal(hst, dev), "host-pointer and device-pointer modes differ"
    want = np.stack([features(k, st, cut(X, n, l, L, d))[0] for n, l in enumerate(lengths) if l > 1])
    e = relerr(hst[:-1], want)
    print(base, difference, "ragged with lags against the truncated sequences:", e,
          [float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(hst[:-1], want)])
    assert e <= 1e-12, e
    # the sequence of one point: no axis, its lagged copies are the point itself
    if difference:
        assert np.array_equal(hst[-1], np.eye(1, F)[0])
    else:
        w1 = one_point_features(k, st, X.reshape(-1, L, d)[-1, 0], base, kw)
        e = relerr(hst[-1], w1)
        print(base, "one point against the hand-built sequence:", e)
        assert e <= 1e-12, e
    # K against the oracle's features of each truncated sequence, assembled here
    lo = O.LowRankOracle(oracle_for(base, L, d, T_M, **kw), st.landmarks, st.jitter_diag, st.sketches)
    lo.k.lags = np.asarray(LAGS[:2])
    rows = [lo.seq_features(cut(X, n, l, L, d)) for n, l in enumerate(lengths) if l > 1]
    Kw = lo._finish(np.stack([np.concatenate([r[m] for r in rows]) @ np.concatenate([r[m] for r in rows]).T for m in range(T_M + 1)]), False)
    Kg = k.K(X, lr_state=st, lengths=lengths)[:-1, :-1]
    e = float(np.abs(Kg - Kw).max() / np.abs(Kw).max())
    print(base, difference, "K against the oracle on the truncated sequences:", e)
    assert e <= (1e-5 if base == "linear" else 1e-7), e


# ---- 2. the wide route -------------------------------------------------------------------------------------------------------------
def wide_setup(d, difference=True):
    rng = np.random.default_rng(33)
    X, full = ragged(rng, W_LEN, W_L, d)
    kw = dict(normalization=False, lengthscales=np.sqrt(d) * (0.6 + rng.random(d)), difference=difference, num_lags=1)
    k = set_lags(make_kernel("rbf", W_L, d, 3, W_C, W_C, **kw), LAGS[:1])
    return k, X, full


@pytest.mark.parametrize("difference", [True, False])
@pytest.mark.parametrize("d", [70, 80])
def test_wide_route_float64(d, difference):
    k, X, full = wide_setup(d, difference)
    # the landmarks: scaled points of the full-length sequence alone (its own axis is the table's)
    st = k.draw_low_rank(X=full[:1])
    hst = features(k, st, X, W_LEN)
    dev = features(k, st, torch.as_tensor(X, device=DEV), W_LEN)
    assert np.isfinite(hst).all() and np.array_equal(hst, dev)
    want = np.stack([features(k, st, cut(X, n, l, W_L, d))[0] for n, l in enumerate(W_LEN)])
    e = relerr(hst, want)
    print(d, difference, "wide block, ragged with lags against the truncated sequences:", e)
    assert e <= 1e-12, e
    # a landmark that is one of the full-length sequence's points stays at distance exactly 0 (kappa = 1): that row has the bits of the dense
    # call, whose cross kernel holds that property (tests/test_gpu_lowrank_eval_wide.py::test_landmarks_among_the_points)
    assert np.array_equal(hst[0], want[0])


# ---- 3. float32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["tiled", "wide"])
def test_float32(route):
    rng = np.random.default_rng(41)
    if route == "tiled":
        L, d, lengths, lags = T_L, T_D, T_LEN, LAGS[:2]
        kw = dict(normalization=True, lengthscales=0.6 + rng.random(d), num_lags=2)
        k = make_kernel("rbf", L, d, T_M, T_C, T_R, "lin", **kw)
    else:
        L, d, lengths, lags = W_L, 160, W_LEN, LAGS[:1]
        kw = dict(normalization=True, lengthscales=np.sqrt(d) * (0.6 + rng.random(d)), num_lags=1)
        k = make_kernel("rbf", L, d, 3, W_C, W_C, **kw)
    set_lags(k, lags)
    X, full = ragged(rng, lengths, L, d)
    X64 = X.astype(np.float32).astype(np.float64)
    X32 = X64.astype(np.float32)
    st = k.draw_low_rank(X=full.astype(np.float32).astype(np.float64))
    k.lr_native_f32 = True
    P32, P64 = features(k, st, X32, lengths), features(k, st, X64, lengths)
    assert P32.dtype == np.float32 and P64.dtype == np.float64 and np.isfinite(P32).all()
    e = relerr(P32, P64)
    print(route, "float32 ragged features with lags:", e)
    assert e <= 1e-4, e
    assert not np.array_equal(P32, P64.astype(np.float32)), "the float32 kernels did not run"


# ---- 4. identities with the existing entry points ---------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["tiled", "wide"])
def test_full_lengths_and_no_lags_keep_the_existing_bits(route):
    rng = np.random.default_rng(51)
    L, d, c, r = (T_L, T_D, T_C, T_R) if route == "tiled" else (W_L, 80, W_C, W_C)
    N = 3
    X = seqs(rng, N, L, d)
    ls = (1.0 if route == "tiled" else np.sqrt(d)) * (0.6 + rng.random(d))
    k = set_lags(make_kernel("rbf", L, d, 3, c, r, "lin", normalization=False, lengthscales=ls, num_lags=1), LAGS[:1])
    st = k.draw_low_rank(X=X)
    assert np.array_equal(features(k, st, X, [L] * N), features(k, st, X)), "full lengths: other bits than gpsig_lr_seq_features"
    # num_lags = 0 through the new entry point
    from gpsig_amd import kernels
    k0 = make_kernel("rbf", L, d, 3, c, r, "lin", normalization=False, lengthscales=ls)
    st0 = k0.draw_low_rank(X=X)
    lengths = np.asarray([L, L // 2 + 1, 2], dtype=np.int32)
    want = features(k0, st0, X, lengths)
    L_ = kernels._Launch(X)
    p, lr = k0._params(L_.keep, L_.dtype_id), st0.as_c(L_.keep)
    Phi, pp = L_.out(want.shape)
    import ctypes as C
    L_.ctx.call("gpsig_lr_seq_features_ragged_lagged", p, lr, L_.inp(X), N, L, C.c_void_p(lengths.ctypes.data), pp)
    assert np.array_equal(host(Phi), want), "num_lags = 0: other bits than gpsig_lr_seq_features_ragged"


# ---- 5. the Python surface ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "cuda"])
def test_python_surface_equals_the_truncated_sequences(device):
    from gpsig_amd import inducing_variables as iv, models
    L, d, M, lengths = S_L, S_D, S_M, S_LEN
    rng = np.random.default_rng(61)
    X, full = ragged(rng, lengths, L, d)
    Z = rng.standard_normal((M * (M + 1) // 2, 5, 2, 2 * d))       # (d' = d (num_lags + 1) columns)
    conv = (lambda a: torch.as_tensor(a, device=DEV)) if device else (lambda a: a)
    k = set_lags(make_kernel("rbf", L, d, M, 8, 6, normalization=False, lengthscales=np.asarray([0.7, 1.1, 0.9]), num_lags=1), LAGS[:1])
    st = k.draw_low_rank(X=full, Z=Z, increments=True)
    k.draw_low_rank = lambda *a, **kw: st                      # the evaluations that draw their own state: this one, in every call
    Xg, Zg = conv(X), conv(Z)
    m = models.SVGP(k, iv.InducingTensors(Zg, M, increments=True), q_mu=rng.standard_normal((Z.shape[1], 2)))
    cuts = [conv(cut(X, n, l, L, d)) for n, l in enumerate(lengths)]
    N = len(lengths)

    def check(name, got, want):
        e = relerr(got, want)
        print(name, "ragged with lags against the truncated sequences:", e)
        assert e <= 1e-9, (name, e)

    check("K", k.K(Xg, Xg, lr_state=st, lengths=lengths, lengths2=np.asarray(lengths)),
          np.block([[host(k.K(a, b, lr_state=st)) for b in cuts] for a in cuts]))
    Ks = host(k.K(Xg, lr_state=st, lengths=lengths))
    check("K, symmetric", Ks[np.triu_indices(N, 1)], np.asarray([host(k.K(cuts[a], cuts[b], lr_state=st))[0, 0] for a, b in zip(*np.triu_indices(N, 1))]))
    check("Kdiag", k.Kdiag(Xg, lr_state=st, lengths=lengths), np.concatenate([host(k.Kdiag(a, lr_state=st)) for a in cuts]))
    got = k.K_tens_n_seq_covs(Zg, Xg, increments=True, lengths=lengths)
    one = [k.K_tens_n_seq_covs(Zg, a, increments=True) for a in cuts]
    check("Kzz", got[0], one[0][0])
    check("Kzx", got[1], np.concatenate([host(o[1]) for o in one], axis=1))
    check("Kxx", got[2], np.concatenate([host(o[2]) for o in one]))
    got = m.predict_f(Xg, lengths=lengths)
    one = [m.predict_f(a) for a in cuts]
    check("predict_f mean", got[0], np.concatenate([host(o[0]) for o in one]))
    check("predict_f variance", got[1], np.concatenate([host(o[1]) for o in one]))


# ---- 6. training -------------------------------------------------------------------------------------------------------------------
def _covs(d, lr_hip):
    from gpsig_amd import autodiff, kernels
    N, L, M, T = len(R_LEN), R_L, 3, 6
    rng = np.random.default_rng(71)
    kern = kernels.SignatureRBF(L * d, d, M, lengthscales=np.sqrt(d) * (0.6 + rng.random(d)), low_rank=True, num_components=12, rank_bound=10, num_lags=1)
    set_lags(kern, LAGS[:1])
    mod = autodiff.SignatureKernelModule(kern, device=DEV)
    mod.lr_hip = lr_hip
    Xn, _ = ragged(rng, R_LEN, L, d)
    X = torch.tensor(Xn, device=DEV, requires_grad=True)
    Z = torch.tensor(rng.standard_normal((M * (M + 1) // 2, T, 2, 2 * d)) * 0.7, device=DEV, requires_grad=True)
    W = [torch.tensor(rng.standard_normal(s), device=DEV) for s in ((T, T), (T, N), (N,))]
    kern.rng = np.random.default_rng(11)
    outs = mod.K_tens_n_seq_covs(Z, X, increments=True, lengths=R_LEN)
    sum((o * w).sum() for o, w in zip(outs, W)).backward()
    grads = {"X": X.grad, "Z": Z.grad}
    grads.update({n: p.grad for n, p in mod.named_parameters() if p.grad is not None})
    return [o.detach() for o in outs], grads


def _svgp(d, lr_hip):
    from gpsig_amd import inducing_variables, kernels, likelihoods, models
    N, L, M, T = len(R_LEN), R_L, 3, 6
    rng = np.random.default_rng(8)
    lab = np.repeat([0, 1], N // 2)
    Xn, _ = ragged(rng, R_LEN, L, d)
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, 2 * d)) * 0.5
    kern = kernels.SignatureRBF(L * d, d, M, lengthscales=np.sqrt(d) * (0.6 + rng.random(d)), low_rank=True, num_components=12, rank_bound=10, num_lags=1)
    set_lags(kern, LAGS[:1])
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=DEV)
    m.kernel.lr_hip = lr_hip
    m.q_mu.data = torch.tensor(0.3 * rng.standard_normal((T, 1)), device=DEV)
    kern.rng = np.random.default_rng(3)
    X = torch.tensor(Xn, device=DEV, requires_grad=True)
    elbo = m.elbo(X, torch.tensor(lab[:, None].astype(np.float64), device=DEV), lengths=R_LEN)
    elbo.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.requires_grad}
    grads["X"] = X.grad
    return elbo.detach(), grads


def _compare_grads(tag, got_g, want_g):
    assert set(got_g) == set(want_g)
    seen = " ".join(want_g)
    for part in ("X", "lags", "lengthscales", "variances"):
        assert part in seen, (part, seen)
    for n in want_g:
        assert (got_g[n] is None) == (want_g[n] is None), n
        if want_g[n] is None:
            continue
        e = relerr(got_g[n], want_g[n])
        print(tag, "gradient", n, e)
        assert e <= 1e-9, (n, e)
    X = got_g["X"].reshape(len(R_LEN), R_L, -1)
    for n, l in enumerate(R_LEN):
        assert bool((X[n, l:] == 0).all()), n


@pytest.mark.parametrize("d", [2, 70])
def test_module_matches_the_torch_route(d):
    got, got_g = _covs(d, True)
    want, want_g = _covs(d, False)
    for name, g, w in zip(("Kzz", "Kzx", "Kxx"), got, want):
        e = relerr(g, w)
        print(d, name, e)
        assert e <= 1e-11, (name, e)
    assert "Z" in want_g
    _compare_grads("module d = %d" % d, got_g, want_g)


@pytest.mark.parametrize("d", [2, 70])
def test_svgp_step_matches_the_torch_route(d):
    got, got_g = _svgp(d, True)
    want, want_g = _svgp(d, False)
    e = abs(float(got) - float(want)) / max(1.0, abs(float(want)))
    print("elbo", d, float(got), float(want), e)
    assert e <= 1e-11, e
    assert any("Z" in n or "feature" in n or "inducing" in n for n in want_g), list(want_g)
    _compare_grads("svgp d = %d" % d, got_g, want_g)


def test_the_module_runs_the_lag_op(monkeypatch):
    """with lr_hip the ragged, lagged scaling goes through the library's op, and not through its torch restatement"""
    from gpsig_amd import autodiff

    def no_torch(*a, **kw):
        raise AssertionError("the lags took the torch route")

    calls = []
    op = autodiff._SeqLagsRagged

    class Spy:
        @staticmethod
        def apply(*a):
            calls.append(1)
            return op.apply(*a)

    monkeypatch.setattr(autodiff, "_add_lags_ragged", no_torch)
    monkeypatch.setattr(autodiff, "_SeqLagsRagged", Spy)
    _covs(2, True)
    assert calls
