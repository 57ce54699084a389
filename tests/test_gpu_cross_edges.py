"""The three families of float64 matrix-core cross kernels where their loops wrap and their shapes end: the training cross op (gpsig_lr_cross /
gpsig_lr_cross_grad, csrc/lr_cross_kernel.hpp), the wide spectral cross op (gpsig_spectral_cross / _grad beyond 32 columns,
csrc/lr_cross_spectral_kernel.hpp) and the evaluation form (lr_cross_eval_kernel behind gpsig_lr_seq_features, _ragged and gpsig_lr_tens_features).
All of them launch at most 1,024 workgroups of 64 points and stride over the rest; the shapes here are the smallest that enter a second round,
several shares of the landmark sums with a short last one, both chunk loops of the spectral op, nt = (c + 15) / 16 in {1, 2, 3, 4}, and
d in {1, .., 4, 63, 64, 128, 4096}.

The two raw ops are compared with the host reference of tests/cross_reference.py (np.longdouble; tests/test_cross_reference.py pins it to
autodiff.base_kernel_matrix under torch autograd) on the data of tests/test_gpu_lowrank_cross.py: a grid of 1/256, half the landmarks copied from
points.  relerr = max|got - want| / max|want|: 1e-11 for values, 1e-9 for each gradient.  The evaluation form goes through the public entry points:
a call of more than 65,536 points must have the bits of the same call in chunks of one round each (wide_chunk_mb = 1, the regime of
tests/test_gpu_lowrank_eval_wide.py) and lie within the project's 1e-9 per feature column scale of the multi-pass route, 1e-4 of the largest entry
for float32 against float64.

The largest errors a run on an MI355X printed, by group (value, gradient):
  training, rounds and many shares        (n = 65,617, c = 17, d = 5)          2.8e-16, 3.1e-15 (g_base of mix)
  training, a short last share            (n = 2,051, c = 40, d = 67)          2.3e-16, 1.8e-15 (g_base of mix)
  training, c edges                       (c in 16, 32, 33, 48, 49)            7.5e-17, 1.3e-14 (g_base of poly, c = 48)
  training, d edges                       (d in 1 .. 4, 63, 64, 128, 4096)     3.0e-16, 1.1e-15 (dP of rbf, d = 63)
  training, padded rows                   (n = 40, 13 dead)                    -, 7.6e-16 (dS of matern32)
  training, 9,001 points                  (tests/test_gpu_lowrank_cross.py)    -, 1.3e-15 (dS, eight shares)
  spectral, rounds                        (n = 65,617, c = 5, d = 33, Q = 2)   5.8e-16, 1.1e-14 (dalpha of rbf)
  spectral, forward chunks and Q = 64     (n = 1,030, c = 5, d = 33)           1.1e-16, 1.9e-15 (dgamma); K and dP bit-equal
  spectral, c and d edges                                                      3.3e-16, 3.4e-15 (dgamma, d = 4096)
  evaluation, float64 sequences           (937 x 70, d = 160)                  bit-equal to the chunks; 0.0 against the multi-pass route
  evaluation, ragged                      (lengths 70, 1, 33, 69)              bit-equal to the chunks; 0.0 against the multi-pass route
  evaluation, float32 sequences           (937 x 70, d = 320)                  bit-equal to the chunks; 4.0e-7 against float64
  evaluation, float64 tensors             (T = 2,190, M = 5, d = 240)          bit-equal to the chunks; 0.0 against the multi-pass route"""
import numpy as np
import pytest
import torch

import cross_reference as R
from test_gpu_lowrank_cross import P0, P1, data, raw_grad, spec_of
from test_gpu_lowrank_eval_long import both_routes, colerr, features, host, seqs, with_lr_fused
from test_gpu_lowrank_eval_wide import make_kernel, tens_features, wide_ls, with_chunk_mb
from test_gpu_lowrank_spectral_wide import NAMES, data as spectral_data, on_device, raw_grad as spectral_raw_grad

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
VALUE_BOUND, GRAD_BOUND = 1e-11, 1e-9


def relerr(got, want):
    """against the longdouble reference, in longdouble"""
    got = np.asarray(host(got), dtype=R.LD)
    want = np.asarray(want, dtype=R.LD)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + R.LD(1e-300)))


def report(group, case, value, grads):
    """one line per case, as the existing tests print theirs: the value error and every gradient's"""
    print("cross-edges", group, *case, "values", value, *(x for ne in grads for x in ne))


# ---- the training cross op --------------------------------------------------------------------------------------------------------------------
def check_cross(group, base, n, c, d, seed):
    from gpsig_amd import autodiff
    Pn, Sn = data(n, c, d, seed)
    Gn = np.random.default_rng(seed + 1).standard_normal((n, c))
    leaf = lambda a: torch.tensor(a, device=DEV, requires_grad=True)
    P, S = leaf(Pn), leaf(Sn)
    p0 = leaf(np.float64(P0[base])) if base in P0 else None
    leaves = (P, S) + ((p0,) if p0 is not None else ())
    got = autodiff._LrCross.apply(P, S, p0, spec_of(base))
    grads = torch.autograd.grad(got, leaves, torch.tensor(Gn, device=DEV))
    args = (P0.get(base, 0.0), P1.get(base, 0.0))
    err = relerr(got, R.cross(base, Pn, Sn, *args))
    errs = [(name, relerr(a, b)) for name, a, b in zip(("dP", "dS", "g_base"), grads, R.cross_grad(base, Pn, Sn, Gn, *args))]
    report(group, (base, n, c, d), err, errs)
    assert err <= VALUE_BOUND, err
    for name, e in errs:
        assert e <= GRAD_BOUND, (name, e)
    assert len(errs) == (3 if base in P0 else 2)


@pytest.mark.parametrize("base", ["rbf", "mix", "matern32"])
def test_training_rounds_and_many_shares(base):
    """65,617 points: 1,024 workgroups and two more blocks in a second round, the last with 17 rows (one full wavefront, one with a single row,
    two empty); 65 shares of 1,012 points of the landmark sums.  mix: g_base too (the per-lane accP carried across the rounds)."""
    check_cross("training-rounds", base, 65617, 17, 5, seed=21)


@pytest.mark.parametrize("base", R.FAMILIES)
def test_training_short_last_share(base):
    """2,051 points are three shares of 684, the last of 683: its final step of 4 is cut; c = 40 is nt == 3; d = 67 ends three columns into
    its second tile"""
    check_cross("training-share", base, 2051, 40, 67, seed=22)


@pytest.mark.parametrize("base", ["rbf", "poly"])
@pytest.mark.parametrize("c", [16, 32, 33, 48, 49])
def test_training_c_edges(base, c):
    check_cross("training-c", base, 20, c, 9, seed=23 + c)


@pytest.mark.parametrize("base,d", [("rbf", 1)] + [(b, d) for d in (2, 3, 4, 63, 64, 128, 4096) for b in ("rbf", "poly", "matern52")])
def test_training_d_edges(base, d):
    check_cross("training-d", base, 33, 5 if d <= 4 else 64, d, seed=24 + d)


def test_training_padded_rows_take_no_part():
    """NaN in P with zeros in G: exact zeros in dP, the other sums as if the rows were not there (against the reference on the live rows; the
    column sums of this op are per lane, so bit equality with a call on the live rows is not promised)"""
    n, c, d = 40, 9, 40
    Pn, Sn = data(n, c, d, seed=5)
    rng = np.random.default_rng(6)
    dead = np.sort(rng.choice(n, 13, replace=False))
    live = np.setdiff1d(np.arange(n), dead)
    Sn[: (c + 1) // 2] = Pn[live[: (c + 1) // 2]]           # the copied landmarks are live points
    Gn = rng.standard_normal((n, c))
    want_P, want_G = Pn[live].copy(), Gn[live].copy()
    Pn[dead] = np.nan
    Gn[dead] = 0.0
    P, S, G = on_device((Pn, Sn, Gn))
    for base in R.FAMILIES:
        dP, dS, gb = raw_grad(P, S, G, base)
        assert bool((dP[dead] == 0).all())                  # written, exactly zero
        assert bool(torch.isfinite(dP).all()) and bool(torch.isfinite(dS).all()) and bool(torch.isfinite(gb[0]))
        wP, wS, wb = R.cross_grad(base, want_P, Sn, want_G, P0.get(base, 0.0), P1.get(base, 0.0))
        errs = [("dP", relerr(dP[live], wP)), ("dS", relerr(dS, wS))]
        if base in P0:
            errs.append(("g_base", relerr(gb[0], wb)))
        else:
            assert float(gb[0]) == 0.0
        report("training-padded", (base, n, c, d), 0.0, errs)
        for name, e in errs:
            assert e <= GRAD_BOUND, (base, name, e)


# ---- the wide spectral cross op ---------------------------------------------------------------------------------------------------------------
def check_spectral(group, family, n, c, d, Q, seed):
    from gpsig_amd import autodiff
    arrays = spectral_data(n, c, d, Q, seed)
    Gn = np.random.default_rng(seed + 1).standard_normal((n, c))
    leaves = on_device(arrays, requires_grad=True)
    got = autodiff._SpectralCross.apply(*leaves, family)
    grads = torch.autograd.grad(got, leaves, torch.tensor(Gn, device=DEV))
    err = relerr(got, R.spectral_cross(family, *arrays))
    errs = [(name, relerr(a, b)) for name, a, b in zip(NAMES, grads, R.spectral_cross_grad(family, *arrays, Gn))]
    report(group, (family, n, c, d, Q), err, errs)
    assert err <= VALUE_BOUND, err
    for name, e in errs:
        assert e <= GRAD_BOUND, (name, e)


@pytest.mark.parametrize("family", R.SPECTRAL_FAMILIES)
def test_spectral_rounds(family):
    """65,617 points: a second round of the phase kernel, the value kernel and the points kernel, 65 shares in the landmarks kernel"""
    check_spectral("spectral-rounds", family, 65617, 5, 33, 2, seed=31)


def test_spectral_forward_chunks_and_the_widest_q():
    """Q = 64 under a budget of 1 MB: the forward pass has room for 1,024 points' phases and runs chunks of 1,024 and 6 points; the reverse pass
    for 73 points and runs fifteen chunks"""
    from gpsig_amd import autodiff
    family, n, c, d, Q = "mixed", 1030, 5, 33, 64
    arrays = spectral_data(n, c, d, Q, seed=32)
    Gn = np.random.default_rng(33).standard_normal((n, c))
    ten = on_device(arrays)
    G = torch.tensor(Gn, device=DEV)
    K = autodiff._SpectralCross.apply(*ten, family)
    whole = spectral_raw_grad(*ten, G, family)
    ctx = autodiff._ctx_for(G)
    try:
        ctx.set_option("wide_chunk_mb", 1)
        K_capped = autodiff._SpectralCross.apply(*ten, family)
        capped = spectral_raw_grad(*ten, G, family)
    finally:
        ctx.set_option("wide_chunk_mb", 0)
    err = relerr(K, R.spectral_cross(family, *arrays))
    want = R.spectral_cross_grad(family, *arrays, Gn)
    errs = [(name + tag, relerr(a, b)) for tag, grads in (("", whole), (" capped", capped)) for name, a, b in zip(NAMES, grads, want)]
    report("spectral-chunks", (family, n, c, d, Q), err, errs)
    assert torch.equal(K, K_capped)
    assert err <= VALUE_BOUND, err
    assert torch.equal(whole[0], capped[0])                 # (dP does not go through the partials)
    for name, e in errs:
        assert e <= GRAD_BOUND, (name, e)


@pytest.mark.parametrize("c", [16, 33, 48, 49])
def test_spectral_c_edges(c):
    check_spectral("spectral-edges", "mixed", 20, c, 40, 3, seed=34 + c)


@pytest.mark.parametrize("d", [33, 34, 35, 36, 63, 64, 128, 4096])
def test_spectral_d_edges(d):
    check_spectral("spectral-edges", "mixed", 20, 17, d, 2, seed=35 + d)


# ---- the evaluation form, through the public entry points ------------------------------------------------------------------------------------
E_N, E_L, E_C, E_M = 937, 70, 8, 3
E_LENGTHS = np.resize(np.array([70, 1, 33, 69], dtype=np.int32), E_N)


@pytest.fixture(scope="module")
def table_f64():
    """937 sequences of 70 points in 160 columns (65,590 points), on the device; left unchanged by the tests that share it"""
    rng = np.random.default_rng(91)
    d = 160
    X = seqs(rng, E_N, E_L, d)
    return d, wide_ls(rng, d), X[:8].copy(), torch.as_tensor(X, device=DEV)


def in_chunks(fn):
    """the default call and the same call under wide_chunk_mb = 1: equal bits"""
    whole = fn()
    parts = with_chunk_mb(1, fn)
    assert np.isfinite(whole).all() and whole.dtype == parts.dtype and np.array_equal(whole, parts)
    return whole


@pytest.mark.parametrize("base", ["rbf", "matern32"])
def test_eval_rounds_float64(base, table_f64):
    """one launch of 65,590 points against chunks of 234 sequences, one round each; and against the multi-pass route"""
    d, ls, head, X = table_f64
    k = make_kernel(base, E_L, d, E_M, E_C, E_C, normalization=False, lengthscales=ls)
    st = k.draw_low_rank(X=head)
    got, want = both_routes(k, st, X)                       # (asserts 1e-9 per feature column scale)
    whole = in_chunks(lambda: features(k, st, X))
    assert np.array_equal(whole, got)
    report("eval-float64", (base, E_N, E_L, d), colerr(got, want), [])


@pytest.mark.parametrize("base", ["rbf", "matern32"])
def test_eval_rounds_ragged(base, table_f64):
    """the same table with lengths cycling through (70, 1, 33, 69) and NaN beyond them; the multi-pass route sees the sequences of one length
    as a dense batch of their truncated copies"""
    d, ls, head, full = table_f64
    X = full.clone().reshape(E_N, E_L, d)
    for l in (1, 33, 69):
        X[torch.as_tensor(E_LENGTHS == l, device=DEV), l:] = float("nan")
    X = X.reshape(E_N, E_L * d)
    k = make_kernel(base, E_L, d, E_M, E_C, E_C, normalization=False, lengthscales=ls)
    st = k.draw_low_rank(X=head)
    got = in_chunks(lambda: features(k, st, X, E_LENGTHS))
    assert (got[:, 0] == 1.0).all()
    want = np.empty_like(got)
    want[E_LENGTHS == 1] = np.eye(1, got.shape[1])[0]       # (a single point has no increments: the constant feature alone)
    for l in (70, 33, 69):
        rows = torch.as_tensor(E_LENGTHS == l, device=DEV)
        Xl = full.reshape(E_N, E_L, d)[rows, :l].reshape(-1, l * d).contiguous()
        want[E_LENGTHS == l] = with_lr_fused(0, lambda: features(k, st, Xl))
    e = colerr(got, want)
    report("eval-ragged", (base, E_N, E_L, d), e, [])
    assert e <= 1e-9, e


def test_eval_rounds_float32():
    d = 320
    rng = np.random.default_rng(92)
    X64 = seqs(rng, E_N, E_L, d).astype(np.float32).astype(np.float64)
    k = make_kernel("rbf", E_L, d, E_M, E_C, E_C, normalization=True, lengthscales=wide_ls(rng, d))
    st = k.draw_low_rank(X=X64[:8])
    k.lr_native_f32 = True
    X32 = torch.as_tensor(X64.astype(np.float32), device=DEV)
    P32 = in_chunks(lambda: features(k, st, X32))
    P64 = features(k, st, torch.as_tensor(X64, device=DEV))
    assert P32.dtype == np.float32 and P64.dtype == np.float64
    e = float(np.abs(P32 - P64).max() / np.abs(P64).max())
    report("eval-float32", ("rbf", E_N, E_L, d), e, [])
    assert e <= 1e-4, e
    assert not np.array_equal(P32, P64.astype(np.float32)), "the float32 kernels did not run: every entry equals the rounded float64 result"


def test_eval_rounds_tensors_float64():
    """2,190 inducing tensors with increments at M = 5: 15 x 2,190 x 2 = 65,700 points"""
    M, c, d, T = 5, 16, 240, 2190
    rng = np.random.default_rng(93)
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d))
    k = make_kernel("rbf", E_L, d, M, c, c, normalization=False, lengthscales=wide_ls(rng, d))
    st = k.draw_low_rank(Z=Z[:, :8].copy(), increments=True)
    Z = torch.as_tensor(Z, device=DEV)
    got = in_chunks(lambda: tens_features(k, st, Z, True))
    want = with_lr_fused(0, lambda: tens_features(k, st, Z, True))
    e = colerr(got, want)
    report("eval-tensors", ("rbf", T, M, d), e, [])
    assert (got[:, 0] == 1.0).all() and e <= 1e-9, e
