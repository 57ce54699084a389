"""The low-rank EVALUATION path on WIDE state spaces: gpsig_lr_seq_features, gpsig_lr_seq_features_ragged and gpsig_lr_tens_features where the points
of not even one 64-step tile (one inducing tensor) fit the LDS.  The library then computes the Nystrom cross matrix on the float64 matrix cores
from the caller's raw points (csrc/lr_cross_kernel.hpp: lr_cross_eval_kernel) and runs the feature kernels that take it from memory; which calls
do is csrc/lr_tile_plan.hpp: lr_eval_route / lr_eval_tens_route (tests/test_lr_eval_route.py).

The smallest shapes that reach the route, from the footprints of lr_tile_plan.hpp (doubles; 19,968 fit the LDS, 8,192 the tensor kernel's 64 KB):
  float64 sequences   c = r = 8, d' = 160:    65 c + 138 max(c, r, d') = 22,600 > 19,968
  float32 sequences   c = r = 8, d' = 320:    44,680 > 39,936
  float64 tensors     M = 5, c = r = 16:      lt E (d' + 2 c) + lt c + 2 c > 8,192: d' = 240 with increments (E = 2), 512 without
  float32 tensors     twice that:             d' = 512 with increments, 1,056 without
L = 70 and 130: one and three 64-step chunks of lanes; N = 5 sequences, T = 3 tensors.

Tolerances are the project's own (the docstring of tests/test_gpu_lowrank_eval_long.py): the default route against lr_fused = 0 <= 1e-9 per feature
column scale; K against oracle.LowRankOracle 1e-7 of the largest entry (1e-5 linear); identities between the library's own kernels relerr <= 1e-12;
float32 against float64 on the same state <= 1e-4 of the largest entry; the Python surface, ragged against padded by repetition, <= 1e-9."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sigkern_oracle as O
from test_gpu_lowrank_eval_long import both_routes, colerr, features, host, oracle_for, relerr, seqs, with_lr_fused

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CLASS = {"linear": "SignatureLinear", "rbf": "SignatureRBF", "matern12": "SignatureMatern12", "matern32": "SignatureMatern32",
         "matern52": "SignatureMatern52"}
N, M = 5, 3


def make_kernel(base, L, d, M_, c, r, **kw):
    from gpsig_amd import kernels
    if base == "spectral":
        rng = np.random.default_rng(2)
        k = kernels.SignatureSpectral(L * d, d, M_, family="rbf", Q=3, low_rank=True, num_components=c, rank_bound=r, **kw)
        k.alpha, k.omega, k.gamma = rng.uniform(0.3, 1.2, 3), 0.5 * rng.standard_normal((3, d)) / np.sqrt(d), rng.uniform(0.4, 1.3, (3, d)) / np.sqrt(d)
    else:
        k = getattr(kernels, CLASS[base])(L * d, d, M_, low_rank=True, num_components=c, rank_bound=r, **kw)
    k.rng = np.random.default_rng(5)
    return k


def wide_ls(rng, d):
    """lengthscales of the order of sqrt(d): squared distances add up over the columns"""
    return np.sqrt(d) * (0.6 + rng.random(d))


def tens_features(k, st, Z, increments):
    from gpsig_amd import kernels
    L_ = kernels._Launch(Z)
    Phi, _, _ = k._lr_features(L_, k._params(L_.keep, L_.dtype_id), st.as_c(L_.keep), Z, tensors=True, increments=increments)
    if L_.device_mode:
        torch.cuda.current_stream(DEV).synchronize()
    return host(Phi)


# ---- 1. dense float64 against the multi-pass route ------------------------------------------------------------------------------------
def check_dense(base, L, d, c, r, difference=True, **kw):
    rng = np.random.default_rng(77)
    X = seqs(rng, N, L, d)
    kw = dict(normalization=False, lengthscales=wide_ls(rng, d), difference=difference, **kw)
    k = make_kernel(base, L, d, M, c, r, **kw)
    st = k.draw_low_rank(X=X)
    got, want = both_routes(k, st, X)                      # host pointers
    dev = features(k, st, torch.as_tensor(X, device=DEV))
    e = colerr(dev, want)
    print(base, L, "device pointers against lr_fused = 0:", e, "equal to host pointers:", np.array_equal(dev, got))
    assert e <= 1e-9 and np.array_equal(dev, got)
    lo = O.LowRankOracle(oracle_for(base, L, d, M, **kw), st.landmarks, st.jitter_diag, st.sketches)
    Kw = lo.K(X)
    e = float(np.abs(k.K(X, lr_state=st) - Kw).max() / np.abs(Kw).max())
    print(base, L, difference, "K against the oracle:", e)
    assert e <= (1e-5 if base == "linear" else 1e-7), e
    return k, st, X, got


@pytest.mark.parametrize("L", [70, 130])
@pytest.mark.parametrize("base", ["linear", "rbf", "matern32"])
def test_dense_float64_against_the_multipass_route(base, L):
    check_dense(base, L, 160, 8, 8)


def test_dense_float64_lags_and_lengthscales():
    """d = 80 columns and one lag: d' = 160; the lagged half of a point is interpolated on the sequence's own time axis"""
    check_dense("rbf", 70, 80, 8, 8, num_lags=1)


def test_dense_float64_without_the_difference():
    check_dense("rbf", 130, 160, 8, 7, difference=False)


# ---- 2. route evidence ---------------------------------------------------------------------------------------------------------------
def test_route_evidence_by_scratch():
    """The multi-pass route keeps five (N, L, max(c, r)) arrays in the context's scratch, the wide route one (N, L, c) array of kxs.  On a
    context of its own (device pointers: nothing is staged) the default call leaves the scratch below the five arrays; the lr_fused = 0 call
    after it grows it to at least that."""
    from gpsig_amd import _lib
    n, L, d, c = 20, 70, 160, 8
    rng = np.random.default_rng(78)
    X = seqs(rng, n, L, d)
    k = make_kernel("rbf", L, d, M, c, c, normalization=False, lengthscales=wide_ls(rng, d))
    st = k.draw_low_rank(X=X)
    want = features(k, st, X)
    stream = torch.cuda.current_stream(DEV)
    ctx = _lib.Context(0, stream.cuda_stream)
    try:
        ctx.set_pointer_mode(_lib.PTR_DEVICE)
        keep = []
        p, lr = k._params(keep), st.as_c(keep)
        Xd = torch.as_tensor(X, device=DEV)
        Phi = torch.full(want.shape, float("nan"), device=DEV, dtype=torch.float64)
        call = lambda: ctx.call("gpsig_lr_seq_features", p, lr, C.c_void_p(Xd.data_ptr()), n, L, C.c_void_p(Phi.data_ptr()))   # noqa: E731
        call()
        stream.synchronize()
        assert np.array_equal(host(Phi), want)
        before = ctx.scratch_bytes()
        ctx.set_option("lr_fused", 0)
        call()
        stream.synchronize()
        after = ctx.scratch_bytes()
        arrays = 8 * n * (L - 1) * 5 * c
        print("scratch bytes, default then lr_fused = 0:", before, after, "five (N, L - 1, c) arrays:", arrays)
        assert before < arrays <= after, (before, after, arrays)
        assert colerr(host(Phi), want) <= 1e-9
    finally:
        ctx.close()


# ---- 3. landmarks among the points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["matern12", "matern32", "matern52"])
def test_landmarks_among_the_points(base):
    """The state is drawn from the evaluated table itself: every landmark is one of the points, at distance exactly 0 on both routes (sqrt of a
    rounding residue would show at 1e-8, and its derivative is infinite for matern12)."""
    rng = np.random.default_rng(79)
    L, d = 70, 160
    X = seqs(rng, N, L, d)
    k = make_kernel(base, L, d, M, 8, 8, normalization=False, lengthscales=wide_ls(rng, d))
    st = k.draw_low_rank(X=X)
    pts = (X.reshape(N * L, d) / np.asarray(k.lengthscales)[None, :])
    assert all((np.abs(pts - s[None, :]).max(axis=1) == 0).any() for s in st.landmarks), "a landmark is no point of the table"
    both_routes(k, st, X)


# ---- 4. ragged -----------------------------------------------------------------------------------------------------------------------
def ragged_table(rng, lengths, L, d):
    X = seqs(rng, len(lengths), L, d).reshape(len(lengths), L, d)
    for n, l in enumerate(lengths):
        X[n, l:] = np.nan
    return X.reshape(len(lengths), L * d)


@pytest.mark.parametrize("difference", [True, False])
@pytest.mark.parametrize("L", [70, 130])
def test_ragged_float64(L, difference):
    """each sequence against its truncated copy evaluated alone, densely, by the same route; the padded rows hold NaN"""
    d, c = 160, 8
    lengths = [1, 2, 64, 65, 66, L]
    rng = np.random.default_rng(31)
    X = ragged_table(rng, lengths, L, d)
    k = make_kernel("rbf", L, d, M, c, c, normalization=False, lengthscales=wide_ls(rng, d), difference=difference)
    st = k.draw_low_rank(X=X, lengths=lengths)
    assert np.isfinite(st.landmarks).all()
    F = 1 + c + (M - 1) * c
    want = []
    for n, l in enumerate(lengths):
        if difference and l == 1:
            want.append(np.eye(1, F)[0])
            continue
        want.append(features(k, st, np.ascontiguousarray(X.reshape(len(lengths), L, d)[n:n + 1, :l].reshape(1, l * d)))[0])
    want = np.stack(want)
    hst = features(k, st, X, lengths)
    dev = features(k, st, torch.as_tensor(X, device=DEV), lengths)
    for name, got in (("host pointers", hst), ("device pointers", dev)):
        e = relerr(got, want)
        print(L, difference, name, "ragged against truncated copies:", e)
        assert (got[:, 0] == 1.0).all() and e <= 1e-12, (name, e)
    assert np.array_equal(hst, dev)
    with_lr_fused(0, lambda: np.testing.assert_array_equal(features(k, st, X, lengths), hst))       # ragged: whatever lr_fused says


S_L, S_D, S_LEN = 70, 160, [70, 1, 2, 33, 64, 65, 66, 69]


@pytest.mark.parametrize("method", ["K", "Kdiag", "K_tens_n_seq_covs", "predict_f"])
def test_python_surface_ragged_equals_padded_by_repetition(method):
    from gpsig_amd import inducing_variables as iv, models
    rng = np.random.default_rng(61)
    nan = ragged_table(rng, S_LEN, S_L, S_D).reshape(len(S_LEN), S_L, S_D)
    rep = nan.copy()
    for n, l in enumerate(S_LEN):
        rep[n, l:] = rep[n, l - 1]
    Z = torch.as_tensor(rng.standard_normal((M * (M + 1) // 2, 5, 2, S_D)), device=DEV)
    k = make_kernel("rbf", S_L, S_D, M, 16, 12, normalization=method != "Kdiag", lengthscales=wide_ls(rng, S_D))

    def run(table, lens):
        k.rng = np.random.default_rng(21)
        X = torch.as_tensor(table.reshape(len(S_LEN), -1), device=DEV)
        if method == "K":
            out = k.K(X, **lens)
        elif method == "Kdiag":
            out = k.Kdiag(X, return_levels=True, **lens)
        elif method == "K_tens_n_seq_covs":
            out = k.K_tens_n_seq_covs(Z, X, increments=True, full_X_cov=True, **lens)
        else:
            m = models.SVGP(k, iv.InducingTensors(Z, M, increments=True), q_mu=np.random.default_rng(3).standard_normal((Z.shape[1], 2)))
            out = m.predict_f(X, **lens)
        return [host(o) for o in (out if isinstance(out, tuple) else (out,))]

    want = run(rep, {})
    got = run(nan, {"lengths": S_LEN})
    for g, w in zip(got, want):
        e = relerr(g, w)
        print(method, "ragged against padded by repetition:", e)
        assert e <= 1e-9, (method, e)


# ---- 5. float32 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["rbf", "matern32"])
def test_float32_native(base):
    L, d, c = 130, 320, 8
    rng = np.random.default_rng(41)
    X64 = seqs(rng, N, L, d).astype(np.float32).astype(np.float64)
    X32 = X64.astype(np.float32)
    for difference in (True, False):
        k = make_kernel(base, L, d, M, c, c, normalization=True, lengthscales=wide_ls(rng, d), difference=difference)
        st = k.draw_low_rank(X=X64)
        k.lr_native_f32 = True
        P32, P64 = features(k, st, X32), features(k, st, X64)
        assert P32.dtype == np.float32 and P64.dtype == np.float64
        e = relerr(P32, P64)
        print(base, difference, "float32 features:", e)
        assert e <= 1e-4, e
        K64, K32 = k.K(X64, lr_state=st), k.K(X32, lr_state=st)
        assert K32.dtype == np.float32
        e = relerr(K32, K64)
        print(base, difference, "float32 Gram:", e)
        assert e <= 1e-4, e
        assert not np.array_equal(K32, K64.astype(np.float32)), "the float32 kernels did not run: every entry equals the rounded float64 result"
        # lr_fused = 0 keeps its behaviour: the library refuses, the Python layer computes in float64 and rounds
        K64p, K32p = with_lr_fused(0, lambda: (k.K(X64, lr_state=st), k.K(X32, lr_state=st)))
        assert K32p.dtype == np.float32 and np.array_equal(K32p, K64p.astype(np.float32))


def test_float32_ragged():
    L, d, c = 130, 320, 8
    lengths = [1, 2, 64, 65, 66, L]
    rng = np.random.default_rng(43)
    full = seqs(rng, len(lengths), L, d).astype(np.float32).astype(np.float64)
    X64 = full.reshape(-1, L, d).copy()
    for n, l in enumerate(lengths):
        X64[n, l:] = np.nan
    X64 = X64.reshape(-1, L * d)
    X32 = X64.astype(np.float32)
    k = make_kernel("rbf", L, d, M, c, c, normalization=True, lengthscales=wide_ls(rng, d))
    st = k.draw_low_rank(X=full)                      # (distinct points: test_gpu_lowrank_eval_long.py::test_float32_ragged)
    k.lr_native_f32 = True
    P32, P64 = features(k, st, X32, lengths), features(k, st, X64, lengths)
    assert P32.dtype == np.float32 and np.isfinite(P32).all()
    e = relerr(P32, P64)
    print("float32 ragged features:", e)
    assert e <= 1e-4, e


# ---- 6. inducing tensors -------------------------------------------------------------------------------------------------------------
T_M, T_C, T_T = 5, 16, 3


def tens_case(d, increments, L=70):
    rng = np.random.default_rng(51)
    lt = T_M * (T_M + 1) // 2
    Z = rng.standard_normal((lt, T_T, 2, d) if increments else (lt, T_T, d)).astype(np.float32).astype(np.float64)
    X = seqs(rng, N, L, d).astype(np.float32).astype(np.float64)
    kw = dict(normalization=False, lengthscales=wide_ls(rng, d))
    k = make_kernel("rbf", L, d, T_M, T_C, T_C, **kw)
    st = k.draw_low_rank(X=X, Z=Z, increments=increments)
    return k, st, Z, X, kw


@pytest.mark.parametrize("increments,d", [(True, 240), (False, 512)], ids=["increments", "plain"])
def test_tensors_float64(increments, d):
    k, st, Z, X, kw = tens_case(d, increments)
    got = tens_features(k, st, Z, increments)
    want = with_lr_fused(0, lambda: tens_features(k, st, Z, increments))
    dev = tens_features(k, st, torch.as_tensor(Z, device=DEV), increments)
    e = colerr(got, want)
    print("tensors, default against lr_fused = 0:", e)
    assert (got[:, 0] == 1.0).all() and e <= 1e-9 and np.array_equal(dev, got)
    lo = O.LowRankOracle(oracle_for("rbf", 70, d, T_M, **kw), st.landmarks, st.jitter_diag, st.sketches)
    for name, g, w in (("K_tens", k.K_tens(Z, increments=increments, lr_state=st), lo.K_tens(Z, increments=increments)),
                       ("K_tens_vs_seq", k.K_tens_vs_seq(Z, X, increments=increments, lr_state=st), lo.K_tens_vs_seq(Z, X, increments=increments))):
        e = float(np.abs(host(g) - w).max() / np.abs(w).max())
        print(name, "against the oracle:", e)
        assert e <= 1e-7, (name, e)


@pytest.mark.parametrize("increments,d", [(True, 512), (False, 1056)], ids=["increments", "plain"])
def test_tensors_float32(increments, d):
    k, st, Z, X, kw = tens_case(d, increments)
    k.lr_native_f32 = True
    P32, P64 = tens_features(k, st, Z.astype(np.float32), increments), tens_features(k, st, Z, increments)
    assert P32.dtype == np.float32
    e = relerr(P32, P64)
    print("float32 tensor features:", e)
    assert e <= 1e-4, e
    assert not np.array_equal(P32, P64.astype(np.float32)), "the float32 kernel did not run"
    with pytest.raises(NotImplementedError):           # lr_fused = 0: refused as before (the Python layer then computes in float64)
        with_lr_fused(0, lambda: tens_features(k, st, Z.astype(np.float32), increments))


# ---- 7. chunking ---------------------------------------------------------------------------------------------------------------------
def with_chunk_mb(value, fn):
    from gpsig_amd import _lib
    ctx = _lib.context(0, torch.cuda.current_stream(DEV).cuda_stream)
    try:
        ctx.set_option("wide_chunk_mb", value)
        return fn()
    finally:
        ctx.set_option("wide_chunk_mb", 0)


def test_chunks_do_not_change_the_bits():
    """wide_chunk_mb = 1: 64 sequences of L = 130 at c = 8 take 0.53 MB of kxs, so N = 400 goes in four chunks; a tensor at M = 5, c = 16 with
    increments takes 3,840 bytes of kzs, so T = 700 goes in three"""
    L, d, c, n = 130, 160, 8, 400
    rng = np.random.default_rng(91)
    X = torch.as_tensor(seqs(rng, n, L, d), device=DEV)
    k = make_kernel("rbf", L, d, M, c, c, normalization=False, lengthscales=wide_ls(rng, d))
    st = k.draw_low_rank(X=host(X[:8]))
    lengths = rng.integers(1, L + 1, size=n)
    for lens in (None, lengths):
        whole = features(k, st, X, lens)
        parts = with_chunk_mb(1, lambda: features(k, st, X, lens))
        assert np.isfinite(whole).all() and np.array_equal(whole, parts)
    d, T = 240, 700
    Z = torch.as_tensor(rng.standard_normal((T_M * (T_M + 1) // 2, T, 2, d)), device=DEV)
    k = make_kernel("rbf", 70, d, T_M, T_C, T_C, normalization=False, lengthscales=wide_ls(rng, d))
    st = k.draw_low_rank(Z=host(Z[:, :8]), increments=True)
    whole = tens_features(k, st, Z, True)
    parts = with_chunk_mb(1, lambda: tens_features(k, st, Z, True))
    assert np.isfinite(whole).all() and np.array_equal(whole, parts)


# ---- 8. unchanged ground -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,L", [(8, 70), (64, 130)], ids=["fused", "tiled"])
def test_narrow_shapes_keep_their_kernels(c, L):
    """d' = 3: the whole-sequence kernel (c = 8, L = 70) and the tiled kernel (c = r = 64, L = 130) serve these calls; the wide route's chunk
    option does not reach them (same bits with wide_chunk_mb = 1), a second call gives the same bits, lr_fused = 0 agrees to 1e-9"""
    rng = np.random.default_rng(95)
    X = seqs(rng, N, L, 3)
    k = make_kernel("rbf", L, 3, M, c, c, normalization=False, lengthscales=0.6 + rng.random(3))
    st = k.draw_low_rank(X=X)
    got, _ = both_routes(k, st, X)
    Xd = torch.as_tensor(X, device=DEV)
    a = features(k, st, Xd)
    b = with_chunk_mb(1, lambda: features(k, st, Xd))
    assert np.array_equal(a, b) and np.array_equal(a, got)


def test_spectral_keeps_its_route():
    """SignatureSpectral is built for at most 32 columns and no lags: d' = 160 is refused before any route is chosen, as it was.  What it can
    reach beyond the tiled kernels is a wide rank bound (c = 16, r = 160 at d' = 32: 65 c + 138 r doubles exceed the LDS): the multi-pass
    route, as before -- finite, and the bits of lr_fused = 0."""
    rng = np.random.default_rng(96)
    L = 70
    X = seqs(rng, N, L, 160)
    k = make_kernel("spectral", L, 160, M, 8, 8, normalization=False)
    with pytest.raises(NotImplementedError, match="at most 32 features"):
        features(k, k.draw_low_rank(X=X), X)
    X = seqs(rng, N, L, 32)
    k = make_kernel("spectral", L, 32, M, 16, 160, normalization=False)
    st = k.draw_low_rank(X=X)
    got, want = both_routes(k, st, X)
    assert np.array_equal(got, want)


def test_more_than_64_components_ragged_is_refused():
    rng = np.random.default_rng(97)
    L, d, c = 70, 160, 65
    lengths = [70, 3, 1, 66, 65]
    X = ragged_table(rng, lengths, L, d)
    k = make_kernel("rbf", L, d, M, c, c, normalization=False, lengthscales=wide_ls(rng, d))
    st = k.draw_low_rank(X=X, lengths=lengths)
    with pytest.raises(NotImplementedError, match="ragged low-rank features"):
        features(k, st, X, lengths)
