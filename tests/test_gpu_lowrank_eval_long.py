"""The low-rank EVALUATION path on long and ragged batches: gpsig_lr_seq_features beyond the whole-sequence kernels and
gpsig_lr_seq_features_ragged, both on the time-tiled kernels of csrc/lr_eval_tiled_inst.hip, and the ``lengths=`` keywords of
gpsig_amd.kernels.SignatureKernel / models.SVGP.predict_f.

Tile lengths (csrc/lr_tile_plan.hpp, 156 KB of LDS): at 64 rows (c = r = 64) a float64 tile is 64 steps and whole sequences stop at L = 64, a
float32 tile is 192 steps and whole sequences stop at L = 192; at c = 12, r = 7 whole float64 sequences fit up to L = 512; at c = 4, r = 3
with two lags (9 staging rows) a tile is 896 steps.

Tolerances are the project's own:
  * default route against lr_fused = 0 (the multi-pass route): <= 1e-9 per feature column scale (test_gpu_parity.py::test_low_rank_fused_feature_kernel);
  * K against oracle.LowRankOracle on the same random objects: 1e-7 of the largest entry, 1e-5 for the linear kernel (same test);
  * identities between the library's own fused kernels: relerr = max|got - want| / max|want| <= 1e-12 (test_gpu_lowrank_ragged.py);
  * float32 against float64 on the same state: <= 1e-4 of the largest entry (test_gpu_lowrank_f32.py);
  * the Python surface, ragged against the table padded by repetition: <= 1e-9 of the result's largest entry."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sigkern_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RAGGED_LENGTHS = [1, 2, 64, 65, 66, 128, 129, 130, 192, 193, 194, 256, 257, 385, 386, 33]
CLASS = {"linear": "SignatureLinear", "rbf": "SignatureRBF", "matern32": "SignatureMatern32"}


def host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def relerr(got, want):
    got, want = np.asarray(host(got), dtype=np.float64), np.asarray(host(want), dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300))


def colerr(got, want):
    """per feature column scale"""
    got, want = host(got), host(want)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    return float((np.abs(got - want) / (np.abs(want).max(axis=0, keepdims=True) + 1e-300)).max())


def seqs(rng, N, L, d):
    return np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, L * d)


def make_kernel(base, L, d, M, c, r, sparsity="sqrt", **kw):
    from gpsig_amd import kernels
    if base.startswith("spectral"):
        rng = np.random.default_rng(2)
        Q = 3
        k = kernels.SignatureSpectral(L * d, d, M, family=base.split("-")[1], Q=Q, low_rank=True, num_components=c, rank_bound=r,
                                      sparsity=sparsity, **kw)
        k.alpha, k.omega, k.gamma = rng.uniform(0.3, 1.2, Q), 0.5 * rng.standard_normal((Q, d)), rng.uniform(0.4, 1.3, (Q, d))
    else:
        k = getattr(kernels, CLASS[base])(L * d, d, M, low_rank=True, num_components=c, rank_bound=r, sparsity=sparsity, **kw)
    k.rng = np.random.default_rng(5)
    return k


def oracle_for(base, L, d, M, **kw):
    kw = {n: v for n, v in kw.items() if n not in ("num_components", "rank_bound", "sparsity")}
    return O.SignatureKernelOracle(input_dim=L * d, num_features=d, num_levels=M, base=base, **kw)


def host_ctx():
    from gpsig_amd import _lib
    ctx = _lib.context(0, 0)
    ctx.set_pointer_mode(_lib.PTR_HOST)
    return ctx


def features(k, st, A, lengths=None):
    """gpsig_lr_seq_features / gpsig_lr_seq_features_ragged in the dtype and the pointer mode of A"""
    from gpsig_amd import kernels
    L_ = kernels._Launch(A)
    p = k._params(L_.keep, L_.dtype_id)
    lr = st.as_c(L_.keep)
    Phi, _, _ = k._lr_features(L_, p, lr, A, lengths=None if lengths is None else np.asarray(lengths, dtype=np.int32))
    if L_.device_mode:
        torch.cuda.current_stream(DEV).synchronize()
    return host(Phi)


def with_lr_fused(value, fn):
    """lr_fused on the host-pointer context and on the device-pointer one of the current stream; the default restored"""
    from gpsig_amd import _lib
    ctxs = [_lib.context(0, 0), _lib.context(0, torch.cuda.current_stream(DEV).cuda_stream)]
    try:
        for ctx in ctxs:
            ctx.set_option("lr_fused", value)
        return fn()
    finally:
        for ctx in ctxs:
            ctx.set_option("lr_fused", 1)


def both_routes(k, st, X):
    """the default route and the multi-pass one (lr_fused = 0) on host pointers: checked to 1e-9 per feature column scale"""
    got = features(k, st, X)
    want = with_lr_fused(0, lambda: features(k, st, X))
    assert np.isfinite(got).all() and (got[:, 0] == 1.0).all()
    e = colerr(got, want)
    print("default against lr_fused = 0:", e)
    assert e <= 1e-9, e
    return got, want


def assert_tiled_route(k, st, X, got):
    """Route evidence.  The two routes add the same terms in the same order (the multi-pass route's whitening GEMM included, at these
    widths): their bits are equal, so bits cannot tell them apart.  What can: the multi-pass route keeps five (N, L, max(c, r)) arrays in the
    context's scratch, the tiled kernels none.  On a context of its own the default call comes first; the lr_fused = 0 call after it
    must then grow the scratch by those five arrays -- it would not, had the default call taken that route."""
    from gpsig_amd import _lib
    ctx = _lib.Context(0, 0)
    try:
        ctx.set_pointer_mode(_lib.PTR_HOST)
        keep = []
        p, lr = k._params(keep), st.as_c(keep)
        N, L = k._seq_dims(X)
        c, r = int(k.num_components), int(k.rank_bound)
        Phi = np.full(got.shape, np.nan)
        Xc = np.ascontiguousarray(X)
        call = lambda: ctx.call("gpsig_lr_seq_features", p, lr, Xc.ctypes.data_as(C.c_void_p), N, L, Phi.ctypes.data_as(C.c_void_p))   # noqa: E731
        call()
        assert np.array_equal(Phi, got)
        before = ctx.scratch_bytes()
        ctx.set_option("lr_fused", 0)
        call()
        after = ctx.scratch_bytes()
        arrays = 8 * N * (L - 1) * (2 * c + 3 * max(c, r))
        print("scratch bytes, default then lr_fused = 0:", before, after, "the multi-pass arrays:", arrays)
        assert after - before >= arrays, (before, after, arrays)
    finally:
        ctx.close()


def check_plain(base, sparsity, N, L, d, M, c, r, difference, evidence, **kw):
    rng = np.random.default_rng(77)
    X = seqs(rng, N, L, d)
    kw = dict(normalization=False, lengthscales=0.6 + rng.random(d), difference=difference, **kw)
    k = make_kernel(base, L, d, M, c, r, sparsity, **kw)
    st = k.draw_low_rank(X=X)
    got, want = both_routes(k, st, X)
    if evidence:
        print("bits differ from lr_fused = 0:", not np.array_equal(got, want))
        assert_tiled_route(k, st, X, got)
    lo = O.LowRankOracle(oracle_for(base, L, d, M, **kw), st.landmarks, st.jitter_diag, st.sketches)
    Kw = lo.K(X)
    e = float(np.abs(k.K(X, lr_state=st) - Kw).max() / np.abs(Kw).max())
    print(base, sparsity, L, difference, "K against the oracle:", e)
    assert e <= (1e-5 if base == "linear" else 1e-7), e


# ---- 1. tile boundaries, float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sparsity", ["sqrt", "log", "lin"])
@pytest.mark.parametrize("base", ["rbf", "linear", "matern32"])
def test_tile_boundaries_float64(base, sparsity):
    """c = r = 64: a tile is 64 steps.  L = 65, 66, 129, 130 with and without the difference: one to three tiles, last tiles of one step."""
    for L in (65, 66, 129, 130):
        for difference in (True, False):
            check_plain(base, sparsity, 6, L, 3, 3, 64, 64, difference, evidence=L == 130)


# ---- 2. wide tiles and lags --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["rbf", "linear", "matern32"])
def test_wide_tiles_off_the_batch_widths(base):
    """c = 12, r = 7: ranks off the widths of the scalar-load batches; whole sequences fit up to L = 512, L = 515 is two tiles."""
    for difference in (True, False):
        check_plain(base, "sqrt", 4, 515, 3, 3, 12, 7, difference, evidence=True)


@pytest.mark.parametrize("base", ["rbf", "linear", "matern32"])
def test_lagged_points_across_tile_boundaries(base):
    """c = 4, r = 3, two lags: d_eff = 9 > max(c, r) -- the staging rows; a tile of 896 steps, L = 900: lagged points of the second tile are
    interpolated from rows of the first."""
    for difference in (True, False):
        check_plain(base, "lin", 3, 900, 3, 5, 4, 3, difference, evidence=True, num_lags=2)


# ---- 3. ragged ---------------------------------------------------------------------------------------------------------------------
def ragged_table(rng, lengths, L, d):
    X = seqs(rng, len(lengths), L, d).reshape(len(lengths), L, d)
    for n, l in enumerate(lengths):
        X[n, l:] = np.nan
    return X.reshape(len(lengths), L * d)


def truncated_reference(k, st, X, lengths, L, d, whole_limit):
    """sequence by sequence: gpsig_lr_seq_features on X[n, :l] alone.  Up to `whole_limit` points that is a fused whole-sequence kernel;
    beyond, the multi-pass route (lr_fused = 0).  Returns (rows, fused?)."""
    F = 1 + k.num_components + (k.num_levels - 1) * k.rank_bound
    rows, fused = [], []
    for n, l in enumerate(lengths):
        if k.difference and l == 1:
            rows.append(np.eye(1, F)[0])
            fused.append(True)
            continue
        Xn = np.ascontiguousarray(X.reshape(len(lengths), L, d)[n:n + 1, :l].reshape(1, l * d))
        whole = l <= whole_limit
        rows.append((features(k, st, Xn) if whole else with_lr_fused(0, lambda: features(k, st, Xn)))[0])
        fused.append(whole)
    return np.stack(rows), np.asarray(fused)


def check_ragged(k, st, X, lengths, L, d, whole_limit=64):
    want, fused = truncated_reference(k, st, X, lengths, L, d, whole_limit)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        Xd = torch.as_tensor(X, device=DEV)
        dev1 = features(k, st, Xd, lengths)
        dev2 = features(k, st, Xd, lengths)
    torch.cuda.synchronize()
    hst = features(k, st, X, lengths)
    for name, got in (("device pointers", dev1), ("host pointers", hst)):
        assert np.isfinite(got).all(), name
        assert (got[:, 0] == 1.0).all()
        e12, e9 = relerr(got[fused], want[fused]), colerr(got[~fused], want[~fused])
        print(name, "against fused whole sequences:", e12, "against the multi-pass route:", e9)
        assert e12 <= 1e-12 and e9 <= 1e-9, (name, e12, e9)
        if k.difference:
            for n, l in enumerate(lengths):
                if l == 1:
                    assert (got[n, 1:] == 0).all()
    assert np.array_equal(dev1, dev2), "a second call gave other bits"


@pytest.mark.parametrize("difference", [True, False])
def test_ragged_float64(difference):
    L, d, M, c = 386, 3, 3, 64
    rng = np.random.default_rng(31)
    X = ragged_table(rng, RAGGED_LENGTHS, L, d)
    k = make_kernel("rbf", L, d, M, c, c, normalization=False, lengthscales=0.6 + rng.random(d), difference=difference)
    st = k.draw_low_rank(X=X, lengths=RAGGED_LENGTHS)
    assert np.isfinite(st.landmarks).all()
    check_ragged(k, st, X, RAGGED_LENGTHS, L, d)


# ---- 4. float32 --------------------------------------------------------------------------------------------------------------------
# (rbf and matern32: the linear kernel's landmark Gram has rank d = 3 at c = 64, test_gpu_lowrank_f32.py keeps it at c = 3 for that reason)
@pytest.mark.parametrize("base", ["rbf", "matern32"])
def test_float32_beyond_the_whole_sequence_kernels(base):
    """L = 386 at 64 rows: beyond the float32 whole-sequence limit of 192; tiles of 192 steps."""
    N, L, d, M, c = 6, 386, 3, 3, 64
    rng = np.random.default_rng(41)
    X64 = seqs(rng, N, L, d).astype(np.float32).astype(np.float64)
    X32 = X64.astype(np.float32)
    for difference in (True, False):
        k = make_kernel(base, L, d, M, c, c, normalization=True, lengthscales=0.6 + rng.random(d), difference=difference)
        st = k.draw_low_rank(X=X64)
        k.lr_native_f32 = True
        P32, P64 = features(k, st, X32), features(k, st, X64)
        assert P32.dtype == np.float32 and P64.dtype == np.float64
        e = relerr(P32, P64)
        print(base, difference, "float32 features:", e)
        assert e <= 1e-4, e
        K64 = k.K(X64, lr_state=st)
        K32 = k.K(X32, lr_state=st)
        assert K32.dtype == np.float32
        e = relerr(K32, K64)
        print(base, difference, "float32 Gram:", e)
        assert e <= 1e-4, e
        assert not np.array_equal(K32, K64.astype(np.float32)), "the float32 kernels did not run: every entry equals the rounded float64 result"


def test_float32_ragged():
    """the ragged table of case 3 in float32: sequences of one, two and three 192-step tiles"""
    L, d, M, c = 386, 3, 3, 64
    rng = np.random.default_rng(43)
    full = seqs(rng, len(RAGGED_LENGTHS), L, d).astype(np.float32).astype(np.float64)
    X64 = full.reshape(-1, L, d).copy()
    for n, l in enumerate(RAGGED_LENGTHS):
        X64[n, l:] = np.nan
    X64 = X64.reshape(-1, L * d)
    X32 = X64.astype(np.float32)
    for difference in (True, False):
        k = make_kernel("rbf", L, d, M, c, c, normalization=True, lengthscales=0.6 + rng.random(d), difference=difference)
        # landmarks from the table before it was cut: distinct points.  (The pool of a ragged draw repeats each sequence's last point, and
        # landmarks drawn twice make the whitening as large as 1 / sqrt(jitter): that measures the draw, not the float32 kernels.)
        st = k.draw_low_rank(X=full)
        k.lr_native_f32 = True
        P32, P64 = features(k, st, X32, RAGGED_LENGTHS), features(k, st, X64, RAGGED_LENGTHS)
        assert P32.dtype == np.float32 and np.isfinite(P32).all()
        e = relerr(P32, P64)
        print(difference, "float32 ragged features:", e)
        assert e <= 1e-4, e
        K64 = k.K(X64, lr_state=st, lengths=RAGGED_LENGTHS)
        K32 = k.K(X32, lr_state=st, lengths=RAGGED_LENGTHS)
        e = relerr(K32, K64)
        print(difference, "float32 ragged Gram:", e)
        assert K32.dtype == np.float32 and e <= 1e-4, e
        assert not np.array_equal(K32, K64.astype(np.float32))


# ---- 5. spectral, float64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["rbf", "exp", "mixed"])
def test_spectral_float64(family):
    N, L, d, M, c = 6, 130, 3, 3, 64
    rng = np.random.default_rng(51)
    X = seqs(rng, N, L, d)
    for difference in (True, False):
        k = make_kernel("spectral-" + family, L, d, M, c, c, normalization=False, difference=difference)
        st = k.draw_low_rank(X=X)
        got, want = both_routes(k, st, X)
        assert_tiled_route(k, st, X, got)
        lengths = [130, 129, 66, 65, 2, 1]
        Xr = X.reshape(N, L, d).copy()
        for n, l in enumerate(lengths):
            Xr[n, l:] = np.nan
        check_ragged(k, st, Xr.reshape(N, L * d), lengths, L, d)


# ---- 6. the Python surface ---------------------------------------------------------------------------------------------------------
SURFACE = ["K", "K_X2", "Kdiag", "K_tens_vs_seq", "K_tens_n_seq_covs", "K_seq_n_seq_covs", "predict_f"]
S_L, S_D, S_M = 70, 3, 3
S_LEN = [70, 1, 2, 33, 64, 65, 66, 69]
S_LEN2 = [5, 70, 66, 1, 40]


def surface_data():
    rng = np.random.default_rng(61)
    out = {}
    for name, lens in (("X", S_LEN), ("Y", S_LEN2)):
        nan = ragged_table(rng, lens, S_L, S_D).reshape(len(lens), S_L, S_D)
        rep = nan.copy()
        for n, l in enumerate(lens):
            rep[n, l:] = rep[n, l - 1]
        out[name] = (nan.reshape(len(lens), -1), rep.reshape(len(lens), -1))
    out["Z"] = rng.standard_normal((S_M * (S_M + 1) // 2, 5, 2, S_D))
    out["Zs"] = np.cumsum(0.3 * rng.standard_normal((4, 6, S_D)), axis=1)
    return out


def surface_call(k, method, X, Y, Z, Zs, lens, lens2):
    from gpsig_amd import inducing_variables as iv, models
    if method == "K":
        return k.K(X, **lens)
    if method == "K_X2":
        return k.K(X, Y, return_levels=True, **lens, **lens2)
    if method == "Kdiag":
        return k.Kdiag(X, return_levels=True, **lens)
    if method == "K_tens_vs_seq":
        return k.K_tens_vs_seq(Z, X, increments=True, **lens)
    if method == "K_tens_n_seq_covs":
        return k.K_tens_n_seq_covs(Z, X, increments=True, full_X_cov=True, **lens)
    if method == "K_seq_n_seq_covs":
        return k.K_seq_n_seq_covs(Zs.reshape(Zs.shape[0], -1), Y, **lens2)
    feat = iv.InducingTensors(Z, S_M, increments=True)
    rng = np.random.default_rng(3)
    m = models.SVGP(k, feat, q_mu=rng.standard_normal((Z.shape[1], 2)))
    return m.predict_f(X, **lens)


@pytest.mark.parametrize("device", [False, True], ids=["numpy", "cuda"])
@pytest.mark.parametrize("method", SURFACE)
def test_python_surface_ragged_equals_padded_by_repetition(method, device):
    data = surface_data()
    conv = (lambda a: torch.as_tensor(a, device=DEV)) if device else (lambda a: a)
    k = make_kernel("rbf", S_L, S_D, S_M, 16, 12, normalization=method != "Kdiag", lengthscales=np.asarray([0.7, 1.1, 0.9]), difference=True)
    Z, Zs = conv(data["Z"]), conv(data["Zs"])

    def run(which, lens, lens2):
        k.rng = np.random.default_rng(21)
        out = surface_call(k, method, conv(data["X"][which]), conv(data["Y"][which]), Z, Zs, lens, lens2)
        return [host(o) for o in (out if isinstance(out, tuple) else (out,))]

    want = run(1, {}, {})
    as_given = (lambda v: torch.as_tensor(v, device=DEV)) if device else (lambda v: list(v))
    got = run(0, {"lengths": as_given(S_LEN)}, {"lengths2": np.asarray(S_LEN2)})
    for g, w in zip(got, want):
        e = relerr(g, w)
        print(method, "ragged against padded by repetition:", e)
        assert e <= 1e-9, (method, e)


# ---- 7. refusals are typed ---------------------------------------------------------------------------------------------------------
def test_refusals_are_typed():
    from gpsig_amd import kernels
    rng = np.random.default_rng(71)
    L, d, M = 10, 2, 2
    X = seqs(rng, 4, L, d)
    good = [10, 3, 1, 7]
    exact = kernels.SignatureRBF(L * d, d, M)
    with pytest.raises(NotImplementedError, match="repeating its last observation"):
        exact.K(X, lengths=good)
    lagged = kernels.SignatureRBF(L * d, d, M, num_lags=1, low_rank=True, num_components=6, rank_bound=5)
    with pytest.raises(NotImplementedError, match="num_lags"):
        lagged.K(X, lengths=good)
    k = kernels.SignatureRBF(L * d, d, M, low_rank=True, num_components=6, rank_bound=5)
    for bad in (np.asarray(good, dtype=np.float64), good[:3], [0, 3, 1, 7], [L + 1, 3, 1, 7]):
        with pytest.raises(ValueError, match="lengths"):
            k.K(X, lengths=bad)
    # the C entry point with lags
    lagged.rng = np.random.default_rng(1)
    st = lagged.draw_low_rank(X=X)
    ctx = host_ctx()
    keep = []
    p, lr = lagged._params(keep), st.as_c(keep)
    Phi = np.zeros((4, 1 + 6 + 5))
    lens = np.asarray(good, dtype=np.int32)
    with pytest.raises(NotImplementedError, match="num_lags"):
        ctx.call("gpsig_lr_seq_features_ragged", p, lr, X.ctypes.data_as(C.c_void_p), 4, L, lens.ctypes.data_as(C.c_void_p),
                 Phi.ctypes.data_as(C.c_void_p))
