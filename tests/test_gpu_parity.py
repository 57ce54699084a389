"""GPU parity tests proper: the HIP path, called through the C ABI (gpsig_amd -> ctypes ->
libgpsig_hip.so), against (a) the committed golden fixtures, (b) the CPU oracle on the same seeded
inputs at sizes the oracle finishes in seconds, (c) size-independent properties at BASELINE.json's
full configuration.

Tolerance (north_star / SURVEY.md 8d): fp64, max |K - K_ref| / (|K_ref| + 1e-6 * max|K_ref|) <= 1e-6 per
level and on the summed matrix.  Observed agreement is ~1e-13; the bound is the contract.
"""
import numpy as np
import pytest

from oracle import sigkern_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-6


def relerr(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    scale = np.abs(want).max() if want.size else 1.0
    return float((np.abs(got - want) / (np.abs(want) + 1e-6 * scale + 1e-300)).max()) if want.size else 0.0


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    from gpsig_amd import kernels
    return kernels


CLASS = {"spectral": "SignatureSpectral", "linear": "SignatureLinear", "rbf": "SignatureRBF", "cosine": "SignatureCosine", "poly": "SignaturePoly",
         "mix": "SignatureMix", "matern12": "SignatureMatern12", "matern32": "SignatureMatern32", "matern52": "SignatureMatern52"}


def make_kernel(K, kw):
    kw = dict(kw)
    base = kw.pop("base")
    bp = kw.pop("base_params", None) or {}
    for k in ("variances", "lengthscales"):
        if isinstance(kw.get(k), list):
            kw[k] = np.asarray(kw[k])
    extra = {}
    if base == "poly":
        extra = dict(gamma=bp.get("gamma", 1), degree=bp.get("degree", 3))
    kern = getattr(K, CLASS[base])(**kw, **extra)
    if base == "mix":
        kern.mixing = bp.get("mixing", 0.5)
    return kern


def make_oracle(kw):
    kw = {k: (np.asarray(v) if isinstance(v, list) else v) for k, v in kw.items()}
    return O.SignatureKernelOracle(**kw)


# ------------------------------------------------------------------------------------------------
# (a) committed golden fixtures
# ------------------------------------------------------------------------------------------------
def _run_case(K, c, arr):
    from gpsig_amd import inducing_variables as IV
    n = c["name"]
    kern = make_kernel(K, c["kern"])
    g = lambda key: arr[n + "/" + key]  # noqa: E731
    call = c["call"]
    m = c["method"]
    if m == "K":
        return [kern.K(g("X"), g("X2") if "X2" in c["has"] else None, **call)]
    if m == "Kdiag":
        return [kern.Kdiag(g("X"), **call)]
    if m == "K_tens":
        return [kern.K_tens(g("Z"), **call)]
    if m == "K_tens_vs_seq":
        return [kern.K_tens_vs_seq(g("Z"), g("X"), **call)]
    if m == "K_tens_n_seq_covs":
        return list(kern.K_tens_n_seq_covs(g("Z"), g("X"), **call))
    if m == "K_seq_n_seq_covs":
        return list(kern.K_seq_n_seq_covs(g("X"), g("X2"), **call))
    if m == "Kuu_Kuf_Kff_tensors":
        call = dict(call)
        feat = IV.InducingTensors(g("Z"), kern.num_levels, increments=call.pop("increments", False),
                                  learn_weights="W" in c["has"])
        if "W" in c["has"]:
            feat.W = g("W")
        return list(IV.Kuu_Kuf_Kff(feat, kern, g("X"), **call))
    if m == "Kuu_Kuf_Kff_sequences":
        Zs = g("X")
        d = kern.num_features
        feat = IV.InducingSequences(Zs.reshape(Zs.shape[0], -1, d), kern.num_levels, learn_weights="W" in c["has"])
        if "W" in c["has"]:
            feat.W = g("W")
        return list(IV.Kuu_Kuf_Kff(feat, kern, g("X2"), **call))
    raise ValueError(m)


def test_golden_fixtures(K, golden):
    cases, arr = golden
    not_built, worst = [], 0.0
    for c in cases:
        outs = _run_case(K, c, arr)
        assert len(outs) == c["n_out"]
        for i, o in enumerate(outs):
            e = relerr(o, arr[f"{c['name']}/out{i}"])
            worst = max(worst, e)
            assert e <= TOL, (c["name"], i, e)
    print(f"golden: {len(cases)} cases, worst rel.err {worst:.2e}")
    assert len(cases) >= 90


def test_notebook_identities_against_signature_features(K):
    """The reference's own validation, notebooks/signature_kernel.ipynb, at the notebook's shapes (cells 4, 15):
    SignatureLinear(order=num_levels, normalization=False) against signature features (an independent Chen-identity
    signature stands in for esig): K (cells 8-13), K_tens_vs_seq (cells 19-23), K_tens (cells 25-29)."""
    rng = np.random.default_rng(15)
    M, N, L, d, T = 5, 100, 50, 3, 100
    X = rng.standard_normal((N, L, d))
    Z = rng.standard_normal((M * (M + 1) // 2, T, d))
    sigs = np.stack([O.truncated_signature(x, M) for x in X])
    tens = O.rank1_tensor_features(Z, M)
    kern = K.SignatureLinear(L * d, d, M, order=M, normalization=False)
    Xf = X.reshape(N, -1)
    assert relerr(kern.compute_K_symm(Xf), sigs @ sigs.T) <= 1e-10
    assert relerr(kern.compute_K_tens_vs_seq(Z, Xf), tens @ sigs.T) <= 1e-10
    assert relerr(kern.compute_K_tens(Z), tens @ tens.T) <= 1e-10
    # BASELINE.json configs[0]: N=64, L=32, d=3, num_levels=4, validated against signature features
    N, L, d, M = 64, 32, 3, 4
    X = rng.standard_normal((N, L, d))
    sigs = np.stack([O.truncated_signature(x, M) for x in X])
    kern = K.SignatureLinear(L * d, d, M, order=M, normalization=False)
    Kl = kern.K(X.reshape(N, -1), return_levels=True)
    for m, sl in enumerate(O.signature_level_slices(d, M)):
        assert relerr(Kl[m], sigs[:, sl] @ sigs[:, sl].T) <= 1e-10


@pytest.mark.parametrize("L,M,order", [(20, 4, 2), (20, 5, 3), (60, 6, 6), (100, 5, 4), (100, 4, 2), (300, 3, 2)])
def test_higher_order_shapes(K, L, M, order):
    rng = np.random.default_rng(L + M + order)
    d = 3
    X = np.cumsum(0.2 * rng.standard_normal((7, L, d)), axis=1).reshape(7, -1)
    Y = np.cumsum(0.2 * rng.standard_normal((4, L, d)), axis=1).reshape(4, -1)
    Z = rng.standard_normal((M * (M + 1) // 2, 5, 2, d))
    for base in ("linear", "rbf"):
        kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, order=order)
        kx, ko = make_kernel(K, kw), make_oracle(kw)
        assert relerr(kx.K(X), ko.K(X)) <= TOL
        assert relerr(kx.K(X, Y, return_levels=True), ko.K(X, Y, return_levels=True)) <= TOL
        assert relerr(kx.K_tens_vs_seq(Z, X, increments=True), ko.K_tens_vs_seq(Z, X, increments=True)) <= TOL
    # without differences (a non-linear base kernel then feeds kappa itself into the recursion), and in float32
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base="rbf", order=order, difference=False)
    kx, ko = make_kernel(K, kw), make_oracle(kw)
    Xs, Ys = 0.3 * X, 0.3 * Y
    assert relerr(kx.K(Xs), ko.K(Xs)) <= TOL
    assert relerr(kx.K(Xs, Ys, return_levels=True), ko.K(Xs, Ys, return_levels=True)) <= TOL
    for base in ("linear", "rbf"):
        kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, order=order)
        kx, ko = make_kernel(K, kw), make_oracle(kw)
        got = kx.K(X.astype(np.float32), Y.astype(np.float32))
        assert got.dtype == np.float32
        assert relerr32(got, ko.K(X.astype(np.float32).astype(np.float64), Y.astype(np.float32).astype(np.float64))) <= TOL32
        assert relerr32(kx.K(X.astype(np.float32)), ko.K(X.astype(np.float32).astype(np.float64))) <= TOL32


# ------------------------------------------------------------------------------------------------
# (b) oracle on the same seeded inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["linear", "rbf"])
@pytest.mark.parametrize("norm", [False, True])
def test_baseline_config1(K, base, norm):
    """BASELINE.json configs[0] shape: N=64, L=32, d=3, num_levels=4 (order 1)."""
    rng = np.random.default_rng(0)
    N, L, d, M = 64, 32, 3, 4
    X = rng.standard_normal((N, L * d))
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, normalization=norm)
    got = make_kernel(K, dict(kw, base=base)).compute_K_symm(X)
    assert relerr(got, make_oracle(dict(kw, base=base)).K(X)) <= TOL
    np.testing.assert_array_equal(got, got.T)


@pytest.mark.parametrize("base", ["linear", "rbf"])
def test_config2_shape_reduced_n(K, base):
    """BASELINE.json configs[1] shape (L=64, d=8, num_levels=5, fp64) at N=160: every kernel-shape parameter of the
    benchmark kernel, at a size the tiled oracle finishes in seconds."""
    rng = np.random.default_rng(1)
    N, L, d, M = 160, 64, 8, 5
    X = (rng.standard_normal((N, L, d)) if base == "linear" else np.cumsum(0.2 * rng.standard_normal((N, L, d)), axis=1)).reshape(N, -1)
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, normalization=True,
              lengthscales=np.sqrt(d) * np.ones(d) if base == "rbf" else 1)
    got = make_kernel(K, dict(kw, base=base)).compute_K_symm(X)
    want = O.K_symm_tiled(make_oracle(dict(kw, base=base)), X, tile=32)
    assert relerr(got, want) <= TOL
    lv = make_kernel(K, dict(kw, base=base, normalization=False)).K(X[:40], return_levels=True)
    assert relerr(lv, make_oracle(dict(kw, base=base, normalization=False)).K(X[:40], return_levels=True)) <= TOL


def test_config3_shape_reduced(K):
    """BASELINE.json configs[2] shape (L=50, d=6, num_levels=4, RBF, Kzz + Kzx + Kxx-diag) at T=40, N=200."""
    rng = np.random.default_rng(2)
    T, N, L, d, M = 40, 200, 50, 6, 4
    X = np.cumsum(0.2 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base="rbf", lengthscales=np.sqrt(d) * np.ones(d))
    for incr in (False, True):
        Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d) if incr else (M * (M + 1) // 2, T, d))
        got = make_kernel(K, kw).K_tens_n_seq_covs(Z, X, increments=incr)
        want = make_oracle(kw).K_tens_n_seq_covs(Z, X, increments=incr)
        for g, w in zip(got, want):
            assert relerr(g, w) <= TOL


@pytest.mark.parametrize("L1,L2", [(1, 1), (2, 2), (1, 7), (3, 40), (40, 3), (17, 64), (64, 65), (130, 9), (9, 130), (300, 20)])
def test_ragged_and_extreme_lengths(K, L1, L2):
    rng = np.random.default_rng(L1 * 1000 + L2)
    d, M = 2, 3
    X = np.cumsum(0.3 * rng.standard_normal((9, L1, d)), axis=1).reshape(9, -1)
    Y = np.cumsum(0.3 * rng.standard_normal((5, L2, d)), axis=1).reshape(5, -1)
    for base in ("linear", "rbf"):
        for norm in (False, True):
            kx = make_kernel(K, dict(input_dim=L1 * d, num_features=d, num_levels=M, base=base, normalization=norm))
            ko = make_oracle(dict(input_dim=L1 * d, num_features=d, num_levels=M, base=base, normalization=norm))
            if norm and min(L1, L2) == 1:
                continue   # a single observation has zero-norm levels: the reference divides by sqrt(jitter) noise
            # presliced: GPflow's Kernel._slice would cut X2 down to the constructor's input_dim columns
            assert relerr(kx.K(X, Y, presliced=True), ko.K(X, Y)) <= TOL, (base, norm)
            assert relerr(kx.K(Y, presliced=True), ko.K(Y)) <= TOL, (base, norm)


def test_long_sequences_use_the_whole_wave_group(K):
    """L > 128 rows on the register side: G = 64 (one pair per wavefront, wave_shr carries)."""
    rng = np.random.default_rng(7)
    N, L, d, M = 6, 400, 2, 4
    X = np.cumsum(0.1 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    for base in ("linear", "rbf"):
        kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base)
        assert relerr(make_kernel(K, kw).K(X), make_oracle(kw).K(X)) <= TOL


def test_empty_inputs(K):
    kern = K.SignatureLinear(12, 3, 3)
    assert kern.K(np.zeros((0, 12))).shape == (0, 0)
    assert kern.K(np.zeros((0, 12)), np.zeros((4, 12))).shape == (0, 4)
    assert kern.K(np.ones((3, 12)), np.zeros((0, 12)), return_levels=True).shape == (4, 3, 0)


def test_num_levels_1_to_8(K):
    rng = np.random.default_rng(8)
    X = np.cumsum(0.2 * rng.standard_normal((12, 15, 3)), axis=1).reshape(12, -1)
    for M in range(1, 9):
        kw = dict(input_dim=45, num_features=3, num_levels=M, base="rbf", normalization=True)
        assert relerr(make_kernel(K, kw).K(X, return_levels=True), make_oracle(kw).K(X, return_levels=True)) <= TOL, M
        Z = rng.standard_normal((M * (M + 1) // 2, 5, 3))
        assert relerr(make_kernel(K, kw).K_tens_vs_seq(Z, X), make_oracle(kw).K_tens_vs_seq(Z, X)) <= TOL, M


def test_active_dims_and_presliced(K):
    rng = np.random.default_rng(9)
    L, d = 10, 2
    X = rng.standard_normal((7, L * d + 3))
    # GPflow: input_dim is the number of ACTIVE columns (kernels.py:53, :56)
    kern = K.SignatureRBF(L * d, d, 3, active_dims=list(range(1, 1 + L * d)))
    ko = O.SignatureKernelOracle(L * d, d, 3, base="rbf")
    assert relerr(kern.K(X), ko.K(X[:, 1:1 + L * d])) <= TOL
    assert relerr(kern.K(X[:, 1:1 + L * d], presliced=True), ko.K(X[:, 1:1 + L * d])) <= TOL


def test_hyperparameters_are_live_attributes(K):
    rng = np.random.default_rng(10)
    L, d, M = 12, 3, 3
    X = rng.standard_normal((8, L * d))
    kern = K.SignatureRBF(L * d, d, M)
    kern.sigma = 2.5
    kern.variances = np.array([0.3, 1.1, 0.7, 2.0])
    kern.lengthscales = np.array([0.5, 2.0, 1.3])
    ko = O.SignatureKernelOracle(L * d, d, M, base="rbf", variances=kern.variances, lengthscales=kern.lengthscales)
    ko.sigma = 2.5
    assert relerr(kern.K(X), ko.K(X)) <= TOL
    assert relerr(kern.Kdiag(X), ko.Kdiag(X)) <= TOL


# ------------------------------------------------------------------------------------------------
# transport: pointer modes, staging paths, kernel variants, shards
# ------------------------------------------------------------------------------------------------
def test_device_pointer_mode_matches_host_mode(K):
    import torch
    rng = np.random.default_rng(11)
    N, L, d, M = 50, 20, 4, 4
    X = rng.standard_normal((N, L * d))
    Y = rng.standard_normal((13, L * d))
    Z = rng.standard_normal((M * (M + 1) // 2, 6, d))
    kern = K.SignatureRBF(L * d, d, M)
    Xd, Yd, Zd = (torch.as_tensor(a, device="cuda:0") for a in (X, Y, Z))
    np.testing.assert_array_equal(kern.K(Xd).cpu().numpy(), kern.K(X))
    np.testing.assert_array_equal(kern.K(Xd, Yd).cpu().numpy(), kern.K(X, Y))
    np.testing.assert_array_equal(kern.K_tens_vs_seq(Zd, Xd).cpu().numpy(), kern.K_tens_vs_seq(Z, X))
    np.testing.assert_array_equal(kern.K_tens(Zd).cpu().numpy(), kern.K_tens(Z))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = kern.K(Xd)
    s.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), kern.K(X))


def test_lds_dma_staging_and_generic_kernels_agree_bitwise(K):
    """The three code paths that must not change a single bit: x records staged by load + ds_write vs
    global_load_lds (LDS DMA); kernels specialised on num_levels vs the run-time-levels kernels."""
    from gpsig_amd import _lib
    rng = np.random.default_rng(12)
    N, L, d, M = 70, 64, 8, 5
    X = rng.standard_normal((N, L * d))
    kern = K.SignatureLinear(L * d, d, M)
    ctx = _lib.context(0, 0)
    base = kern.K(X)
    try:
        ctx.set_option("glds", 0)
        np.testing.assert_array_equal(kern.K(X), base)
        ctx.set_option("exact", 0)
        np.testing.assert_array_equal(kern.K(X), base)
        ctx.set_option("glds", 1)
        np.testing.assert_array_equal(kern.K(X), base)
        ctx.set_option("exact", 1)
        ctx.set_option("max_run", 3)
        np.testing.assert_array_equal(kern.K(X), base)
    finally:
        ctx.set_option("glds", 1); ctx.set_option("exact", 1); ctx.set_option("max_run", 0)


def test_shards_partition_the_gram(K):
    from gpsig_amd import _lib
    rng = np.random.default_rng(13)
    N, L, d, M = 90, 16, 3, 3
    X = rng.standard_normal((N, L * d))
    kern = K.SignatureRBF(L * d, d, M)
    full = kern.K(X)
    ctx = _lib.context(0, 0)
    ctx.set_option("max_run", 8)
    try:
        import torch
        acc = None
        for r in range(4):
            ctx2 = _lib.context(0, torch.cuda.current_stream().cuda_stream)
            ctx2.set_shard(r, 4); ctx2.set_option("max_run", 8)
            out = torch.full((N, N), float("nan"), dtype=torch.float64, device="cuda:0")
            Xd = torch.as_tensor(X, device="cuda:0")
            p = kern._params([])
            import ctypes as C
            ctx2.set_pointer_mode(_lib.PTR_DEVICE)
            ctx2.call("gpsig_kernel_K", p, C.c_void_p(Xd.data_ptr()), None, N, N, L, L, 0, C.c_void_p(out.data_ptr()))
            ctx2.sync()
            o = out.cpu().numpy()
            acc = o if acc is None else np.where(np.isnan(acc), o, acc)
            ctx2.set_shard(0, 1); ctx2.set_option("max_run", 0)
        np.testing.assert_array_equal(acc, full)
    finally:
        ctx.set_option("max_run", 0)


@pytest.mark.parametrize("base", ["linear", "rbf", "matern32"])
def test_wide_state_spaces(K, base):
    """d * (num_lags + 1) up to 32 (the reference's benchmarks run with num_lags = 1 on data sets with more than 8 channels)."""
    rng = np.random.default_rng(77)
    for (N, N2, L, d, M, lags, f32) in [(9, 5, 20, 20, 4, 0, False), (7, 6, 100, 12, 3, 1, False), (6, 4, 30, 32, 5, 0, False), (8, 8, 40, 17, 4, 0, True)]:
        X, X2 = rng.standard_normal((N, L * d)) * 0.4, rng.standard_normal((N2, L * d)) * 0.4
        cls = {"linear": K.SignatureLinear, "rbf": K.SignatureRBF, "matern32": K.SignatureMatern32}[base]
        kw = dict(num_lags=lags or None, lengthscales=rng.uniform(0.8, 1.5, d))
        k = cls(L * d, d, M, **kw)
        ko = O.SignatureKernelOracle(L * d, d, M, base=base, **kw)
        dt = np.float32 if f32 else np.float64
        tol = 1e-4 if f32 else 1e-6
        for got, want in ((k.K(X.astype(dt)), ko.K(X)), (k.K(X.astype(dt), X2.astype(dt)), ko.K(X, X2)), (k.Kdiag(X.astype(dt)), ko.Kdiag(X))):
            assert np.abs(np.asarray(got, dtype=np.float64) - want).max() <= tol * np.abs(want).max(), (base, d, lags, f32)
        Z = rng.standard_normal((M * (M + 1) // 2, 5, d * (lags + 1))) * 0.4
        got, want = k.K_tens_vs_seq(Z.astype(dt), X.astype(dt)), ko.K_tens_vs_seq(Z, X)
        assert np.abs(np.asarray(got, dtype=np.float64) - want).max() <= tol * np.abs(want).max()


def test_compute_base_kern_symm(K):
    """kernels.py:150-157: the static kernel between all observations, (N, N, L, L), after scaling and lags."""
    rng = np.random.default_rng(90)
    N, L, d, M = 5, 9, 3, 3
    X = rng.standard_normal((N, L * d))
    for base, kw in (("rbf", dict(lengthscales=rng.uniform(0.7, 1.4, d))), ("matern32", dict(num_lags=1)), ("linear", {})):
        kx, ko = make_kernel(K, dict(input_dim=L * d, num_features=d, num_levels=M, base=base, **kw)), \
            make_oracle(dict(input_dim=L * d, num_features=d, num_levels=M, base=base, **kw))
        got, want = kx.compute_base_kern_symm(X), ko.compute_base_kern_symm(X)
        assert got.shape == (N, N, L, L) and relerr(got, want) <= TOL


@pytest.mark.parametrize("family", ["gauss", "exp", "mixed"])
def test_spectral_base_kernel(K, family):
    """SignatureSpectral (kernels.py:894-942): every evaluation of the exact mode against the oracle."""
    rng = np.random.default_rng(88)
    N, N2, L, d, M, T, Q = 9, 6, 14, 3, 4, 5, 5
    X, X2 = 0.5 * rng.standard_normal((N, L * d)), 0.5 * rng.standard_normal((N2, L * d))
    for order, norm, diff in ((1, True, True), (1, False, True), (1, True, False)):
        k = K.SignatureSpectral(L * d, d, M, family=family, Q=Q, order=order, normalization=norm, difference=diff, variances=rng.uniform(0.5, 1.5, M + 1))
        k.alpha, k.omega, k.gamma = rng.uniform(0.3, 1.2, Q), 0.3 * rng.standard_normal((Q, d)), rng.uniform(0.4, 1.3, (Q, d))
        fam = {"gauss": "rbf", "exp": "exp", "mixed": "mixed"}[family]
        ko = O.SignatureKernelOracle(L * d, d, M, base="spectral", order=order, normalization=norm, difference=diff, lengthscales=None,
                                     variances=k.variances, base_params=dict(alpha=k.alpha, omega=k.omega, gamma=k.gamma, family=fam))
        assert relerr(k.K(X), ko.K(X)) <= TOL
        assert relerr(k.K(X, X2, return_levels=True), ko.K(X, X2, return_levels=True)) <= TOL
        assert relerr(k.Kdiag(X), ko.Kdiag(X)) <= TOL
        for incr in (False, True):
            Z = 0.5 * rng.standard_normal((M * (M + 1) // 2, T, 2, d) if incr else (M * (M + 1) // 2, T, d))
            assert relerr(k.K_tens(Z, increments=incr), ko.K_tens(Z, increments=incr)) <= TOL
            assert relerr(k.K_tens_vs_seq(Z, X, increments=incr, return_levels=True), ko.K_tens_vs_seq(Z, X, increments=incr, return_levels=True)) <= TOL
            got, want = k.K_tens_n_seq_covs(Z, X, increments=incr), ko.K_tens_n_seq_covs(Z, X, increments=incr)
            for g, w in zip(got, want):
                assert relerr(g, w) <= TOL
    with pytest.raises(ValueError):
        K.SignatureSpectral(L * d, d, M, family="nope")
    got32 = k.K(X.astype(np.float32))                    # no float32 spectral kernel: float64 kernels, rounded
    assert got32.dtype == np.float32 and relerr32(got32, ko.K(X.astype(np.float32).astype(np.float64))) <= TOL32
    k2 = K.SignatureSpectral(L * d, d, M, family=family, Q=Q, order=2, normalization=False)       # higher order: through the fallback too
    k2.alpha, k2.omega, k2.gamma = k.alpha, k.omega, k.gamma
    ko2 = O.SignatureKernelOracle(L * d, d, M, base="spectral", order=2, normalization=False, lengthscales=None,
                                  base_params=dict(alpha=k.alpha, omega=k.omega, gamma=k.gamma, family=fam))
    assert relerr(k2.K(X, X2), ko2.K(X, X2)) <= TOL


@pytest.mark.parametrize("family", ["gauss", "exp", "mixed"])
def test_spectral_wavefront_kernels(K, family):
    """SignatureSpectral's sequence-vs-sequence evaluations through the wavefront kernels with the family at compile time
    (seq_step_spectral; float64, first order, differences, d <= 16) against the one-pair-per-thread kernel they replace and the
    oracle: 16- and 64-lane pair groups, ragged lengths on both sides, every padded width, symmetric / cross / diagonal."""
    from gpsig_amd import _lib
    rng = np.random.default_rng(89)
    fam = {"gauss": "rbf", "exp": "exp", "mixed": "mixed"}[family]
    for N, N2, L, L2, d, M, Q in ((9, 6, 14, 14, 3, 4, 5), (5, 7, 70, 33, 6, 3, 2), (6, 4, 130, 9, 11, 5, 3), (4, 4, 300, 20, 2, 2, 4), (3, 5, 40, 40, 16, 3, 2)):
        X = np.cumsum(0.2 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
        X2 = np.cumsum(0.2 * rng.standard_normal((N2, L2, d)), axis=1).reshape(N2, -1)
        for norm in (True, False):
            k = K.SignatureSpectral(L * d, d, M, family=family, Q=Q, normalization=norm, variances=rng.uniform(0.5, 1.5, M + 1))
            k.alpha, k.omega, k.gamma = rng.uniform(0.3, 1.2, Q), 0.3 * rng.standard_normal((Q, d)), rng.uniform(0.4, 1.3, (Q, d))
            ko = O.SignatureKernelOracle(L * d, d, M, base="spectral", normalization=norm, lengthscales=None, variances=k.variances,
                                         base_params=dict(alpha=k.alpha, omega=k.omega, gamma=k.gamma, family=fam))
            ctx = _lib.context(0, 0)
            got = {}
            try:
                for wave in (1, 0):
                    ctx.set_option("spectral_wave", wave)
                    got[wave] = (k.K(X), k.K(X, X2, presliced=True, return_levels=True), k.Kdiag(X, return_levels=True))
            finally:
                ctx.set_option("spectral_wave", 1)
            for a, b in zip(got[1], got[0]):
                assert np.abs(a - b).max() <= 1e-11 * np.abs(b).max(), (N, L, d)
            assert relerr(got[1][0], ko.K(X)) <= TOL
            assert relerr(got[1][2], ko.Kdiag(X, return_levels=True)) <= TOL


@pytest.mark.parametrize("base", ["linear", "rbf"])
def test_state_spaces_wider_than_64_features(K, base):
    """More than 64 features per lag copy (the reference's benchmark suite has PEMS with 963): the lengthscales travel to the kernels
    through device memory instead of by value (ScaleParams::ls_dev) and the evaluations run through the any-shape kernels."""
    rng = np.random.default_rng(97)
    for N, L, d, M, T, lags in ((6, 9, 100, 3, 4, 0), (4, 7, 70, 2, 3, 1), (3, 6, 963, 2, 2, 0)):
        X = np.cumsum(0.3 / np.sqrt(d) * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
        X2 = np.cumsum(0.3 / np.sqrt(d) * rng.standard_normal((5, L, d)), axis=1).reshape(5, -1)
        kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, lengthscales=0.7 + rng.random(d), variances=0.5 + rng.random(M + 1))
        if lags:
            kw["num_lags"] = lags
        kx, ko = make_kernel(K, kw), make_oracle(kw)
        de = d * (lags + 1)
        assert relerr(kx.K(X), ko.K(X)) <= TOL
        assert relerr(kx.K(X, X2), ko.K(X, X2)) <= TOL
        assert relerr(kx.Kdiag(X), ko.Kdiag(X)) <= TOL
        for incr in (False, True):
            Z = rng.standard_normal((M * (M + 1) // 2, T, 2, de) if incr else (M * (M + 1) // 2, T, de)) / np.sqrt(d)
            got, want = kx.K_tens_n_seq_covs(Z, X, increments=incr), ko.K_tens_n_seq_covs(Z, X, increments=incr)
            for g, w in zip(got, want):
                assert relerr(g, w) <= TOL, (d, incr)
        got32 = kx.K(X.astype(np.float32))
        assert got32.dtype == np.float32 and relerr32(got32, ko.K(X.astype(np.float32).astype(np.float64))) <= TOL32


def test_any_shape_fallback(K):
    """Shapes the wavefront kernel is not built for -- both sides longer than its column capacity, more than 32 state-space
    dimensions after lags -- go through the one-pair-per-thread fallback (float64, order 1) and must match the oracle too."""
    rng = np.random.default_rng(91)
    cases = [("linear", 5, 4, 600, 2, 3, None, True, 1), ("rbf", 4, 3, 530, 2, 3, None, True, 1), ("matern32", 3, 3, 300, 12, 3, None, True, 1),
             ("rbf", 4, 4, 40, 20, 4, 1, True, 1), ("linear", 4, 3, 140, 20, 3, None, False, 1), ("mix", 3, 3, 30, 24, 3, 1, True, 1),
             ("linear", 4, 3, 140, 3, 4, None, False, 4), ("rbf", 3, 3, 70, 2, 6, None, True, 6), ("matern52", 3, 2, 20, 24, 3, 1, True, 2),
             ("linear", 3, 3, 540, 2, 3, None, True, 2), ("rbf", 4, 3, 12, 40, 3, None, True, 1), ("linear", 3, 3, 9, 64, 3, None, True, 2),
             ("matern32", 3, 2, 10, 33, 2, 1, True, 1)]
    for base, N, N2, L, d, M, lags, norm, order in cases:
        X = np.cumsum(0.05 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
        X2 = np.cumsum(0.05 * rng.standard_normal((N2, L, d)), axis=1).reshape(N2, -1)
        kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, num_lags=lags, normalization=norm, lengthscales=0.8 + 0.4 * rng.random(d),
                  order=order)
        kx, ko = make_kernel(K, kw), make_oracle(kw)
        assert relerr(kx.K(X), ko.K(X)) <= TOL, (base, L, d, order)
        assert relerr(kx.K(X, X2, return_levels=True), ko.K(X, X2, return_levels=True)) <= TOL
        assert relerr(kx.Kdiag(X), ko.Kdiag(X)) <= TOL
        Z = 0.3 * rng.standard_normal((M * (M + 1) // 2, 4, d * ((lags or 0) + 1)))
        got, want = kx.K_tens_n_seq_covs(Z, X), ko.K_tens_n_seq_covs(Z, X)
        for g, w in zip(got, want):
            assert relerr(g, w) <= TOL


def test_unsupported_shapes_fail_loudly(K):
    assert K.SignatureLinear(2 * 600, 2, 3, order=2).K(np.zeros((2, 1200), dtype=np.float32)).dtype == np.float32   # float64 fallback, rounded
    wide = K.SignatureLinear(70 * 5, 70, 3).K(np.zeros((2, 350)))    # beyond 64 features per lag copy: any-shape kernels, lengthscales from device memory
    assert np.isfinite(wide).all() and np.allclose(np.diag(wide), 4.0)
    with pytest.raises(NotImplementedError):
        K.SignatureLinear(5000 * 2, 5000, 2).K(np.zeros((2, 10000)))      # more than 4096 features per lag copy
    assert K.SignatureRBF(12, 3, 3, low_rank=True, num_components=4).K(np.zeros((4, 12), dtype=np.float32)).dtype == np.float32   # via float64
    with pytest.raises(ValueError):
        K.SignatureLinear(12, 3, 3).K_tens(np.zeros((5, 4, 3)))            # lt must be 6


# ------------------------------------------------------------------------------------------------
# (c) full-size properties (BASELINE.json configs[1]: N=4096, L=64, d=8, num_levels=5, fp64)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", ["linear", "rbf"])
def test_full_config2_properties(K, base):
    import torch
    rng = np.random.default_rng(2)
    N, L, d, M = 4096, 64, 8, 5
    X = (rng.standard_normal((N, L, d)) if base == "linear" else np.cumsum(0.2 * rng.standard_normal((N, L, d)), axis=1)).reshape(N, -1)
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, lengthscales=np.sqrt(d) * np.ones(d) if base == "rbf" else 1)
    kern = make_kernel(K, kw)
    G = kern.K(torch.as_tensor(X, device="cuda:0"))
    torch.cuda.synchronize()
    assert torch.isfinite(G).all()
    assert torch.equal(G, G.T)                                              # exactly symmetric (one pair, two stores)
    assert (G.diagonal() - (M + 1.0)).abs().max().item() < 1e-12           # normalised levels: diag = sum of variances
    # sub-blocks equal the oracle on the corresponding sub-sample (normalisation is per sequence)
    idx = np.concatenate([np.arange(0, 24), np.arange(2040, 2064), np.arange(N - 24, N)])
    want = make_oracle(kw).K(X[idx])
    got = G[np.ix_(idx, idx)].cpu().numpy() if False else G.cpu().numpy()[np.ix_(idx, idx)]
    assert relerr(got, want) <= TOL
    # cross Gram of two halves == the off-diagonal block of the symmetric Gram (different code path: PRED_ALL)
    A, B = torch.as_tensor(X[:512], device="cuda:0"), torch.as_tensor(X[3000:3300], device="cuda:0")
    C = kern.K(A, B).cpu().numpy()
    assert relerr(C, G.cpu().numpy()[:512, 3000:3300]) <= 1e-9
    # positive semi-definite up to rounding
    ev = torch.linalg.eigvalsh(G[:1024, :1024])
    assert ev.min().item() > -1e-8
    if base == "linear":
        # the two evaluations of the linear kernel -- the contraction of explicit level features on the matrix cores (what ran above)
        # and the pair recursion on the vector unit -- agree entry by entry at full size
        from gpsig_amd import _lib
        ctx = _lib.context(0, torch.cuda.current_stream().cuda_stream)
        try:
            ctx.set_option("sig_features", 0)
            G0 = kern.K(torch.as_tensor(X, device="cuda:0"))
        finally:
            ctx.set_option("sig_features", -1)
        assert float((G - G0).abs().max()) <= 1e-11 * float(G0.abs().max())


@pytest.mark.parametrize("base,incr", [("rbf", False), ("rbf", True), ("linear", True)])
def test_full_config3_properties(K, base, incr):
    """BASELINE configs[2] at its full size (T=512 inducing tensors, N=16384, L=50, d=6, num_levels=4): the three covariances of
    K_tens_n_seq_covs through the tile kernel -- sub-blocks against the oracle (first / middle / last tensors and sequences:
    tile, run and workgroup boundaries), the whole Kzx against the round-1 tensor-lane kernel, Kzz symmetric, Kxx-diag = the sum
    of the variances (normalised levels)."""
    import torch
    from gpsig_amd import _lib
    rng = np.random.default_rng(3)
    T, N, L, d, M = 512, 16384, 50, 6, 4
    X = np.cumsum(0.2 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d) if incr else (M * (M + 1) // 2, T, d))
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, lengthscales=np.sqrt(d) * np.ones(d), variances=0.5 + rng.random(M + 1))
    kx, ko = make_kernel(K, kw), make_oracle(kw)
    Xd, Zd = torch.as_tensor(X, device="cuda:0"), torch.as_tensor(Z, device="cuda:0")
    Kzz, Kzx, Kxx = kx.K_tens_n_seq_covs(Zd, Xd, increments=incr)
    torch.cuda.synchronize()
    assert Kzx.shape == (T, N) and bool(torch.isfinite(Kzx).all())
    assert float((Kzz - Kzz.T).abs().max() / Kzz.abs().max()) <= 1e-14       # (t, t') and (t', t) multiply their components in different orders
    assert (Kxx - float(np.sum(kw["variances"]))).abs().max().item() < 1e-10
    ti = np.concatenate([np.arange(0, 5), np.arange(62, 67), np.arange(T - 4, T)])
    ni = np.concatenate([np.arange(0, 6), np.arange(14, 19), np.arange(8190, 8195), np.arange(N - 5, N)])
    want = ko.K_tens_n_seq_covs(Z[:, ti], X[ni], increments=incr)
    h = Kzx.cpu().numpy()
    assert relerr(h[np.ix_(ti, ni)], want[1]) <= TOL
    assert relerr(Kzz.cpu().numpy()[np.ix_(ti, ti)], want[0]) <= TOL
    ctx = _lib.context(0, torch.cuda.current_stream().cuda_stream)
    try:
        ctx.set_option("tvs_tile", 0)
        old = kx.K_tens_vs_seq(Zd, Xd, increments=incr)
    finally:
        ctx.set_option("tvs_tile", -1)
    assert float((old - Kzx).abs().max() / Kzx.abs().max()) <= 1e-12


def test_owned_row_blocks_reassemble_the_symmetric_gram(K):
    """The multi-GPU decomposition (gpsig_kernel_K_symm_rows + gpsig_symmetrize_owned_rows) on one GPU: the row
    blocks of a 3-rank partition, stacked and symmetrised, are bit-identical to K(X)."""
    import ctypes as C
    import torch
    from gpsig_amd import _lib, parallel
    rng = np.random.default_rng(14)
    for n in (90, 37):
        L, d, M = 16, 3, 3
        X = torch.as_tensor(rng.standard_normal((n, L * d)), device="cuda:0")
        kern = K.SignatureRBF(L * d, d, M)
        full = kern.K(X)
        ctx = _lib.context(0, torch.cuda.current_stream().cuda_stream)
        ctx.set_pointer_mode(_lib.PTR_DEVICE)
        world = 3
        b = parallel.row_partition(n, world)
        half = torch.zeros((n, n), dtype=torch.float64, device="cuda:0")
        keep = []
        p = kern._params(keep)
        for r in range(world):
            blk = half[b[r]:b[r + 1]]
            ctx.call("gpsig_kernel_K_symm_rows", p, C.c_void_p(X.data_ptr()), n, L, b[r], b[r + 1], C.c_void_p(blk.data_ptr()))
        out = torch.empty_like(half)
        ctx.check(ctx._lib.gpsig_symmetrize_owned_rows(ctx._h, _lib.F64, C.c_void_p(half.data_ptr()), n, C.c_void_p(out.data_ptr())))
        torch.cuda.synchronize()
        assert torch.equal(out, full)
        want, owned = parallel.symmetrize_reference(half.cpu().numpy())
        np.testing.assert_array_equal(want, full.cpu().numpy())
        assert (half.cpu().numpy()[~owned] == 0).all()          # nothing outside a row's owned columns is touched
    # ShardedGram with world == 1 is kern.K
    g = parallel.ShardedGram(kern, n, torch.device("cuda", 0))
    assert torch.equal(g(X), full)


@pytest.mark.parametrize("n,world,chunks", [(90, 3, 1), (37, 2, 2), (4096, 8, 4)])
def test_compact_row_blocks_reassemble_the_symmetric_gram(K, n, world, chunks):
    """What every rank of ShardedGram does, rank after rank on one GPU: chunked compact row blocks
    (gpsig_kernel_K_symm_rows_compact) of a `world`-rank partition, stacked and symmetrised
    (gpsig_symmetrize_compact_rows), are bit-identical to K(X) -- at BASELINE configs[1]'s size for an 8-rank partition."""
    import ctypes as C
    import torch
    from gpsig_amd import _lib, parallel
    rng = np.random.default_rng(n)
    L, d, M = (64, 8, 5) if n >= 4096 else (16, 3, 3)
    X = torch.as_tensor(rng.standard_normal((n, L * d)), device="cuda:0")
    kern = K.SignatureLinear(L * d, d, M) if n >= 4096 else K.SignatureRBF(L * d, d, M)
    full = kern.K(X)
    ctx = _lib.context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_pointer_mode(_lib.PTR_DEVICE)
    g = parallel.ShardedGram(kern, n, torch.device("cuda", 0), 0, world, chunks=chunks)
    W = n // 2 + 1
    half = torch.full((g.per * world, W), float("nan"), dtype=torch.float64, device="cuda:0")
    keep = []
    p = kern._params(keep)
    for r in range(world):
        b0, b1 = g.bounds[r], g.bounds[r + 1]
        for k in range(chunks):
            r0 = min(b0 + k * g.chunk_rows, b1)
            r1 = min(r0 + g.chunk_rows, b1)
            if r1 > r0:
                blk = half[r * g.per + k * g.chunk_rows:]
                ctx.call("gpsig_kernel_K_symm_rows_compact", p, C.c_void_p(X.data_ptr()), n, L, r0, r1, C.c_void_p(blk.data_ptr()))
    out = torch.empty((n, n), dtype=torch.float64, device="cuda:0")
    ctx.symmetrize_compact_rows(_lib.F64, C.c_void_p(half.data_ptr()), n, C.c_void_p(out.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out, full)
    h = half[:n].cpu().numpy()
    assert np.isnan(h).sum() == (n // 2 if n % 2 == 0 else 0)      # every owned slot written, the tie slots untouched
    if n <= 128:
        np.testing.assert_array_equal(parallel.symmetrize_compact_reference(np.nan_to_num(h)), full.cpu().numpy())
    if n >= 4096:
        # "sig_features_keep": a rank's chunks build SignatureLinear's feature matrix once; same numbers, fewer feature launches; new
        # sequence values or parameters behind the same pointer are NOT picked up inside the window (the caller's promise) but are after it
        b0 = g.bounds[3]
        blocks = lambda: [(b0 + k * g.chunk_rows, b0 + (k + 1) * g.chunk_rows) for k in range(chunks)]
        ref = half[3 * g.per:4 * g.per].clone()
        got = torch.full_like(ref, float("nan"))
        ctx.timing_reset()
        try:
            ctx.set_option("sig_features_keep", 1)
            for k, (r0, r1) in enumerate(blocks()):
                ctx.call("gpsig_kernel_K_symm_rows_compact", p, C.c_void_p(X.data_ptr()), n, L, r0, r1, C.c_void_p(got[k * g.chunk_rows:].data_ptr()))
        finally:
            ctx.set_option("sig_features_keep", 0)
        torch.cuda.synchronize()
        assert torch.equal(torch.nan_to_num(got), torch.nan_to_num(ref))
        X.mul_(1.5)                                                  # outside the window: the next call sees the new values
        r0, r1 = blocks()[0]
        ctx.call("gpsig_kernel_K_symm_rows_compact", p, C.c_void_p(X.data_ptr()), n, L, r0, r1, C.c_void_p(got.data_ptr()))
        torch.cuda.synchronize()
        want = kern.K(X)[r0:r0 + 4]
        j = torch.arange(W, device="cuda:0")
        for i in range(4):                                            # row r0 + i owns columns r0 + i - n/2 .. r0 + i
            cols = (r0 + i - n // 2 + j) % n
            own = torch.isfinite(got[i])
            assert torch.equal(got[i][own], want[i][cols][own])


def test_full_config4_single_gpu_properties(K):
    """BASELINE configs[3]'s problem (N=32768, L=64, d=8, num_levels=5) on ONE GPU: the 8-rank compact row blocks, stacked and
    symmetrised, against size-independent properties and against the oracle / the single-call K on sub-blocks."""
    import ctypes as C
    import torch
    from gpsig_amd import _lib, parallel
    rng = np.random.default_rng(4)
    N, L, d, M, world, chunks = 32768, 64, 8, 5, 8, 4
    Xh = rng.standard_normal((N, L * d))
    X = torch.as_tensor(Xh, device="cuda:0")
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base="linear")
    kern = make_kernel(K, kw)
    ctx = _lib.context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_pointer_mode(_lib.PTR_DEVICE)
    g = parallel.ShardedGram(kern, N, torch.device("cuda", 0), 0, world, chunks=chunks)
    keep = []
    p = kern._params(keep)
    for r in range(world):
        for k in range(chunks):
            r0 = g.bounds[r] + k * g.chunk_rows
            blk = g.half[r * g.per + k * g.chunk_rows:]
            ctx.call("gpsig_kernel_K_symm_rows_compact", p, C.c_void_p(X.data_ptr()), N, L, r0, r0 + g.chunk_rows, C.c_void_p(blk.data_ptr()))
    ctx.symmetrize_compact_rows(_lib.F64, C.c_void_p(g.half.data_ptr()), N, C.c_void_p(g.out.data_ptr()))
    G = g.out
    torch.cuda.synchronize()
    assert torch.isfinite(G).all()
    for r0 in range(0, N, 4096):                                           # exactly symmetric, block by block (no N x N temporary)
        assert torch.equal(G[r0:r0 + 4096], G[:, r0:r0 + 4096].T)
    assert (G.diagonal() - (M + 1.0)).abs().max().item() < 1e-12
    # sub-blocks near the diagonal, across the wrap-around and at the ownership tie (distance N/2) against the oracle
    idx = np.concatenate([np.arange(0, 12), np.arange(N // 2 - 6, N // 2 + 6), np.arange(N - 12, N)])
    want = make_oracle(kw).K(Xh[idx])
    got = G[torch.as_tensor(idx, device="cuda:0")][:, torch.as_tensor(idx, device="cuda:0")].cpu().numpy()
    assert relerr(got, want) <= TOL
    # a block of rows of one rank against the cross Gram of the same sequences (different code path: PRED_ALL)
    A, B = X[20000:20256], X[3000:3300]
    assert relerr(G[20000:20256, 3000:3300].cpu().numpy(), kern.K(A, B).cpu().numpy()) <= 1e-9
    # the leading 4096 x 4096 block is the Gram of the first 4096 sequences (normalisation is per sequence)
    assert relerr(G[:4096, :4096].cpu().numpy(), kern.K(X[:4096]).cpu().numpy()) <= 1e-9


def _sharded_worker(rank, world, port, n, ret):
    import os
    import torch
    import torch.distributed as dist
    from gpsig_amd import kernels, parallel
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        L, d, M = 16, 3, 4
        X = torch.as_tensor(np.random.default_rng(5).standard_normal((n, L * d)), device="cuda:0")
        kern = kernels.SignatureRBF(L * d, d, M)
        out = parallel.ShardedGram(kern, n, torch.device("cuda", 0), rank, world, chunks=2)(X)
        if rank == 0:
            ret["equal"] = bool(torch.equal(out, kern.K(X)))
    finally:
        dist.destroy_process_group()


def test_sharded_gram_two_processes_one_gpu(K):
    """ShardedGram.__call__ on the real library with two ranks (two processes sharing cuda:0, gloo collectives staged through
    the host): rank 0's gathered, symmetrised Gram is bit-identical to K(X)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_sharded_worker, args=(2, port, 203, ret), nprocs=2, join=True)
        assert ret["equal"]


@pytest.mark.parametrize("T", [5, 40, 130])
def test_tensor_vs_sequence_lane_mappings_agree(K, T):
    """Kzx has two kernels: one lane per sequence (few tensors) and one lane per tensor (>= 32 tensors).  Both must
    match the oracle, for every base kernel family, increments, higher order, levels and lags."""
    from gpsig_amd import _lib
    rng = np.random.default_rng(T)
    N, L, d, M = 37, 23, 3, 4
    X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    ctx = _lib.context(0, 0)
    try:
        for base in ("linear", "rbf", "matern32"):
            for incr in (False, True):
                for order, lags in ((1, None), (3, None), (1, 1)):
                    dd = d * ((lags or 0) + 1)
                    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, dd) if incr else (M * (M + 1) // 2, T, dd))
                    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, order=order, num_lags=lags,
                              lengthscales=0.5 + rng.random(d))
                    want = make_oracle(kw).K_tens_vs_seq(Z, X, increments=incr, return_levels=True)
                    for mode, tile in ((0, -1), (1, 0), (1, 1)):      # sequence lanes, tensor lanes, tile kernel (order 1)
                        ctx.set_option("tensor_lanes", mode)
                        ctx.set_option("tvs_tile", tile)
                        got = make_kernel(K, kw).K_tens_vs_seq(Z, X, increments=incr, return_levels=True)
                        assert relerr(got, want) <= TOL, (base, incr, order, lags, mode, tile)
    finally:
        ctx.set_option("tensor_lanes", -1)
        ctx.set_option("tvs_tile", -1)


@pytest.mark.parametrize("base", ["linear", "rbf", "matern12", "matern32", "matern52", "poly"])
@pytest.mark.parametrize("incr", [False, True])
def test_tile_kernel_for_many_tensors(K, base, incr):
    """The Kzx tile kernel (tvs_tile_kernel.hpp; round 5: a wavefront per (64 tensors, run of sequences) drawn from a queue, the levels in
    one, two or three sets swept one after the other, rows by scalar loads, hand-scheduled table-driven exps for RBF and -- compile-time
    instances of their own -- the Matern families, result tiles of 16 sequences): ragged tensor / sequence counts across tile, run and
    tensor-block boundaries, every number of level sets, with and without the difference along time, level tensors and the normalised
    weighted sum."""
    from gpsig_amd import _lib
    rng = np.random.default_rng(5)
    L = 19
    ctx = _lib.context(0, 0)
    try:
        for T, N, nw, diff, M, d in ((70, 37, 1, True, 4, 5), (130, 83, 2, True, 4, 5), (64, 16, 2, False, 4, 6), (33, 49, 1, False, 3, 4),
                                     (65, 21, 3, True, 5, 3), (40, 17, 0, True, 5, 6), (40, 35, 0, True, 2, 8), (64, 33, 3, True, 6, 4),
                                     (50, 20, 0, False, 6, 7), (200, 150, 0, True, 4, 6), (520, 70, 0, True, 3, 4), (70, 300, 2, True, 4, 6)):
            X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
            Z = 0.7 * rng.standard_normal((M * (M + 1) // 2, T, 2, d) if incr else (M * (M + 1) // 2, T, d))
            kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, difference=diff, lengthscales=0.6 + rng.random(d),
                      variances=0.5 + rng.random(M + 1))
            ko = make_oracle(kw)
            ctx.set_option("tvs_tile", 1)
            ctx.set_option("tvs_tile_nw", nw)
            kx = make_kernel(K, kw)
            assert relerr(kx.K_tens_vs_seq(Z, X, increments=incr, return_levels=True),
                          ko.K_tens_vs_seq(Z, X, increments=incr, return_levels=True)) <= TOL, (T, N, nw, diff, "levels")
            got = kx.K_tens_vs_seq(Z, X, increments=incr)
            # (Matern-1/2's NORMALISED values inherit the rounding noise of kappa(x, x) = exp(-sqrt(max(noise, 1e-40))) at coincident points,
            # kernels.py:779-781, through the sequences' level diagonals: NumPy's matmul-based squared distance and the GPU's leave different
            # noise under the square root.  Seen: 2.8e-6 on one small entry of the 70 x 300 case, identically through the tile kernel in every
            # form, the round-1 kernel and round 4's library -- the reference's own conditioning, not a kernel's.  Its levels pass at 1e-6.)
            assert relerr(got, ko.K_tens_vs_seq(Z, X, increments=incr)) <= (1e-5 if base == "matern12" else TOL), (T, N, nw, diff, "sum")
            ctx.set_option("tvs_tile", 0)                          # the older tensor-lane kernel writes the same matrix
            assert relerr(make_kernel(K, kw).K_tens_vs_seq(Z, X, increments=incr), got) <= 1e-9
    finally:
        ctx.set_option("tvs_tile", -1)
        ctx.set_option("tvs_tile_nw", 0)


@pytest.mark.parametrize("base", ["linear", "cosine"])
@pytest.mark.parametrize("incr", [False, True])
def test_tensor_vs_sequence_through_level_features(K, base, incr):
    """K_tens_vs_seq and the Kzx of K_tens_n_seq_covs of the linear / cosine kernel as ONE product of the tensors' rank-one level features
    and the sequences' level features (option tvs_features = 1; signature_algs.py:101-160: K_m(z, x) = <z_1 (x) .. (x) z_m, Phi_m(x)>) against
    the oracle and against the tile kernel: normalisation on and off, differences, lags, higher orders, ragged sizes, host and device pointers."""
    import torch
    from gpsig_amd import _lib
    rng = np.random.default_rng(15)
    ctx = _lib.context(0, 0)
    off = 1.0 if base == "cosine" else 0.0
    try:
        for T, N, L, diff, M, d, norm, lags, order in ((70, 37, 19, True, 4, 5, True, 0, 1), (130, 83, 12, True, 4, 3, False, 1, 1),
                                                      (64, 16, 9, False, 3, 6, True, 0, 1), (33, 49, 15, True, 5, 3, True, 0, 3),
                                                      (40, 35, 8, True, 2, 8, False, 0, 2), (9, 200, 30, True, 4, 4, True, 2, 1)):
            X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1) + off
            de = d * (lags + 1)
            Z = 0.7 * rng.standard_normal((M * (M + 1) // 2, T, 2, de) if incr else (M * (M + 1) // 2, T, de)) + off
            kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, difference=diff, lengthscales=0.6 + rng.random(d),
                      variances=0.5 + rng.random(M + 1), normalization=norm, num_lags=lags or None, order=order)
            ko = make_oracle(kw)
            want = ko.K_tens_vs_seq(Z, X, increments=incr)
            ctx.set_option("tvs_features", 1)
            kx = make_kernel(K, kw)
            got = kx.K_tens_vs_seq(Z, X, increments=incr)
            assert relerr(got, want) <= TOL, (T, N, M, d, norm, lags, order)
            covs = kx.K_tens_n_seq_covs(Z, X, increments=incr)
            for a, b in zip(covs, ko.K_tens_n_seq_covs(Z, X, increments=incr)):
                assert relerr(a, b) <= TOL, (T, N, M, d, norm, lags, order, "covs")
            gd = kx.K_tens_vs_seq(torch.tensor(Z, device="cuda:0"), torch.tensor(X, device="cuda:0"), increments=incr)
            assert np.array_equal(gd.cpu().numpy(), got)                                   # device pointers: the same evaluation
            ctx.set_option("tvs_features", 0)                                               # the tile kernel writes the same matrix
            ref = make_kernel(K, kw).K_tens_vs_seq(Z, X, increments=incr)
            assert np.abs(ref - got).max() <= 1e-11 * max(1.0, np.abs(ref).max()), (T, N, M, d, norm, lags, order)
    finally:
        ctx.set_option("tvs_features", -1)


# ------------------------------------------------------------------------------------------------
# float32 (BASELINE.json configs[4]: RBF, fp32).  Tolerance, stated by SURVEY.md 8(d): 1e-4 on normalised entries
# (float32 rounding of O(1e-7) per operation through an L1 x L2 x M recursion; the fp64 oracle is the reference).
# ------------------------------------------------------------------------------------------------
TOL32 = 1e-4


def relerr32(got, want):
    """float32 bound: max |K - K_ref| <= 1e-4 * max |K_ref| (matrix-relative: tensor-vs-sequence entries are signed sums that
    pass through zero, so an entry-relative bound has no meaning in float32)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("base", ["linear", "rbf", "matern32"])
def test_float32_matches_the_float64_oracle(K, base):
    rng = np.random.default_rng(32)
    N, L, d, M = 40, 30, 5, 4
    X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    Y = np.cumsum(0.3 * rng.standard_normal((11, L, d)), axis=1).reshape(11, -1)
    Z = rng.standard_normal((M * (M + 1) // 2, 9, d))
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, lengthscales=0.7 + rng.random(d))
    kx, ko = make_kernel(K, kw), make_oracle(kw)
    X32, Y32, Z32 = X.astype(np.float32), Y.astype(np.float32), Z.astype(np.float32)
    got = kx.K(X32)
    assert got.dtype == np.float32
    assert relerr32(got, ko.K(X32.astype(np.float64))) <= TOL32
    assert relerr32(kx.K(X32, Y32), ko.K(X32.astype(np.float64), Y32.astype(np.float64))) <= TOL32
    assert relerr32(kx.K_tens_vs_seq(Z32, X32), ko.K_tens_vs_seq(Z32.astype(np.float64), X32.astype(np.float64))) <= TOL32
    assert relerr32(kx.K_tens(Z32), ko.K_tens(Z32.astype(np.float64))) <= TOL32
    assert relerr32(kx.Kdiag(X32), ko.Kdiag(X32.astype(np.float64))) <= TOL32
    # mixed precision inputs are computed in float64
    assert kx.K(X32, Y).dtype == np.float64
    # without differences (kappa itself feeds the recursion): smaller inputs keep the levels in float32 range
    kw = dict(kw, difference=False)
    kx, ko = make_kernel(K, kw), make_oracle(kw)
    Xs, Ys = 0.3 * X32, 0.3 * Y32
    assert relerr32(kx.K(Xs), ko.K(Xs.astype(np.float64))) <= TOL32
    assert relerr32(kx.K(Xs, Ys), ko.K(Xs.astype(np.float64), Ys.astype(np.float64))) <= TOL32


def test_float32_config5_shape_reduced_n(K):
    """BASELINE.json configs[4] shape: L=128, d=16, num_levels=6, fp32, RBF, at N=48."""
    import torch
    rng = np.random.default_rng(5)
    N, L, d, M = 48, 128, 16, 6
    X = np.cumsum(0.1 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1).astype(np.float32)
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base="rbf", lengthscales=np.sqrt(d) * np.ones(d))
    got = make_kernel(K, kw).K(torch.as_tensor(X, device="cuda:0"))
    assert got.dtype == torch.float32
    want = O.K_symm_tiled(make_oracle(kw), X.astype(np.float64), tile=16)
    assert relerr(got.cpu().numpy(), want) <= TOL32
    assert torch.equal(got, got.T)


@pytest.mark.parametrize("base", ["linear", "rbf"])
def test_float32_packed_kernels(K, base):
    """seq_pk2_kernel.hpp (two y sequences per pair group on the packed float32 instructions) against the float64 oracle and
    against the one-sequence float32 kernels: odd sequence counts (the second sequence of the last group is missing), cross
    Grams with both sides odd, diagonals, level tensors, both built lane shapes (16 lanes x 4 columns, 64 x 2)."""
    from gpsig_amd import _lib
    rng = np.random.default_rng(77)
    ctx = _lib.context(0, 0)
    try:
        for N, N2, L, d, M in ((41, 17, 30, 5, 4), (23, 9, 61, 8, 5), (19, 7, 128, 16, 6), (12, 5, 100, 7, 5)):
            X = np.cumsum(0.15 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1).astype(np.float32)
            Y = np.cumsum(0.15 * rng.standard_normal((N2, L - 3, d)), axis=1).reshape(N2, -1).astype(np.float32)
            kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, lengthscales=(0.8 + rng.random(d)) * np.sqrt(d))
            kx, ko = make_kernel(K, kw), make_oracle(kw)
            X64, Y64 = X.astype(np.float64), Y.astype(np.float64)
            res = {}
            for pk2, waves in ((2, 1), (0, 0), (2, 4)):       # pk2 = 2: the packed kernels for the linear family too; 4 waves on one ring
                ctx.set_option("pk2", pk2)
                ctx.set_option("f32_waves", waves)
                res[pk2 + waves] = (kx.K(X), kx.K(X, Y), kx.K(Y, X), kx.Kdiag(X, return_levels=True), kx.K(X, return_levels=True))
            want = (ko.K(X64), ko.K(X64, Y64), ko.K(Y64, X64), ko.Kdiag(X64, return_levels=True), ko.K(X64, return_levels=True))
            for got, unpacked, shared, w in zip(res[3], res[0], res[6], want):
                assert got.dtype == np.float32 and relerr32(got, w) <= TOL32, (N, L, d, M)
                assert relerr32(got, unpacked.astype(np.float64)) <= TOL32
                assert np.array_equal(got, shared)            # the same arithmetic per pair, whatever the workgroup shape
            assert np.array_equal(res[3][0], res[3][0].T)
    finally:
        ctx.set_option("pk2", 1)
        ctx.set_option("f32_waves", 0)


def test_float32_full_config5_properties(K):
    """BASELINE.json configs[4] at its full size (N=2048, L=128, d=16, num_levels=6, fp32, RBF): exact symmetry, unit diagonal,
    sub-blocks against the float64 oracle, and the cross Gram of a row block against the symmetric one."""
    import torch
    rng = np.random.default_rng(0)
    N, L, d, M = 2048, 128, 16, 6
    X = np.cumsum(0.1 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1).astype(np.float32)
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base="rbf", lengthscales=np.sqrt(d) * np.ones(d))
    kx, ko = make_kernel(K, kw), make_oracle(kw)
    Xd = torch.as_tensor(X, device="cuda:0")
    G = kx.K(Xd)
    assert G.dtype == torch.float32 and torch.equal(G, G.T) and bool(torch.isfinite(G).all())
    Gh = G.cpu().numpy().astype(np.float64)
    assert np.abs(np.diag(Gh) - (M + 1)).max() <= 1e-4 * (M + 1)          # normalised levels: diagonal = sum of the variances
    for rows, cols in ((np.arange(0, 12), None), (np.arange(1000, 1008), np.arange(2040, 2048)),
                       (np.array([3, 1025, 2047]), np.array([0, 1023, 1024, 1026]))):
        # a diagonal block is the symmetric branch (jitter before normalising, kernels.py:431), anything else the cross one
        want = ko.K(X[rows].astype(np.float64)) if cols is None else ko.K(X[rows].astype(np.float64), X[cols].astype(np.float64))
        assert np.abs(Gh[np.ix_(rows, rows if cols is None else cols)] - want).max() <= TOL32 * np.abs(want).max()
    blk = kx.K(Xd[512:640], Xd).cpu().numpy().astype(np.float64)
    off = np.ones_like(blk, dtype=bool)
    off[np.arange(128), 512 + np.arange(128)] = False      # K(x, x) differs between the two branches by the jitter placement
    assert np.abs(blk - Gh[512:640])[off].max() <= TOL32 * np.abs(Gh).max()


def test_linear_gram_as_feature_contraction(K):
    """SignatureLinear, order 1, evaluated as ONE contraction of explicit level features on the float64 matrix cores (round 3,
    sig_feat_kernel.hpp: K_m(x, y) = <Phi_m(x), Phi_m(y)>) against the oracle and against the lattice kernels: symmetric and cross
    Grams, unequal lengths, levels, normalisation on / off, differences off, lags, ragged sizes across tile and depth-split boundaries,
    the raw level primitive, and the owned row blocks of the multi-GPU decomposition."""
    import ctypes as C
    from gpsig_amd import _lib, parallel
    rng = np.random.default_rng(311)
    ctx = _lib.context(0, 0)
    cases = [dict(N=37, N2=21, L=9, L2=9, d=3, M=4), dict(N=130, N2=50, L=20, L2=7, d=2, M=6), dict(N=260, N2=129, L=15, L2=12, d=8, M=3),
             dict(N=70, N2=9, L=11, L2=6, d=2, M=2, lags=1), dict(N=140, N2=33, L=10, L2=10, d=5, M=4, normalization=False),
             dict(N=45, N2=45, L=8, L2=8, d=4, M=5, difference=False), dict(N=150, N2=66, L=12, L2=10, d=2, M=8),
             dict(N=131, N2=40, L=10, L2=9, d=8, M=4, lags=0), dict(N=129, N2=3, L=66, L2=20, d=8, M=5),
             # the higher-order algorithm (signature_algs.py:37-74) as truncated-exponential features: every order up to num_levels,
             # both feature kernels (strided parents: d = 3, 2; sibling parents: d = 8 M = 4, d = 4 M = 5)
             dict(N=37, N2=21, L=9, L2=9, d=3, M=4, order=2), dict(N=40, N2=33, L=8, L2=7, d=3, M=4, order=4),
             dict(N=130, N2=50, L=12, L2=7, d=2, M=6, order=3), dict(N=131, N2=40, L=10, L2=9, d=8, M=4, order=3),
             dict(N=45, N2=45, L=8, L2=8, d=4, M=5, order=5, difference=False), dict(N=70, N2=9, L=11, L2=6, d=2, M=3, lags=1, order=2),
             dict(N=60, N2=17, L=20, L2=13, d=8, M=5, order=2, normalization=False),
             # SignatureCosine = the linear kernel of the unit vectors x / |x| (kernels.py:820-828): the same route
             dict(N=37, N2=21, L=9, L2=9, d=3, M=4, base="cosine"), dict(N=131, N2=40, L=10, L2=9, d=8, M=4, base="cosine", order=2),
             dict(N=70, N2=9, L=11, L2=6, d=2, M=3, lags=1, base="cosine", difference=False),
             # wider state spaces (d <= 16 with d^M <= 32,768), also reached through lags (5 features x 3 lag copies)
             dict(N=50, N2=33, L=12, L2=9, d=16, M=3), dict(N=140, N2=20, L=9, L2=9, d=12, M=4, order=2), dict(N=60, N2=61, L=14, L2=8, d=16, M=2),
             dict(N=45, N2=30, L=10, L2=7, d=10, M=3, order=3, normalization=False), dict(N=40, N2=12, L=12, L2=10, d=5, M=3, lags=2),
             dict(N=33, N2=8, L=9, L2=9, d=13, M=3, base="cosine"),
             dict(N=40, N2=20, L=8, L2=8, d=32, M=3), dict(N=36, N2=9, L=10, L2=7, d=24, M=3, order=3), dict(N=70, N2=31, L=9, L2=9, d=32, M=2),
             dict(N=30, N2=14, L=12, L2=8, d=10, M=3, lags=1, order=2), dict(N=25, N2=11, L=7, L2=7, d=19, M=3, normalization=False)]
    for cs in cases:
        N, N2, L, L2, d, M = (cs[k] for k in ("N", "N2", "L", "L2", "d", "M"))
        kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=cs.get("base", "linear"), lengthscales=0.7 + rng.random(d), variances=0.5 + rng.random(M + 1),
                  normalization=cs.get("normalization", True), difference=cs.get("difference", True), order=cs.get("order", 1))
        if cs.get("lags"):
            kw["num_lags"] = cs["lags"]
        kx, ko = make_kernel(K, kw), make_oracle(kw)
        kx.sigma = ko.sigma = 1.3
        shift = 1.0 if cs.get("base") == "cosine" else 0.0          # (away from the origin, where x / |x| is undefined)
        X = (shift + np.cumsum(0.4 * rng.standard_normal((N, L, d)), axis=1)).reshape(N, -1)
        Y = (shift + np.cumsum(0.4 * rng.standard_normal((N2, L2, d)), axis=1)).reshape(N2, -1)
        got = {}
        try:
            for route in (1, 0):
                ctx.set_option("sig_features", route)
                got[route] = (kx.K(X), kx.K(X, Y), kx.K(X, return_levels=True), kx.K(X, Y, return_levels=True))
        finally:
            ctx.set_option("sig_features", -1)
        want = (ko.K(X), ko.K(X, Y), ko.K(X, return_levels=True), ko.K(X, Y, return_levels=True))
        for a, b, w in zip(got[1], got[0], want):
            assert relerr(a, w) <= TOL and relerr(a, b) <= 1e-10, (cs, relerr(a, w), relerr(a, b))
        assert np.array_equal(got[1][0], got[1][0].T)                               # mirrored, not recomputed
        if L2 == L:         # the inducing-sequence covariances (kernels.py:674-761), including the X side divided twice (:713 + :750)
            try:
                ctx.set_option("sig_features", 1)
                for full in (False, True):
                    for lev in (False, True):
                        g3 = kx.K_seq_n_seq_covs(Y.reshape(N2, L2, -1), X, full_X2_cov=full, return_levels=lev)
                        w3 = ko.K_seq_n_seq_covs(Y.reshape(N2, L2, -1), X, full_X2_cov=full, return_levels=lev)
                        for a, w in zip(g3, w3):
                            assert relerr(a, w) <= TOL, (cs, full, lev, relerr(a, w))
            finally:
                ctx.set_option("sig_features", -1)
        try:            # the register-staged form of the contraction adds the same products in the same order as the LDS-DMA form
            ctx.set_option("sig_features", 1)
            ctx.set_option("sig_gemm_dma", 0)
            assert np.array_equal(kx.K(X), got[1][0]) and np.array_equal(kx.K(X, Y), got[1][1])
        finally:
            ctx.set_option("sig_gemm_dma", 1)
            ctx.set_option("sig_features", -1)
        if kw["normalization"]:
            assert np.array_equal(np.diag(got[1][0]), np.full(N, np.sum(kx.sigma * kx.variances)))       # kernels.py:430-433: exactly
    # float32 calls take the same route: computed in float64, rounded on the way out -- float32 rounding of the result is all that is left
    N, N2, L, d, M = 200, 90, 20, 16, 3
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base="linear", lengthscales=0.7 + rng.random(d))
    kx, ko = make_kernel(K, kw), make_oracle(kw)
    X32 = np.cumsum(0.2 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1).astype(np.float32)
    Y32 = np.cumsum(0.2 * rng.standard_normal((N2, L, d)), axis=1).reshape(N2, -1).astype(np.float32)
    for got, want in ((kx.K(X32), ko.K(X32.astype(np.float64))), (kx.K(X32, Y32), ko.K(X32.astype(np.float64), Y32.astype(np.float64))),
                      (kx.K(X32, return_levels=True), ko.K(X32.astype(np.float64), return_levels=True))):
        assert got.dtype == np.float32
        assert np.abs(got - want).max() <= 5e-7 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
    # the unscaled level primitive (what gpsig_seq_gram_levels returns) and the packed row blocks of the multi-GPU path
    N, L, d, M = 300, 14, 3, 4
    X = np.cumsum(0.4 * rng.standard_normal((N, L, d)), axis=1)
    kx = make_kernel(K, dict(input_dim=L * d, num_features=d, num_levels=M, base="linear", lengthscales=None))
    ko = make_oracle(dict(input_dim=L * d, num_features=d, num_levels=M, base="linear", lengthscales=None))
    try:
        ctx.set_option("sig_features", 1)
        lev = kx._K_seq(X)
        full = kx.K(X.reshape(N, -1))
        keep = []
        p = kx._params(keep)
        H = N // 2
        half = np.zeros((N, H + 1))
        for r0, r1 in ((0, 96), (96, 100), (100, 300)):
            blk = np.zeros((r1 - r0, H + 1))
            ctx.call("gpsig_kernel_K_symm_rows_compact", p, C.c_void_p(X.ctypes.data), N, L, r0, r1, C.c_void_p(blk.ctypes.data))
            half[r0:r1] = blk
    finally:
        ctx.set_option("sig_features", -1)
    assert relerr(lev, ko._K_seq(X)) <= TOL
    assert np.abs(parallel.symmetrize_compact_reference(half) - full).max() <= 1e-12 * np.abs(full).max()


# ------------------------------------------------------------------------------------------------
# low-rank mode (gpsig/low_rank_calculations.py, signature_algs.py:162-222): the reference's randomness is TF's and
# cannot be reproduced, so (i) given the SAME landmarks and projections the HIP path must equal the restatement of
# the intended maths exactly, (ii) in the exact limit it must reproduce the exact kernel, (iii) statistically the
# approximation error must shrink as num_components / rank_bound grow.
# ------------------------------------------------------------------------------------------------
def _lr_pair(K, base, L, d, M, **kw):
    kx = make_kernel(K, dict(input_dim=L * d, num_features=d, num_levels=M, base=base, low_rank=True, **kw))
    okw = {k: v for k, v in kw.items() if k not in ("num_components", "rank_bound", "sparsity")}
    return kx, make_oracle(dict(input_dim=L * d, num_features=d, num_levels=M, base=base, **okw))


# Low-rank parity.  Given the same random objects the two sides differ by rounding only, but the Nystrom step inverts the
# landmark Gram down to eigenvalues of the size of the jitter (1e-6): two correct eigendecompositions of a Gram with condition
# number ~1e6 agree to ~1e-16 * 1e6 per entry of the inverse, and the features inherit that.  Tolerance: 1e-7 for RBF.
# The LINEAR kernel's landmark Gram has rank d = 3 < c = 11: eight eigenvalues sit at the jitter draw (1e-7 .. 1e-6) with gaps of
# 1e-8 and less, so their eigenvectors -- a basis of the near-null space -- differ between two correct eigensolvers by rotations
# no sign rule removes; the level >= 2 features see them through the coordinate-pair projections at ~1e-6 of a level's scale
# (observed 9e-7 .. 2.4e-5 entry-relative from box to box, rocSOLVER against LAPACK).  Tolerance there: 1e-5 of the largest entry of
# each compared array, with (W + jitter)^-1 itself still at 1e-7.
LR_TOLS = {"rbf": 1e-7, "linear": 1e-5}


@pytest.mark.parametrize("sparsity", ["sqrt", "log", "lin"])
@pytest.mark.parametrize("base", ["rbf", "linear"])
def test_low_rank_equals_restatement_given_the_same_randomness(K, sparsity, base):
    rng = np.random.default_rng(41)
    LR_TOL = LR_TOLS[base]
    if base == "linear":          # rank-deficient landmark Gram (comment above): errors are judged on the scale of the whole array
        def relerr(got, want):
            got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
            assert got.shape == want.shape and np.isfinite(got).all()
            return float(np.abs(got - want).max() / np.abs(want).max())
    else:
        relerr = globals()["relerr"]
    N, L, d, M, T = 23, 12, 3, 4, 7
    X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    Y = np.cumsum(0.3 * rng.standard_normal((9, L, d)), axis=1).reshape(9, -1)
    for norm in (True, False):
        for incr in (False, True):
            Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d) if incr else (M * (M + 1) // 2, T, d))
            kx, ko = _lr_pair(K, base, L, d, M, normalization=norm, num_components=11, rank_bound=9, sparsity=sparsity,
                              lengthscales=0.6 + rng.random(d), variances=0.5 + rng.random(M + 1))
            kx.rng = np.random.default_rng(7)
            st = kx.draw_low_rank(X=X, X2=Y, Z=Z, increments=incr)
            # the oracle whitens the same landmarks with the same jitter draw on its own (NumPy eigh against the product's
            # rocSOLVER dsyevd, both with the largest component of every eigenvector positive); (W + jitter)^-1 = Wh Wh^T
            # does not depend on that convention
            lo = O.LowRankOracle(ko, st.landmarks, st.jitter_diag, st.sketches)
            inv_p, inv_o = st.whitening @ st.whitening.T, lo.Wh @ lo.Wh.T
            assert np.abs(inv_p - inv_o).max() <= 1e-7 * np.abs(inv_o).max()
            assert relerr(kx.K(X, lr_state=st), lo.K(X)) <= LR_TOL
            assert relerr(kx.K(X, Y, lr_state=st, return_levels=True), lo.K(X, Y, return_levels=True)) <= LR_TOL
            assert relerr(kx.K_tens(Z, increments=incr, lr_state=st), lo.K_tens(Z, increments=incr)) <= LR_TOL
            assert relerr(kx.K_tens_vs_seq(Z, X, increments=incr, lr_state=st, return_levels=True),
                          lo.K_tens_vs_seq(Z, X, increments=incr, return_levels=True)) <= LR_TOL
            assert relerr(kx.Kdiag(X, lr_state=st), lo.Kdiag(X)) <= LR_TOL
            if not incr:     # inducing sequences (kernels.py:674-761, low-rank branch): all three covariances, both layouts of Kx2x2
                for full in (False, True):
                    for lev in (False, True):
                        got = kx.K_seq_n_seq_covs(Y.reshape(9, L, d), X, full_X2_cov=full, return_levels=lev, lr_state=st)
                        want = lo.K_seq_n_seq_covs(Y, X, full_X2_cov=full, return_levels=lev)
                        for g, w in zip(got, want):
                            assert relerr(g, w) <= LR_TOL, (full, lev)


@pytest.mark.parametrize("base", ["linear", "rbf", "poly", "matern52"])
def test_tensor_gram_tiles(K, base):
    """Kzz in 16 x 16 tiles with the tensors staged in LDS (tens_gram_tile_kernel) against the one-thread-per-entry kernel
    (bit-identical: the same operations in the same order) and the oracle; ragged tensor counts, both layouts, float32."""
    from gpsig_amd import _lib
    rng = np.random.default_rng(93)
    for T, d, M, lags in ((1, 2, 2, 0), (37, 6, 4, 0), (64, 3, 5, 1), (100, 16, 3, 0)):
        kw = dict(input_dim=10 * d, num_features=d, num_levels=M, base=base, lengthscales=0.7 + rng.random(d), variances=0.5 + rng.random(M + 1))
        if base == "poly":
            lags = 0                        # SignaturePoly has no lags (the reference overwrites the lag weights)
        if lags:
            kw["num_lags"] = lags
        kx, ko = make_kernel(K, kw), make_oracle(kw)
        for incr in (False, True):
            Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d * (lags + 1)) if incr else (M * (M + 1) // 2, T, d * (lags + 1)))
            ctx = _lib.context(0, 0)
            got = {}
            try:
                for tile in (1, 0):
                    ctx.set_option("tens_tile", tile)
                    got[tile] = (kx.K_tens(Z, increments=incr), kx.K_tens(Z, increments=incr, return_levels=True),
                                 kx.K_tens(Z.astype(np.float32), increments=incr))
            finally:
                ctx.set_option("tens_tile", 1)
            for a, b in zip(got[1], got[0]):
                assert np.array_equal(a, b), (T, d, M, incr)
            assert relerr(got[1][0], ko.K_tens(Z, increments=incr)) <= TOL
            assert relerr(got[1][1], ko.K_tens(Z, increments=incr, return_levels=True)) <= TOL


@pytest.mark.parametrize("base,order", [("linear", 1), ("rbf", 1), ("matern32", 1), ("linear", 3), ("rbf", 2)])
def test_diagonal_pass_with_one_sequence_per_pair_group(K, base, order):
    """The diagonal pass (level diagonals for normalisation, Kdiag) with every pair group of a wavefront sweeping its own
    sequence (SeqGramArgs::diag_own) against the round-1 form (all groups sweep the same 64/G sequences, one emitted pair each):
    the same per-pair arithmetic, so bit-identical; and against the oracle."""
    from gpsig_amd import _lib
    rng = np.random.default_rng(91)
    for N, L, d, M in ((37, 20, 3, 4), (5, 64, 8, 5), (130, 9, 2, 3)):        # ragged last block; the headline shape; short records (deeper ring)
        X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
        Y = np.cumsum(0.3 * rng.standard_normal((7, L, d)), axis=1).reshape(7, -1)
        kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, order=order, lengthscales=0.7 + rng.random(d))
        ctx = _lib.context(0, 0)
        got = {}
        try:
            for own in (1, 0):
                ctx.set_option("diag_own", own)
                kx = make_kernel(K, dict(kw, normalization=False))
                kn = make_kernel(K, dict(kw, normalization=True))
                got[own] = (kx.Kdiag(X, return_levels=True), kn.K(X), kn.K(Y, X))
        finally:
            ctx.set_option("diag_own", 1)
        for a, b in zip(got[1], got[0]):
            assert np.array_equal(a, b), (N, L, base, order)
        ko = make_oracle(dict(kw, normalization=False))
        assert relerr(got[1][0], ko.Kdiag(X, return_levels=True)) <= TOL
        assert relerr(got[1][2], make_oracle(dict(kw, normalization=True)).K(Y, X)) <= TOL


@pytest.mark.parametrize("shape", [dict(N=37, L=50, d=6, M=4, c=50, r=50, sp="sqrt"),      # BASELINE configs[2]'s sequences, default ranks
                                   dict(N=9, L=131, d=2, M=3, c=20, r=33, sp="log"),       # three time chunks of 64, r > c
                                   dict(N=5, L=7, d=3, M=5, c=4, r=3, sp="lin", lags=2),   # d_eff = 9 > max(c, r): the staging rows; lags
                                   dict(N=6, L=2, d=2, M=2, c=3, r=2, sp="sqrt"),          # one increment
                                   dict(N=4, L=20, d=3, M=1, c=8, r=8, sp="sqrt")])        # level 1 only: no sketch
@pytest.mark.parametrize("base", ["rbf", "linear", "matern32"])
def test_low_rank_fused_feature_kernel(K, shape, base):
    """gpsig_lr_seq_features through the fused kernel (lr_fused_kernel.hpp: a workgroup per sequence, intermediates in LDS)
    against the one-kernel-per-op path it replaces (same random objects: differences are summation order in the whitening
    product only) and, through K / Kdiag, against the oracle's restatement of signature_algs.py:166-193."""
    import ctypes as C
    from gpsig_amd import _lib
    rng = np.random.default_rng(77)
    N, L, d, M, c, r = (shape[k] for k in ("N", "L", "d", "M", "c", "r"))
    lags = shape.get("lags")
    X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    for difference in (True, False):
        if not difference and L == 2:
            continue
        kw = dict(normalization=False, num_components=c, rank_bound=r, sparsity=shape["sp"], lengthscales=0.6 + rng.random(d),
                  difference=difference)
        if lags:
            kw["num_lags"] = lags
        kx, ko = _lr_pair(K, base, L, d, M, **kw)
        kx.rng = np.random.default_rng(5)
        st = kx.draw_low_rank(X=X)
        ctx = _lib.context(0, 0)
        ctx.set_pointer_mode(_lib.PTR_HOST)
        keep = []
        p, lr = kx._params(keep), st.as_c(keep)
        F = 1 + c + (M - 1) * r
        out = {}
        try:
            for fused in (1, 0):
                ctx.set_option("lr_fused", fused)
                Phi = np.full((N, F), np.nan)
                ctx.call("gpsig_lr_seq_features", p, lr, X.ctypes.data_as(C.c_void_p), N, L, Phi.ctypes.data_as(C.c_void_p))
                out[fused] = Phi
        finally:
            ctx.set_option("lr_fused", 1)
        assert np.isfinite(out[1]).all() and (out[1][:, 0] == 1.0).all()
        scale = np.abs(out[0]).max(axis=0, keepdims=True) + 1e-300          # per feature column
        assert (np.abs(out[1] - out[0]) / scale).max() <= 1e-9, (difference, (np.abs(out[1] - out[0]) / scale).max())
        lo = O.LowRankOracle(ko, st.landmarks, st.jitter_diag, st.sketches)
        tol = 1e-5 if base == "linear" else 1e-7                             # comment above LR_TOLS
        want = lo.K(X)
        assert np.abs(kx.K(X, lr_state=st) - want).max() <= tol * np.abs(want).max(), difference


@pytest.mark.parametrize("base", ["rbf", "linear", "matern12"])
def test_low_rank_fused_tensor_features(K, base):
    """gpsig_lr_tens_features through the one-workgroup-per-tensor kernel (lr_tens_features_fused_kernel) against the
    one-kernel-per-op path (same random objects) and, through K_tens, against the oracle's tensor_kern_lr_feature restatement."""
    import ctypes as C
    from gpsig_amd import _lib
    rng = np.random.default_rng(79)
    for T, d, M, c, r, sp, lags in ((37, 6, 4, 50, 50, "sqrt", 0), (5, 2, 5, 9, 13, "log", 0), (130, 3, 3, 12, 7, "lin", 1), (3, 2, 1, 4, 4, "sqrt", 0)):
        kw = dict(normalization=False, num_components=c, rank_bound=r, sparsity=sp, lengthscales=0.6 + rng.random(d))
        if lags:
            kw["num_lags"] = lags
        kx, ko = _lr_pair(K, base, 8, d, M, **kw)
        kx.rng = np.random.default_rng(6)
        de = d * (lags + 1)
        lt = M * (M + 1) // 2
        for incr in (False, True):
            Z = rng.standard_normal((lt, T, 2, de) if incr else (lt, T, de))
            X = np.cumsum(0.3 * rng.standard_normal((max(c, 8), 8, d)), axis=1).reshape(max(c, 8), -1)     # enough points for the landmarks
            st = kx.draw_low_rank(X=X, Z=Z, increments=incr)
            ctx = _lib.context(0, 0)
            ctx.set_pointer_mode(_lib.PTR_HOST)
            keep = []
            p, lr = kx._params(keep), st.as_c(keep)
            F = 1 + c + (M - 1) * r
            out = {}
            Zc = np.ascontiguousarray(Z)
            try:
                for fused in (1, 0):
                    ctx.set_option("lr_fused", fused)
                    Phi = np.full((T, F), np.nan)
                    ctx.call("gpsig_lr_tens_features", p, lr, Zc.ctypes.data_as(C.c_void_p), T, int(incr), Phi.ctypes.data_as(C.c_void_p))
                    out[fused] = Phi
            finally:
                ctx.set_option("lr_fused", 1)
            assert np.isfinite(out[1]).all() and (out[1][:, 0] == 1.0).all()
            scale = np.abs(out[0]).max(axis=0, keepdims=True) + 1e-300
            assert (np.abs(out[1] - out[0]) / scale).max() <= 1e-9, (T, incr)
            lo = O.LowRankOracle(ko, st.landmarks, st.jitter_diag, st.sketches)
            want = lo.K_tens(Z, increments=incr)
            # (1e-7 for RBF; the linear kernel's rank-deficient and Matern-1/2's non-smooth landmark Grams: comment above LR_TOLS)
            assert np.abs(kx.K_tens(Z, increments=incr, lr_state=st) - want).max() <= (1e-7 if base == "rbf" else 1e-5) * np.abs(want).max()


def test_low_rank_gram_products_in_lds_tiles(K):
    """The low-rank Gram products (Phi_a Phi_b^T per level, or summed) through the 128 x 128-tile MFMA kernel with k-slabs staged
    in LDS against the round-1 kernel (fragments straight from L2) and the oracle: ragged sizes across tile boundaries, feature
    widths that are no multiple of the 16-column slab, levels and sums, symmetric and cross."""
    from gpsig_amd import _lib
    rng = np.random.default_rng(57)
    L, d, M = 6, 2, 3
    X = np.cumsum(0.3 * rng.standard_normal((261, L, d)), axis=1).reshape(261, -1)
    Y = np.cumsum(0.3 * rng.standard_normal((130, L, d)), axis=1).reshape(130, -1)
    for c_, r_ in ((11, 9), (16, 16), (37, 21)):
        kx, ko = _lr_pair(K, "rbf", L, d, M, normalization=True, num_components=c_, rank_bound=r_, sparsity="sqrt",
                          lengthscales=0.6 + rng.random(d), variances=0.5 + rng.random(M + 1))
        kx.rng = np.random.default_rng(9)
        st = kx.draw_low_rank(X=X, X2=Y)
        ctx = _lib.context(0, 0)
        got = {}
        try:
            for tiled in (1, 0):
                ctx.set_option("lr_gemm", tiled)
                got[tiled] = (kx.K(X, lr_state=st), kx.K(X, Y, lr_state=st, return_levels=True), kx.K(Y, X, lr_state=st))
        finally:
            ctx.set_option("lr_gemm", 1)
        for a, b in zip(got[1], got[0]):
            assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()
        # against the oracle on the scale of the whole array: up to 37 landmarks in a 2-dimensional state space make a landmark
        # Gram whose small eigenvalues sit at the jitter, where rocSOLVER and LAPACK eigenvectors differ (comment above LR_TOLS)
        lo = O.LowRankOracle(ko, st.landmarks, st.jitter_diag, st.sketches)
        for g, w in ((got[1][0], lo.K(X)), (got[1][1], lo.K(X, Y, return_levels=True))):
            assert np.abs(g - w).max() <= 1e-4 * np.abs(w).max()


def test_low_rank_golden_fixtures(K, golden_lowrank):
    """The committed low-rank fixtures (tests/golden/lowrank.npz: inputs, random objects, oracle outputs) through the C ABI: the
    whitening is computed on the device from the committed landmarks and jitter draw (kern.low_rank_state), the features by the
    fused kernels, the products on the matrix cores."""
    cases, arr, sketches = golden_lowrank
    for c in cases:
        n = c["name"]
        kern = make_kernel(K, dict(c["kern"], low_rank=True, num_components=c["num_components"], rank_bound=c["rank_bound"], sparsity=c["sparsity"]))
        st = kern.low_rank_state(arr[f"{n}/landmarks"], arr[f"{n}/jitter_diag"], sketches(n, c["kern"]["num_levels"]))
        X, X2, Z, incr = arr[f"{n}/X"], arr[f"{n}/X2"], arr[f"{n}/Z"], c["increments"]
        got = dict(K=kern.K(X, lr_state=st), Kx=kern.K(X, X2, return_levels=True, lr_state=st),
                   Kzx=kern.K_tens_vs_seq(Z, X, increments=incr, lr_state=st), Kzz=kern.K_tens(Z, increments=incr, lr_state=st))
        if "Kdiag" in c["outputs"]:
            got["Kdiag"] = kern.Kdiag(X, lr_state=st)
        tol = 1e-7 if c["kern"]["base"] == "rbf" else 1e-5         # comment above LR_TOLS
        for k in c["outputs"]:
            want = arr[f"{n}/out/{k}"]
            assert np.abs(np.asarray(got[k]) - want).max() <= tol * np.abs(want).max(), (n, k, np.abs(np.asarray(got[k]) - want).max() / np.abs(want).max())


def test_low_rank_fresh_draw_on_device_tensors(K):
    """Low-rank evaluations of CUDA tensors WITHOUT lr_state: the draw (landmark gather, whitening) happens half way through a sequence
    of device-pointer calls on the tensors' own context and must leave its pointer mode alone (round-2 advisor finding: the whitening
    used to switch the shared context to host pointers).  Same generator state -> the same matrices as with the draw made up front,
    and as the host-array evaluation."""
    import torch
    rng = np.random.default_rng(77)
    N, N2, L, d, M, T = 20, 7, 9, 3, 3, 6
    X = np.cumsum(0.4 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    X2 = np.cumsum(0.4 * rng.standard_normal((N2, L, d)), axis=1).reshape(N2, -1)
    Z = rng.standard_normal((M * (M + 1) // 2, T, d))
    dev = torch.device("cuda:0")
    Xc, X2c, Zc = (torch.tensor(a, device=dev) for a in (X, X2, Z))
    kern = K.SignatureRBF(L * d, d, M, low_rank=True, num_components=14, rank_bound=9, lengthscales=1.2)
    for call in (lambda k_, st: k_.K(Xc, lr_state=st), lambda k_, st: k_.K(Xc, X2c, lr_state=st), lambda k_, st: k_.Kdiag(Xc, lr_state=st),
                 lambda k_, st: k_.K_tens_vs_seq(Zc, Xc, lr_state=st), lambda k_, st: k_.K_tens(Zc, lr_state=st)):
        kern.rng = np.random.default_rng(5)
        fresh = call(kern, None)
        assert fresh.is_cuda and bool(torch.isfinite(fresh).all())
    # the same draw made up front, on device tensors and on host arrays
    kern.rng = np.random.default_rng(5)
    fresh = kern.K(Xc, X2c)
    kern.rng = np.random.default_rng(5)
    st = kern.draw_low_rank(X=Xc, X2=X2c)
    assert torch.equal(fresh, kern.K(Xc, X2c, lr_state=st))
    np.testing.assert_allclose(fresh.cpu().numpy(), kern.K(X, X2, lr_state=st.export()), rtol=0, atol=1e-12 * float(fresh.abs().max()))
    # the host-side draw on the same tensors still works (kern.device_draw = False) and goes through the same contexts
    kern.device_draw = False
    kern.rng = np.random.default_rng(5)
    sth = kern.draw_low_rank(X=Xc, X2=X2c)
    assert bool(torch.isfinite(kern.K(Xc, X2c, lr_state=sth)).all())
    kern.device_draw = True
    kern.rng = np.random.default_rng(5)
    Kzz, Kzx, Kxx = kern.K_tens_n_seq_covs(Zc, Xc)
    assert Kzz.is_cuda and Kzx.shape == (T, N) and bool(torch.isfinite(Kzx).all())


def test_low_rank_states_handed_out_belong_to_the_caller(K):
    """Round-3 advisor finding: for CUDA inputs draw_low_rank() used to hand out the kernel object's ONE cached device state, which
    every later draw -- explicit or the implicit draw of an evaluation without lr_state -- overwrote.  A state the caller holds now
    stays what it was: evaluations from it are reproducible across other draws and evaluations, as with host arrays; only the
    implicit per-evaluation draws share a block.  And a state that outlives its context is released without touching the context."""
    import torch
    from gpsig_amd import _lib
    rng = np.random.default_rng(3)
    N, L, d, M, T = 18, 8, 3, 3, 5
    dev = torch.device("cuda:0")
    Xc = torch.tensor(np.cumsum(0.4 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1), device=dev)
    Yc = torch.tensor(np.cumsum(0.4 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1), device=dev)
    Zc = torch.tensor(rng.standard_normal((M * (M + 1) // 2, T, d)), device=dev)
    kern = K.SignatureRBF(L * d, d, M, low_rank=True, num_components=12, rank_bound=8)
    kern.rng = np.random.default_rng(11)
    st1 = kern.draw_low_rank(X=Xc)
    ref1 = kern.K(Xc, lr_state=st1).clone()
    landmarks1 = st1.export().landmarks.copy()
    st2 = kern.draw_low_rank(X=Yc)                      # another explicit draw, from other sequences
    assert st2 is not st1 and st2._h.value != st1._h.value
    kern.K(Yc); kern.Kdiag(Yc); kern.K_tens_vs_seq(Zc, Yc); kern.K_tens(Zc)      # implicit draws: the kernel object's own block
    assert kern._device_lr_state is not st1 and kern._device_lr_state is not st2
    np.testing.assert_array_equal(st1.export().landmarks, landmarks1)
    assert torch.equal(kern.K(Xc, lr_state=st1), ref1)
    assert not torch.equal(kern.K(Xc, lr_state=st2), ref1)
    # implicit draws reuse one block (no allocation per evaluation)
    h = kern._device_lr_state._h.value
    kern.K(Xc)
    assert kern._device_lr_state._h.value == h
    # a state outliving its context: the context detaches it; destroying it afterwards only frees the block
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        k2 = K.SignatureRBF(L * d, d, M, low_rank=True, num_components=12, rank_bound=8)
        k2.rng = np.random.default_rng(12)
        st3 = k2.draw_low_rank(X=Xc)
        v = k2.K(Xc, lr_state=st3)
        side.synchronize()
        assert bool(torch.isfinite(v).all())
    _lib.release(0, side.cuda_stream)                   # closes the side stream's context
    with pytest.raises(RuntimeError):
        st3.export()
    st3.close()                                         # no use-after-free: a detached state frees its memory only
    del st3, k2
    torch.cuda.synchronize()
    assert bool(torch.isfinite(kern.K(Xc)).all())


def test_decomposed_gram_through_rccl_on_one_rank(K):
    """Every collective of the N-rank path executed by RCCL itself (backend "nccl" on ROCm), on the one GPU a test box has: a
    one-rank process group and ShardedGram(force=True) -- row-block calls in chunks, the all-reduced verdict, an asynchronous
    dist.gather per chunk on the collective's own stream while the next chunk is computed, the stream-ordered wait, the tiled
    symmetrisation.  Bit-identical to K(X) for both routes (feature contraction: SignatureLinear; pair recursion: SignatureRBF), and
    a refused shape takes the rank-0 fallback through the same all-reduce."""
    import socket
    import torch
    import torch.distributed as dist
    from gpsig_amd import parallel
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        rng = np.random.default_rng(21)
        dev = torch.device("cuda:0")
        for cls, n, L, d, M in ((K.SignatureLinear, 1024, 32, 4, 4), (K.SignatureRBF, 520, 16, 3, 3)):
            X = torch.as_tensor(rng.standard_normal((n, L * d)), device=dev)
            kern = cls(L * d, d, M)
            want = kern.K(X)
            g = parallel.ShardedGram(kern, n, dev, 0, 1, chunks=4, force=True)
            for _ in range(2):                       # a second call reuses rows / half / out behind the first one's waits
                got = g(X)
                torch.cuda.synchronize()
                assert g.fallback is None
                assert torch.equal(got, want)
        # a shape the row-block kernels refuse: the verdict goes through RCCL's all-reduce, rank 0 evaluates alone
        n, L, d, M = 40, 700, 3, 3
        X = torch.as_tensor(0.1 * rng.standard_normal((n, L * d)), device=dev)
        kern = K.SignatureRBF(L * d, d, M)
        g = parallel.ShardedGram(kern, n, dev, 0, 1, chunks=2, force=True)
        got = g(X)
        assert g.fallback is not None
        assert torch.equal(got, kern.K(X))
    finally:
        dist.destroy_process_group()


def test_failure_votes_and_sharded_covariances_through_rccl_on_one_rank(K):
    """Round 6: what a multi-GPU run does when something goes wrong, and the SVGP covariances' sequence split, executed by
    RCCL itself on a one-rank group: (a) a row-block call that FAILS on the first chunk -- the MIN all-reduce of the verdict, the fallback's barrier,
    the error raised after them; (b) a failure on a LATER chunk -- the rank keeps joining the asynchronous gathers, the closing vote, the error;
    (c) ShardedCovs(force=True): Kzx / Kxx-diag blocks gathered by dist.gather on the nccl backend, equal to the direct evaluation."""
    import socket
    import torch
    import torch.distributed as dist
    from gpsig_amd import _lib, parallel
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=torch.device("cuda:0"))
    try:
        rng = np.random.default_rng(33)
        dev = torch.device("cuda:0")

        class FailingContext:
            """the library's context, failing for good from the k-th row-block call on"""
            def __init__(self, fail_from):
                self.inner = _lib.context(0, torch.cuda.current_stream(dev).cuda_stream)
                self.inner.set_pointer_mode(_lib.PTR_DEVICE)
                self.fail_from, self.calls = fail_from, 0

            def call(self, name, *a):
                self.calls += 1
                if self.calls >= self.fail_from:
                    raise MemoryError("libgpsig_hip: out of device memory")
                return self.inner.call(name, *a)

            def __getattr__(self, k):
                return getattr(self.inner, k)
        n, L, d, M = 520, 16, 3, 3
        X = torch.as_tensor(rng.standard_normal((n, L * d)), device=dev)
        kern = K.SignatureRBF(L * d, d, M)
        for fail_from in (1, 3):
            g = parallel.ShardedGram(kern, n, dev, 0, 1, chunks=4, force=True, ctx=FailingContext(fail_from))
            with pytest.raises(MemoryError, match="out of device memory"):
                g(X)
            torch.cuda.synchronize()
        g = parallel.ShardedGram(kern, n, dev, 0, 1, chunks=4, force=True)              # and the group still works afterwards
        assert torch.equal(g(X), kern.K(X))
        T = 40
        for increments in (False, True):
            Z = torch.as_tensor(rng.standard_normal((M * (M + 1) // 2, T, 2, d) if increments else (M * (M + 1) // 2, T, d)), device=dev)
            covs = parallel.ShardedCovs(kern, n, dev, 0, 1, force=True)
            got = covs(Z, X, increments=increments)
            want = kern.K_tens_n_seq_covs(Z, X, increments=increments)
            torch.cuda.synchronize()
            for a, b in zip(got, want):
                assert torch.equal(a, b)
    finally:
        dist.destroy_process_group()


def test_empty_row_block_takes_the_routes_a_block_with_rows_takes(K):
    """Round-3 advisor finding: a rank that owns no rows used to validate the shape with the pair kernels' planner only, while ranks
    with rows ask the feature contraction first -- which takes shapes the pair kernels refuse (SignatureLinear with more than 512
    lattice rows at d <= 8; orders beyond the higher-order tables).  The empty block now gives the same verdict as its peers:
    accepted where a block with rows is accepted, refused where it is refused."""
    import ctypes as C
    import torch
    from gpsig_amd import _lib
    rng = np.random.default_rng(8)
    ctx = _lib.context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_pointer_mode(_lib.PTR_DEVICE)
    n, L, d, M = 64, 600, 4, 3                          # 599 lattice rows: beyond the pair kernels' register-resident side
    X = torch.as_tensor(0.1 * rng.standard_normal((n, L * d)), device="cuda:0")
    W = n // 2 + 1
    out = torch.full((8, W), float("nan"), dtype=torch.float64, device="cuda:0")
    for kern, accepted in ((K.SignatureLinear(L * d, d, M), True), (K.SignatureRBF(L * d, d, M), False)):
        keep = []
        p = kern._params(keep)
        verdicts = []
        for r0, r1 in ((8, 16), (n, n), (0, 0)):        # a block with rows, an empty block at the end, an empty block at the start
            try:
                ctx.call("gpsig_kernel_K_symm_rows_compact", p, C.c_void_p(X.data_ptr()), n, L, r0, r1, C.c_void_p(out.data_ptr()))
                verdicts.append(True)
            except NotImplementedError:
                verdicts.append(False)
        assert verdicts == [accepted] * 3, (type(kern).__name__, verdicts)
    torch.cuda.synchronize()
    # and what the accepted block computed is the Gram's owned entries
    kern = K.SignatureLinear(L * d, d, M)
    keep = []
    ctx.call("gpsig_kernel_K_symm_rows_compact", kern._params(keep), C.c_void_p(X.data_ptr()), n, L, 8, 16, C.c_void_p(out.data_ptr()))
    full = kern.K(X)
    j = torch.arange(W, device="cuda:0")
    for i in range(8):
        cols = (8 + i - n // 2 + j) % n
        own = torch.isfinite(out[i])
        assert int(own.sum()) >= W - 1
        assert torch.allclose(out[i][own], full[8 + i][cols][own], rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize("sparsity", ["sqrt", "log", "lin"])
@pytest.mark.parametrize("base", ["rbf", "linear"])
def test_low_rank_objects_drawn_on_the_device(K, sparsity, base):
    """gpsig_lr_draw (round 3): landmarks, jitter diagonal, whitening (one-workgroup Jacobi eigendecomposition) and the projections of
    every level drawn on the device with a counter-based generator.  (i) what was drawn is well formed and a function of the seed;
    (ii) exported to the host, the oracle -- which whitens the same landmarks itself with NumPy's eigh and applies the same
    projections -- reproduces every covariance of the device evaluation; (iii) the Jacobi whitening equals rocSOLVER's."""
    import torch
    from gpsig_amd import _lib
    rng = np.random.default_rng(141)
    LR_TOL = LR_TOLS[base]
    N, N2, L, d, M, T = 23, 9, 12, 3, 4, 7
    c, r = 11, 9
    X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    Y = np.cumsum(0.3 * rng.standard_normal((N2, L, d)), axis=1).reshape(N2, -1)
    dev = torch.device("cuda:0")
    Xc, Yc = torch.tensor(X, device=dev), torch.tensor(Y, device=dev)

    def rel(got, want):
        got, want = np.asarray(got.cpu() if torch.is_tensor(got) else got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert got.shape == want.shape and np.isfinite(got).all()
        return float(np.abs(got - want).max() / np.abs(want).max())
    for incr in (False, True):
        Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d) if incr else (M * (M + 1) // 2, T, d))
        Zc = torch.tensor(Z, device=dev)
        kx, ko = _lr_pair(K, base, L, d, M, normalization=True, num_components=c, rank_bound=r, sparsity=sparsity,
                          lengthscales=0.6 + rng.random(d), variances=0.5 + rng.random(M + 1))
        kx.rng = np.random.default_rng(7)
        st = kx.draw_low_rank(X=Xc, X2=Yc, Z=Zc, increments=incr)
        assert isinstance(st, K.DeviceLowRankState)
        h = st.export()
        # (i) well formed: c distinct candidates in ascending order (so every landmark is a scaled point of Z, X or Y, in that order), a
        # jitter draw inside (0, 1e-6), projections stored by column with rows ascending inside a column
        ztot = Z.reshape(-1, d).shape[0]
        cand = np.concatenate([Z.reshape(-1, d) / kx.lengthscales, X.reshape(-1, d) / kx.lengthscales, Y.reshape(-1, d) / kx.lengthscales])
        where = [int(np.argmin(np.abs(cand - row).sum(1))) for row in h.landmarks]
        assert all(np.abs(cand[w] - row).max() < 1e-12 for w, row in zip(where, h.landmarks)) and ztot > 0
        assert where == sorted(where) and len(set(where)) == c
        assert (h.jitter_diag > 0).all() and (h.jitter_diag < 1e-6).all()
        k2 = c
        for sk in h.sketches:
            assert (sk.k1, sk.k2, sk.r) == (c, k2, r) and sk.colptr[0] == 0 and (np.diff(sk.colptr) >= 0).all() and sk.colptr[-1] == len(sk.val)
            assert (sk.i1 >= 0).all() and (sk.i1 < c).all() and (sk.i2 >= 0).all() and (sk.i2 < k2).all()
            if sparsity == "lin":
                assert len(sk.val) == r and set(np.abs(sk.val)) == {1.0} and len(set(zip(sk.i1, sk.i2))) == r
            else:
                for j in range(r):
                    rows = (sk.i1 + c * sk.i2)[sk.colptr[j]:sk.colptr[j + 1]]
                    assert (np.diff(rows) > 0).all()
            k2 = r
        # ... a function of the seed
        kx.rng = np.random.default_rng(7)
        h2 = kx.draw_low_rank(X=Xc, X2=Yc, Z=Zc, increments=incr).export()
        assert np.array_equal(h.landmarks, h2.landmarks) and np.array_equal(h.whitening, h2.whitening)
        assert all(np.array_equal(a.val, b.val) and np.array_equal(a.i1, b.i1) for a, b in zip(h.sketches, h2.sketches))
        kx.rng = np.random.default_rng(8)
        h3 = kx.draw_low_rank(X=Xc, X2=Yc, Z=Zc, increments=incr).export()
        assert not np.array_equal(h.landmarks, h3.landmarks)
        # (ii) the restatement on the exported objects against the device evaluation on the device-resident ones
        kx.rng = np.random.default_rng(7)
        st = kx.draw_low_rank(X=Xc, X2=Yc, Z=Zc, increments=incr)
        h = st.export()
        lo = O.LowRankOracle(ko, h.landmarks, h.jitter_diag, h.sketches)
        inv_p, inv_o = h.whitening @ h.whitening.T, lo.Wh @ lo.Wh.T
        assert np.abs(inv_p - inv_o).max() <= 1e-7 * np.abs(inv_o).max()
        assert rel(kx.K(Xc, lr_state=st), lo.K(X)) <= LR_TOL
        assert rel(kx.K(Xc, Yc, lr_state=st, return_levels=True), lo.K(X, Y, return_levels=True)) <= LR_TOL
        assert rel(kx.K_tens(Zc, increments=incr, lr_state=st), lo.K_tens(Z, increments=incr)) <= LR_TOL
        assert rel(kx.K_tens_vs_seq(Zc, Xc, increments=incr, lr_state=st, return_levels=True), lo.K_tens_vs_seq(Z, X, increments=incr, return_levels=True)) <= LR_TOL
        assert rel(kx.Kdiag(Xc, lr_state=st), lo.Kdiag(X)) <= LR_TOL
        # the unfused per-op feature path reads the same state (its transposed whitening)
        ctx = _lib.context(0, torch.cuda.current_stream(dev).cuda_stream)
        ctx.set_option("lr_fused", 0)
        try:
            assert rel(kx.K(Xc, Yc, lr_state=st), lo.K(X, Y)) <= LR_TOL
        finally:
            ctx.set_option("lr_fused", 1)
        # (iii) rocSOLVER instead of the Jacobi kernel: the same (W + jitter)^-1
        ctx.set_option("lr_jacobi", 0)
        try:
            kx.rng = np.random.default_rng(7)
            hs = kx.draw_low_rank(X=Xc, X2=Yc, Z=Zc, increments=incr).export()
        finally:
            ctx.set_option("lr_jacobi", 1)
        assert np.array_equal(hs.landmarks, h.landmarks)
        assert np.abs(hs.whitening @ hs.whitening.T - inv_p).max() <= 1e-7 * np.abs(inv_p).max()
        assert np.abs(hs.eigenvalues - h.eigenvalues).max() <= 1e-12 * np.abs(h.eigenvalues).max()


def test_device_drawn_projections_are_unbiased(K):
    """Statistics of the device generator: the number of entries of a 'sqrt' projection follows Binomial(D r, 1/s), its values are
    N(0, s/r), and the sketched product is unbiased -- E[<P(a (x) b), P(a' (x) b')>] = <a, a'><b, b'> -- with an error that shrinks as
    the rank bound grows (low_rank_calculations.py:152-193)."""
    import torch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    L, d, M, c = 10, 2, 2, 24
    X = torch.tensor(np.cumsum(0.3 * rng.standard_normal((40, L, d)), axis=1).reshape(40, -1), device=dev)
    a, b, a2, b2 = (rng.standard_normal(c) for _ in range(4))
    exact = (a @ a2) * (b @ b2)
    errs = {}
    for r in (8, 64):
        kx = K.SignatureRBF(L * d, d, M, low_rank=True, num_components=c, rank_bound=r, sparsity="sqrt")
        est, counts, vals = [], [], []
        for seed in range(200):
            kx.rng = np.random.default_rng(seed)
            sk = kx.draw_low_rank(X=X).export().sketches[0]
            est.append(float(sk.apply(a, b) @ sk.apply(a2, b2)))
            counts.append(len(sk.val))
            vals.append(sk.val)
        D, s = c * c, float(c)
        mean_n, sd_n = D * r / s, np.sqrt(D * r / s * (1 - 1 / s))
        assert abs(np.mean(counts) - mean_n) < 5 * sd_n / np.sqrt(len(counts))
        v = np.concatenate(vals) / np.sqrt(s / r)
        assert abs(v.mean()) < 5 / np.sqrt(len(v)) and abs(v.var() - 1.0) < 0.1 and abs((np.abs(v) < 1).mean() - 0.6827) < 0.03
        errs[r] = float(np.std(est))
        assert abs(np.mean(est) - exact) < 5 * errs[r] / np.sqrt(len(est)) + 1e-12
    assert errs[64] < 0.6 * errs[8]


def test_low_rank_exact_limit_and_convergence(K):
    rng = np.random.default_rng(43)
    N, L, d = 8, 5, 2
    X = np.cumsum(0.5 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    # every point a landmark + every coordinate pair kept ('lin', rank_bound = c^2 at level 2): the exact kernel
    c = N * L
    kx, ko = _lr_pair(K, "rbf", L, d, 2, normalization=False, num_components=c, rank_bound=c * c, sparsity="lin", lengthscales=None)
    kx.rng = np.random.default_rng(1)
    exact = ko.K(X)
    assert np.abs(kx.K(X) - exact).max() <= 1e-4 * np.abs(exact).max()      # only the Nystrom jitter (1e-6) separates them
    # statistically: mean error over draws shrinks as the rank grows
    N, L, d, M = 30, 10, 2, 3
    X = np.cumsum(0.4 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    ko = make_oracle(dict(input_dim=L * d, num_features=d, num_levels=M, base="rbf"))
    exact = ko.K(X)
    errs = []
    for c_, r_ in ((10, 10), (40, 40), (120, 160)):
        kx = make_kernel(K, dict(input_dim=L * d, num_features=d, num_levels=M, base="rbf", low_rank=True, num_components=c_,
                                 rank_bound=r_, sparsity="sqrt"))
        kx.rng = np.random.default_rng(3)
        errs.append(np.mean([np.linalg.norm(kx.K(X) - exact) / np.linalg.norm(exact) for _ in range(6)]))
    assert errs[0] > errs[1] > errs[2] and errs[2] < 0.5 * errs[0], errs


def test_low_rank_validation(K):
    with pytest.raises(NotImplementedError):
        K.SignatureRBF(12, 3, 3, low_rank=True, order=2)                  # kernels.py:59-60
    kx = K.SignatureRBF(12, 3, 3, low_rank=True, num_components=1000)
    with pytest.raises(ValueError, match="num_components"):
        kx.K(np.zeros((2, 12)))
    # the three SVGP matrices share one draw
    rng = np.random.default_rng(5)
    kx = K.SignatureRBF(12, 3, 3, low_rank=True, num_components=8, rank_bound=8)
    Z, X = rng.standard_normal((6, 4, 3)), rng.standard_normal((10, 12))
    Kzz, Kzx, Kxx = kx.K_tens_n_seq_covs(Z, X)
    assert Kzz.shape == (4, 4) and Kzx.shape == (4, 10) and Kxx.shape == (10,)
    # float32 arguments never reach the float64-only low-rank entry points as float32 buffers: every branch is computed in
    # float64 and rounded (all-float32 arguments) or converted on the way in (mixed), and agrees with the float64 call
    Z32, X32 = Z.astype(np.float32), X.astype(np.float32)
    kx.normalization = False
    st = kx.draw_low_rank(X=X32.astype(np.float64), Z=Z32.astype(np.float64))
    for got, want in ((kx.K_tens(Z32, lr_state=st), kx.K_tens(Z32.astype(np.float64), lr_state=st)),
                      (kx.Kdiag(X32, lr_state=st), kx.Kdiag(X32.astype(np.float64), lr_state=st)),
                      (kx.K_tens_vs_seq(Z32, X32, lr_state=st), kx.K_tens_vs_seq(Z32.astype(np.float64), X32.astype(np.float64), lr_state=st)),
                      (kx.K_tens_vs_seq(Z32, X, lr_state=st), kx.K_tens_vs_seq(Z32.astype(np.float64), X, lr_state=st))):
        assert np.isfinite(got).all() and np.abs(np.asarray(got, dtype=np.float64) - want).max() <= 1e-5 * np.abs(want).max()
    Kzz, Kzx, Kxx = kx.K_tens_n_seq_covs(Z32, X)
    assert Kzz.shape == (4, 4) and np.isfinite(Kzz).all() and np.isfinite(Kzx).all() and np.isfinite(Kxx).all()


# ------------------------------------------------------------------------------------------------
# SVGP prediction (gpsig/models.py:62-73): Kuu_Kuf_Kff on the HIP kernels + base_conditional / gauss_kl on
# rocSOLVER / rocBLAS through torch.linalg, against the NumPy/SciPy restatement fed with the oracle's covariances.
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("whiten", [True, False])
@pytest.mark.parametrize("q_diag", [False, True])
def test_svgp_predict_and_kl(K, whiten, q_diag):
    from gpsig_amd import inducing_variables as IV, models
    from oracle import svgp_oracle as SO
    rng = np.random.default_rng(60 + whiten + 2 * q_diag)
    N, L, d, M, T, R = 21, 14, 3, 3, 9, 2
    X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    kw = dict(input_dim=L * d, num_features=d, num_levels=M, base="rbf", lengthscales=0.7 + rng.random(d))
    kx, ko = make_kernel(K, kw), make_oracle(kw)
    q_mu = rng.standard_normal((T, R))
    q_sqrt = 0.5 + rng.random((T, R)) if q_diag else np.tril(0.3 * rng.standard_normal((R, T, T))) + np.eye(T)[None]
    for kind in ("tensors", "sequences"):
        if kind == "tensors":
            Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d))
            feat = IV.InducingTensors(Z, M, increments=True)
            cov = lambda full: O.inducing_tensors_Kuu_Kuf_Kff(ko, Z, X, increments=True, jitter=1e-6, full_f_cov=full)  # noqa: E731
            kzz = O.inducing_tensors_Kuu(ko, Z, increments=True, jitter=1e-6)
        else:
            Zs = np.cumsum(0.3 * rng.standard_normal((T, 8, d)), axis=1)
            feat = IV.InducingSequences(Zs, M)
            cov = lambda full: O.inducing_sequences_Kuu_Kuf_Kff(ko, Zs, X, jitter=1e-6, full_f_cov=full)  # noqa: E731
            kzz = O.inducing_sequences_Kuu(ko, Zs, jitter=1e-6)
        m = models.SVGP(kx, feat, q_diag=q_diag, whiten=whiten, q_mu=q_mu, q_sqrt=q_sqrt)
        for full in (False, True):
            if kind == "sequences" and full:
                continue        # kernels.py:723-728 is broken in the reference; covered by the golden fixtures' evident-intent case
            Kzz, Kzx, Kxx = cov(full)
            want_mean, want_var = SO.base_conditional(Kzx, Kzz, Kxx, q_mu, full_cov=full, q_sqrt=q_sqrt, white=whiten)
            mean, var = m.predict_f(X, full_cov=full)
            assert relerr(mean.cpu().numpy(), want_mean) <= 1e-6 and relerr(var.cpu().numpy(), want_var) <= 1e-6, (kind, full)
        want_kl = SO.gauss_kl(q_mu, q_sqrt, K=None if whiten else kzz)
        assert abs(float(m.prior_kl()) - want_kl) <= 1e-8 * abs(want_kl), kind


def test_feature_contraction_gives_way_on_a_full_device(K):
    """The contraction needs the feature matrix and its partial sums in scratch memory; where the device cannot hold them the
    evaluation goes through the pair recursion (which needs neither) instead of failing with an allocation error."""
    import torch
    from gpsig_amd import _lib
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(77)
    N, L, d, M = 2048, 64, 8, 5                                  # 0.6 GB of features + 1.1 GB of partial sums
    X = torch.as_tensor(rng.standard_normal((N, L * d)), device=dev)
    kern = K.SignatureLinear(L * d, d, M)
    want = kern.K(X)                                             # the contraction, on the default stream's context
    import gc
    hog = []
    for _ in range(4):                                           # leave 0.9 GB (objects of earlier tests may still give memory back: collect first, re-measure)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(dev)
        if free <= 0.95e9:
            break
        hog.append(torch.empty(int(free - 0.9e9), dtype=torch.uint8, device=dev))
    side = torch.cuda.Stream(dev)                                # a stream of its own: a context without scratch buffers yet
    _lib.release(0, side.cuda_stream)                            # (torch hands out side streams from a pool: drop what an earlier test left on it)
    side.wait_stream(torch.cuda.current_stream(dev))
    try:
        with torch.cuda.stream(side):
            got = kern.K(X)
        side.synchronize()
    finally:
        del hog
        _lib.release(0, side.cuda_stream)
        torch.cuda.empty_cache()
    assert not torch.equal(got, want)                            # the pair recursion ran (other last digits) ...
    assert float((got - want).abs().max()) <= 1e-11 * float(want.abs().max())      # ... and agrees


# ------------------------------------------------------------------------------------------------
# (e) the cases round 4's randomised sweeps reported above tolerance (profiles/r04_fuzz.txt), as fixtures with their adjudication
#     (tests/golden/make_fuzz_cases.py)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fuzz_cases():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_cases.npz"))


def _fuzz_kernel(K, fz, key):
    M, order, d, lags, L1, L2, norm, diff, f32, incr, T = (int(v) for v in fz[key + "_meta"])
    base = str(fz[key + "_base"])
    kw = dict(input_dim=L1 * d, num_features=d, num_levels=M, base=base, order=order, normalization=bool(norm), difference=bool(diff),
              num_lags=lags or None, lengthscales=fz[key + "_ls"], variances=fz[key + "_var"])
    if base == "poly":
        kw["base_params"] = {"gamma": 1.0, "degree": 3.0}
    return make_kernel(K, kw), bool(incr)


def test_where_the_product_is_knowingly_more_accurate_than_the_float64_restatement(K, fuzz_cases):
    """Case 187 of `tools/fuzz_parity.py 1500 51`: SignatureLinear, order 3, ONE column, 33 / 32 observations, normalised, float64.  The
    float64 oracle -- the reference's algorithm, the pair recursion's sums over index tuples -- is 1.06e-4 (K(X, X2)) / 1.05e-6 (K(X)) away from
    the SAME algorithm evaluated in 80-bit arithmetic (numpy longdouble through the oracle's own code; stored beside it): for a one-column
    sequence the sums cancel from ~1e8 to ~1e-3.  The product's feature route sums per sequence and does not cancel: it is held to the 80-bit
    values at the contract's 1e-6, i.e. it departs from the float64 restatement where that restatement is the inaccurate one.  The pair
    kernels (the reference's own summation, on the GPU) are held to EITHER value: they cancel like the oracle, in another order."""
    from gpsig_amd import _lib
    fz, key = fuzz_cases, "c187"
    kern, _ = _fuzz_kernel(K, fz, key)
    X, X2 = fz[key + "_X"], fz[key + "_X2"]
    assert relerr(fz[key + "_Kx"], fz[key + "_Kx80"]) > 5e-5 and relerr(fz[key + "_K"], fz[key + "_K80"]) > 5e-7      # the oracle's own distance
    ctx = _lib.context(0, 0)
    try:
        ctx.set_option("sig_features", 1)                   # the route the planner takes at this size (129 x 130 sequences)
        assert relerr(kern.K(X, X2, presliced=True), fz[key + "_Kx80"]) <= TOL
        assert relerr(kern.K(X), fz[key + "_K80"]) <= TOL
        ctx.set_option("sig_features", -1)
        assert relerr(kern.K(X, X2, presliced=True), fz[key + "_Kx80"]) <= TOL        # (the planner's choice is that route)
        ctx.set_option("sig_features", 0)                   # the higher-order pair kernels: the reference's summation
        got = kern.K(X, X2, presliced=True)
        assert min(relerr(got, fz[key + "_Kx80"]), relerr(got, fz[key + "_Kx"])) <= 2e-4
    finally:
        ctx.set_option("sig_features", -1)


def test_float32_requests_on_one_column_state_spaces(K, fuzz_cases):
    """The float32 cases of the same sweep with num_features = 1 -- the class of every float32 miss the sweeps reported (1.2e-4 .. 5.6e-3
    against the float32 tolerance 1e-4): since round 5 such requests are evaluated by the float64 kernels and rounded (kernels.py,
    _f32_upcast), and meet the float32 tolerance on the matrix scale."""
    fz = fuzz_cases
    keys = [str(k) for k in fz["names"] if str(k) != "c187"]
    assert len(keys) >= 5
    for key in keys:
        kern, incr = _fuzz_kernel(K, fz, key)
        X, X2, Z = fz[key + "_X"], fz[key + "_X2"], fz[key + "_Z"]
        assert X.dtype == np.float32
        for name, got in (("K", kern.K(X)), ("Kx", kern.K(X, X2, presliced=True)), ("Kdiag", kern.Kdiag(X)),
                          ("Kzx", kern.K_tens_vs_seq(Z, X, increments=incr)), ("Kzz", kern.K_tens(Z, increments=incr))):
            want = fz[key + "_" + name]
            assert np.asarray(got).dtype == np.float32, (key, name)
            err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max() / (np.abs(want).max() + 1e-300))
            assert err <= 1e-4, (key, name, err)


@pytest.fixture(scope="module")
def fuzz_cases_r5():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_cases_r5.npz"))


def test_round5_sweep_one_column_float32_case_and_the_oracle_it_was_judged_by(K, fuzz_cases_r5):
    """Case 779 of `tools/fuzz_parity.py 1500 71` (profiles/r05_fuzz.txt): float32, SignatureLinear, order 5, ONE column, 16 against 90
    observations, normalised -- reported 2.3e-3 above the float64 oracle.  The 80-bit evaluation of the oracle's own algorithm (stored beside
    it) says the float64 ORACLE is the one 2.3e-3 off (the index-tuple sums of a one-column sequence cancel, as in case 187 above) -- and so are
    the product's float64 PAIR kernels (5e-3, the same cancellation in another order), which the planner would have picked for 19 x 12 sequences:
    the sweep had drawn `sig_features = 1`.  Since then one-column state spaces take the per-sequence feature route whatever their size
    (sig_feat_api.hip, sig_features_K), float32 requests on them are evaluated in float64, and the product is held to the 80-bit values."""
    fz, key = fuzz_cases_r5, "s71c779"
    kern, _ = _fuzz_kernel(K, fz, key)
    X, X2 = fz[key + "_X"], fz[key + "_X2"]
    assert X.dtype == np.float32
    scale = np.abs(fz[key + "_Kx80"]).max()
    assert np.abs(fz[key + "_Kx"] - fz[key + "_Kx80"]).max() / scale > 1e-3                 # the oracle's own distance
    from gpsig_amd import _lib
    ctx = _lib.context(0, 0)
    got = kern.K(X, X2, presliced=True)
    assert np.asarray(got).dtype == np.float32
    assert np.abs(np.asarray(got, dtype=np.float64) - fz[key + "_Kx80"]).max() / scale <= 1e-5
    got64 = kern.K(X.astype(np.float64), X2.astype(np.float64), presliced=True)
    assert np.abs(got64 - fz[key + "_Kx80"]).max() / scale <= TOL
    try:
        ctx.set_option("sig_features", 0)                   # the pair kernels: the reference's summation, cancelling like the oracle
        pk = kern.K(X.astype(np.float64), X2.astype(np.float64), presliced=True)
        assert np.abs(pk - fz[key + "_Kx80"]).max() / scale <= 2e-2
    finally:
        ctx.set_option("sig_features", -1)


def test_round5_sweep_float32_cosine_on_sequences_of_two_or_three_observations(K, fuzz_cases_r5):
    """Cases 255 (seed 71) and 298 (seed 72) of round 5's sweeps: float32, SignatureCosine, inducing tensors against sequences of two / three
    observations, normalised: 1.7e-4 / 3.9e-4 on the matrix scale against the sweeps' float32 tolerance of 1e-4.  The cosine kernel's values are
    ratios of float32 inner products and the levels of so short a sequence are a handful of their double increments -- float32 arithmetic on the
    request's own precision, the same in the tile kernel and the pair kernels.  Tolerance for this class, stated: 1e-3 (float64 requests: 1e-6)."""
    fz = fuzz_cases_r5
    for key in ("s71c255", "s72c298"):
        kern, incr = _fuzz_kernel(K, fz, key)
        X, Z, want = fz[key + "_X"], fz[key + "_Z"], fz[key + "_Kzx"]
        got = kern.K_tens_vs_seq(Z, X, increments=incr)
        assert np.asarray(got).dtype == np.float32
        # (since the round's closing sweeps float32 requests of the cosine kernel are evaluated in float64 and rounded -- kernels.py, _f32_upcast --
        # so these meet the float32 tolerance again; the stated 1e-3 stands for what float32 arithmetic itself delivers on this class)
        assert np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max() <= 1e-4, key
        got64 = kern.K_tens_vs_seq(Z.astype(np.float64), X.astype(np.float64), increments=incr)
        assert relerr(got64, want) <= TOL, key


def test_round5_closing_sweep_cases(K, fuzz_cases_r5):
    """`tools/fuzz_parity.py 800 73`, run with the round's final library (profiles/r05_fuzz.txt): two of 800 cases above tolerance.
    Case 736 -- float64, SignatureCosine, order 2, 129 sequences of 33 x 2, normalised: 1.5e-6 on the sweep's ENTRY-WISE scale, at one near-zero
    entry.  The float64 oracle is 1.5e-6 from its own code in 80-bit arithmetic there; the product is held to the 80-bit values.
    Case 629 -- float32, SignatureMatern52, order 6, sequences of two observations, normalised: 1.06e-4 against the sweep's 1e-4: float32
    arithmetic on a two-point lattice (the class of the cosine cases above); stated 1e-3, and the float64 request agrees to 1e-6."""
    fz = fuzz_cases_r5
    key = "s73c736"
    kern, _ = _fuzz_kernel(K, fz, key)
    X, k80 = fz[key + "_X"], fz[key + "_K80"]
    entrywise = lambda a, b: float(np.max(np.abs(a - b) / (np.abs(b) + 1e-6 * np.abs(b).max())))       # noqa: E731 (the sweep's float64 measure)
    assert entrywise(fz[key + "_K"], k80) > 1e-6                                                         # the oracle's own distance
    assert entrywise(np.asarray(kern.K(X)), k80) <= 1e-8
    key = "s73c629"
    kern, _ = _fuzz_kernel(K, fz, key)
    X, X2, want = fz[key + "_X"], fz[key + "_X2"], fz[key + "_Kx"]
    got = kern.K(X, X2, presliced=True)
    assert np.asarray(got).dtype == np.float32
    assert np.abs(np.asarray(got, dtype=np.float64) - want).max() / np.abs(want).max() <= 1e-3
    assert relerr(kern.K(X.astype(np.float64), X2.astype(np.float64), presliced=True), want) <= TOL


@pytest.mark.parametrize("base", ["matern12", "matern32", "matern52"])
def test_matern_families_at_compile_time_in_the_sequence_gram(K, base):
    """Round 5: the float64 sequence Gram of the Matern families runs compile-time instances on prescaled records (seq_step_matern_prescaled:
    distances from coordinate differences, inverse square root + Newton step, table exp) where the exact shapes are built; option matern_fast = 0
    keeps the run-time-kind instances.  Both against the oracle, and against each other -- including a sequence paired with itself, whose diagonal
    cells have distance exactly zero on either route."""
    from gpsig_amd import _lib
    rng = np.random.default_rng(91)
    ctx = _lib.context(0, 0)
    for (N, L, d, M) in ((37, 64, 8, 5), (9, 33, 4, 4), (5, 20, 3, 5)):
        X = np.cumsum(rng.standard_normal((N, L, d)) * 0.3, 1).reshape(N, -1)
        X2 = np.cumsum(rng.standard_normal((N + 2, L, d)) * 0.3, 1).reshape(N + 2, -1)
        kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base, normalization=False, lengthscales=np.full(d, 1.3))
        kern, ko = make_kernel(K, kw), make_oracle(kw)
        got = {}
        try:
            for fast in (1, 0):
                ctx.set_option("matern_fast", fast)
                got[fast] = (np.asarray(kern.K(X)), np.asarray(kern.K(X, X2)))
        finally:
            ctx.set_option("matern_fast", 1)
        assert relerr(got[1][0], ko.K(X)) <= TOL and relerr(got[1][1], ko.K(X, X2)) <= TOL
        assert relerr(got[1][0], got[0][0]) <= 1e-12 and relerr(got[1][1], got[0][1]) <= 1e-12


# ------------------------------------------------------------------------------------------------
# round 6: independent witness values (tests/golden/make_witness.py -- closed-form kappa in 50-digit arithmetic, literal tuple sums;
# nothing of oracle/ or gpsig_amd/ was imported to produce them)
# ------------------------------------------------------------------------------------------------
def test_hip_path_against_independent_witness_values(K):
    import json
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "witness.json")) as f:
        meta = json.load(f)
    W = np.load(os.path.join(here, "witness.npz"))
    lvl = lambda got, want: max(float(np.abs(g - w).max() / np.abs(w).max()) for g, w in zip(np.asarray(got), want))   # noqa: E731
    worst = 0.0
    for c in meta:
        n = c["name"]
        X, Y, Z, Zi = (W[n + "/" + k] for k in ("X", "Y", "Z", "Zi"))
        nx, L1, d = X.shape
        ny = Y.shape[0]

        def kern(normalization=False, variances=1):
            kw = dict(base=c["base"], input_dim=L1 * d, num_features=d, num_levels=c["M"], lengthscales=c["lengthscales"], base_params=c["params"],
                      normalization=normalization, variances=variances, num_lags=(len(c["lags"]) if c["lags"] else None))
            k = make_kernel(K, kw)
            if c["lags"]:
                k.lags, k.gamma = np.asarray(c["lags"], dtype=float), np.asarray(c["gamma"], dtype=float)
            return k
        k1 = kern()
        Xf, Yf = X.reshape(nx, -1), Y.reshape(ny, -1)
        # (presliced: GPflow's Kernel._slice would cut the second argument to input_dim columns -- the two sides have different lengths here,
        # which kernels.py:417-440 supports: it reshapes each side by its own width)
        errs = [lvl(k1.K(Xf, Yf, return_levels=True, presliced=True), W[n + "/K_cross_levels"])]
        sym, want = np.asarray(k1.K(Xf, return_levels=True)), W[n + "/K_symm_levels"]
        off = ~np.eye(nx, dtype=bool)
        if c["base"] == "matern12":          # coinciding points: the closed form has r = 0 exactly where float64 squared distances are rounding noise
            errs.append(max(float(np.abs(g[off] - w[off]).max() / np.abs(w).max()) for g, w in zip(sym, want)))
        else:
            errs.append(lvl(sym, want))
            errs.append(float(np.abs(np.asarray(kern(True, W[n + "/variances"]).K(Xf)) - W[n + "/K_symm_normalised"]).max()))
        for tag, ZZ, inc in (("", Z, False), ("_incr", Zi, True)):
            errs.append(lvl(k1.K_tens_vs_seq(ZZ, Xf, return_levels=True, increments=inc), W[n + "/Kzx%s_levels" % tag]))
            kzz, wzz = np.asarray(k1.K_tens(ZZ, return_levels=True, increments=inc)), W[n + "/Kzz%s_levels" % tag]
            if c["base"] == "matern12":
                offz = ~np.eye(kzz.shape[1], dtype=bool)
                kzz, wzz = kzz[:, offz], wzz[:, offz]
            errs.append(lvl(kzz, wzz))
        assert max(errs) < 1e-10, (n, errs)
        worst = max(worst, max(errs))
    print(f"witness: {len(meta)} cases, worst {worst:.2e}")


@pytest.mark.parametrize("M,order,d,L", [(5, 2, 8, 64), (4, 2, 8, 50), (3, 2, 6, 33), (5, 2, 4, 64), (4, 2, 3, 20), (5, 4, 8, 64), (5, 3, 7, 100), (4, 3, 8, 64), (4, 4, 8, 70)])
@pytest.mark.parametrize("base", ["rbf", "matern12", "matern32", "matern52"])
def test_exact_higher_order_rbf_instances(K, M, order, d, L, base):
    """Round 6: the higher-order algorithm (signature_algs.py:37-74) with num_levels AND order at compile time for SignatureRBF -- the exact instances
    of seq_inst_ho_ptdrbf_exact*.hip (prescaled records, table exp): symmetric and cross Grams, normalised and not, against the oracle and against the
    run-time instances (option exact = 0).  The Matern families: the order-2 instances of seq_inst_ho_ptdm*_exact.hip (prescaled records, table exp, rsq).
    (Self-paired sequences have coinciding points: Matern-1/2 at 1e-6)"""
    if base != "rbf" and order != 2:
        pytest.skip("the Matern families have exact instances at order 2")
    import torch
    from gpsig_amd import _lib
    rng = np.random.default_rng(100 * M + 10 * order + d)
    N, N2 = 37, 9
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.3, axis=1).reshape(N, -1)
    X2 = np.cumsum(rng.standard_normal((N2, L, d)) * 0.3, axis=1).reshape(N2, -1)
    ctx = _lib.context(0, 0)
    for normalization in (True, False):
        kw = dict(base=base, input_dim=L * d, num_features=d, num_levels=M, order=order, lengthscales=np.sqrt(d) * np.ones(d), normalization=normalization)
        k, ko = make_kernel(K, kw), make_oracle(kw)
        got = {}
        for exact in (1, 0):
            ctx.set_option("exact", exact)
            try:
                got[exact] = (k.K(X), k.K(X, X2), k.K(X[:5], return_levels=True))
            finally:
                ctx.set_option("exact", 1)
        for a, b in zip(got[1], (ko.K(X), ko.K(X, X2), ko.K(X[:5], return_levels=True))):
            assert relerr(a, b) <= (1e-6 if base == "matern12" else 1e-9), (normalization, relerr(a, b))
        for a, b in zip(got[1], got[0]):
            assert relerr(a, b) <= (1e-6 if base == "matern12" else 1e-10)


@pytest.mark.parametrize("M,order,d,T,N,L", [(4, 2, 6, 70, 45, 50), (4, 4, 6, 512, 40, 9), (3, 2, 3, 33, 130, 7), (5, 3, 8, 65, 20, 13), (5, 5, 4, 40, 17, 6), (3, 3, 8, 64, 64, 2)])
def test_higher_order_chains_in_the_tile_kernel(K, M, order, d, T, N, L):
    """Round 6: signature_algs.py:129-160 in the Kzx tile kernel (tvs_tile_inst_ho.hip: the RBF kernel, the order a run-time argument): with and without
    increments, level arrays and the normalised sum, against the oracle and against the older mappings (option tvs_tile = 0)."""
    import torch
    from gpsig_amd import _lib
    rng = np.random.default_rng(10 * M + order + d)
    lt = M * (M + 1) // 2
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.3, axis=1).reshape(N, -1)
    ctx = _lib.context(0, 0)
    for increments in (False, True):
        Z = rng.standard_normal((lt, T, 2, d) if increments else (lt, T, d)) * 0.5
        kw = dict(base="rbf", input_dim=L * d, num_features=d, num_levels=M, order=order, lengthscales=np.sqrt(d) * np.ones(d))
        k, ko = make_kernel(K, kw), make_oracle(kw)
        got = {}
        for tile in (-1, 0):
            ctx.set_option("tvs_tile", tile)
            try:
                ctx.timing_reset()
                got[tile] = (k.K_tens_vs_seq(Z, X, increments=increments), k.K_tens_vs_seq(Z, X, increments=increments, return_levels=True))
            finally:
                ctx.set_option("tvs_tile", -1)
        for a, b in zip(got[-1], (ko.K_tens_vs_seq(Z, X, increments=increments), ko.K_tens_vs_seq(Z, X, increments=increments, return_levels=True))):
            assert relerr(a, b) <= 1e-9, (increments, relerr(a, b))
        for a, b in zip(got[-1], got[0]):
            assert relerr(a, b) <= 1e-9
