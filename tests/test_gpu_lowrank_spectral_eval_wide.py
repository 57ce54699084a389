"""Low-rank SignatureSpectral EVALUATION on wide state spaces (33 .. 4,096 columns) behind the kernel object's opt-in ``lr_spectral_wide``:
gpsig_lr_seq_features, gpsig_lr_seq_features_ragged and gpsig_lr_tens_features through the evaluation form of the spectral cross kernel
(csrc/lr_eval_spectral_wide_inst.hip: lr_spx_eval_kernel, the points' phases inside its walk) and the feature kernels that take kxs / kzs from
memory; the landmark Gram of gpsig_lr_whitening / gpsig_lr_draw by the thread-per-pair kernel with row stride d.  Which calls take the route:
csrc/lr_tile_plan.hpp: lr_spectral_eval_wide / lr_spectral_eval_tens_wide (tests/test_lr_spectral_eval_route.py).

Parameters are scaled as tests/test_gpu_lowrank_eval_wide.py::make_kernel("spectral", ...) scales them (omega, gamma ~ 1 / sqrt(d)); landmarks are
drawn from the evaluated points, so the zero-distance, zero-phase case is in every test.  N = 5 sequences, T = 3 tensors, M = 3 unless said.

Tolerances are the project's own: identities between the library's own kernels relerr <= 1e-12 (here against the training op gpsig_spectral_cross
on the flat points followed by gpsig_lr_*_features_kx_dev, both of the parent commit); K against oracle.LowRankOracle 1e-7 of the largest entry
(tests/test_gpu_lowrank_spectral.py: LR_TOL); the Python surface, ragged against padded by repetition, <= 1e-9; pointer modes, chunk counts and
lr_fused = 0: the same bits."""
import numpy as np
import pytest
import torch

from test_gpu_lowrank_eval_long import SURFACE, features, host, ragged_table, relerr, seqs, surface_call, with_lr_fused
from test_gpu_lowrank_eval_wide import tens_features, with_chunk_mb
from test_gpu_lowrank_spectral import LR_TOL, make_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N, T, M = 5, 3, 3
FAMILIES = ["rbf", "exp", "mixed"]


def make_kernel(family, L, d, c, r, Q=3, M_=M, wide=True, low_rank=True, **kw):
    from gpsig_amd import kernels
    rng = np.random.default_rng(2)
    k = kernels.SignatureSpectral(L * d, d, M_, family=family, Q=Q, low_rank=low_rank, num_components=c, rank_bound=r, **kw)
    k.alpha, k.omega, k.gamma = rng.uniform(0.3, 1.2, Q), 0.5 * rng.standard_normal((Q, d)) / np.sqrt(d), rng.uniform(0.4, 1.3, (Q, d)) / np.sqrt(d)
    k.rng = np.random.default_rng(5)
    k.lr_spectral_wide = wide
    return k


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def kx_params(k, c, keep):
    """the parameter block the kx entry points take: the levels and the difference flag of k, c columns, no spectral table"""
    from gpsig_amd import kernels
    aux = kernels.SignatureRBF(c, c, k.num_levels, lengthscales=None, difference=k.difference, normalization=k.normalization, low_rank=True,
                               num_components=c, rank_bound=int(k.rank_bound))
    return aux._params(keep)


def composed(k, st, P, shape, tensors=False, increments=False):
    """what a user of the parent commit computes: gpsig_spectral_cross on the points P (n, d) as they lie in memory, then
    gpsig_lr_seq_features_kx_dev (shape = (N, L)) / gpsig_lr_tens_features_kx_dev (shape = (T,)) on the same whitening and projections"""
    from gpsig_amd import autodiff
    P = dev(P)
    n, d = P.shape
    c, r, Q = st.num_components, st.rank_bound, k.Q
    S, a, o, g, Wh = (dev(v) for v in (st.landmarks, k.alpha, k.omega, k.gamma, st.whitening))
    kxs = torch.full((n, c), float("nan"), dtype=torch.float64, device=DEV)
    lc = autodiff._ctx_for(P)
    ptr = autodiff._ptr
    lc.check(lc._lib.gpsig_spectral_cross(lc._h, Q, autodiff._SPECTRAL_FAMILY[k.family], d, ptr(P), n, ptr(S), c, ptr(a), ptr(o), ptr(g), ptr(kxs)))
    keep = []
    p = kx_params(k, c, keep)
    arr = autodiff._sketch_array(st.sketches, keep)
    out = torch.full((shape[0], 1 + c + len(st.sketches) * r), float("nan"), dtype=torch.float64, device=DEV)
    if tensors:
        lc.call("gpsig_lr_tens_features_kx_dev", p, c, r, len(st.sketches), arr, ptr(kxs), shape[0], int(increments), ptr(Wh), ptr(out))
    else:
        lc.call("gpsig_lr_seq_features_kx_dev", p, c, r, len(st.sketches), arr, ptr(kxs), shape[0], shape[1], None, ptr(Wh), ptr(out))
    torch.cuda.current_stream(DEV).synchronize()
    return host(out)


# ---- 1. composition identity, sequences -------------------------------------------------------------------------------------------------
def check_seq_identity(family, d, c, Q, L, difference, n=N, seed=77):
    rng = np.random.default_rng(seed)
    X = seqs(rng, n, L, d)
    k = make_kernel(family, L, d, c, c, Q=Q, normalization=False, difference=difference)
    st = k.draw_low_rank(X=X)
    pts = X.reshape(n * L, d)
    assert all((np.abs(pts - s[None, :]).max(axis=1) == 0).any() for s in st.landmarks), "a landmark is no point of the table"
    got = features(k, st, dev(X))
    want = composed(k, st, pts, (n, L))
    e = relerr(got, want)
    print(family, "d", d, "c", c, "Q", Q, "L", L, "difference", difference, "against the composition:", e, "bits equal:", np.array_equal(got, want))
    assert (got[:, 0] == 1.0).all() and e <= 1e-12, e
    return k, st, X, got


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("d", [33, 64, 65, 160])
def test_sequences_every_width_and_family(d, family):
    """one past the line (a last k-step with one live column), exactly the tile, a second 64-column pass of one column, three passes"""
    check_seq_identity(family, d, 8, 3, 70, True)


@pytest.mark.parametrize("c", [8, 20, 50])
@pytest.mark.parametrize("L,difference", [(70, False), (130, True)])
def test_sequences_landmark_tiles(c, L, difference):
    """one, two and four landmark tiles with a short last one, at d = 65; both lengths, with and without the difference"""
    check_seq_identity("mixed", 65, c, 3, L, difference)


@pytest.mark.parametrize("d,family,L", [(33, "exp", 130), (160, "mixed", 70)])
def test_sequences_second_phase_tile(d, family, L):
    """Q = 17: a second 16-component tile of phases, fetched from the other accumulator"""
    check_seq_identity(family, d, 8, 17, L, True)


# ---- 2. the same for tensors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("increments", [True, False], ids=["increments", "plain"])
@pytest.mark.parametrize("d,family", [(33, "exp"), (160, "rbf")])
def test_tensors_against_the_composition(d, family, increments):
    rng = np.random.default_rng(51)
    lt = M * (M + 1) // 2
    Z = rng.standard_normal((lt, T, 2, d) if increments else (lt, T, d))
    k = make_kernel(family, 70, d, 8, 8, normalization=False)
    st = k.draw_low_rank(Z=Z, increments=increments)
    got = tens_features(k, st, dev(Z), increments)
    want = composed(k, st, Z.reshape(-1, d), (T,), tensors=True, increments=increments)
    e = relerr(got, want)
    print("tensors", family, d, increments, "against the composition:", e, "bits equal:", np.array_equal(got, want))
    assert (got[:, 0] == 1.0).all() and e <= 1e-12, e


# ---- 3. oracle --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_against_the_oracle(family):
    rng = np.random.default_rng(53)
    L, d, c = 70, 160, 8
    X = seqs(rng, N, L, d)
    Z = 0.5 * rng.standard_normal((M * (M + 1) // 2, T, 2, d))
    k = make_kernel(family, L, d, c, c, normalization=True)
    st = k.draw_low_rank(X=X, Z=Z, increments=True)
    lo = make_oracle(k, st)
    for name, g, w in (("K", k.K(X, lr_state=st), lo.K(X)), ("Kdiag", k.Kdiag(X, lr_state=st), lo.Kdiag(X)),
                       ("K_tens", k.K_tens(Z, increments=True, lr_state=st), lo.K_tens(Z, increments=True)),
                       ("K_tens_vs_seq", k.K_tens_vs_seq(Z, X, increments=True, lr_state=st), lo.K_tens_vs_seq(Z, X, increments=True))):
        e = relerr(g, w)
        print(family, name, "against the oracle:", e)
        assert e <= LR_TOL, (name, e)


# ---- 4. pointer modes and chunks --------------------------------------------------------------------------------------------------------
def test_pointer_modes_and_chunks_give_the_same_bits():
    """wide_chunk_mb = 1: a sequence of L = 70 at c = 8 takes 4,480 bytes of kxs, so 234 fit and N = 240 goes in two
    chunks; a tensor at M = 3, c = 8 with increments takes 768 bytes of kzs, so 1,365 fit and T = 1,400 goes in two"""
    L, d, c, n = 70, 33, 8, 240
    rng = np.random.default_rng(91)
    X = seqs(rng, n, L, d)
    k = make_kernel("exp", L, d, c, c, normalization=False)
    st = k.draw_low_rank(X=X[:8])
    hst = features(k, st, X)
    whole = features(k, st, dev(X))
    parts = with_chunk_mb(1, lambda: features(k, st, dev(X)))
    assert np.isfinite(whole).all() and np.array_equal(hst, whole) and np.array_equal(whole, parts)
    lengths = rng.integers(1, L + 1, size=n)
    whole = features(k, st, dev(X), lengths)
    parts = with_chunk_mb(1, lambda: features(k, st, dev(X), lengths))
    assert np.isfinite(whole).all() and np.array_equal(whole, parts) and np.array_equal(features(k, st, X, lengths), whole)
    Tn = 1400
    Z = rng.standard_normal((M * (M + 1) // 2, Tn, 2, d))
    st = k.draw_low_rank(Z=Z[:, :8], increments=True)
    hst = tens_features(k, st, Z, True)
    whole = tens_features(k, st, dev(Z), True)
    parts = with_chunk_mb(1, lambda: tens_features(k, st, dev(Z), True))
    assert np.isfinite(whole).all() and np.array_equal(hst, whole) and np.array_equal(whole, parts)


# ---- 5. ragged --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [65, 160])
@pytest.mark.parametrize("L,lengths", [(70, [70, 3, 1, 66, 65]), (130, [130, 129, 66, 65, 2])])
def test_ragged(L, lengths, d):
    """each sequence against the dense call on its truncated copy; NaN beyond each length; lr_fused = 0 gives the same bits, dense and ragged"""
    c = 8
    rng = np.random.default_rng(31)
    X = ragged_table(rng, lengths, L, d)
    k = make_kernel("mixed", L, d, c, c, normalization=False)
    st = k.draw_low_rank(X=X, lengths=lengths)
    assert np.isfinite(st.landmarks).all()
    F = 1 + c + (M - 1) * c
    want = []
    for n, l in enumerate(lengths):
        if l == 1:                                  # (difference: no step, the constant feature alone)
            want.append(np.eye(1, F)[0])
            continue
        want.append(features(k, st, np.ascontiguousarray(X.reshape(len(lengths), L, d)[n:n + 1, :l].reshape(1, l * d)))[0])
    want = np.stack(want)
    hst = features(k, st, X, lengths)
    got = features(k, st, dev(X), lengths)
    e = relerr(got, want)
    print(L, d, "ragged against truncated copies:", e)
    assert np.isfinite(got).all() and (got[:, 0] == 1.0).all() and e <= 1e-12, e
    assert np.array_equal(hst, got)
    with_lr_fused(0, lambda: np.testing.assert_array_equal(features(k, st, X, lengths), hst))
    full = seqs(rng, N, L, d)
    dense = features(k, st, full)
    with_lr_fused(0, lambda: np.testing.assert_array_equal(features(k, st, full), dense))


# ---- 6. the stride wraps ----------------------------------------------------------------------------------------------------------------
def test_the_grid_stride_wraps():
    """1,010 sequences of L = 65: 65,650 points, a second round of the 1,024 workgroups x 64 points whose last block is partial"""
    check_seq_identity("rbf", 33, 8, 1, 65, True, n=1010, seed=93)


# ---- 7. device draw ---------------------------------------------------------------------------------------------------------------------
def test_device_draw():
    """gpsig_lr_draw at d = 160: the exported whitening against low_rank_state on the host route, to the bound tests/test_gpu_parity.py:1645
    holds two whitenings of the same landmarks to ((W + jitter)^-1 = Wh Wh^T to 1e-7 of its largest entry: the eigenvectors' signs and
    the solver may differ); K from the device state against the oracle"""
    rng = np.random.default_rng(57)
    L, d, c = 70, 160, 8
    X = seqs(rng, N, L, d)
    k = make_kernel("exp", L, d, c, c, normalization=True)
    assert k.device_draw
    st = k.draw_low_rank(X=dev(X))
    h = st.export()
    assert all((np.abs(X.reshape(N * L, d) - s[None, :]).max(axis=1) == 0).any() for s in h.landmarks)
    hs = k.low_rank_state(h.landmarks, h.jitter_diag, h.sketches)
    inv_d, inv_h = h.whitening @ h.whitening.T, hs.whitening @ hs.whitening.T
    e = float(np.abs(inv_d - inv_h).max() / np.abs(inv_h).max())
    print("device whitening against the host route:", e)
    assert e <= 1e-7, e
    lo = make_oracle(k, h)
    e = relerr(k.K(dev(X), lr_state=st), lo.K(X))
    print("K from the device state against the oracle:", e)
    assert e <= LR_TOL, e


# ---- 8. the Python surface --------------------------------------------------------------------------------------------------------------
S_L, S_D = 70, 40
S_LEN, S_LEN2 = [70, 1, 2, 33, 64, 65, 66, 69], [5, 70, 66, 1, 40]


def surface_data():
    rng = np.random.default_rng(61)
    out = {}
    for name, lens in (("X", S_LEN), ("Y", S_LEN2)):
        nan = ragged_table(rng, lens, S_L, S_D).reshape(len(lens), S_L, S_D)
        rep = nan.copy()
        for n, l in enumerate(lens):
            rep[n, l:] = rep[n, l - 1]
        out[name] = (nan.reshape(len(lens), -1), rep.reshape(len(lens), -1))
    out["Z"] = rng.standard_normal((M * (M + 1) // 2, 5, 2, S_D))
    out["Zs"] = np.cumsum(0.3 * rng.standard_normal((4, 6, S_D)), axis=1)
    return out


@pytest.mark.parametrize("method", SURFACE)
def test_python_surface_ragged_equals_padded_by_repetition(method):
    data = surface_data()
    k = make_kernel("mixed", S_L, S_D, 16, 12, normalization=method != "Kdiag")
    Z, Zs = dev(data["Z"]), dev(data["Zs"])

    def run(which, lens, lens2):
        k.rng = np.random.default_rng(21)
        out = surface_call(k, method, dev(data["X"][which]), dev(data["Y"][which]), Z, Zs, lens, lens2)
        return [host(o) for o in (out if isinstance(out, tuple) else (out,))]

    want = run(1, {}, {})
    got = run(0, {"lengths": torch.as_tensor(S_LEN, device=DEV)}, {"lengths2": np.asarray(S_LEN2)})
    for g, w in zip(got, want):
        e = relerr(g, w)
        print(method, "ragged against padded by repetition:", e)
        assert e <= 1e-9, (method, e)
    if method == "predict_f":
        assert len(got) == 2 and all(np.isfinite(g).all() for g in got)


# ---- 9. float32 -------------------------------------------------------------------------------------------------------------------------
def test_float32_is_the_rounded_float64_evaluation():
    """the library has no float32 spectral kernel at these widths: with lr_native_f32 it refuses the float32 call, and the Python layer computes
    it in float64 from the same state and rounds"""
    rng = np.random.default_rng(41)
    L, d, c = 70, 40, 8
    X64 = seqs(rng, N, L, d).astype(np.float32).astype(np.float64)
    k = make_kernel("rbf", L, d, c, c, normalization=True)
    st = k.draw_low_rank(X=X64)
    k.lr_native_f32 = True
    K64, K32 = k.K(X64, lr_state=st), k.K(X64.astype(np.float32), lr_state=st)
    assert K32.dtype == np.float32 and np.isfinite(K64).all() and np.array_equal(K32, K64.astype(np.float32))
    with pytest.raises(NotImplementedError, match="float64 only"):
        features(k, st, X64.astype(np.float32))


# ---- 10. refusals and the default -------------------------------------------------------------------------------------------------------
def test_the_default_refuses_as_before():
    rng = np.random.default_rng(96)
    L = 70
    X = seqs(rng, N, L, 160)
    k = make_kernel("rbf", L, 160, 8, 8, wide=False, normalization=False)
    with pytest.raises(NotImplementedError, match="at most 32 features"):
        features(k, k.draw_low_rank(X=X), X)


def test_refusals_name_their_bound():
    rng = np.random.default_rng(97)
    L = 70
    X = seqs(rng, N, L, 160)
    k = make_kernel("rbf", L, 160, 65, 8, normalization=False)
    st = k.draw_low_rank(X=X)
    with pytest.raises(NotImplementedError, match="num_components <= 64"):
        features(k, st, X)
    with pytest.raises(NotImplementedError, match="num_components <= 64"):
        features(k, st, X, [70, 3, 1, 66, 65])
    k = make_kernel("rbf", L, 160, 8, 8, M_=9, normalization=False)
    with pytest.raises(NotImplementedError, match="num_levels <= 8"):
        features(k, k.draw_low_rank(X=X), X)
    X = seqs(rng, 2, 6, 4097)
    k = make_kernel("rbf", 6, 4097, 8, 8, normalization=False)
    with pytest.raises(NotImplementedError, match="4096"):
        features(k, k.draw_low_rank(X=X), X)
    X = seqs(rng, N, 10, 40)
    k = make_kernel("rbf", 10, 40, 8, 8, low_rank=False)
    assert k.lr_spectral_wide and not k.low_rank
    with pytest.raises(NotImplementedError, match="at most 32 features"):
        k.compute_K_symm(X)


def test_32_columns_keep_their_bits_with_the_flag():
    rng = np.random.default_rng(98)
    L, d = 70, 32
    X = seqs(rng, N, L, d)
    k = make_kernel("mixed", L, d, 8, 8, wide=False, normalization=False)
    st = k.draw_low_rank(X=X)
    without = features(k, st, X)
    k.lr_spectral_wide = True
    st2 = k.low_rank_state(st.landmarks, st.jitter_diag, st.sketches)
    assert np.array_equal(st2.whitening, st.whitening)
    assert np.array_equal(features(k, st, X), without) and np.array_equal(features(k, st, dev(X)), without)
