"""Every kernel form the options of gpsig_set_option select, and both sides of the automatic rules that choose between forms, through the C ABI.

tests/kernel_forms.py maps each option to the tests here (or elsewhere) that run its values.  Tolerances: values 1e-10 relative to the largest entry
against oracle/sigkern_oracle.py, gradients 1e-9 against autograd of oracle/sigkern_oracle_torch.py, float32 1e-4 on the matrix scale.  Forms that
issue the same arithmetic in the same order are held to each other bit for bit.  Every test sets its options through _Opts, whose exit restores the
csrc/ctx.hpp default even when an assertion fails: contexts are shared per stream across tests.

Route checks (the default result bitwise equal to the form the rule should pick, forced by its option) are made only where both candidates are free
of atomics: the wide-route kernels and the contraction reduce, the forward pair and tile kernels, the reverse tile kernel of Kzx.  By values only:
the fused reverse kernel against the wavefront kernel (grad_impl 0 / 4: grad_fused_kernel.hpp and grad_wave_kernel.hpp add with atomics), the
tensor-lane gradient of tvs_zreg and the round-1 Kzx reverse kernels of tvs_grad_matern 0 (grad_kernels.hpp), the low-rank reverse pass at 512 /
1,024 threads, the reverse passes of Kzz on both sides of the wide rule, and the higher-order reverse sweeps of ho_g32, whose point route around
the sweeps adds with atomics (grad_core.hpp).  A route check is a check only where the two candidates give different bits: the tests assert that
for Kzx at 8 / 9 columns, Kzz at 12 / 13, the `few` rule and sig_graded; where the candidates give the same bits (tvs_tile at 32 tensors,
wide_o1_sweeps, wide_lat_waves, ho_g32, rocBLAS against the hand-written contraction) the test's docstring says so."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sigkern_oracle as O
from oracle import sigkern_oracle_torch as OT
from kernel_forms import OPTIONS
from test_gpu_grad import _P, _host_ctx, _params, _t_kern, _vp, rel

pytestmark = pytest.mark.gpu


class _Opts:
    """set options on a context, restore the ctx.hpp defaults on exit (as kernel_forms.OPTIONS records them, checked against ctx.hpp on the CPU)"""
    def __init__(self, ctx, **kw):
        self.ctx, self.names = ctx, set()
        self.set(**kw)

    def set(self, **kw):
        for k, v in kw.items():
            self.names.add(k)
            self.ctx.set_option(k, v)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for k in self.names:
            self.ctx.set_option(k, OPTIONS[k]["default"])


def _dev_ctx():
    from gpsig_amd import _lib
    return _lib.context(0, torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape and np.isfinite(a).all(), (a.shape, b.shape)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def _seqs(rng, N, L, d, s=0.4):
    return np.cumsum(rng.standard_normal((N, L, d)) * s / np.sqrt(d), axis=1)


# ---- the narrow contraction of the wide route's reverse passes (wide_api.hip: contract_both) -------------------------------------------------

def _contract_groups(R, CW, DA, form):
    """the `groups` of contract_both for one call (form 0 and DA > 32: rocBLAS, None)"""
    if form == 0 or DA > 32:
        return None
    strips, ntiles = -(-R // 64), -(-CW // 64)
    g = -(-((8192 if DA <= 16 and form != 2 else 4096)) // strips)
    return max(1, min(g, ntiles))


def _check_forms(res, calls, DA):
    """forms 1 and 3 (DA <= 16: wide_contract16_kernel<16> / <32>; DA 17 .. 32: both wide_contract_kernel<32>) issue the same MFMA steps in the
    same k order and deal column tiles to the same `groups`: bitwise.  Form 2 (wide_contract_kernel<16>) issues those steps too, but deals the
    tiles to 4,096 / strips groups instead of 8,192 / strips: its gXA partial sums are added in another order wherever the two counts differ
    (both are clamped to the column tiles, so small arrays coincide) -- bitwise where they coincide, 1e-13 where not; gZA is summed per strip
    whatever the groups: bitwise.  At DA 17 .. 32 forms 1, 2 and 3 launch the same wide_contract_kernel<32> with the same groups, so their bitwise
    agreement there says nothing beyond determinism; at DA > 32 all four forms are the same rocBLAS calls.  Form 0 (rocBLAS) agrees to 1e-12; at
    these shapes it happens to give the same bits as the hand-written forms, so the comparison with it cannot tell the routes apart -- the oracle
    and the 1 / 3 comparison can (dropping the last k-step of phase 2 of wide_contract16_kernel fails both).  res[form] = (gZA side, gXA side)."""
    side_z, side_x = 0, 1
    for k in (side_z, side_x):
        assert np.array_equal(res[1][k], res[3][k]), (DA, k, relmax(res[3][k], res[1][k]))
    assert np.array_equal(res[1][side_z], res[2][side_z]), (DA, relmax(res[2][side_z], res[1][side_z]))
    if all(_contract_groups(R, CW, DA, 1) == _contract_groups(R, CW, DA, 2) for R, CW in calls):
        assert np.array_equal(res[1][side_x], res[2][side_x]), (DA, calls, relmax(res[2][side_x], res[1][side_x]))
    else:
        assert relmax(res[2][side_x], res[1][side_x]) < 1e-13
    for k in (side_z, side_x):
        assert relmax(res[0][k], res[1][k]) < 1e-12, (DA, k, relmax(res[0][k], res[1][k]))


KZX_FORM_SHAPES = [  # M, T, N, L, increments, wide_chunk_mb: adjoint rows N L per chunk 1, 63, 64, 65, 130; columns lt E Tpad
    (1, 1, 1, 1, False, 0), (2, 5, 1, 63, True, 0), (1, 70, 1, 64, False, 0), (2, 65, 1, 65, False, 0), (1, 3, 2, 65, True, 0),
    (2, 65, 5, 65, True, 1)]


@pytest.mark.parametrize("d", [1, 8, 14, 15, 30, 31])
def test_wide_contract_forms_in_the_kzx_reverse_pass(d):
    """gpsig_tens_vs_seq_levels_grad on the wide route (wide = 1), wide_contract 0 / 1 / 2 / 3: augmented widths DA = d + 2 of 3 .. 16 (the
    16-column forms), 17 .. 32 (the 32-column kernel) and 33 (rocBLAS whatever the option); adjoint arrays of 1, 63, 64, 65 and 130 rows, the
    last case in three chunks (wide_chunk_mb = 1: the accumulating branch of contract_both).  Every form against autograd of the oracle."""
    rng = np.random.default_rng(500 + d)
    ctx = _host_ctx()
    DA = d + 2
    with _Opts(ctx, wide=1) as o:
        for M, T, N, L, incr, mb in KZX_FORM_SHAPES:
            difference = L > 1
            lt = M * (M + 1) // 2
            Z = rng.standard_normal((lt, T, 2, d) if incr else (lt, T, d)) * 0.5 / np.sqrt(d)
            X = _seqs(rng, N, L, d)
            G = rng.standard_normal((M + 1, T, N))
            kt = OT.SignatureKernelTorchOracle(d, M, "rbf", difference=difference)
            tZ, tX = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
            (kt.K_tens_vs_seq_levels(tZ, tX, incr) * torch.tensor(G)).sum().backward()
            keep = []
            p = _params("rbf", d, M, difference, keep)
            o.set(wide_chunk_mb=mb)
            res = {}
            for form in (0, 1, 2, 3):
                o.set(wide_contract=form)
                gZ, gX, gb = np.full_like(Z, np.nan), np.full_like(X, np.nan), np.zeros(2)
                ctx.call("gpsig_tens_vs_seq_levels_grad", p, _vp(Z), _vp(X), T, N, L, int(incr), _vp(G), _vp(gZ), _vp(gX), gb.ctypes.data_as(_P))
                assert rel(gZ, tZ.grad) < 1e-9 and rel(gX, tX.grad) < 1e-9, (form, M, T, N, L, rel(gZ, tZ.grad), rel(gX, tX.grad))
                res[form] = (gZ, gX)
            CW = lt * (2 if incr else 1) * (-(-T // 64) * 64)
            chunk = N if mb == 0 else max(1, min(N, (1 << 20) // (8 * L * CW)))
            calls = [(min(chunk, N - n0) * L, CW) for n0 in range(0, N, chunk)]
            if mb:
                assert len(calls) == 3
            _check_forms(res, calls, DA)


LAT_FORM_SHAPES = [  # N1, L1, N2, L2, wide_chunk_mb: adjoint rows N1 L1 (per chunk) and columns N2 L2 of 1, 63, 64, 65, 130
    (1, 1, 1, 64, 0), (1, 63, 1, 65, 0), (1, 64, 1, 1, 0), (1, 65, 1, 63, 0), (2, 65, 2, 65, 0), (1, 130, 1, 64, 0), (9, 65, 2, 65, 1)]


@pytest.mark.parametrize("d", [1, 8, 14, 15, 30, 31])
def test_wide_contract_forms_in_the_lattice_reverse_pass(d):
    """gpsig_seq_gram_levels_grad (cross Gram) on the wide route (wide = 1), wide_contract 0 / 1 / 2 / 3: partial 64-row strips and partial
    64-column tiles at every form (rows N1 L1, columns N2 L2 of 1 .. 130), several chunks of left sequences (wide_chunk_mb = 1), widths as above.
    Values of the forward call against the oracle, every form's gradients against autograd of the oracle."""
    rng = np.random.default_rng(600 + d)
    ctx = _host_ctx()
    DA, M = d + 2, 3
    with _Opts(ctx, wide=1) as o:
        for N1, L1, N2, L2, mb in LAT_FORM_SHAPES:
            X, Y = _seqs(rng, N1, L1, d), _seqs(rng, N2, L2, d)
            G = rng.standard_normal((M + 1, N1, N2))
            kt = OT.SignatureKernelTorchOracle(d, M, "rbf", difference=False)
            tX, tY = torch.tensor(X, requires_grad=True), torch.tensor(Y, requires_grad=True)
            lev = kt.K_seq_levels(tX, tY)
            (lev * torch.tensor(G)).sum().backward()
            keep = []
            p = _params("rbf", d, M, False, keep)
            o.set(wide_chunk_mb=mb)
            out = np.full((M + 1, N1, N2), np.nan)
            ctx.call("gpsig_seq_gram_levels", p, _vp(X), _vp(Y), N1, N2, L1, L2, _vp(out))
            assert rel(out, lev.detach()) < 1e-10, (N1, L1, N2, L2, rel(out, lev.detach()))
            res = {}
            for form in (0, 1, 2, 3):
                o.set(wide_contract=form)
                gX, gY, gb = np.full_like(X, np.nan), np.full_like(Y, np.nan), np.zeros(2)
                ctx.call("gpsig_seq_gram_levels_grad", p, _vp(X), _vp(Y), N1, N2, L1, L2, _vp(G), _vp(gX), _vp(gY), gb.ctypes.data_as(_P))
                assert rel(gX, tX.grad) < 1e-9 and rel(gY, tY.grad) < 1e-9, (form, N1, L1, N2, L2, rel(gX, tX.grad), rel(gY, tY.grad))
                res[form] = (gY, gX)
            per_i = 8 * L1 * L2 * N2 * 2
            chunk = N1 if mb == 0 else max(1, min(N1, (1 << 20) // per_i))
            calls = [(min(chunk, N1 - i0) * L1, N2 * L2) for i0 in range(0, N1, chunk)]
            if mb:
                assert len(calls) == 2
            _check_forms(res, calls, DA)


def test_wide_contract_strip_grid_stride():
    """More than 65,535 strips of 64 adjoint rows in one contraction: the grid is clamped to 65,535 and the strips are walked by the grid-stride
    loop.  A cross Gram of 65,600 sequences of 64 observations against one of 2 (first order, no differences): 4,198,400 rows, 2 columns,
    0.6 GB on the device.  The hand-written form (wide_contract 1) against rocBLAS (0); the gradients of sampled sequences (their upstream
    gradient only) against autograd of the oracle."""
    rng = np.random.default_rng(65600)
    N1, L1, N2, L2, d, M = 65600, 64, 1, 2, 1, 2
    assert -(-N1 * L1 // 64) > 65535
    X, Y = _seqs(rng, N1, L1, d), _seqs(rng, N2, L2, d)
    G = rng.standard_normal((M + 1, N1, N2))
    ctx = _host_ctx()
    keep = []
    p = _params("rbf", d, M, False, keep)
    res = {}
    with _Opts(ctx, wide=1) as o:
        for form in (0, 1):
            o.set(wide_contract=form)
            gX, gY, gb = np.full_like(X, np.nan), np.full_like(Y, np.nan), np.zeros(2)
            ctx.call("gpsig_seq_gram_levels_grad", p, _vp(X), _vp(Y), N1, N2, L1, L2, _vp(G), _vp(gX), _vp(gY), gb.ctypes.data_as(_P))
            res[form] = (gX, gY)
    assert relmax(res[1][0], res[0][0]) < 1e-12 and relmax(res[1][1], res[0][1]) < 1e-12, (relmax(res[1][0], res[0][0]), relmax(res[1][1], res[0][1]))
    idx = np.array([0, 1, 65535 * 64 // L1 - 1, 65535 * 64 // L1, N1 - 1])        # sequences on both sides of the last strip of the first grid pass
    kt = OT.SignatureKernelTorchOracle(d, M, "rbf", difference=False)
    tX = torch.tensor(X[idx], requires_grad=True)
    (kt.K_seq_levels(tX, torch.tensor(Y)) * torch.tensor(G[:, idx])).sum().backward()
    assert rel(res[1][0][idx], tX.grad) < 1e-9, rel(res[1][0][idx], tX.grad)


# ---- keep_reset: accumulators cleared through SeqLane::keep (1) or by reset() at pair boundaries (0) ------------------------------------------

KEEP_SHAPES = [(70, 1, 9, 2), (33, 2, 40, 9), (20, 9, 21, 1), (17, 12, 5, 7)]     # N1, L1, N2, L2: many short pairs per lane, L = 1 and 2


@pytest.mark.parametrize("base,opts", [("poly", {}), ("mix", {}), ("linear", {"sig_features": 0}), ("matern32", {"matern_fast": 0}),
                                       ("rbf", {})])
def test_keep_reset_in_the_float64_pair_kernel(base, opts):
    """seq_gram_kernel with keep_reset 0 and 1: with finite accumulators acc * 0 + inc == inc, so the two are bitwise equal; both against the
    oracle (symmetric and cross Grams, level arrays, ragged lengths across the two sides)."""
    from gpsig_amd import _lib, kernels
    from test_gpu_parity import make_kernel, make_oracle
    rng = np.random.default_rng(hash(base) % 1000)
    ctx = _lib.context(0, 0)
    d, M = 3, 3
    for N1, L1, N2, L2 in KEEP_SHAPES:
        X, Y = _seqs(rng, N1, L1, d).reshape(N1, -1), _seqs(rng, N2, L2, d).reshape(N2, -1)
        kw = dict(input_dim=L1 * d, num_features=d, num_levels=M, base=base, normalization=False)
        if base in ("poly", "mix"):
            kw["base_params"] = {"gamma": 1.0, "degree": 3} if base == "poly" else {"mixing": 0.4}
        kx, ko = make_kernel(kernels, kw), make_oracle(kw)
        got = {}
        for keep in (1, 0):
            with _Opts(ctx, keep_reset=keep, **opts):
                got[keep] = (kx.K(X, Y, presliced=True, return_levels=True), kx.K(X, presliced=True), kx.K(Y, presliced=True))
        for a, b in zip(got[0], got[1]):
            assert np.array_equal(a, b), (N1, L1, N2, L2)
        want = (ko.K(X, Y, return_levels=True), ko.K(X), ko.K(Y))
        for g, w in zip(got[1], want):
            assert relmax(g, w) < 1e-10, (N1, L1, N2, L2, relmax(g, w))


@pytest.mark.parametrize("base", ["rbf", "linear"])
def test_keep_reset_in_the_float32_packed_kernel(base):
    """seq_pk2_kernel (float32; pk2 = 2 takes it for the linear family too) with keep_reset 0 / 1 at f32_pack 1 / 2 and f32_waves 1 / 4: the two
    keep_reset settings bitwise equal, every form against the float64 oracle at 1e-4 of the matrix scale."""
    from gpsig_amd import _lib, kernels
    from test_gpu_parity import make_kernel, make_oracle
    rng = np.random.default_rng(32 + len(base))
    ctx = _lib.context(0, 0)
    d, M = 5, 4
    for N, L, N2, L2 in ((41, 30, 17, 27), (70, 2, 9, 2), (33, 9, 8, 12)):
        X = _seqs(rng, N, L, d, 0.8).reshape(N, -1).astype(np.float32)
        Y = _seqs(rng, N2, L2, d, 0.8).reshape(N2, -1).astype(np.float32)
        kw = dict(input_dim=L * d, num_features=d, num_levels=M, base=base)
        kx, ko = make_kernel(kernels, kw), make_oracle(kw)
        want = (ko.K(X.astype(np.float64)), ko.K(X.astype(np.float64), Y.astype(np.float64)))
        for pack in (1, 2):
            for waves in (1, 4):
                got = {}
                for keep in (1, 0):
                    with _Opts(ctx, pk2=2, f32_pack=pack, f32_waves=waves, keep_reset=keep):
                        got[keep] = (kx.K(X), kx.K(X, Y, presliced=True))
                for a, b, w in zip(got[0], got[1], want):
                    assert a.dtype == np.float32 and np.array_equal(a, b), (N, L, pack, waves)
                    assert relmax(b, w) < 1e-4, (N, L, pack, waves, relmax(b, w))


# ---- sig_graded: the feature contraction's last depth piece cut into finer ones (1) or equal pieces (0) ---------------------------------------

def test_sig_graded_pieces():
    """SignatureLinear's Gram at BASELINE configs[1] (4,096 sequences of 64 x 8, 5 levels: where the graded split is taken) with sig_graded 1 and
    0: the two agree to 1e-13, sampled sub-blocks match the oracle, and with sig_graded 0 the owned row blocks of a 3-rank partition
    (gpsig_kernel_K_symm_rows) reassemble the one-call Gram bit for bit."""
    from gpsig_amd import _lib, kernels, parallel
    rng = np.random.default_rng(4096)
    n, L, d, M = 4096, 64, 8, 5
    Xh = rng.standard_normal((n, L * d))
    X = torch.as_tensor(Xh, device="cuda:0")
    kern = kernels.SignatureLinear(L * d, d, M)
    ctx = _dev_ctx()
    full = {}
    with _Opts(ctx, sig_features=1) as o:
        for g in (1, 0):
            o.set(sig_graded=g)
            full[g] = kern.K(X)
        ctx.set_pointer_mode(_lib.PTR_DEVICE)
        b = parallel.row_partition(n, 3)
        half = torch.zeros((n, n), dtype=torch.float64, device="cuda:0")
        keep = []
        p = kern._params(keep)
        for r in range(3):
            ctx.call("gpsig_kernel_K_symm_rows", p, C.c_void_p(X.data_ptr()), n, L, b[r], b[r + 1], C.c_void_p(half[b[r]:b[r + 1]].data_ptr()))
        out = torch.empty_like(half)
        ctx.check(ctx._lib.gpsig_symmetrize_owned_rows(ctx._h, _lib.F64, C.c_void_p(half.data_ptr()), n, C.c_void_p(out.data_ptr())))
        torch.cuda.synchronize()
    assert torch.equal(out, full[0])
    assert not torch.equal(full[0], full[1]), "sig_graded 0 and 1 give the same bits: the graded split did not take effect"
    f1, f0 = full[1].cpu().numpy(), full[0].cpu().numpy()
    assert relmax(f0, f1) < 1e-13, relmax(f0, f1)
    ko = O.SignatureKernelOracle(L * d, d, M, base="linear")
    for I, J in ((np.arange(6), np.arange(4090, 4096)), (rng.choice(n, 5, replace=False), rng.choice(n, 7, replace=False))):
        want = ko.K(Xh[I], Xh[J])
        assert relmax(f0[np.ix_(I, J)], want) < 1e-10 and relmax(f1[np.ix_(I, J)], want) < 1e-10


# ---- the tensor-vs-sequence reverse pass --------------------------------------------------------------------------------------------------------

def _tvs_grad_case(rng, base, M, T, N, L, d, difference, incr):
    lt = M * (M + 1) // 2
    Z = rng.standard_normal((lt, T, 2, d) if incr else (lt, T, d)) * 0.5
    X = rng.standard_normal((N, L, d)) * 0.5
    G = rng.standard_normal((M + 1, T, N))
    kt = _t_kern(base, d, M, difference=difference)
    tZ, tX = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
    (kt.K_tens_vs_seq_levels(tZ, tX, incr) * torch.tensor(G)).sum().backward()
    return Z, X, G, tZ.grad, tX.grad


def _tvs_grad(ctx, p, Z, X, G, T, N, L, incr):
    gZ, gX, gb = np.full_like(Z, np.nan), np.full_like(X, np.nan), np.zeros(2)
    ctx.call("gpsig_tens_vs_seq_levels_grad", p, _vp(Z), _vp(X), T, N, L, int(incr), _vp(G), _vp(gZ), _vp(gX), gb.ctypes.data_as(_P))
    return gZ, gX


@pytest.mark.parametrize("base", ["rbf", "linear", "matern32"])
def test_tvs_zreg_in_the_tensor_lane_gradient(base):
    """tvs_grad_lanet_kernel (tvs_grad_tile 0, first order, <= 4 levels, <= 8 columns) with the tensor components in registers (tvs_zreg 1, the
    planner's choice -1) or in LDS (0): 1, 2 and 4 levels, padded widths 4 and 8, increments on / off (lane pairs), ragged tensor counts."""
    rng = np.random.default_rng(70 + len(base))
    ctx = _host_ctx()
    for M, T, N, L, d in ((1, 5, 7, 4, 1), (2, 70, 9, 6, 4), (4, 33, 13, 9, 7), (4, 65, 4, 3, 8)):
        for difference, incr in ((True, False), (False, True), (True, True)):
            Z, X, G, wZ, wX = _tvs_grad_case(rng, base, M, T, N, L, d, difference, incr)
            keep = []
            p = _params(base, d, M, difference, keep)
            for z in (-1, 0, 1):
                with _Opts(ctx, tvs_grad_tile=0, tvs_zreg=z):
                    gZ, gX = _tvs_grad(ctx, p, Z, X, G, T, N, L, incr)
                assert rel(gZ, wZ) < 1e-9 and rel(gX, wX) < 1e-9, (z, M, d, difference, incr, rel(gZ, wZ), rel(gX, wX))


@pytest.mark.parametrize("base", ["matern12", "matern32", "matern52"])
def test_tvs_grad_matern(base):
    """The Kzx reverse pass of the Matern families: the run-time family in the reverse tile kernel (tvs_grad_matern 1, default) or the round-1
    kernels (0), 1 .. 6 levels, with and without increments, against autograd of the oracle."""
    rng = np.random.default_rng(80 + len(base))
    ctx = _host_ctx()
    for M, T, N, L, d in ((1, 9, 5, 4, 2), (2, 40, 11, 6, 3), (3, 33, 7, 5, 5), (4, 65, 6, 7, 4), (5, 20, 9, 4, 6), (6, 12, 5, 5, 3)):
        for incr in (False, True):
            Z, X, G, wZ, wX = _tvs_grad_case(rng, base, M, T, N, L, d, True, incr)
            keep = []
            p = _params(base, d, M, True, keep)
            for m in (1, 0):
                with _Opts(ctx, tvs_grad_matern=m):
                    gZ, gX = _tvs_grad(ctx, p, Z, X, G, T, N, L, incr)
                assert rel(gZ, wZ) < 1e-9 and rel(gX, wX) < 1e-9, (m, M, incr, rel(gZ, wZ), rel(gX, wX))


# ---- ho_g32: higher-order sweeps of 33 .. 64 lattice columns in 32-lane groups -------------------------------------------------------------------

@pytest.mark.parametrize("order", [2, 3, 4])
def test_ho_g32(order):
    """The higher-order reverse sweeps (grad_wave_ho_kernel.hpp) with ho_g32 -1 (rule: 32-lane groups from order 3), 0 and 1, lattices of 33 .. 64
    columns on both sides (symmetric Gram of 40 observations) and one cross case of unequal lengths (20 against 50): values and gradients against
    the oracle; the default's gradients are those of the form its rule picks, to 1e-13 (values only: see the module docstring).  The 32-lane and
    16-lane sweeps give the same bits here, so which form ran is not visible in the results: the test holds every setting to the oracle only."""
    rng = np.random.default_rng(90 + order)
    ctx = _host_ctx()
    d, M, base = 3, 4, "rbf"
    for N1, L1, N2, L2, cross in ((6, 40, 6, 40, False), (5, 20, 4, 50, True)):
        X = rng.standard_normal((N1, L1, d)) * 0.5
        Y = rng.standard_normal((N2, L2, d)) * 0.5 if cross else None
        G = rng.standard_normal((M + 1, N1, N2 if cross else N1))
        kt = _t_kern(base, d, M, difference=True, order=order)
        tX = torch.tensor(X, requires_grad=True)
        tY = torch.tensor(Y, requires_grad=True) if cross else None
        lev = kt.K_seq_levels(tX, tY)
        (lev * torch.tensor(G)).sum().backward()
        keep = []
        p = _params(base, d, M, True, keep, order=order)
        n2, l2 = (N2, L2) if cross else (N1, L1)
        res = {}
        for g in (-1, 0, 1):
            with _Opts(ctx, ho_g32=g):
                out = np.full((M + 1, N1, n2), np.nan)
                ctx.call("gpsig_seq_gram_levels", p, _vp(X), _vp(Y), N1, n2, L1, l2, _vp(out))
                gX, gY, gb = np.full_like(X, np.nan), (np.full_like(Y, np.nan) if cross else None), np.zeros(2)
                ctx.call("gpsig_seq_gram_levels_grad", p, _vp(X), _vp(Y), N1, n2, L1, l2, _vp(G), _vp(gX), _vp(gY), gb.ctypes.data_as(_P))
            assert rel(out, lev.detach()) < 1e-10, (g, rel(out, lev.detach()))
            assert rel(gX, tX.grad) < 1e-9, (g, cross, rel(gX, tX.grad))
            if cross:
                assert rel(gY, tY.grad) < 1e-9, (g, rel(gY, tY.grad))
            res[g] = gX
        picked = 1 if order >= 3 else 0
        assert relmax(res[-1], res[picked]) < 1e-13


# ---- grad_fused_piece: streamed sequences per workgroup of the backward sweep from the stash -----------------------------------------------------

@pytest.mark.parametrize("kind", ["sym", "cross"])
def test_grad_fused_piece(kind):
    """gpsig_seq_gram_levels_stash and the backward call from it (autodiff._SeqGramLevels) with grad_fused_piece 0 (16), 1, 3, 16, 17 and 64, N1 = 37
    and N2 = 19 multiples of none of them: every piece kept the stash and matches autograd of the oracle."""
    from gpsig_amd.autodiff import _SeqGramLevels, _Spec
    dev = torch.device("cuda:0")
    ctx = _dev_ctx()
    rng = np.random.default_rng(37)
    M, N1, N2, L, d, base = 4, 37, 19, 33, 5, "rbf"
    X = np.cumsum(rng.standard_normal((N1, L, d)) * 0.3, 1)
    Y = np.cumsum(rng.standard_normal((N2, L, d)) * 0.3, 1) if kind == "cross" else None
    G = rng.standard_normal((M + 1, N1, N2 if Y is not None else N1))
    kt = _t_kern(base, d, M, difference=True)
    tX = torch.tensor(X, requires_grad=True)
    tY = None if Y is None else torch.tensor(Y, requires_grad=True)
    (kt.K_seq_levels(tX, tY) * torch.tensor(G)).sum().backward()
    spec = _Spec(base, M, True, 0.0, order=1)
    for piece in (0, 1, 3, 16, 17, 64):
        with _Opts(ctx, grad_fused_piece=piece):
            Xg = torch.tensor(X, device=dev, requires_grad=True)
            Yg = None if Y is None else torch.tensor(Y, device=dev, requires_grad=True)
            lev = _SeqGramLevels.apply(Xg, Yg, None, spec)
            assert lev.grad_fn.stash is not None
            (lev * torch.tensor(G, device=dev)).sum().backward()
            torch.cuda.synchronize()
        assert rel(Xg.grad, tX.grad) < 1e-9, (piece, rel(Xg.grad, tX.grad))
        if Y is not None:
            assert rel(Yg.grad, tY.grad) < 1e-9, (piece, rel(Yg.grad, tY.grad))


# ---- low-rank mode ---------------------------------------------------------------------------------------------------------------------------------

def _lr_reverse(base, M, L, d, c, r, difference, sparsity, seed, settings):
    """Phi (the low-rank sequence features) and its reverse pass through the HIP kernels under each option setting and through the torch-op
    route (as test_gpu_grad.py::test_low_rank_sequence_features_and_their_reverse_pass)."""
    from gpsig_amd import autodiff, kernels, low_rank as lrm
    rng = np.random.default_rng(seed)
    dev = torch.device("cuda:0")
    cls = {"rbf": kernels.SignatureRBF, "linear": kernels.SignatureLinear, "matern12": kernels.SignatureMatern12, "matern32": kernels.SignatureMatern32}[base]
    kern = cls(L * d, d, M, difference=difference, lengthscales=None, low_rank=True, num_components=c, rank_bound=r, sparsity=sparsity)
    mod = autodiff.SignatureKernelModule(kern, device=dev)
    N = 37
    sk = lrm.draw_level_sketches(rng, M, c, r, sparsity)
    draw = autodiff.LowRankDraw(np.arange(c), 1e-6 * rng.random(c), sk)
    X0 = np.cumsum(0.4 * rng.standard_normal((N, L, d)), axis=1)
    S0 = 0.7 * rng.standard_normal((c, d))
    W0 = rng.standard_normal((c, c)) / np.sqrt(c)
    G0 = rng.standard_normal((N, 1 + c + (M - 1) * r))
    ctx = _dev_ctx()
    out = {}
    for key, opts in list(settings.items()) + [("torch", None)]:
        X = torch.tensor(X0, device=dev, requires_grad=True)
        S = torch.tensor(S0, device=dev, requires_grad=True)
        Wh = torch.tensor(W0, device=dev, requires_grad=True)
        mod.zero_grad()
        scope = autodiff._LowRankScope.__new__(autodiff._LowRankScope)
        scope.mod, scope.S, scope.Wh, scope._seq, scope._tens = mod, S, Wh, {}, {}
        _, _, scope.sk = draw.on(dev)
        scope.host_sketches = draw.sketches
        mod.lr_hip = opts is not None
        try:
            with _Opts(ctx, **(opts or {})):
                Phi = torch.cat(scope.seq(X), dim=1)
                (Phi * torch.tensor(G0, device=dev)).sum().backward()
                torch.cuda.synchronize()
        finally:
            mod.lr_hip = True
        out[key] = (Phi.detach().cpu().numpy(), X.grad.cpu().numpy(), S.grad.cpu().numpy(), Wh.grad.cpu().numpy())
    return out


@pytest.mark.parametrize("base,M,L,d,c,r,difference,sparsity", [("rbf", 4, 50, 6, 50, 50, True, "sqrt"), ("linear", 3, 70, 4, 12, 20, True, "log"),
                                                                ("rbf", 3, 130, 3, 16, 16, True, "sqrt"), ("matern12", 3, 2, 3, 5, 7, True, "log"),
                                                                ("matern32", 5, 33, 2, 9, 5, False, "sqrt")])
def test_lr_grad_threads(base, M, L, d, c, r, difference, sparsity):
    """lr_seq_features_grad_kernel<1024> (default) and <512> (lr_grad_threads 512) against the torch-op route: features to 1e-11, d/dX, d/dS and
    d/dWh to 1e-9; the two workgroup sizes agree with each other to 1e-12."""
    out = _lr_reverse(base, M, L, d, c, r, difference, sparsity, 1000 + M * 10 + d,
                      {1024: {"lr_grad_threads": 1024}, 512: {"lr_grad_threads": 512}})
    for t in (1024, 512):
        assert relmax(out[t][0], out["torch"][0]) < 1e-11
        for k in (1, 2, 3):
            assert relmax(out[t][k], out["torch"][k]) < 1e-9, (t, k, relmax(out[t][k], out["torch"][k]))
    for k in (1, 2, 3):
        assert relmax(out[512][k], out[1024][k]) < 1e-12, (k, relmax(out[512][k], out[1024][k]))


LR_FUSED_FORMS = [(v, pad) for v in range(4) for pad in (0, 1, 3)]


@pytest.mark.parametrize("L,c,r", [(64, 9, 5), (65, 9, 9), (66, 12, 5), (66, 9, 9)])
def test_lr_fused_variants_and_pads(L, c, r):
    """The three-array fused low-rank feature kernel (lr_fused 2) at every instance -- lr_fused_variant 0 <512, 8>, 1 <256, 4>, 2 <256, 8>,
    3 <512, 4> -- and LDS row strides lr_fused_pad 0, 1 and 3: 63, 64 and 65 time steps, ranks just past the batch widths of 4 and 8 entries.
    Forward: K, Kdiag and Kzx against the oracle's restatement given the same random objects; the instances agree to 1e-14.  Reverse
    (gpsig_lr_seq_features_dev / _grad, which take the same variant and stride): against the torch-op route at 1e-9."""
    from gpsig_amd import _lib, kernels
    from test_gpu_parity import LR_TOLS, _lr_pair
    rng = np.random.default_rng(L * 100 + c + r)
    N, d, M, T = 23, 3, 4, 7
    X = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, -1)
    Z = rng.standard_normal((M * (M + 1) // 2, T, d))
    kx, ko = _lr_pair(kernels, "rbf", L, d, M, num_components=c, rank_bound=r, sparsity="sqrt", lengthscales=0.6 + rng.random(d))
    kx.rng = np.random.default_rng(7)
    st = kx.draw_low_rank(X=X, Z=Z)
    lo = O.LowRankOracle(ko, st.landmarks, st.jitter_diag, st.sketches)
    want = (lo.K(X, return_levels=True), lo.Kdiag(X), lo.K_tens_vs_seq(Z, X))
    ctx = _lib.context(0, 0)
    got = {}
    for v, pad in LR_FUSED_FORMS:
        with _Opts(ctx, lr_fused=2, lr_fused_variant=v, lr_fused_pad=pad):
            got[(v, pad)] = (kx.K(X, lr_state=st, return_levels=True), kx.Kdiag(X, lr_state=st), kx.K_tens_vs_seq(Z, X, lr_state=st))
    for key, g in got.items():
        for a, w, a0 in zip(g, want, got[(0, 1)]):
            assert relmax(a, w) < LR_TOLS["rbf"], (key, relmax(a, w))
            assert relmax(a, a0) < 1e-14, (key, relmax(a, a0))
    out = _lr_reverse("rbf", M, L, d, c, r, True, "sqrt", L + c + r,
                      {(v, pad): {"lr_fused_variant": v, "lr_fused_pad": pad} for v, pad in LR_FUSED_FORMS})
    for key in LR_FUSED_FORMS:
        assert relmax(out[key][0], out["torch"][0]) < 1e-11 and relmax(out[key][0], out[(0, 1)][0]) < 1e-14, key
        for k in (1, 2, 3):
            assert relmax(out[key][k], out["torch"][k]) < 1e-9, (key, k, relmax(out[key][k], out["torch"][k]))


# ---- pinned_staging: host-pointer transfers through pinned bounce buffers -------------------------------------------------------------------------

def test_pinned_staging_in_host_pointer_mode():
    """Host-pointer mode on pageable NumPy memory with pinned_staging 1 (chunks of 16 MiB through two pinned buffers from 2 MiB on: staged_h2d /
    staged_d2h) and 0 (plain copies): inputs (Kdiag of 64 x 16 sequences) and outputs (K) just under 2 MiB, at 2 MiB, just over one chunk and of
    three chunks (an odd count: N = 2,100 for the output); bitwise identical to each other and to device-pointer mode.  The device-pointer calls
    go through a context on a stream of its own: the context of torch's default stream is the host-pointer one of _host_ctx (one context per
    stream), and a host pointer handed to a context left in device-pointer mode is dereferenced on the GPU."""
    from gpsig_amd import _lib, kernels
    rng = np.random.default_rng(2)
    hctx = _host_ctx()
    side = torch.cuda.Stream(torch.device("cuda:0"))
    dctx = _lib.context(0, side.cuda_stream)
    assert dctx is not hctx
    dctx.set_pointer_mode(_lib.PTR_DEVICE)
    cases = [("Kdiag", 255, 64, 16), ("Kdiag", 256, 64, 16), ("Kdiag", 2049, 64, 16), ("Kdiag", 4100, 64, 16),
             ("K", 511, 4, 2), ("K", 512, 4, 2), ("K", 1449, 4, 2), ("K", 2100, 4, 2)]
    mib = 1 << 20
    sizes = [8 * n * L * d if f == "Kdiag" else 8 * n * n for f, n, L, d in cases]
    assert sizes[0] < 2 * mib == sizes[1] and 16 * mib < sizes[2] < 17 * mib and 32 * mib < sizes[3] < 48 * mib
    assert sizes[4] < 2 * mib == sizes[5] and 16 * mib < sizes[6] < 17 * mib and 32 * mib < sizes[7] < 48 * mib
    for f, n, L, d in cases:
        X = rng.standard_normal((n, L, d)) * 0.3 / np.sqrt(d)
        kern = kernels.SignatureRBF(L * d, d, 2)
        keep = []
        p = kern._params(keep)
        shape = (n,) if f == "Kdiag" else (n, n)
        res = {}
        for pin in (1, 0):
            out = np.full(shape, np.nan)
            with _Opts(hctx, pinned_staging=pin):
                if f == "Kdiag":
                    hctx.call("gpsig_kernel_Kdiag", p, _vp(X), n, L, 0, _vp(out))
                else:
                    hctx.call("gpsig_kernel_K", p, _vp(X), None, n, n, L, L, 0, _vp(out))
            res[pin] = out
        Xd = torch.tensor(X, device="cuda:0")
        outd = torch.full(shape, float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        if f == "Kdiag":
            dctx.call("gpsig_kernel_Kdiag", p, C.c_void_p(Xd.data_ptr()), n, L, 0, C.c_void_p(outd.data_ptr()))
        else:
            dctx.call("gpsig_kernel_K", p, C.c_void_p(Xd.data_ptr()), None, n, n, L, L, 0, C.c_void_p(outd.data_ptr()))
        side.synchronize()
        assert np.isfinite(res[1]).all() and np.array_equal(res[1], res[0]) and np.array_equal(res[1], outd.cpu().numpy()), (f, n)
        I = np.array([0, 1, n // 2, n - 1])
        want = O.SignatureKernelOracle(L * d, d, 2, base="rbf").Kdiag(X[I].reshape(len(I), -1)) if f == "Kdiag" else \
            O.SignatureKernelOracle(L * d, d, 2, base="rbf").K(X[I].reshape(len(I), -1))
        assert relmax(res[1][I] if f == "Kdiag" else res[1][np.ix_(I, I)], want) < 1e-10, (f, n)


# ---- threshold edges of the automatic rules (default options) ----------------------------------------------------------------------------------

def _tvs_fwd(ctx, p, Z, X, T, N, L, incr, M):
    out = np.full((M + 1, T, N), np.nan)
    ctx.call("gpsig_tens_vs_seq_levels", p, _vp(Z), _vp(X), T, N, L, int(incr), _vp(out))
    return out


def _tvs_route_check(base, M, T, N, L, d, incr, forced, other, rng, grad=True, grad_route=True, common=None, differ=True):
    """the default call against the oracle and bitwise against the form forced by `forced` (an option dict), forward and (grad_route) reverse;
    with differ, the form of `other` (the candidate the rule declines) gives other bits in the forward pass -- else the route check could not tell
    the two apart; without, it agrees with the oracle only.  `common`: options of every call"""
    lt = M * (M + 1) // 2
    Z = rng.standard_normal((lt, T, 2, d) if incr else (lt, T, d)) * 0.5 / np.sqrt(d)
    X = _seqs(rng, N, L, d)
    ctx = _host_ctx()
    keep = []
    p = _params(base, d, M, True, keep)
    kt = _t_kern(base, d, M, difference=True)
    tZ, tX = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
    lev = kt.K_tens_vs_seq_levels(tZ, tX, incr)
    G = rng.standard_normal((M + 1, T, N))
    (lev * torch.tensor(G)).sum().backward()
    res = {}
    for key, opts in (("default", dict(common or {})), ("forced", dict(common or {}, **forced)), ("other", dict(common or {}, **other))):
        with _Opts(ctx, **opts):
            out = _tvs_fwd(ctx, p, Z, X, T, N, L, incr, M)
            g = _tvs_grad(ctx, p, Z, X, G, T, N, L, incr) if grad and key != "other" else None
        res[key] = (out, g)
    assert rel(res["default"][0], lev.detach()) < 1e-10, rel(res["default"][0], lev.detach())
    assert rel(res["other"][0], lev.detach()) < 1e-10, rel(res["other"][0], lev.detach())
    assert np.array_equal(res["default"][0], res["forced"][0]), ("default is not the forced form", forced)
    if differ:
        assert not np.array_equal(res["default"][0], res["other"][0]), ("the two candidate forms give the same bits", forced, other)
    if grad:
        assert rel(res["default"][1][0], tZ.grad) < 1e-9 and rel(res["default"][1][1], tX.grad) < 1e-9
        assert rel(res["forced"][1][0], tZ.grad) < 1e-9 and rel(res["forced"][1][1], tX.grad) < 1e-9
        if grad_route:
            assert np.array_equal(res["default"][1][0], res["forced"][1][0]) and np.array_equal(res["default"][1][1], res["forced"][1][1])
    return res


def test_threshold_wide_kzx_beyond_8_columns():
    """Kzx takes the wide route beyond 8 columns: at 8 the default is the tile kernels' result (forced: wide 0), at 9 the wide route's (wide 1),
    forward and reverse, bitwise; on both sides the declined route gives other bits (so the check can tell them apart)."""
    rng = np.random.default_rng(8)
    _tvs_route_check("rbf", 3, 40, 10, 7, 8, False, {"wide": 0}, {"wide": 1}, rng)
    _tvs_route_check("rbf", 3, 40, 10, 7, 9, False, {"wide": 1}, {"wide": 0}, rng)


def test_threshold_wide_kzz_beyond_12_columns():
    """Kzz (gpsig_tens_gram_levels) takes the wide route beyond 12 columns: the default bitwise equal to wide 0 at 12 and to wide 1 at 13, and not
    to the declined route; values against the oracle, the reverse pass (values only) against autograd of the oracle."""
    rng = np.random.default_rng(12)
    ctx = _host_ctx()
    M, T = 3, 40
    for d, forced in ((12, 0), (13, 1)):
        for incr in (False, True):
            lt = M * (M + 1) // 2
            Z = rng.standard_normal((lt, T, 2, d) if incr else (lt, T, d)) * 0.5 / np.sqrt(d)
            kt = _t_kern("rbf", d, M, difference=True)
            tZ = torch.tensor(Z, requires_grad=True)
            lev = kt.K_tens_levels(tZ, incr)
            G = rng.standard_normal(tuple(lev.shape))
            (lev * torch.tensor(G)).sum().backward()
            keep = []
            p = _params("rbf", d, M, True, keep)
            res = {}
            for key, opts in (("default", {}), ("forced", {"wide": forced}), ("other", {"wide": 1 - forced})):
                with _Opts(ctx, **opts):
                    out = np.full(tuple(lev.shape), np.nan)
                    ctx.call("gpsig_tens_gram_levels", p, _vp(Z), T, int(incr), _vp(out))
                    gZ, gb = np.full_like(Z, np.nan), np.zeros(2)
                    ctx.call("gpsig_tens_gram_levels_grad", p, _vp(Z), T, int(incr), _vp(G), _vp(gZ), gb.ctypes.data_as(_P))
                res[key] = (out, gZ)
            assert rel(res["default"][0], lev.detach()) < 1e-10 and rel(res["default"][1], tZ.grad) < 1e-9, (d, incr)
            assert np.array_equal(res["default"][0], res["forced"][0]), (d, incr)
            assert rel(res["other"][0], lev.detach()) < 1e-10 and not np.array_equal(res["default"][0], res["other"][0]), ("same bits", d, incr)


def test_threshold_tvs_tile_from_32_tensors():
    """The Kzx tile kernel from 32 tensors: 31 tensors take the default equal to tvs_tile 0, 32 equal to tvs_tile 1 (forward, bitwise).  The tile
    kernel and the lane kernels it replaces give the same bits at these shapes, so this route check cannot tell the two apart: it pins values
    (oracle) and determinism on both sides of the rule only."""
    rng = np.random.default_rng(31)
    for base, M, d in (("rbf", 3, 4), ("linear", 2, 3)):
        _tvs_route_check(base, M, 31, 9, 6, d, False, {"tvs_tile": 0}, {"tvs_tile": 1}, rng, grad=False, differ=False)
        _tvs_route_check(base, M, 32, 9, 6, d, False, {"tvs_tile": 1}, {"tvs_tile": 0}, rng, grad=False, differ=False)


def test_threshold_few_rule():
    """The `few` rule of the Kzx route (api.hip): RBF, increments, 4 < d <= 8 (wide_few_cols: the upper bound), N <= 256 take the wide route.
    Edges: d = 4 / 5 and 8, N = 256 / 257, increments off, wide_few_cols 6 at d = 6 / 7 -- the default bitwise equal to the forced form
    (wide 1 where the rule takes the wide route, wide 0 where not) and not to the declined one in the forward pass; the reverse pass has no such rule (the reverse tile kernel
    continues from the same chain totals), so it is held to the forced form bitwise only where the rule does not fire, else by values."""
    rng = np.random.default_rng(5)
    M, T, L = 2, 40, 5
    for d, N, incr, few in ((4, 20, True, False), (5, 20, True, True), (8, 256, True, True), (8, 257, True, False), (5, 20, False, False)):
        _tvs_route_check("rbf", M, T, N, L, d, incr, {"wide": 1 if few else 0}, {"wide": 0 if few else 1}, rng, grad_route=not few)
    for d, few in ((6, True), (7, False)):
        _tvs_route_check("rbf", M, T, 20, L, d, True, {"wide": 1 if few else 0}, {"wide": 0 if few else 1}, rng, grad_route=not few,
                         common={"wide_few_cols": 6})


def _lat_sampled(rng, N1, N2, L1, L2, d, M, I, J):
    """sequences and an upstream gradient that is zero outside the pairs I x J: the oracle differentiates the sub-Gram only"""
    X, Y = _seqs(rng, N1, L1, d), _seqs(rng, N2, L2, d)
    G = np.zeros((M + 1, N1, N2))
    G[:, I[:, None], J[None, :]] = rng.standard_normal((M + 1, len(I), len(J)))
    kt = _t_kern("rbf", d, M, difference=True)
    tX, tY = torch.tensor(X[I], requires_grad=True), torch.tensor(Y[J], requires_grad=True)
    lev = kt.K_seq_levels(tX, tY)
    (lev * torch.tensor(G[:, I[:, None], J[None, :]])).sum().backward()
    return X, Y, G, lev.detach().numpy(), tX.grad.numpy(), tY.grad.numpy()


def _lat_route(ctx, opts_list, p, X, Y, G, N1, N2, L1, L2, M):
    res = []
    for opts in opts_list:
        with _Opts(ctx, **opts):
            out = np.full((M + 1, N1, N2), np.nan)
            ctx.call("gpsig_seq_gram_levels", p, _vp(X), _vp(Y), N1, N2, L1, L2, _vp(out))
            gX, gY, gb = np.full_like(X, np.nan), np.full_like(Y, np.nan), np.zeros(2)
            ctx.call("gpsig_seq_gram_levels_grad", p, _vp(X), _vp(Y), N1, N2, L1, L2, _vp(G), _vp(gX), _vp(gY), gb.ctypes.data_as(_P))
        res.append((out, gX, gY))
    return res


def test_threshold_wide_o1_sweeps_at_1024_lattices():
    """The wide route's first-order reverse pass sweeps many short lattices four to a wavefront from 1,024 lattices on (wide_o1_sweeps 1): a cross
    Gram of 31 x 33 = 1,023 lattices takes the default equal to wide_o1_sweeps 0, one of 32 x 32 equal to wide_o1_sweeps 2 (bitwise, gradients
    and values; 40 columns: the wide route by default); sampled pairs against the oracle.  The two sweeps give the same bits (the per-lattice
    arithmetic is the same), so the route check cannot tell them apart: the declined form is held to 1e-12 of the default."""
    ctx = _host_ctx()
    d, M, L1, L2 = 40, 3, 6, 7
    keep = []
    p = _params("rbf", d, M, True, keep)
    for N1, N2, forced in ((31, 33, 0), (32, 32, 2)):
        rng = np.random.default_rng(N1 * N2)
        I, J = np.array([0, 5, N1 - 1]), np.array([1, N2 - 2, N2 - 1])
        X, Y, G, lev, wX, wY = _lat_sampled(rng, N1, N2, L1, L2, d, M, I, J)
        dflt, frc, other = _lat_route(ctx, [{}, {"wide_o1_sweeps": forced}, {"wide_o1_sweeps": 2 - forced}], p, X, Y, G, N1, N2, L1, L2, M)
        assert rel(dflt[0][:, I[:, None], J[None, :]], lev) < 1e-10
        assert rel(dflt[1][I], wX) < 1e-9 and rel(dflt[2][J], wY) < 1e-9
        assert not dflt[1][np.setdiff1d(np.arange(N1), I)].any()
        for a, b in zip(dflt, frc):
            assert np.array_equal(a, b), (N1, N2)
        assert rel(other[1], dflt[1]) < 1e-12 and rel(other[2], dflt[2]) < 1e-12


def test_threshold_lat_waves_at_128_lattices():
    """Lattices of more than 256 columns (8 per lane) are swept by eight wavefronts per lattice for at most 128 lattices (wide_lat_waves -1): 128
    lattices take the default equal to wide_lat_waves 1, 129 equal to wide_lat_waves 0 (bitwise, values and gradients); sampled pairs against the
    oracle.  One and eight wavefronts per lattice give the same bits, so the route check cannot tell them apart: both are held to 1e-12."""
    ctx = _host_ctx()
    d, M, L1, L2 = 40, 2, 4, 258
    keep = []
    p = _params("rbf", d, M, True, keep)
    for N1, forced in ((128, 1), (129, 0)):
        rng = np.random.default_rng(N1)
        I, J = np.array([0, 64, N1 - 1]), np.array([0])
        X, Y, G, lev, wX, wY = _lat_sampled(rng, N1, 1, L1, L2, d, M, I, J)
        dflt, frc, other = _lat_route(ctx, [{}, {"wide_lat_waves": forced}, {"wide_lat_waves": 1 - forced}], p, X, Y, G, N1, 1, L1, L2, M)
        assert rel(dflt[0][:, I[:, None], J[None, :]], lev) < 1e-10
        assert rel(dflt[1][I], wX) < 1e-9 and rel(dflt[2][J], wY) < 1e-9
        for a, b in zip(dflt, frc):
            assert np.array_equal(a, b), N1
        assert rel(other[1], dflt[1]) < 1e-12 and rel(other[2], dflt[2]) < 1e-12


@pytest.mark.parametrize("M,L1,L2,d,difference", [
    (1, 20, 17, 4, True), (2, 20, 17, 4, True), (6, 40, 37, 8, True), (7, 40, 37, 8, True),        # levels: 2 .. 6
    (2, 256, 256, 8, True), (2, 257, 257, 8, True),                                                  # column-side points at <= 8 columns: 64 x 4
    (2, 128, 128, 12, True), (2, 129, 129, 12, True),                                                # ... at 9 .. 16 columns (two per lane): 64 x 2
    (2, 40, 37, 16, True), (2, 40, 37, 17, True),                                                    # columns with differences: <= 16
    (2, 40, 37, 8, False), (2, 40, 37, 9, False)])                                                   # columns without differences: <= 8
def test_fused_reverse_kernel_edges(M, L1, L2, d, difference):
    """The first-order reverse pass of the stationary kernels in one launch (grad_impl 0: grad_fused_kernel.hpp where fused_grad_plan allows it)
    and the scratch-free wavefront kernel (grad_impl 4) on both sides of each bound of that plan: 2 .. 6 levels; at most 256 points on the
    register-resident (column) side at <= 8 padded columns, 128 at 9 .. 16 (L1 >= L2 keeps Y on that side: the plan swaps the sides only when
    X is the shorter); padded columns <= 16 with differences, <= 8 without.  Values only against autograd of the oracle (both add with atomics)."""
    rng = np.random.default_rng(M * 1000 + L1 + d)
    ctx = _host_ctx()
    N1, N2 = 3, 2
    X, Y = _seqs(rng, N1, L1, d), _seqs(rng, N2, L2, d)
    G = rng.standard_normal((M + 1, N1, N2))
    kt = _t_kern("rbf", d, M, difference=difference)
    tX, tY = torch.tensor(X, requires_grad=True), torch.tensor(Y, requires_grad=True)
    (kt.K_seq_levels(tX, tY) * torch.tensor(G)).sum().backward()
    keep = []
    p = _params("rbf", d, M, difference, keep)
    for impl in (0, 4):
        with _Opts(ctx, grad_impl=impl):
            gX, gY, gb = np.full_like(X, np.nan), np.full_like(Y, np.nan), np.zeros(2)
            ctx.call("gpsig_seq_gram_levels_grad", p, _vp(X), _vp(Y), N1, N2, L1, L2, _vp(G), _vp(gX), _vp(gY), gb.ctypes.data_as(_P))
        assert rel(gX, tX.grad) < 1e-9 and rel(gY, tY.grad) < 1e-9, (impl, rel(gX, tX.grad), rel(gY, tY.grad))
