"""The wide-state-space route (csrc/wide_api.hip, wide_kernels.hpp) for SignatureMix, kappa = p0 exp(-|z - x|^2 / 2) + (1 - p0) <z, x>: the mix kind of
the wide kernels on the distance kernels' augmented rows -- psi(a) = p0 exp(a) + (1 - p0) a of the dgemm's number, plus the one-sided half-norm terms where
they survive the differences (tests/test_wide_mix_identity.py restates which) --, and the gradient of the mixing p0 as a fixed-order sum (g_base[0]),
through the C ABI against autograd of oracle/sigkern_oracle_torch.py (p0 a leaf tensor).

Modelled test for test on tests/test_gpu_wide_poly.py, with its helpers and tolerances: values 1e-10, primitive gradients 1e-9 relative to the largest
entry, the mixing abs(gb[0] - p0.grad) < 1e-9 max(1, abs(gb[0])), module gradients 1e-8.  Data are scaled as _data does (entries ~ 1 / sqrt(d))."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sigkern_oracle_torch as OT

from test_gpu_wide import _data, _host_ctx, _vp, rel

pytestmark = pytest.mark.gpu
_P = C.POINTER(C.c_double)
DEFAULT = (0.4,)
OTHERS = [(0.05,), (0.9,), (1.0,)]


def _mix(d, M, difference, mixing, order=1):
    """(params, oracle, p0 leaf)"""
    from gpsig_amd.autodiff import _Spec
    keep = []
    p = _Spec("mix", M, difference, order=order).params(d, mixing, keep)
    p0 = torch.tensor(float(mixing), dtype=torch.float64, requires_grad=True)
    kt = OT.SignatureKernelTorchOracle(d, M, "mix", difference=difference, p0=p0, order=order)
    return p, kt, p0, keep


def _gb_ok(gb, p0):
    want = float(p0.grad)
    print("   mixing", gb[0], want)
    return abs(gb[0] - want) < 1e-9 * max(1.0, abs(gb[0]))


TVS = [(4, 70, 9, 13, 12), (3, 20, 5, 11, 28), (4, 65, 4, 17, 126), (2, 64, 7, 1, 8), (1, 5, 3, 4, 3), (4, 7, 66, 5, 300)]


@pytest.mark.parametrize("M,T,N,L,d,mixing", [s + DEFAULT for s in TVS] + [(3, 20, 5, 11, 28) + OTHERS[0]])
def test_wide_mix_tensor_vs_sequence_levels_and_gradient(M, T, N, L, d, mixing):
    """gpsig_tens_vs_seq_levels / _grad on the wide route (forced; the feature route off): tensor counts below, at and across a 64-lane block, one
    observation, one level, augmented rows of <= 16, <= 32 and more columns; differences x increments are the four rows of the table (neither one-sided
    term, the rows', the columns', both); the argument array in one chunk and in several.  gZ, gX and the mixing's gradient; the latter bit-identical
    between the chunkings and between repeated calls, gZ and gX bit-identical between repeated calls.  Beyond 64 columns (126, 300) the parent of this
    route refuses the call."""
    rng = np.random.default_rng(1000 * M + T + d)
    ctx = _host_ctx()
    ctx.set_option("wide", 1)
    ctx.set_option("tvs_features", 0)
    try:
        for difference in (True, False):
            for increments in (False, True):
                if L == 1 and difference:
                    continue
                Z, X = _data(rng, M, T, N, L, d, increments)
                G = rng.standard_normal((M + 1, T, N))
                p, kt, p0, keep = _mix(d, M, difference, mixing)
                tZ, tX = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
                want = kt.K_tens_vs_seq_levels(tZ, tX, increments)
                (want * torch.tensor(G)).sum().backward()
                bits, grads = [], []
                for mb in (0, 1, 1):
                    ctx.set_option("wide_chunk_mb", mb)
                    out = np.full((M + 1, T, N), np.nan)
                    ctx.timing_reset()
                    ctx.call("gpsig_tens_vs_seq_levels", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(out))
                    assert "wide_tvs" in str(ctx.timing_info()[0])
                    print(difference, increments, mb, "value", rel(out, want))
                    assert rel(out, want) < 1e-10, (difference, increments, mb, rel(out, want))
                    gZ, gX, gb = np.full_like(Z, np.nan), np.full_like(X, np.nan), np.full(2, np.nan)
                    ctx.call("gpsig_tens_vs_seq_levels_grad", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(G), _vp(gZ), _vp(gX), gb.ctypes.data_as(_P))
                    print(difference, increments, mb, "gradients", rel(gZ, tZ.grad), rel(gX, tX.grad))
                    assert rel(gZ, tZ.grad) < 1e-9 and rel(gX, tX.grad) < 1e-9, (difference, increments, mb, rel(gZ, tZ.grad), rel(gX, tX.grad))
                    assert _gb_ok(gb, p0), (difference, increments, mb, gb[0], float(p0.grad))
                    bits.append(gb[0])
                    grads.append((gZ, gX))
                assert bits[0] == bits[1] == bits[2], bits
                assert np.array_equal(grads[1][0], grads[2][0]) and np.array_equal(grads[1][1], grads[2][1]), (difference, increments)
    finally:
        ctx.set_option("wide", -1)
        ctx.set_option("tvs_features", -1)
        ctx.set_option("wide_chunk_mb", 0)


def test_wide_mix_weighted_sum_and_gradient():
    """gpsig_tens_vs_seq_weighted / _grad at 126 columns as the planner routes them (beyond 64 columns: the wide route): host pointers and device
    pointers, the chain totals handed over or rebuilt, increments on and off; gZ, gX, the factors' gradient and the mixing's."""
    from gpsig_amd import _lib
    M, T, N, L, d = 3, 40, 12, 6, 126
    mixing, = DEFAULT
    rng = np.random.default_rng(7 * M + T + d)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(dev)
    dctx = _lib.context(0, side.cuda_stream)
    dctx.set_pointer_mode(_lib.PTR_DEVICE)
    hctx = _host_ctx()
    ptr = lambda t_: C.c_void_p(t_.data_ptr())      # noqa: E731
    for increments in (False, True):
        Z, X = _data(rng, M, T, N, L, d, increments)
        F = rng.uniform(0.5, 1.5, (N, M + 1))
        G = rng.standard_normal((T, N))
        p, kt, p0, keep = _mix(d, M, True, mixing)
        tZ, tX, tF = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True), torch.tensor(F, requires_grad=True)
        want = (kt.K_tens_vs_seq_levels(tZ, tX, increments) * tF.t()[:, None, :]).sum(0)
        (want * torch.tensor(G)).sum().backward()
        out = np.empty((T, N))
        hctx.call("gpsig_tens_vs_seq_weighted", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(F), _vp(out), None, None)
        assert rel(out, want) < 1e-10, rel(out, want)
        gZ, gX, gF, gb = np.empty_like(Z), np.empty_like(X), np.empty_like(F), np.full(2, np.nan)
        hctx.call("gpsig_tens_vs_seq_weighted_grad", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(F), _vp(G), None, _vp(gZ), _vp(gX), _vp(gF),
                  gb.ctypes.data_as(_P))
        assert rel(gZ, tZ.grad) < 1e-9 and rel(gX, tX.grad) < 1e-9 and rel(gF, tF.grad) < 1e-9, (increments, rel(gZ, tZ.grad), rel(gX, tX.grad), rel(gF, tF.grad))
        assert _gb_ok(gb, p0), (increments, gb[0], float(p0.grad))
        dZ, dX, dF, dG = (torch.tensor(a, device=dev) for a in (Z, X, F, G))
        dgZ, dgX, dgF = torch.empty_like(dZ), torch.empty_like(dX), torch.empty_like(dF)
        aux = torch.empty(int(_lib.load().gpsig_tens_vs_seq_aux_elems(C.byref(p), T, N)), dtype=torch.float64, device=dev)
        dout, wrote = torch.empty((T, N), dtype=torch.float64, device=dev), C.c_int32(0)
        torch.cuda.synchronize()
        dctx.timing_reset()
        dctx.call("gpsig_tens_vs_seq_weighted", p, ptr(dZ), ptr(dX), T, N, L, int(increments), ptr(dF), ptr(dout), ptr(aux), C.byref(wrote))
        side.synchronize()
        assert "wide_tvs" in str(dctx.timing_info()[0])
        assert rel(dout, want) < 1e-10 and wrote.value == 1
        for use_aux in (False, True):
            dgb = torch.full((2,), float("nan"), dtype=torch.float64, device=dev)
            dctx.call("gpsig_tens_vs_seq_weighted_grad", p, ptr(dZ), ptr(dX), T, N, L, int(increments), ptr(dF), ptr(dG), ptr(aux) if use_aux else None,
                      ptr(dgZ), ptr(dgX), ptr(dgF), C.cast(dgb.data_ptr(), _P))
            side.synchronize()
            assert rel(dgZ, tZ.grad) < 1e-9 and rel(dgX, tX.grad) < 1e-9 and rel(dgF, tF.grad) < 1e-9, (use_aux, rel(dgZ, tZ.grad), rel(dgX, tX.grad))
            assert _gb_ok(dgb.cpu().numpy(), p0), (use_aux, float(dgb[0]), float(p0.grad))


@pytest.mark.parametrize("M,order,T,N,L,d,forced", [(4, 2, 70, 9, 13, 12, True), (5, 3, 40, 4, 8, 126, False)])
def test_wide_mix_higher_order_chains_and_gradient(M, order, T, N, L, d, forced):
    """The higher-order tensor-vs-sequence chains (the chain kernel's order is a run-time argument): forced at 12 columns, as routed at 126; all four
    combinations of differences and increments."""
    mixing, = DEFAULT
    rng = np.random.default_rng(10 * M + order + d)
    ctx = _host_ctx()
    if forced:
        ctx.set_option("wide", 1)
        ctx.set_option("tvs_features", 0)
    try:
        for increments in (False, True):
            for difference in (True, False):
                Z, X = _data(rng, M, T, N, L, d, increments)
                G = rng.standard_normal((M + 1, T, N))
                p, kt, p0, keep = _mix(d, M, difference, mixing, order=order)
                tZ, tX = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
                want = kt.K_tens_vs_seq_levels(tZ, tX, increments)
                (want * torch.tensor(G)).sum().backward()
                out = np.full((M + 1, T, N), np.nan)
                ctx.timing_reset()
                ctx.call("gpsig_tens_vs_seq_levels", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(out))
                assert "wide_tvs" in str(ctx.timing_info()[0])
                gZ, gX, gb = np.full_like(Z, np.nan), np.full_like(X, np.nan), np.full(2, np.nan)
                ctx.call("gpsig_tens_vs_seq_levels_grad", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(G), _vp(gZ), _vp(gX), gb.ctypes.data_as(_P))
                print(increments, difference, rel(out, want), rel(gZ, tZ.grad), rel(gX, tX.grad))
                assert rel(out, want) < 1e-10, (increments, difference, rel(out, want))
                assert rel(gZ, tZ.grad) < 1e-9 and rel(gX, tX.grad) < 1e-9, (increments, difference, rel(gZ, tZ.grad), rel(gX, tX.grad))
                assert _gb_ok(gb, p0), (increments, difference, gb[0], float(p0.grad))
    finally:
        ctx.set_option("wide", -1)
        ctx.set_option("tvs_features", -1)


LAT = [(4, 7, 5, 9, 13, 12, "cross"), (3, 6, 6, 65, 65, 40, "sym"), (3, 6, 6, 66, 66, 40, "sym"), (4, 9, 9, 33, 33, 46, "diag"), (4, 3, 3, 131, 131, 126, "diag")]


@pytest.mark.parametrize("M,N1,N2,L1,L2,d,kind,mixing", [s + DEFAULT for s in LAT] + [(4, 7, 5, 9, 13, 12, "cross") + OTHERS[1]])
def test_wide_mix_sequence_lattices_and_gradient(M, N1, N2, L1, L2, d, kind, mixing):
    """gpsig_seq_gram_levels / gpsig_seq_diag_levels and their gradients on the wide route (forced): cross, symmetric and diagonal lattices, 64 and 65
    lattice columns, differences on (no one-sided term) and off (both), the option tuples of tests/test_gpu_wide_poly.py (chunk, wavefronts per lattice,
    symmetric fold, short-lattice sweeps); gX / gY and the mixing's gradient under each.  At 126 columns also the symmetric Gram and its gradient,
    served (no test pins a refusal for SignatureMix)."""
    rng = np.random.default_rng(100 * M + L2 + d)
    ctx = _host_ctx()
    ctx.set_option("wide", 1)
    ctx.set_option("sig_features", 0)
    s = 1.0 / np.sqrt(d)
    try:
        for difference in (True, False):
            X = np.cumsum(rng.standard_normal((N1, L1, d)) * 0.5 * s, axis=1)
            Y = np.cumsum(rng.standard_normal((N2, L2, d)) * 0.5 * s, axis=1) if kind == "cross" else None
            G = rng.standard_normal((M + 1, N1) if kind == "diag" else (M + 1, N1, N2 if kind == "cross" else N1))
            p, kt, p0, keep = _mix(d, M, difference, mixing)
            tX = torch.tensor(X, requires_grad=True)
            tY = None if Y is None else torch.tensor(Y, requires_grad=True)
            want = kt.K_seq_diag_levels(tX) if kind == "diag" else kt.K_seq_levels(tX, tY)
            (want * torch.tensor(G)).sum().backward()
            for mb, waves, fold, o1 in ((0, -1, 1, 1), (1, -1, 1, 1), (1, -1, 1, 2), (0, 0, 1, 0), (0, 1, 1, 1)) + (((0, -1, 0, 2), (0, -1, 0, 0)) if kind == "sym" else ()):
                ctx.set_option("wide_chunk_mb", mb)
                ctx.set_option("wide_lat_waves", waves)
                ctx.set_option("wide_sym_fold", fold)
                ctx.set_option("wide_o1_sweeps", o1)
                out = np.full(G.shape, np.nan)
                gX, gY, gb = np.full_like(X, np.nan), (None if Y is None else np.full_like(Y, np.nan)), np.full(2, np.nan)
                ctx.timing_reset()
                if kind == "diag":
                    ctx.call("gpsig_seq_diag_levels", p, _vp(X), N1, L1, _vp(out))
                    assert "wide_lattice" in str(ctx.timing_info()[0])
                    ctx.call("gpsig_seq_diag_levels_grad", p, _vp(X), N1, L1, _vp(G), _vp(gX), gb.ctypes.data_as(_P))
                else:
                    n2, l2 = (N2, L2) if Y is not None else (N1, L1)
                    ctx.call("gpsig_seq_gram_levels", p, _vp(X), _vp(Y), N1, n2, L1, l2, _vp(out))
                    assert "wide_lattice" in str(ctx.timing_info()[0])
                    ctx.call("gpsig_seq_gram_levels_grad", p, _vp(X), _vp(Y), N1, n2, L1, l2, _vp(G), _vp(gX), _vp(gY), gb.ctypes.data_as(_P))
                print(difference, mb, waves, fold, o1, rel(out, want), rel(gX, tX.grad), None if Y is None else rel(gY, tY.grad))
                assert rel(out, want) < 1e-10, (difference, mb, waves, o1, rel(out, want))
                assert rel(gX, tX.grad) < 1e-9, (difference, mb, waves, o1, rel(gX, tX.grad))
                if Y is not None:
                    assert rel(gY, tY.grad) < 1e-9, (difference, mb, waves, o1, rel(gY, tY.grad))
                assert _gb_ok(gb, p0), (difference, mb, waves, fold, o1, gb[0], float(p0.grad))
            if d > 64:        # the symmetric Gram and its gradient beyond 64 columns
                Gs = rng.standard_normal((M + 1, N1, N1))
                p, kt, p0, keep = _mix(d, M, difference, mixing)
                tX = torch.tensor(X, requires_grad=True)
                want = kt.K_seq_levels(tX, None)
                (want * torch.tensor(Gs)).sum().backward()
                out, gX, gb = np.full((M + 1, N1, N1), np.nan), np.full_like(X, np.nan), np.full(2, np.nan)
                ctx.call("gpsig_seq_gram_levels", p, _vp(X), None, N1, N1, L1, L1, _vp(out))
                assert rel(out, want) < 1e-10
                ctx.call("gpsig_seq_gram_levels_grad", p, _vp(X), None, N1, N1, L1, L1, _vp(Gs), _vp(gX), None, gb.ctypes.data_as(_P))
                assert rel(gX, tX.grad) < 1e-9, (difference, rel(gX, tX.grad))
                assert _gb_ok(gb, p0), (difference, gb[0], float(p0.grad))
    finally:
        ctx.set_option("wide", -1)
        ctx.set_option("sig_features", -1)
        ctx.set_option("wide_chunk_mb", 0)
        ctx.set_option("wide_lat_waves", -1)
        ctx.set_option("wide_sym_fold", 1)
        ctx.set_option("wide_o1_sweeps", 1)


def test_wide_mix_order_two_lattice_gradients_stay_refused():
    """Order > 1 sequence lattices of SignatureMix are not on the wide route: beyond 64 columns (70) the C ABI's gradients refuse them as before."""
    M, N, L, d = 3, 3, 6, 70
    rng = np.random.default_rng(70)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.5 / np.sqrt(d), axis=1)
    p, kt, p0, keep = _mix(d, M, True, DEFAULT[0], order=2)
    ctx = _host_ctx()
    gX = np.empty_like(X)
    with pytest.raises(NotImplementedError):
        ctx.call("gpsig_seq_diag_levels_grad", p, _vp(X), N, L, _vp(rng.standard_normal((M + 1, N))), _vp(gX), None)
    with pytest.raises(NotImplementedError):
        ctx.call("gpsig_seq_gram_levels_grad", p, _vp(X), None, N, N, L, L, _vp(rng.standard_normal((M + 1, N, N))), _vp(gX), None, None)


@pytest.mark.parametrize("M,T,d,mixing", [s + DEFAULT for s in [(4, 70, 46), (3, 33, 126), (1, 5, 3), (4, 64, 300)]] + [(3, 33, 126) + OTHERS[2]])
def test_wide_mix_tensor_gram_levels_and_gradient(M, T, d, mixing):
    """gpsig_tens_gram_levels / _grad on the wide route (forced): increments on (no one-sided term) and off (both); gZ and the mixing's gradient, the
    same bits from two calls.  Tensor counts below, at and across a 64-lane block (the padded rows and columns add nothing)."""
    rng = np.random.default_rng(10 * M + T + d)
    ctx = _host_ctx()
    ctx.set_option("wide", 1)
    lt = M * (M + 1) // 2
    try:
        for increments in (False, True):
            Z = rng.standard_normal((lt, T, 2, d) if increments else (lt, T, d)) / np.sqrt(d)
            G = rng.standard_normal((M + 1, T, T))
            p, kt, p0, keep = _mix(d, M, True, mixing)
            tZ = torch.tensor(Z, requires_grad=True)
            want = kt.K_tens_levels(tZ, increments)
            (want * torch.tensor(G)).sum().backward()
            out = np.full((M + 1, T, T), np.nan)
            ctx.timing_reset()
            ctx.call("gpsig_tens_gram_levels", p, _vp(Z), T, int(increments), _vp(out))
            assert "wide_tens" in str(ctx.timing_info()[0])
            assert rel(out, want) < 1e-10, (increments, rel(out, want))
            bits = []
            for _ in range(2):
                gZ, gb = np.full_like(Z, np.nan), np.full(2, np.nan)
                ctx.call("gpsig_tens_gram_levels_grad", p, _vp(Z), T, int(increments), _vp(G), _vp(gZ), gb.ctypes.data_as(_P))
                print(increments, rel(gZ, tZ.grad))
                assert rel(gZ, tZ.grad) < 1e-9, (increments, rel(gZ, tZ.grad))
                assert _gb_ok(gb, p0), (increments, gb[0], float(p0.grad))
                bits.append((gb[0], gZ))
            assert bits[0][0] == bits[1][0] and np.array_equal(bits[0][1], bits[1][1]), (bits[0][0], bits[1][0])
    finally:
        ctx.set_option("wide", -1)


def test_wide_mix_route():
    """kernels.SignatureMix at 46 and 126 columns: the library's timing record names the wide kernels for Kzx, the level diagonals and Kzz at 126
    columns and none of them at 46 (no change of route up to 64 columns).  Beyond 64 columns a first-order module sends all four primitives to the
    library; at order 2 Kzx and Kzz, while the level diagonals and the sequence Grams keep the matrix route."""
    from gpsig_amd import _lib, autodiff, kernels
    rng = np.random.default_rng(3)
    dev = torch.device("cuda:0")
    for d, wide in ((46, False), (126, True)):
        M_, T_, N_, L_ = 4, 64, 6, 12
        kern = kernels.SignatureMix(L_ * d, d, M_, lengthscales=np.sqrt(d), normalization=False)
        Xr = torch.tensor(np.cumsum(rng.standard_normal((N_, L_, d)) * 0.3, axis=1).reshape(N_, -1), device=dev)
        Zr = torch.tensor(rng.standard_normal((M_ * (M_ + 1) // 2, T_, 2, d)), device=dev)
        rctx = _lib.context(0, torch.cuda.current_stream(dev).cuda_stream)
        for call, name in ((lambda: kern.K_tens_vs_seq(Zr, Xr, increments=True), "wide_tvs"), (lambda: kern.Kdiag(Xr, return_levels=True), "wide_lattice"),
                           (lambda: kern.K_tens(Zr, increments=True), "wide_tens")):
            rctx.timing_reset()
            call()
            got = rctx.timing_info()[0]
            assert (name in str(got)) == wide, (d, name, got)
    L, d, M = 6, 126, 3
    mod = autodiff.SignatureKernelModule(kernels.SignatureMix(L * d, d, M), device="cuda:0")
    assert not mod._mx("tvs") and not mod._mx("diag", L) and not mod._mx("tens") and not mod._mx("seq", L)
    mod = autodiff.SignatureKernelModule(kernels.SignatureMix(L * d, d, M, order=2), device="cuda:0")
    assert not mod._mx("tvs") and not mod._mx("tens") and mod._mx("diag", L) and mod._mx("seq", L)
    mod = autodiff.SignatureKernelModule(kernels.SignatureMix(L * 46, 46, M), device="cuda:0")
    assert not mod._mx("tvs")


@pytest.mark.parametrize("d", [126, 150])
def test_wide_mix_evaluation_path_against_the_oracle(d):
    """kernels.SignatureMix (scaling by lengthscales, variances, normalisation on / off) at 126 and 150 columns against the NumPy oracle: K, K(X, X2),
    Kdiag, K_tens, K_tens_vs_seq (sum and levels), K_tens_n_seq_covs."""
    from gpsig_amd import kernels
    import test_gpu_parity as P
    mixing, = DEFAULT
    rng = np.random.default_rng(31 + d)
    M, T, N, N2, L = 4, 70, 9, 5, 8
    lt = M * (M + 1) // 2
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.4, axis=1).reshape(N, -1)
    X2 = np.cumsum(rng.standard_normal((N2, L, d)) * 0.4, axis=1).reshape(N2, -1)
    Z = rng.standard_normal((lt, T, 2, d)) * 0.7
    ls = rng.uniform(0.8, 1.6, d) * np.sqrt(d)
    var = rng.uniform(0.5, 1.5, M + 1)
    for normalization in (True, False):
        kw = dict(base="mix", input_dim=L * d, num_features=d, num_levels=M, lengthscales=ls, variances=var, normalization=normalization,
                  base_params=dict(mixing=mixing))
        k, ko = P.make_kernel(kernels, kw), P.make_oracle(kw)
        pairs = [("K", k.K(X), ko.K(X)), ("K(X, X2)", k.K(X, X2), ko.K(X, X2)), ("Kdiag", k.Kdiag(X), ko.Kdiag(X)),
                 ("K_tens", k.K_tens(Z, increments=True), ko.K_tens(Z, increments=True)),
                 ("K_tens_vs_seq", k.K_tens_vs_seq(Z, X, increments=True), ko.K_tens_vs_seq(Z, X, increments=True))]
        gl = k.K_tens_vs_seq(Z, X, increments=True, return_levels=True)
        wl = ko.K_tens_vs_seq(Z, X, increments=True, return_levels=True)
        pairs += [("K_tens_vs_seq level %d" % i, a, b) for i, (a, b) in enumerate(zip(gl, wl)) if i >= 1]
        pairs += [("K_tens_n_seq_covs[%d]" % i, a, b) for i, (a, b) in
                  enumerate(zip(k.K_tens_n_seq_covs(Z, X, increments=True), ko.K_tens_n_seq_covs(Z, X, increments=True)))]
        for name, a, b in pairs:
            print(d, normalization, name, rel(a, b))
            assert rel(a, b) < 1e-10, (normalization, name, rel(a, b))


@pytest.mark.parametrize("d", [80, 150])
def test_wide_mix_module_gradients(d):
    """autodiff.SignatureKernelModule.K_tens_n_seq_covs at 80 and 150 columns: values and the gradients with respect to the inducing tensors, the
    lengthscales and the mixing (raw_p0, through its transform) against autograd of the differentiable oracle; the library's timing record names wide
    kernels (the matrix route would leave none)."""
    from gpsig_amd import _lib, autodiff, kernels
    import test_gpu_parity as P
    mixing, = DEFAULT
    rng = np.random.default_rng(5 + d)
    M, T, N, L = 4, 40, 7, 9
    lt = M * (M + 1) // 2
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.4, axis=1).reshape(N, -1)
    Z = rng.standard_normal((lt, T, 2, d)) * 0.7
    ls = rng.uniform(0.8, 1.6, d) * np.sqrt(d)
    kw = dict(base="mix", input_dim=L * d, num_features=d, num_levels=M, lengthscales=ls, base_params=dict(mixing=mixing))
    kern = P.make_kernel(kernels, kw)
    mod = autodiff.SignatureKernelModule(kern, device="cuda:0")
    Zg = torch.tensor(Z, device="cuda:0", requires_grad=True)
    Wt = [rng.standard_normal(s) for s in ((T, T), (T, N), (N,))]
    ctx = _lib.context(0, torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
    ctx.timing_reset()
    outs = mod.K_tens_n_seq_covs(Zg, torch.tensor(X, device="cuda:0"), increments=True)
    assert "wide_" in str(ctx.timing_info()[0]), ctx.timing_info()[0]
    sum((o * torch.tensor(w, device="cuda:0")).sum() for o, w in zip(outs, Wt)).backward()
    lsr = torch.tensor(ls, requires_grad=True)
    p0 = mod.p0.detach().cpu().clone().requires_grad_(True)
    orc = OT.SignatureKernelTorchOracle(d, M, "mix", lengthscales=lsr, p0=p0)
    Zc = torch.tensor(Z, requires_grad=True)
    wants = orc.K_tens_n_seq_covs(Zc, torch.tensor(X), increments=True)
    sum((o * torch.tensor(w)).sum() for o, w in zip(wants, Wt)).backward()
    for o, w in zip(outs, wants):
        assert rel(o, w) < 1e-10, rel(o, w)
    assert rel(Zg.grad, Zc.grad) < 1e-8, rel(Zg.grad, Zc.grad)
    sig = lambda r: torch.sigmoid(r.detach().cpu())      # noqa: E731
    assert rel(mod.raw_lengthscales.grad, lsr.grad * sig(mod.raw_lengthscales)) < 1e-8
    got, want = float(mod.raw_p0.grad), float(p0.grad * sig(mod.raw_p0))
    print(d, "raw_p0.grad", got, want)
    assert abs(got - want) < 1e-8 * max(1.0, abs(want)), (got, want)
