"""The wide-state-space route (csrc/wide_api.hip, wide_kernels.hpp) for the two dot-product families, SignatureLinear and SignatureCosine: the
identity kind of the wide kernels (kappa = the number the dgemm yields) on plain rows -- increments where the kernel takes differences -- and on unit
rows, through the C ABI and the Python layers against the oracles.

Helpers and tolerances are those of tests/test_gpu_wide.py: values 1e-10, primitive gradients 1e-9, module gradients 1e-8, relative to the largest
entry, values against oracle/sigkern_oracle.py, gradients against autograd of oracle/sigkern_oracle_torch.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sigkern_oracle_torch as OT

from test_gpu_wide import _data, _host_ctx, _params, _vp, rel

pytestmark = pytest.mark.gpu
_P = C.POINTER(C.c_double)
BASES = ["linear", "cosine"]


@pytest.mark.parametrize("M,T,N,L,d", [(4, 70, 9, 13, 12), (3, 20, 5, 11, 28), (3, 20, 5, 11, 46), (4, 65, 4, 17, 126), (2, 64, 7, 1, 8), (1, 5, 3, 4, 3),
                                       (4, 7, 66, 5, 300)])
@pytest.mark.parametrize("base", BASES)
def test_wide_linear_tensor_vs_sequence_levels_and_gradient(M, T, N, L, d, base):
    """gpsig_tens_vs_seq_levels / _grad on the wide route (forced; the feature route off): tensor counts across a 64-lane block, one observation, one
    level, the three forms of the reverse pass's contraction (augmented rows of 14, 30 and more than 32 columns), differences x increments, the argument
    array in one chunk and in several.  Beyond 64 columns (126, 300) the parent of this route refuses the call."""
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
                kt = OT.SignatureKernelTorchOracle(d, M, base, difference=difference)
                tZ, tX = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
                want = kt.K_tens_vs_seq_levels(tZ, tX, increments)
                (want * torch.tensor(G)).sum().backward()
                keep = []
                p = _params(base, d, M, difference, keep)
                for mb in (0, 1):
                    ctx.set_option("wide_chunk_mb", mb)
                    out = np.full((M + 1, T, N), np.nan)
                    ctx.call("gpsig_tens_vs_seq_levels", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(out))
                    print(base, difference, increments, mb, "value", rel(out, want))
                    assert rel(out, want) < 1e-10, (difference, increments, mb, rel(out, want))
                    gZ, gX, gb = np.full_like(Z, np.nan), np.full_like(X, np.nan), np.zeros(2)
                    ctx.call("gpsig_tens_vs_seq_levels_grad", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(G), _vp(gZ), _vp(gX), gb.ctypes.data_as(_P))
                    print(base, difference, increments, mb, "gradients", rel(gZ, tZ.grad), rel(gX, tX.grad))
                    assert rel(gZ, tZ.grad) < 1e-9 and rel(gX, tX.grad) < 1e-9, (difference, increments, mb, rel(gZ, tZ.grad), rel(gX, tX.grad))
    finally:
        ctx.set_option("wide", -1)
        ctx.set_option("tvs_features", -1)
        ctx.set_option("wide_chunk_mb", 0)


@pytest.mark.parametrize("M,T,N,L,d", [(4, 70, 45, 9, 46), (3, 40, 12, 6, 126)])
@pytest.mark.parametrize("base", BASES)
def test_wide_linear_weighted_sum_and_gradient(base, M, T, N, L, d):
    """gpsig_tens_vs_seq_weighted / _grad as the planner routes them (beyond 32 columns: the wide route): the level sum inside the kernel, the chain
    totals handed from the forward to the reverse call (device pointers) or rebuilt by it, gradients with respect to Z, X and the factors."""
    from gpsig_amd import _lib
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
        kt = OT.SignatureKernelTorchOracle(d, M, base)
        tZ, tX, tF = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True), torch.tensor(F, requires_grad=True)
        want = (kt.K_tens_vs_seq_levels(tZ, tX, increments) * tF.t()[:, None, :]).sum(0)
        (want * torch.tensor(G)).sum().backward()
        keep = []
        p = _params(base, d, M, True, keep)
        out = np.empty((T, N))
        hctx.call("gpsig_tens_vs_seq_weighted", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(F), _vp(out), None, None)
        assert rel(out, want) < 1e-10, rel(out, want)
        gZ, gX, gF, gb = np.empty_like(Z), np.empty_like(X), np.empty_like(F), np.zeros(2)
        hctx.call("gpsig_tens_vs_seq_weighted_grad", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(F), _vp(G), None, _vp(gZ), _vp(gX), _vp(gF),
                  gb.ctypes.data_as(_P))
        assert rel(gZ, tZ.grad) < 1e-9 and rel(gX, tX.grad) < 1e-9 and rel(gF, tF.grad) < 1e-9, (increments, rel(gZ, tZ.grad), rel(gX, tX.grad), rel(gF, tF.grad))
        dZ, dX, dF, dG = (torch.tensor(a, device=dev) for a in (Z, X, F, G))
        dgZ, dgX, dgF, dgb = torch.empty_like(dZ), torch.empty_like(dX), torch.empty_like(dF), torch.zeros(2, dtype=torch.float64, device=dev)
        aux = torch.empty(int(_lib.load().gpsig_tens_vs_seq_aux_elems(C.byref(p), T, N)), dtype=torch.float64, device=dev)
        dout, wrote = torch.empty((T, N), dtype=torch.float64, device=dev), C.c_int32(0)
        torch.cuda.synchronize()
        dctx.timing_reset()
        dctx.call("gpsig_tens_vs_seq_weighted", p, ptr(dZ), ptr(dX), T, N, L, int(increments), ptr(dF), ptr(dout), ptr(aux), C.byref(wrote))
        side.synchronize()
        assert "wide_tvs" in str(dctx.timing_info()[0])
        assert rel(dout, want) < 1e-10 and wrote.value == 1
        for use_aux in (False, True):
            dctx.call("gpsig_tens_vs_seq_weighted_grad", p, ptr(dZ), ptr(dX), T, N, L, int(increments), ptr(dF), ptr(dG), ptr(aux) if use_aux else None,
                      ptr(dgZ), ptr(dgX), ptr(dgF), C.cast(dgb.data_ptr(), _P))
            side.synchronize()
            assert rel(dgZ, tZ.grad) < 1e-9 and rel(dgX, tX.grad) < 1e-9 and rel(dgF, tF.grad) < 1e-9, (use_aux, rel(dgZ, tZ.grad), rel(dgX, tX.grad))


@pytest.mark.parametrize("M,order,T,N,L,d", [(4, 2, 70, 9, 13, 46), (5, 3, 40, 4, 8, 126)])
@pytest.mark.parametrize("base", BASES)
def test_wide_linear_higher_order_chains_and_gradient(M, order, T, N, L, d, base):
    """The higher-order tensor-vs-sequence chains (the chain kernel's order is a run-time argument) of the two families beyond 32 columns, as the
    planner routes them: values and gradients."""
    from gpsig_amd.autodiff import _Spec
    rng = np.random.default_rng(10 * M + order + d)
    ctx = _host_ctx()
    for increments in (False, True):
        for difference in (True, False):
            Z, X = _data(rng, M, T, N, L, d, increments)
            G = rng.standard_normal((M + 1, T, N))
            kt = OT.SignatureKernelTorchOracle(d, M, base, difference=difference, order=order)
            tZ, tX = torch.tensor(Z, requires_grad=True), torch.tensor(X, requires_grad=True)
            want = kt.K_tens_vs_seq_levels(tZ, tX, increments)
            (want * torch.tensor(G)).sum().backward()
            keep = []
            p = _Spec(base, M, difference, 0.0, order=order).params(d, 0.0, keep)
            out = np.full((M + 1, T, N), np.nan)
            ctx.timing_reset()
            ctx.call("gpsig_tens_vs_seq_levels", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(out))
            assert "wide_tvs" in str(ctx.timing_info()[0])
            gZ, gX, gb = np.full_like(Z, np.nan), np.full_like(X, np.nan), np.zeros(2)
            ctx.call("gpsig_tens_vs_seq_levels_grad", p, _vp(Z), _vp(X), T, N, L, int(increments), _vp(G), _vp(gZ), _vp(gX), gb.ctypes.data_as(_P))
            assert rel(out, want) < 1e-10, (increments, difference, rel(out, want))
            assert rel(gZ, tZ.grad) < 1e-9 and rel(gX, tX.grad) < 1e-9, (increments, difference, rel(gZ, tZ.grad), rel(gX, tX.grad))


@pytest.mark.parametrize("M,N1,N2,L1,L2,d,kind", [(4, 7, 5, 9, 13, 12, "cross"), (3, 6, 6, 65, 65, 40, "sym"), (3, 6, 6, 66, 66, 40, "sym"), (4, 9, 9, 33, 33, 46, "diag"),
                                                  (4, 3, 4, 20, 131, 126, "cross")])
@pytest.mark.parametrize("base", BASES)
def test_wide_linear_sequence_lattices_and_gradient(M, N1, N2, L1, L2, d, kind, base):
    """gpsig_seq_gram_levels / gpsig_seq_diag_levels and their gradients on the wide route (forced; the feature contraction off): cross, symmetric and
    diagonal lattices, 64 and 65 lattice columns (one and two columns per lane), differences on / off, the lattices in one chunk and in several, several
    wavefronts per lattice, the symmetric fold on / off, the short-lattice sweeps on / off."""
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
            kt = OT.SignatureKernelTorchOracle(d, M, base, difference=difference)
            tX = torch.tensor(X, requires_grad=True)
            tY = None if Y is None else torch.tensor(Y, requires_grad=True)
            want = kt.K_seq_diag_levels(tX) if kind == "diag" else kt.K_seq_levels(tX, tY)
            (want * torch.tensor(G)).sum().backward()
            keep = []
            p = _params(base, d, M, difference, keep)
            # (chunk MB, wavefronts per lattice, symmetric fold, short-lattice sweeps: as tests/test_gpu_wide.py)
            for mb, waves, fold, o1 in ((0, -1, 1, 1), (1, -1, 1, 2), (0, 0, 1, 0), (0, 1, 1, 1)) + (((0, -1, 0, 2), (0, -1, 0, 0)) if kind == "sym" else ()):
                ctx.set_option("wide_chunk_mb", mb)
                ctx.set_option("wide_lat_waves", waves)
                ctx.set_option("wide_sym_fold", fold)
                ctx.set_option("wide_o1_sweeps", o1)
                out = np.full(G.shape, np.nan)
                gX, gY, gb = np.full_like(X, np.nan), (None if Y is None else np.full_like(Y, np.nan)), np.zeros(2)
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
                print(base, difference, mb, waves, fold, o1, rel(out, want), rel(gX, tX.grad), None if Y is None else rel(gY, tY.grad))
                assert rel(out, want) < 1e-10, (difference, mb, waves, o1, rel(out, want))
                assert rel(gX, tX.grad) < 1e-9, (difference, mb, waves, o1, rel(gX, tX.grad))
                if Y is not None:
                    assert rel(gY, tY.grad) < 1e-9, (difference, mb, waves, o1, rel(gY, tY.grad))
    finally:
        ctx.set_option("wide", -1)
        ctx.set_option("sig_features", -1)
        ctx.set_option("wide_chunk_mb", 0)
        ctx.set_option("wide_lat_waves", -1)
        ctx.set_option("wide_sym_fold", 1)
        ctx.set_option("wide_o1_sweeps", 1)


@pytest.mark.parametrize("M,T,d", [(4, 70, 46), (3, 33, 126), (1, 5, 3), (4, 64, 300)])
@pytest.mark.parametrize("base", BASES)
def test_wide_linear_tensor_gram_levels_and_gradient(M, T, d, base):
    """gpsig_tens_gram_levels / _grad on the wide route (forced): increments on / off -- SignatureLinear's collapse to z^1 - z^0 on both sides,
    SignatureCosine's four-term difference."""
    rng = np.random.default_rng(10 * M + T + d)
    ctx = _host_ctx()
    ctx.set_option("wide", 1)
    lt = M * (M + 1) // 2
    try:
        for increments in (False, True):
            Z = rng.standard_normal((lt, T, 2, d) if increments else (lt, T, d)) / np.sqrt(d)
            G = rng.standard_normal((M + 1, T, T))
            kt = OT.SignatureKernelTorchOracle(d, M, base)
            tZ = torch.tensor(Z, requires_grad=True)
            want = kt.K_tens_levels(tZ, increments)
            (want * torch.tensor(G)).sum().backward()
            keep = []
            p = _params(base, d, M, True, keep)
            out, gZ, gb = np.full((M + 1, T, T), np.nan), np.full_like(Z, np.nan), np.zeros(2)
            ctx.timing_reset()
            ctx.call("gpsig_tens_gram_levels", p, _vp(Z), T, int(increments), _vp(out))
            assert "wide_tens" in str(ctx.timing_info()[0])
            ctx.call("gpsig_tens_gram_levels_grad", p, _vp(Z), T, int(increments), _vp(G), _vp(gZ), gb.ctypes.data_as(_P))
            assert rel(out, want) < 1e-10, (increments, rel(out, want))
            assert rel(gZ, tZ.grad) < 1e-9, (increments, rel(gZ, tZ.grad))
    finally:
        ctx.set_option("wide", -1)


def test_wide_linear_is_translation_invariant_to_rounding():
    """SignatureLinear with differences at 46 columns: the wide route takes the differences on the rows before the dgemm (increments of the sequences,
    z^1 - z^0 of the tensors), so paths shifted by 1e3 give the levels of the unshifted ones to rounding: within 1e-9 of the largest entry.  (In
    NumPy at (d, L) = (46, 11), (126, 17), (12, 40), 4 levels: the increment form stays within 5e-12, a four-term difference of inner products is off by
    2e-8 .. 4e-7 -- the bound holds the design, not just the values.)"""
    rng = np.random.default_rng(46)
    M, T, N, L, d = 4, 20, 6, 11, 46
    ctx = _host_ctx()
    ctx.set_option("wide", 1)
    ctx.set_option("sig_features", 0)
    ctx.set_option("tvs_features", 0)
    try:
        keep = []
        p = _params("linear", d, M, True, keep)
        Z, X = _data(rng, M, T, N, L, d, True)
        outs = []
        for shift in (0.0, 1e3):
            Zs, Xs = Z + shift, X + shift
            kzx, kxx = np.full((M + 1, T, N), np.nan), np.full((M + 1, N, N), np.nan)
            ctx.timing_reset()
            ctx.call("gpsig_tens_vs_seq_levels", p, _vp(Zs), _vp(Xs), T, N, L, 1, _vp(kzx))
            assert "wide_tvs" in str(ctx.timing_info()[0])
            ctx.timing_reset()
            ctx.call("gpsig_seq_gram_levels", p, _vp(Xs), None, N, N, L, L, _vp(kxx))
            assert "wide_lattice" in str(ctx.timing_info()[0])
            outs.append((kzx, kxx))
        for name, a, b in (("Kzx", outs[1][0], outs[0][0]), ("Kxx", outs[1][1], outs[0][1])):
            print(name, "shifted vs unshifted", rel(a, b))
            assert rel(a, b) < 1e-9, (name, rel(a, b))
    finally:
        ctx.set_option("wide", -1)
        ctx.set_option("sig_features", -1)
        ctx.set_option("tvs_features", -1)


def test_wide_linear_route_is_what_wide_state_spaces_take():
    """SignatureLinear / SignatureCosine with num_lags = 1 at 46 and 126 columns: the library's timing record names the wide kernels for Kzx, the level
    diagonals and Kzz; at 28 columns none of them (no change of route up to 32 columns)."""
    from gpsig_amd import _lib, kernels
    rng = np.random.default_rng(3)
    M, T, N, L = 4, 64, 6, 12
    lt = M * (M + 1) // 2
    dev = torch.device("cuda:0")
    for cls in (kernels.SignatureLinear, kernels.SignatureCosine):
        for d, wide in ((14, False), (23, True), (63, True)):
            kern = cls(L * d, d, M, lengthscales=np.sqrt(d), num_lags=1, normalization=False)
            X = torch.tensor(np.cumsum(rng.standard_normal((N, L, d)) * 0.3, axis=1).reshape(N, -1), device=dev)
            Z = torch.tensor(rng.standard_normal((lt, T, 2, 2 * d)), device=dev)
            ctx = _lib.context(0, torch.cuda.current_stream(dev).cuda_stream)
            for call, name in ((lambda: kern.K_tens_vs_seq(Z, X, increments=True), "wide_tvs"), (lambda: kern.Kdiag(X, return_levels=True), "wide_lattice"),
                               (lambda: kern.K_tens(Z, increments=True), "wide_tens")):
                ctx.timing_reset()
                call()
                got = ctx.timing_info()[0]
                assert (name in str(got)) == wide, (cls.__name__, d, name, got)


@pytest.mark.parametrize("d,num_lags", [(23, 1), (63, 1), (150, 0)])
@pytest.mark.parametrize("base", BASES)
def test_wide_linear_evaluation_path_against_the_oracle(base, d, num_lags):
    """kernels.SignatureLinear / SignatureCosine (scaling by lengthscales, lags, lag weights, variances, normalisation on / off) at 46, 126 and 150
    columns against the NumPy oracle: K, K(X, X2), Kdiag, K_tens, K_tens_vs_seq (sum and levels), K_tens_n_seq_covs."""
    from gpsig_amd import kernels
    import test_gpu_parity as P
    rng = np.random.default_rng(31 + d)
    M, T, N, N2, L = 4, 70, 9, 5, 8
    lt = M * (M + 1) // 2
    de = d * (num_lags + 1)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.4, axis=1).reshape(N, -1)
    X2 = np.cumsum(rng.standard_normal((N2, L, d)) * 0.4, axis=1).reshape(N2, -1)
    Z = rng.standard_normal((lt, T, 2, de)) * 0.7
    ls = rng.uniform(0.8, 1.6, d) * np.sqrt(d)
    var = rng.uniform(0.5, 1.5, M + 1)
    for normalization in (True, False):
        kw = dict(base=base, input_dim=L * d, num_features=d, num_levels=M, lengthscales=ls, variances=var, normalization=normalization,
                  num_lags=num_lags or None)
        k, ko = P.make_kernel(kernels, kw), P.make_oracle(kw)
        if num_lags:
            k.lags = ko.lags = np.array([0.23])
            k.gamma = ko.gamma = np.array([0.6, 0.45])
        pairs = [("K", k.K(X), ko.K(X)), ("K(X, X2)", k.K(X, X2), ko.K(X, X2)), ("Kdiag", k.Kdiag(X), ko.Kdiag(X)),
                 ("K_tens", k.K_tens(Z, increments=True), ko.K_tens(Z, increments=True)),
                 ("K_tens_vs_seq", k.K_tens_vs_seq(Z, X, increments=True), ko.K_tens_vs_seq(Z, X, increments=True))]
        gl = k.K_tens_vs_seq(Z, X, increments=True, return_levels=True)
        wl = ko.K_tens_vs_seq(Z, X, increments=True, return_levels=True)
        pairs += [("K_tens_vs_seq level %d" % i, a, b) for i, (a, b) in enumerate(zip(gl, wl)) if i >= 1]
        pairs += [("K_tens_n_seq_covs[%d]" % i, a, b) for i, (a, b) in
                  enumerate(zip(k.K_tens_n_seq_covs(Z, X, increments=True), ko.K_tens_n_seq_covs(Z, X, increments=True)))]
        for name, a, b in pairs:
            print(base, d, normalization, name, rel(a, b))
            assert rel(a, b) < 1e-10, (normalization, name, rel(a, b))


@pytest.mark.parametrize("d,num_lags", [(23, 1), (40, 1), (150, 0)])
@pytest.mark.parametrize("base", BASES)
def test_wide_linear_module_gradients(base, d, num_lags):
    """autodiff.SignatureKernelModule.K_tens_n_seq_covs at 46, 80 and 150 columns: values and the gradients with respect to the inducing tensors,
    lengthscales, lags and lag weights against autograd of the differentiable oracle; beyond 64 columns the library's timing record names wide
    kernels (the matrix route would leave none)."""
    from gpsig_amd import _lib, autodiff, kernels
    import test_gpu_parity as P
    rng = np.random.default_rng(5 + d)
    M, T, N, L = 4, 40, 7, 9
    lt = M * (M + 1) // 2
    de = d * (num_lags + 1)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.4, axis=1).reshape(N, -1)
    Z = rng.standard_normal((lt, T, 2, de)) * 0.7
    ls = rng.uniform(0.8, 1.6, d) * np.sqrt(d)
    kw = dict(base=base, input_dim=L * d, num_features=d, num_levels=M, lengthscales=ls, num_lags=num_lags or None)
    kern = P.make_kernel(kernels, kw)
    mod = autodiff.SignatureKernelModule(kern, device="cuda:0")
    Zg = torch.tensor(Z, device="cuda:0", requires_grad=True)
    Wt = [rng.standard_normal(s) for s in ((T, T), (T, N), (N,))]
    ctx = _lib.context(0, torch.cuda.current_stream(torch.device("cuda:0")).cuda_stream)
    ctx.timing_reset()
    outs = mod.K_tens_n_seq_covs(Zg, torch.tensor(X, device="cuda:0"), increments=True)
    if de > 64:
        assert "wide_" in str(ctx.timing_info()[0]), ctx.timing_info()[0]
    sum((o * torch.tensor(w, device="cuda:0")).sum() for o, w in zip(outs, Wt)).backward()
    lsr = torch.tensor(ls, requires_grad=True)
    okw = dict(lengthscales=lsr)
    if num_lags:
        lagr, gamr = mod.lags.detach().cpu().clone().requires_grad_(True), mod.gamma.detach().cpu().clone().requires_grad_(True)
        okw.update(num_lags=num_lags, lags=lagr, gamma=gamr)
    orc = OT.SignatureKernelTorchOracle(d, M, base, **okw)
    Zc = torch.tensor(Z, requires_grad=True)
    wants = orc.K_tens_n_seq_covs(Zc, torch.tensor(X), increments=True)
    sum((o * torch.tensor(w)).sum() for o, w in zip(wants, Wt)).backward()
    for o, w in zip(outs, wants):
        assert rel(o, w) < 1e-10, rel(o, w)
    assert rel(Zg.grad, Zc.grad) < 1e-8, rel(Zg.grad, Zc.grad)
    sig = lambda r: torch.sigmoid(r.detach().cpu())      # noqa: E731
    assert rel(mod.raw_lengthscales.grad, lsr.grad * sig(mod.raw_lengthscales)) < 1e-8
    if num_lags:
        lg = mod.lags.detach().cpu()
        assert rel(mod.raw_lags.grad, lagr.grad * lg * (1 - lg)) < 1e-8
        assert rel(mod.raw_gamma.grad, gamr.grad * sig(mod.raw_gamma)) < 1e-8


@pytest.mark.parametrize("base", BASES)
def test_wide_linear_order_two_at_70_columns_is_still_served(base):
    """Order 2 on the sequence lattices beyond 64 columns is not on the wide route for these families: the module keeps the matrix route for K and
    Kdiag (the library would answer "d too large"), and agrees with the oracle."""
    from gpsig_amd import autodiff, kernels
    import test_gpu_parity as P
    rng = np.random.default_rng(70)
    M, N, L, d = 3, 6, 8, 70
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.4, axis=1).reshape(N, -1)
    ls = rng.uniform(0.8, 1.6, d) * np.sqrt(d)
    kw = dict(base=base, input_dim=L * d, num_features=d, num_levels=M, lengthscales=ls, order=2)
    mod = autodiff.SignatureKernelModule(P.make_kernel(kernels, kw), device="cuda:0")
    orc = OT.SignatureKernelTorchOracle(d, M, base, lengthscales=torch.tensor(ls), order=2)
    Xg = torch.tensor(X, device="cuda:0")
    assert rel(mod.K(Xg), orc.K(torch.tensor(X))) < 1e-10
    assert rel(mod.Kdiag(Xg), orc.Kdiag(torch.tensor(X))) < 1e-10
