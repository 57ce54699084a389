"""An empty batch through the reverse entry points of the low-rank training path (csrc/lr_grad_api.hip): with N = 0 sequences (T = 0 tensors)
every sum over the batch is an exact zero -- dS, dWh and the base kernel's parameter (SignatureSpectral: dalpha, domega, dgamma) -- whatever the
output buffers held, and the call returns OK (Context.call raises otherwise).  Raw calls, as the _raw_calls helpers of the other low-rank suites."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CC, D, L, M, Q = 8, 3, 9, 3, 2                          # c = r = 8

# entry point -> (SignatureSpectral's, takes lengths, inducing tensors)
ENTRIES = {
    "gpsig_lr_seq_features_grad": (False, False, False),
    "gpsig_lr_seq_features_ragged_grad": (False, True, False),
    "gpsig_lr_seq_features_spectral_grad": (True, False, False),
    "gpsig_lr_seq_features_spectral_ragged_grad": (True, True, False),
    "gpsig_lr_tens_features_grad": (False, False, True),
    "gpsig_lr_tens_features_spectral_grad": (True, False, True),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_empty_batch_gives_exact_zeros(entry):
    from gpsig_amd import kernels, autodiff
    spectral, ragged, tens = ENTRIES[entry]
    kw = dict(low_rank=True, num_components=CC, rank_bound=CC)
    kern = kernels.SignatureSpectral(L * D, D, M, family="mixed", Q=Q, **kw) if spectral else kernels.SignatureRBF(L * D, D, M, **kw)
    kern.rng = np.random.default_rng(1)
    mod = autodiff.SignatureKernelModule(kern, device=DEV)
    sketches = mod.draw_low_rank(2 * CC + 4).sketches
    r = int(sketches[0].r)
    keep = []
    p = mod._spec.params(D, float(Q) if spectral else 1.0, keep)
    if spectral:
        p.base_params[1] = float(autodiff._SPECTRAL_FAMILY["mixed"])
    arr = autodiff._sketch_array(sketches, keep)
    rng = np.random.default_rng(2)
    new = lambda *shape: torch.tensor(rng.uniform(0.5, 1.0, shape), device=DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    ptr = autodiff._ptr
    pts = new(M * (M + 1) // 2, 0, 2, D) if tens else new(0, L, D)          # no tensors / no sequences
    S, Wh, dPhi, g_pts = new(CC, D), new(CC, CC), new(0, 1 + CC + (M - 1) * r), torch.empty_like(pts)
    gS, gWh = nan(CC, D), nan(CC, CC)
    args = [ptr(pts), 0, 1 if tens else L] + ([None] if ragged else []) + [ptr(S), ptr(Wh)]
    if spectral:
        params, outs = [new(Q), new(Q, D), new(Q, D)], [nan(Q), nan(Q, D), nan(Q, D)]
        args += [ptr(t) for t in params] + [ptr(dPhi), ptr(g_pts), ptr(gS), ptr(gWh)] + [ptr(t) for t in outs]
    else:
        outs = [nan(2)]                                                     # the library writes g_base[0]
        args += [ptr(dPhi), ptr(g_pts), ptr(gS), ptr(gWh), C.cast(outs[0].data_ptr(), C.POINTER(C.c_double))]
    autodiff._ctx_for(S).call(entry, p, CC, r, len(sketches), arr, *args)
    torch.cuda.synchronize()
    assert bool((gS == 0).all()) and bool((gWh == 0).all())
    if spectral:
        assert all(bool((t == 0).all()) for t in outs)
    else:
        assert float(outs[0][0]) == 0.0
