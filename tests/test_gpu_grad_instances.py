"""Every reachable compiled instance of the sequence-gradient sweeps (stored lattice, scratch-free, scratch-free with Lam out, higher order) through
gpsig_seq_gram_levels_grad / gpsig_seq_diag_levels_grad against autograd of the float64 oracle.

The cases are tests/grad_instance_cases.py; tests/test_grad_plan_host.py proves on the CPU, from csrc/grad_plan.hpp, which instance each case
runs, and that the emulated per-pair recursion reproduces the oracle to 1e-11 on the same data.  One test per kernel family and lane shape.
gX and gY: finite and within the case's tolerance (1e-9) of the oracle, relative to the oracle's largest entry; SignaturePoly / SignatureMix:
g_base[0] within 1e-9 max(1, |g|).  Outputs are pre-filled with NaN; options are set through _Opts, which restores the ctx.hpp defaults."""
import time

import numpy as np
import pytest
import torch

import grad_instance_cases as T
from test_gpu_grad import _P, _host_ctx, _params, _t_kern, _vp
from test_gpu_kernel_forms import _Opts, relmax

pytestmark = pytest.mark.gpu

GROUPS = ["wave-16x2", "wave-16x4", "wave-64x2", "wave-64x4", "wave-64x8",
          "wave2-16x2", "wave2-16x4", "wave2-64x2", "wave2-64x8",
          "lam_rbf-16x2", "lam_rbf-16x4", "lam_rbf-64x2", "lam_rbf-64x4", "lam_rbf-64x8",
          "lam_gen-16x2", "lam_gen-16x4", "lam_gen-64x2", "lam_gen-64x4", "lam_gen-64x8",
          "ho_undo-16x2", "ho_undo-16x4", "ho_undo-32x2", "ho_undo-64x2", "ho_undo-64x4", "ho_undo-64x8",
          "ho_slot-16x2", "ho_slot-16x4", "ho_slot-64x2", "ho_slot-64x4", "ho_slot-64x8"]


def cases_of(group):
    return [i for i, c in enumerate(T.CASES) if T.group(c) == group]


def run_case(ctx, i, **options):
    """-> error of gX, of gY (None unless a cross Gram), of g_base[0] (None unless poly / mix) of case i, under its own options unless given"""
    case = T.CASES[i]
    X, Y, G = T.data(i)
    N1, N2 = T.sizes(case)
    kt = _t_kern(case.base, case.d, case.num_levels, difference=case.difference, order=case.order)
    tX = torch.tensor(X, requires_grad=True)
    tY = None if Y is None else torch.tensor(Y, requires_grad=True)
    lev = kt.K_seq_diag_levels(tX) if case.kind == "diag" else kt.K_seq_levels(tX, tY)
    (lev * torch.tensor(G)).sum().backward()
    keep = []
    p = _params(case.base, case.d, case.num_levels, case.difference, keep, order=case.order)
    gX, gY, gb = np.full_like(X, np.nan), (None if Y is None else np.full_like(Y, np.nan)), np.full(2, np.nan)
    with _Opts(ctx, **(options or dict(case.options))):
        if case.kind == "diag":
            ctx.call("gpsig_seq_diag_levels_grad", p, _vp(X), N1, case.L1, _vp(G), _vp(gX), gb.ctypes.data_as(_P))
        else:
            ctx.call("gpsig_seq_gram_levels_grad", p, _vp(X), _vp(Y), N1, N2, case.L1, case.L2, _vp(G), _vp(gX), _vp(gY), gb.ctypes.data_as(_P))
    eb = None
    if case.base in ("poly", "mix"):
        want = kt.p0.grad.item()
        eb = abs(gb[0] - want) / max(1.0, abs(want)) if np.isfinite(gb[0]) else np.inf
    return relmax(gX, tX.grad.numpy()), (None if Y is None else relmax(gY, tY.grad.numpy())), eb


@pytest.mark.parametrize("group", GROUPS)
def test_every_compiled_sweep_instance_against_the_oracle(group):
    """A finding of these cases, fixed with them: `lam 2 rbf 64 4 4 7r` (SignatureRBF without differences, num_levels 7, a 5 x 193 lattice) came
    out at gX 1.05e-9 / gY 1.53e-9, and every lattice with fewer rows than kept levels between 1e-11 and 1e-10.  WaveUndo::step
    (csrc/grad_wave_core.hpp) read the undone Q_m[a-1][b-1] where no level-m chain exists yet (a < m or b < m): exactly zero in the recursion,
    but in the sweep the rounding left over from undoing the last row's Q (1e-16 of 1e9), multiplied by U_{m+1}.  seq_lam_undo_kernel now passes
    its row and column, and those entries are exact zeros: 8.6e-15 / 1.5e-14 (profiles/grad_instances.txt)."""
    ctx = _host_ctx()
    t0 = time.perf_counter()
    worst, failed = [0.0, 0.0, 0.0], []
    for i in cases_of(group):
        errs = run_case(ctx, i)
        for k, e in enumerate(errs):
            if e is not None:
                worst[k] = max(worst[k], e)
        print("case %d %s: gX %.2e gY %s g_base %s" % (i, T.CASES[i].expected, errs[0], "-" if errs[1] is None else "%.2e" % errs[1],
                                                      "-" if errs[2] is None else "%.2e" % errs[2]))
        if not (errs[0] < T.CASES[i].tol and (errs[1] is None or errs[1] < T.CASES[i].tol) and (errs[2] is None or errs[2] < 1e-9)):
            failed.append((i, T.CASES[i], errs))
    print("group %s: %d cases, worst gX %.2e gY %.2e g_base %.2e, %.2f s" % (group, len(cases_of(group)), worst[0], worst[1], worst[2],
                                                                            time.perf_counter() - t0))
    assert not failed, failed[:5]
