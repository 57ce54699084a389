"""Which compiled instance of the sequence-gradient sweeps a call runs (csrc/grad_plan.hpp), without a GPU: the plan as a stand-alone host program
under the address and undefined-behaviour sanitizers, against the case table of tests/grad_instance_cases.py; and the conditioning of the table's
data: the per-pair CPU emulator against autograd of the float64 oracle."""
import os
import subprocess

import numpy as np
import pytest
import torch

import grad_instance_cases as T
from emu_grad_util import seq_grad
from oracle import sigkern_oracle_torch as OT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsig_amd", "csrc")
FAMILIES = {"wave": 84, "wave2": 56, "lam": 224, "ho_undo": 54, "ho_slot": 15}        # compiled instances per kernel (the issue's table)


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grad_plan") / "test_grad_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "test_grad_plan.cpp")])
    return exe


def _run(exe, mode, stdin=""):
    res = subprocess.run([exe, mode], input=stdin.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, (res.stdout.decode()[-2000:], res.stderr.decode()[-2000:])
    return res.stdout.decode().splitlines()


def test_every_case_reaches_the_instance_it_names(plan_exe):
    got = _run(plan_exe, "plan", "".join(T.plan_query(c) + "\n" for c in T.CASES))
    assert len(got) == len(T.CASES)
    wrong = [(i, c.expected, g) for i, (c, g) in enumerate(zip(T.CASES, got)) if (g if c.family == "wave2" else g.split(" | ")[0]) != c.expected]
    assert not wrong, wrong[:10]


def test_cases_and_unreachable_are_exactly_the_compiled_list(plan_exe):
    compiled = _run(plan_exe, "list")
    assert len(compiled) == len(set(compiled)) == sum(FAMILIES.values())
    for fam, n in FAMILIES.items():
        assert sum(1 for s in compiled if s.split()[0] == fam) == n, fam
    reached = set(i for c in T.CASES for i in T.instances(c))
    assert not reached & set(T.UNREACHABLE), sorted(reached & set(T.UNREACHABLE))
    assert reached | set(T.UNREACHABLE) == set(compiled), (sorted(set(compiled) - reached - set(T.UNREACHABLE))[:10],
                                                           sorted((reached | set(T.UNREACHABLE)) - set(compiled))[:10])
    assert all(reason.strip() for reason in T.UNREACHABLE.values())


def test_no_plan_leaves_the_compiled_list(plan_exe):
    """every plan over R <= 520, DP 4 / 8 / 16, num_levels <= 8, orders <= 4, every grad_impl and ho_g32; and the unreachable instances are
    never planned there either"""
    bad, plans = _run(plan_exe, "sweep")[-1].split()
    assert int(bad) == 0 and int(plans) > 1000000
    queries = ["wave2 0 %d %d %d %d %d" % (R1, R2, DP, M, one) for DP in (4, 8, 16) for M in (1, 2, 4, 5, 7, 8) for one in (0, 1)
               for R1 in (1, 33, 65, 129, 257, 512) for R2 in range(1, 521, 3 if one == 0 else 600)]
    got = set(i for line in _run(plan_exe, "plan", "\n".join(queries) + "\n") for i in line.split(" | "))
    assert not got & set(T.UNREACHABLE)


def test_the_gpu_tests_consume_every_case():
    import test_gpu_grad_instances as G
    assert len(G.GROUPS) == len(set(G.GROUPS))
    taken = [i for g in G.GROUPS for i in G.cases_of(g)]
    assert sorted(taken) == list(range(len(T.CASES)))
    assert all(G.cases_of(g) for g in G.GROUPS)
    # only the 64 x 8 forms (257 .. 512 lattice columns) may carry the contract's tolerance
    for c in T.CASES:
        assert c.tol == T.TOL or (c.tol == T.TOL_CONTRACT and T.group(c).endswith("64x8")), c


def test_table_covers_what_it_promises():
    """every run-time kind meets every lane shape in the gen Lam-out kernels; every padded width with live padding; both ends of every range"""
    kinds = {}
    for c in T.CASES:
        if c.family == "lam" and " gen " in c.expected:
            kinds.setdefault(T.group(c), set()).add((c.base, c.difference))
    assert len(kinds) == 5
    for g, have in kinds.items():
        assert have >= set((k, True) for k in T.GEN_KINDS) | set((k, False) for k in T.GEN_KINDS + ["linear"]), (g, have)
    dr = lambda c: 1 if c.difference else 0
    for fam in ("wave", "lam", "ho"):
        sides = set(c.L2 - dr(c) for c in T.CASES if c.family == fam and c.kind == "cross")
        assert sides >= {32, 33, 64, 65, 128, 129, 256, 257, 512}, (fam, sorted(sides))
    sides = set(max(c.L1, c.L2) - 1 for c in T.CASES if c.family == "wave2" and c.d == 3)
    assert sides >= {32, 33, 64, 65, 128, 129, 512}, sorted(sides)
    assert all(c.kind == "cross" or T.sizes(c) == (5, 5) for c in T.CASES)
    for fam in ("wave", "wave2", "lam"):
        assert {1, 8} <= set(c.num_levels for c in T.CASES if c.family == fam)


def _oracle(case, X, Y, G):
    p0, p1 = (1.0, 3.0) if case.base == "poly" else ((0.4, 0.0) if case.base == "mix" else (0.0, 0.0))
    kt = OT.SignatureKernelTorchOracle(case.d, case.num_levels, case.base, p0=torch.tensor(p0, dtype=torch.float64, requires_grad=True), p1=p1,
                                       difference=case.difference, order=case.order)
    tX = torch.tensor(X, requires_grad=True)
    tY = None if Y is None else torch.tensor(Y, requires_grad=True)
    lev = kt.K_seq_diag_levels(tX) if case.kind == "diag" else kt.K_seq_levels(tX, tY)
    (lev * torch.tensor(G)).sum().backward()
    return tX.grad.numpy(), (None if Y is None else tY.grad.numpy()), (kt.p0.grad.item() if case.base in ("poly", "mix") else None), (p0, p1)


def _rel(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@pytest.mark.parametrize("family", ["wave", "wave2", "lam"])
def test_first_order_cases_are_well_conditioned(family):
    """The per-pair emulator (tests/emu/emu_grad.cpp: the stored-lattice recursion of grad_core.hpp) agrees with autograd of the oracle to 1e-11
    on every first-order case's own data -- gX, gY and the base-parameter gradient: what the GPU test then measures at 1e-9 is the kernel,
    not the data."""
    worst = 0.0
    for i, case in enumerate(T.CASES):
        if case.family != family:
            continue
        X, Y, G = T.data(i)
        wX, wY, wb, (p0, p1) = _oracle(case, X, Y, G)
        _, gX, gY, gb = seq_grad(X, Y, G, case.num_levels, case.base, case.difference, p0=p0, p1=p1, diag=case.kind == "diag")
        errs = [_rel(gX, wX)] + ([] if Y is None else [_rel(gY, wY)]) + ([] if wb is None else [abs(gb - wb) / max(1.0, abs(wb))])
        worst = max(worst, *errs)
        assert max(errs) < 1e-11, (i, case, errs)
    print(family, "worst emulator-vs-oracle error", worst)


def test_undo_sweep_emulated_on_the_lam_out_cases():
    """The sweep of seq_lam_undo_kernel undoes its forward recursion instead of storing it.  Its CPU emulation (the same grad_wave_core.hpp code,
    lane shape and level count as the case's instance; padded widths 4 and 8) on every Lam-out case's data, against autograd of the oracle: inside
    the contract's 1e-6 everywhere, and it prints the worst figure per lane shape -- what the GPU test then finds.  (Before WaveUndo::step
    zeroed the states of levels that have no chain yet, a 5 x 193 lattice at 7 levels without differences gave 1.6e-9 here as on the GPU;
    now 1.6e-14.)"""
    from emu_grad_util import seq_grad_wave
    worst = {}
    for i, case in enumerate(T.CASES):
        if case.family != "lam" or case.d > 8:
            continue
        X, Y, G = T.data(i)
        wX, wY, _, (p0, p1) = _oracle(case, X, Y, G)
        words = case.expected.split()
        gX, gY, _ = seq_grad_wave(X, Y, G, case.num_levels, case.base, case.difference, p0=p0, p1=p1, diag=case.kind == "diag",
                                  group=int(words[3]), cols=int(words[4]), scratch_free="lam")
        err = max([_rel(gX, wX)] + ([] if Y is None else [_rel(gY, wY)]))
        assert err < 1e-6, (i, case, err)
        key = T.group(case)
        if err > worst.get(key, (0.0, None))[0]:
            worst[key] = (err, i)
    for key, (err, i) in sorted(worst.items()):
        print("undo sweep emulated, %s: worst %.2e (case %d, %s)" % (key, err, i, T.CASES[i].expected))
