"""One case per reachable compiled instance of the sequence-gradient sweeps (csrc/grad_plan.hpp lists them and plans them), and per end of its
range.  A plain module, no tests in it: tests/test_grad_plan_host.py proves on the CPU that every case reaches the instance it names and that the
cases together with UNREACHABLE are exactly the compiled list; tests/test_gpu_grad_instances.py runs every case against autograd of the oracle.

The cases are built from the instances -- for each compiled (family, lane shape, padded width, level variant) a lattice side inside the shape's
range -- while the plan goes the other way, from a call's sizes to an instance: the CPU test compares the two.

Instance names, as tests/emu/test_grad_plan.cpp prints them (variant: levels kept, c = at compile time, r = at run time; mode: 0 increments of
the linear kernel, 1 points with differences, 2 points without):
    wave <mode> <G> <C> <DP> <variant>            seq_grad_wave_kernel (stored lattice), option grad_impl = 3
    wave2 <G> <C> <DP> <variant>                  seq_grad_wave2_kernel, grad_impl = 4, linear with differences; a call names "x side | y side"
    lam <mode> <rbf|gen> <G> <C> <DP> <variant>   seq_lam_undo_kernel, grad_impl = 4, every other kernel
    ho_undo <G> <C> <num_levels> <order>          seq_grad_wave_ho_undo_kernel, grad_impl = 0, wide = 0
    ho_slot <G> <C> <order>                       seq_grad_wave_ho_kernel, grad_impl = 3, wide = 0
"""
import collections
import itertools

import numpy as np

Case = collections.namedtuple("Case", "family base difference order num_levels d L1 L2 kind options expected scale tol")

# lattice columns each lane shape (G, C) holds: first .. last
RANGE = {(16, 2): (1, 32), (16, 4): (33, 64), (32, 2): (33, 64), (64, 2): (65, 128), (64, 4): (129, 256), (64, 8): (257, 512)}
LANE_SHAPES = [(16, 2), (16, 4), (64, 2), (64, 4), (64, 8)]
WIDTHS = {4: 3, 8: 7, 16: 13}                       # padded columns DP -> d with live padding
LEVELS = {"3c": 4, "4c": 5, "4r": 2, "7r": 7}       # level variant -> num_levels
GEN_KINDS = ["cosine", "poly", "mix", "matern12", "matern32", "matern52"]       # base kernel at run time; without differences also linear
TOL, TOL_CONTRACT = 1e-9, 1e-6


def _compiled(G, C, DP):
    return not ((G, C) == (64, 8) and DP == 16)      # GPSIG_WAVE_SHAPES


def _mode(base, difference):
    return 2 if not difference else (0 if base == "linear" else 1)


def _opts(base, **kw):
    o = dict(kw)
    if base in ("linear", "cosine"):
        o["sig_features_grad"] = 0                   # the lattice kernels, whatever the time model says
    return tuple(sorted(o.items()))


def _case(family, base, difference, order, M, d, plan_len, other, kind, options, expected, swap=False, scale=0.4, tol=TOL):
    dr = 1 if difference else 0
    if kind == "cross":
        L1, L2 = other, plan_len + dr
        if swap:
            L1, L2 = L2, L1
    else:
        L1 = L2 = plan_len + dr
    return Case(family, base, difference, order, M, d, L1, L2, kind, options, expected, scale, tol)


def _ends(shape, n):
    """n lattice sides inside the shape's range, the two ends first"""
    first, last = RANGE[shape]
    picks = [first, last, (first + last) // 2 + 1, last - 1]
    return [picks[i % 4] for i in range(n)]


def _scale(base, difference, R):
    """Step of the random walks.  Without differences the lattice holds the kernel of the points themselves, and the walks wander: the unbounded
    kernels (linear, poly, mix) get short steps on long lattices so that the level sums stay within what float64 adds up to 1e-11."""
    if difference or base not in ("linear", "poly", "mix"):
        return 0.4
    return 0.4 if R <= 32 else (0.1 if R <= 128 else 0.03)


def _wave_cases():
    """stored lattice: 14 shapes x 2 level variants x 3 lattice modes"""
    out = []
    bases = {0: itertools.cycle(["linear"]), 1: itertools.cycle(["rbf"] + GEN_KINDS), 2: itertools.cycle(["linear", "rbf"] + GEN_KINDS)}
    other = itertools.cycle([5, 19])
    for (G, C) in LANE_SHAPES:
        for DP in (4, 8, 16):
            if not _compiled(G, C, DP):
                continue
            lens = iter(_ends((G, C), 6))
            for mode in (0, 1, 2):
                for variant, M in (("4r", 5 if mode == 1 else 2), ("7r", 7)):
                    base = next(bases[mode])
                    R = next(lens)
                    out.append(_case("wave", base, mode != 2, 1, M, WIDTHS[DP], R, next(other), "cross", _opts(base, grad_impl=3),
                                     "wave %d %d %d %d %s" % (mode, G, C, DP, variant), scale=_scale(base, mode != 2, R)))
        # one symmetric Gram and one diagonal per lane shape
        first = RANGE[(G, C)][0]
        out.append(_case("wave", "poly", True, 1, 4, 3, first, 0, "sym", _opts("poly", grad_impl=3), "wave 1 %d %d 4 4r" % (G, C)))
        out.append(_case("wave", "linear", True, 1, 3, 7, first + 2, 0, "diag", _opts("linear", grad_impl=3), "wave 0 %d %d 8 4r" % (G, C)))
    # num_levels 1 and 8, and d = DP (no padding columns)
    out.append(_case("wave", "mix", True, 1, 1, 3, 9, 5, "cross", _opts("mix", grad_impl=3), "wave 1 16 2 4 4r"))
    out.append(_case("wave", "rbf", False, 1, 8, 7, 40, 5, "cross", _opts("rbf", grad_impl=3), "wave 2 16 4 8 7r"))
    out.append(_case("wave", "matern32", True, 1, 4, 16, 70, 19, "cross", _opts("matern32", grad_impl=3), "wave 1 64 2 16 4r"))
    out.append(_case("wave", "linear", True, 1, 6, 4, 300, 5, "cross", _opts("linear", grad_impl=3), "wave 0 64 8 4 7r"))
    out.append(_case("wave", "matern52", True, 1, 6, 3, 20, 19, "cross", _opts("matern52", grad_impl=3), "wave 1 16 2 4 7r"))      # the first num_levels of 7r
    return out


def _wave2_shapes(DP):
    """the lane shapes wave2_plan lists, with their ranges at this width: (64, 4) is not listed, C * DP > 32 is skipped"""
    out, prev = [], 0
    for (G, C) in ((16, 2), (16, 4), (64, 2), (64, 8)):
        if C * DP > 32 or not _compiled(G, C, DP):
            continue
        out.append(((G, C), prev + 1, RANGE[(G, C)][1]))
        prev = RANGE[(G, C)][1]
    return out


def _wave2_lds(G, R1, M):
    return 8 * (64 // G) * max(R1, 1) * (3 if M - 1 == 3 else (4 if M - 1 <= 4 else 7))


def _wave2_cases():
    """scratch-free, linear with differences: a cross Gram plans both sides -- the long side on the lanes of one launch, the short one on those
    of the other (always the (16, 2) instance of the same width and variant), each streaming the other side's row totals through LDS.  Where the
    long side's row totals would not fit the LDS of four pairs per wavefront, the other side has 65 increments (one pair per wavefront)."""
    out = []
    swap = itertools.cycle([False, True])
    other = itertools.cycle([5, 19])
    opts = _opts("linear", grad_impl=4)
    for DP in (4, 8, 16):
        for (G, C), first, last in _wave2_shapes(DP):
            lens = [first, last, (first + last) // 2 + 1, last - 1]
            for (variant, M), R in zip(LEVELS.items(), lens):
                oth = next(other)
                short = (16, 2)
                if _wave2_lds(16, R, M) > 64 * 1024:
                    oth, short = 66, (64, 2)
                mine, theirs = "wave2 %d %d %d %s" % (G, C, DP, variant), "wave2 %d %d %d %s" % (short[0], short[1], DP, variant)
                sw = next(swap)
                out.append(_case("wave2", "linear", True, 1, M, WIDTHS[DP], R, oth, "cross", opts, (mine + " | " + theirs) if sw else (theirs + " | " + mine), swap=sw))
    for DP, shape_first in ((4, _wave2_shapes(4)), (8, _wave2_shapes(8))):
        for (G, C), first, last in shape_first:
            if DP == 8 and (G, C) != (16, 4):
                continue
            name = "wave2 %d %d %d " % (G, C, DP)
            out.append(_case("wave2", "linear", True, 1, 4, WIDTHS[DP], first, 0, "sym", opts, name + "3c | " + name + "3c"))
            out.append(_case("wave2", "linear", True, 1, 7, WIDTHS[DP], first + 2, 0, "diag", opts, name + "7r | " + name + "7r"))
    out.append(_case("wave2", "linear", True, 1, 1, 3, 9, 5, "cross", opts, "wave2 16 2 4 4r | wave2 16 2 4 4r"))
    out.append(_case("wave2", "linear", True, 1, 8, 7, 40, 5, "cross", opts, "wave2 16 2 8 7r | wave2 16 4 8 7r"))
    # the last num_levels of the 4-level run-time variant and the first of the 7-level one
    out.append(_case("wave2", "linear", True, 1, 3, 3, 20, 5, "cross", opts, "wave2 16 2 4 4r | wave2 16 2 4 4r"))
    out.append(_case("wave2", "linear", True, 1, 6, 7, 50, 19, "cross", opts, "wave2 16 2 8 7r | wave2 16 4 8 7r"))
    out.append(_case("wave2", "linear", True, 1, 5, 16, 100, 19, "cross", opts, "wave2 16 2 16 4c | wave2 64 2 16 4c"))
    out.append(_case("wave2", "linear", True, 1, 4, 4, 512, 19, "cross", opts, "wave2 16 2 4 3c | wave2 64 8 4 3c"))
    return out


def _lam_cases():
    """scratch-free with Lam out: 14 shapes x 4 level variants x 2 modes x (RBF at compile time / the base kernel at run time)"""
    out = []
    other = itertools.cycle([5, 19])
    for (G, C) in LANE_SHAPES:
        # every run-time kind meets every lane shape: the rotation starts over per lane shape
        kinds = {1: itertools.cycle(GEN_KINDS), 2: itertools.cycle(["linear"] + GEN_KINDS)}
        for DP in (4, 8, 16):
            if not _compiled(G, C, DP):
                continue
            lens = iter(_ends((G, C), 16))
            for mode in (1, 2):
                for variant, M in LEVELS.items():
                    for rbf in (True, False):
                        base = "rbf" if rbf else next(kinds[mode])
                        R = next(lens)
                        out.append(_case("lam", base, mode == 1, 1, M, WIDTHS[DP], R, next(other), "cross", _opts(base, grad_impl=4),
                                         "lam %d %s %d %d %d %s" % (mode, "rbf" if rbf else "gen", G, C, DP, variant), scale=_scale(base, mode == 1, R)))
        first = RANGE[(G, C)][0]
        out.append(_case("lam", "mix", True, 1, 4, 3, first, 0, "sym", _opts("mix", grad_impl=4), "lam 1 gen %d %d 4 3c" % (G, C)))
        out.append(_case("lam", "rbf", False, 1, 5, 7, first + 2, 0, "diag", _opts("rbf", grad_impl=4), "lam 2 rbf %d %d 8 4c" % (G, C)))
    out.append(_case("lam", "poly", True, 1, 1, 3, 9, 5, "cross", _opts("poly", grad_impl=4), "lam 1 gen 16 2 4 4r"))
    out.append(_case("lam", "cosine", False, 1, 8, 7, 40, 5, "cross", _opts("cosine", grad_impl=4), "lam 2 gen 16 4 8 7r"))
    out.append(_case("lam", "cosine", True, 1, 3, 3, 20, 5, "cross", _opts("cosine", grad_impl=4), "lam 1 gen 16 2 4 4r"))
    out.append(_case("lam", "rbf", False, 1, 6, 7, 50, 19, "cross", _opts("rbf", grad_impl=4), "lam 2 rbf 16 4 8 7r"))
    out.append(_case("lam", "matern12", True, 1, 4, 16, 70, 19, "cross", _opts("matern12", grad_impl=4), "lam 1 gen 64 2 16 3c"))
    out.append(_case("lam", "rbf", True, 1, 5, 8, 300, 5, "cross", _opts("rbf", grad_impl=4), "lam 1 rbf 64 8 8 4c"))
    return out


HO_LEVELS = [(2, 2), (3, 2), (3, 3), (4, 2), (4, 3), (4, 4), (5, 2), (5, 3), (5, 4)]     # (num_levels, order): GPSIG_HO_UNDO_LEVELS


def _ho_cases():
    """higher order.  Scratch-free sweeps (grad_impl = 0): 6 lane shapes x 9 (num_levels, order); between 33 and 64 columns the ho_g32 rule takes
    (32, 2) from order 3 on and (16, 4) below, the option forces the other one.  Sweeps through HBM slots (grad_impl = 3): 5 lane shapes x
    orders 2 .. 4, num_levels 2 .. 5 at run time.  wide = 0: the point route around the sweeps for every base kernel."""
    out = []
    bases = itertools.cycle(["rbf", "matern32", "linear"])
    other = itertools.cycle([5, 19])
    widths = itertools.cycle([3, 7, 13])
    diffs = itertools.cycle([True, True, False])
    for (G, C) in [(16, 2), (16, 4), (32, 2), (64, 2), (64, 4), (64, 8)]:
        for R, (M, order) in zip(_ends((G, C), 9), HO_LEVELS):
            base, diff = next(bases), next(diffs)
            g32 = {(16, 4): 0 if order >= 3 else -1, (32, 2): -1 if order >= 3 else 1}.get((G, C), -1)
            out.append(_case("ho", base, diff, order, M, next(widths), R, next(other), "cross", _opts(base, grad_impl=0, wide=0, ho_g32=g32),
                             "ho_undo %d %d %d %d" % (G, C, M, order), scale=0.4 if diff else 0.15 if R <= 128 else 0.05))
    for (G, C) in LANE_SHAPES:
        for R, (M, order) in zip(_ends((G, C), 9), HO_LEVELS):
            base, diff = next(bases), next(diffs)
            out.append(_case("ho", base, diff, order, M, next(widths), R, next(other), "cross", _opts(base, grad_impl=3, wide=0),
                             "ho_slot %d %d %d" % (G, C, order), scale=0.4 if diff else 0.15 if R <= 128 else 0.05))
    for (G, C) in LANE_SHAPES:
        first = RANGE[(G, C)][0]
        out.append(_case("ho", "rbf", True, 2, 3, 3, first, 0, "sym", _opts("rbf", grad_impl=0, wide=0, ho_g32=0), "ho_undo %d %d 3 2" % (G, C)))
        out.append(_case("ho", "linear", True, 3, 4, 7, first + 2, 0, "diag", _opts("linear", grad_impl=3, wide=0), "ho_slot %d %d 3" % (G, C)))
    out.append(_case("ho", "matern32", True, 3, 4, 3, 33, 0, "sym", _opts("matern32", grad_impl=0, wide=0), "ho_undo 32 2 4 3"))
    out.append(_case("ho", "rbf", True, 2, 2, 3, 35, 0, "diag", _opts("rbf", grad_impl=0, wide=0, ho_g32=1), "ho_undo 32 2 2 2"))
    # order beyond num_levels is cut to it; d = DP
    out.append(_case("ho", "rbf", True, 4, 3, 8, 20, 5, "cross", _opts("rbf", grad_impl=0, wide=0), "ho_undo 16 2 3 3"))
    return out


CASES = _wave_cases() + _wave2_cases() + _lam_cases() + _ho_cases()

# compiled instances no call can reach, each with its reason
UNREACHABLE = {}
for _v in LEVELS:
    for _g, _c, _dp in ((64, 4, 4), (64, 4, 8), (64, 4, 16)):
        UNREACHABLE["wave2 %d %d %d %s" % (_g, _c, _dp, _v)] = "wave2_plan does not list the (64, 4) lane shape"
    UNREACHABLE["wave2 16 4 16 %s" % _v] = "wave2_plan skips C * DP > 32 (4 x 16 = 64): larger per-lane tiles spill"
    UNREACHABLE["wave2 64 8 8 %s" % _v] = "wave2_plan skips C * DP > 32 (8 x 8 = 64): larger per-lane tiles spill"


def group(case):
    """the GPU test a case runs in: family (the Lam-out kernels split into their RBF and run-time-kind instances) and lane shape"""
    words = case.expected.split(" | ")[-1 if case.L2 >= case.L1 else 0].split()
    fam = {"wave": "wave", "wave2": "wave2", "lam": "lam_" + words[2], "ho_undo": "ho_undo", "ho_slot": "ho_slot"}[words[0]]
    G, C = {"wave": words[2:4], "wave2": words[1:3], "lam": words[3:5], "ho_undo": words[1:3], "ho_slot": words[1:3]}[words[0]]
    return "%s-%sx%s" % (fam, G, C)


def instances(case):
    return case.expected.split(" | ")


def plan_query(case):
    """the case as a line for tests/emu/test_grad_plan.cpp"""
    dr = 1 if case.difference else 0
    R1, R2 = case.L1 - dr, case.L2 - dr
    DP = min(w for w in (4, 8, 16, 32, 64) if w >= case.d)
    mode = _mode(case.base, case.difference)
    o = dict(case.options)
    name = case.expected.split()[0]
    if case.family == "wave":
        return "wave %d %d %d %d" % (mode, R2, DP, case.num_levels)
    if case.family == "wave2":
        return "wave2 %d %d %d %d %d %d" % (mode, R1, R2, DP, case.num_levels, int(case.kind != "cross"))
    if case.family == "lam":
        return "lam %d %d %d %d %d %d" % (mode, int(case.base == "rbf"), R1, R2, DP, case.num_levels)
    assert name in ("ho_undo", "ho_slot")
    return "ho %d %d %d %d %d %d" % (o["grad_impl"], o.get("ho_g32", -1), case.num_levels, case.order, R1, R2)


def sizes(case):
    return (3, 2) if case.kind == "cross" else (5, 5)


def data(index):
    """X, Y (None unless a cross Gram), upstream gradient of CASES[index]: random walks cumsum(N(0, 1) * scale / sqrt(d)); without differences
    the upstream gradient is scaled by 0.01"""
    case = CASES[index]
    rng = np.random.default_rng(7000 + index)
    N1, N2 = sizes(case)
    walk = lambda N, L: np.cumsum(rng.standard_normal((N, L, case.d)) * case.scale / np.sqrt(case.d), axis=1)
    X = walk(N1, case.L1)
    Y = walk(N2, case.L2) if case.kind == "cross" else None
    G = rng.standard_normal((case.num_levels + 1, N1) if case.kind == "diag" else (case.num_levels + 1, N1, N2))
    if not case.difference:
        G *= 0.01
    return X, Y, G
