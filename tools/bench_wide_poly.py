#!/usr/bin/env python3
"""SignaturePoly on wide state spaces.  tools/reference_shapes.py builds its shapes with num_lags = 1, which SignaturePoly refuses, so the shapes here
have the COLUMNS as features: CMUsubject16's (126 columns, L = 500) and AUSLAN's (46 columns, L = 136), 500 inducing tensors with increments, 4
levels, minibatch 50.

    python tools/bench_wide_poly.py > profiles/wide_poly.txt
    python tools/bench_wide_poly.py --ab libgpsig_hip_parent.so >> profiles/wide_poly.txt     # + a process on gpsig_amd/lib/<that library>

The protocol of tools/bench_wide_linear.py: one process, alternating blocks -- per shape every configuration (base kernel x route) is timed --blocks
times in turn --, per configuration and quantity one JSON line with the median of the block medians, the block medians and their spread (the figure a
difference has to exceed).  Quantities: Kzz, Kzx (weighted level sum) and the level diagonals, forward and forward + backward, and one SVGP step.
Routes: at 126 columns "auto" (what a user gets: the wide route for Kzx, Kzz and the level diagonals) against "matrix" (torch's matrix route: what a
user of a library without this route gets); at 46 columns "auto" (unchanged: the exact-shape kernels) against "wide1" (the wide route forced: the
evidence for a later rule).  SignatureRBF and SignatureLinear run at the same shapes as yardsticks: poly runs the kernels of both, without the
exponential but with differences taken on kappa -- and, in the reverse kernels, with the sum of W that is the offset's gradient: linear's reverse
pass at the same shape is the same kernels without that sum (and on increment rows)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import bench_wide_linear as BL  # noqa: E402
import reference_shapes as RS  # noqa: E402

# name: (columns, L, classes, n_fit) of the data set whose shape it is, and SignaturePoly's routes there
SHAPES = {"CMUsubject16-cols": (126, 500, 2, 23, ("auto", "matrix")), "AUSLAN-cols": (46, 136, 95, 912, ("auto", "wide1"))}
BASES = ("SignaturePoly", "SignatureRBF", "SignatureLinear")


def build(name, base, device, seed=0):
    """reference_shapes.build with num_lags = 0 and the state space's columns as the features"""
    import torch
    from gpsig_amd import inducing_variables as iv, kernels, likelihoods, models
    d, L, classes, n_fit, _ = SHAPES[name]
    N, T, M = min(RS.MINIBATCH, n_fit), RS.NUM_INDUCING, RS.NUM_LEVELS
    rng = np.random.default_rng(seed)
    X = np.cumsum(rng.standard_normal((N, L, d)) / np.sqrt(L), axis=1)
    X[:, :, 0] = np.linspace(0.0, 1.0, L)[None, :]
    lt = M * (M + 1) // 2
    idx_n, idx_t = rng.integers(0, N, size=(lt, T)), rng.integers(0, L - 1, size=(lt, T))
    Z = np.stack([X[idx_n, idx_t], X[idx_n, idx_t + 1]], axis=2)
    Z = Z + 0.4 * rng.standard_normal(Z.shape)
    kern = getattr(kernels, base)(L * d, d, M, lengthscales=np.sqrt(d) * np.ones(d) * 0.7)
    feat = iv.InducingTensors(Z, M, increments=True)
    if classes == 2:
        lik, latent, Y = likelihoods.Bernoulli(), 1, rng.integers(0, 2, size=(N, 1)).astype(np.float64)
    else:
        lik, latent, Y = likelihoods.MultiClass(classes), classes, rng.integers(0, classes, size=(N, 1)).astype(np.float64)
    model = models.SVGPModule(kern, feat, lik, num_latent=latent, num_data=n_fit, device=device)
    return dict(d_eff=d, L=L, N=N, T=T, M=M), model, torch.as_tensor(X.reshape(N, -1), device=device), torch.as_tensor(Y, device=device)


def set_route(model, route):
    RS.set_route(model, {"auto": "auto", "matrix": "matrix", "wide1": "wide"}[route])


def measure(args):
    import torch
    lib = os.path.basename(os.environ.get("GPSIG_LIB") or "libgpsig_hip.so")
    for name in args.shapes:
        configs = []
        for base in BASES:
            for route in (SHAPES[name][4] if base == "SignaturePoly" else ("auto",)):
                if args.routes and route not in args.routes:
                    continue
                s, model, X, Y = build(name, base, "cuda:0")
                model.kernel._auto_matrix_route = model.kernel.matrix_route
                configs.append((base, route, model, X, Y, s))
        times, iters, shape = {}, {}, None
        for b in range(args.blocks):
            for base, route, model, X, Y, shape in configs:
                set_route(model, route)
                try:
                    for q, fn in BL.quantities(model, X, Y).items():
                        key = (base, route, q)
                        if key not in iters:             # first visit: warm up and size the block (at most --block-seconds)
                            fn()
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            fn()
                            torch.cuda.synchronize()
                            iters[key] = max(1, min(args.iters, int(args.block_seconds / max(time.perf_counter() - t0, 1e-6))))
                        times.setdefault(key, []).append(BL.block(fn, iters[key]))
                except NotImplementedError as e:     # the library's refusal of a shape is a line of the record; anything else, a device fault included,
                    times[(base, route, "error")] = "%s: %s" % (type(e).__name__, str(e)[:160])      # ends the process
        for (base, route, q), v in times.items():
            row = dict(lib=lib, shape=name, **shape, base=base, route=route, what=q)
            if isinstance(v, str):
                row["error"] = v
            else:
                row.update(ms=round(float(np.median(v)), 3), ms_blocks=[round(x, 3) for x in v], spread_ms=round(max(v) - min(v), 3))
            print(json.dumps(row), flush=True)
        del configs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--routes", nargs="+", default=None)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--block-seconds", dest="block_seconds", type=float, default=1.5)
    ap.add_argument("--ab", default=None, help="a library under gpsig_amd/lib without this route: its routes ('matrix' at 126 columns, 'auto' at 46) in a "
                                                "process of its own, after this build's")
    ap.add_argument("--child-timeout", type=int, default=420)
    args = ap.parse_args()
    if not args.ab:
        return measure(args)
    common = ["--shapes"] + args.shapes + ["--blocks", str(args.blocks), "--iters", str(args.iters), "--block-seconds", str(args.block_seconds)]
    # (a library without this route refuses SignaturePoly beyond 64 columns: there its user has the matrix route; up to 64 columns "auto" is its own)
    for lib, extra in ((None, []), (args.ab, ["--routes", "matrix", "auto"])):
        env = dict(os.environ)
        env.pop("GPSIG_LIB", None)
        if lib:
            env["GPSIG_LIB"] = os.path.join(ROOT, "gpsig_amd", "lib", lib)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + common + extra, env=env, timeout=args.child_timeout).returncode
        if rc != 0:              # a child that failed ends the run: nothing more is started on the device
            sys.exit(rc)


if __name__ == "__main__":
    main()
