#!/usr/bin/env python3
"""SignatureLinear and SignatureCosine on wide state spaces, at the reference's own run settings (tools/reference_shapes.py: 500 inducing tensors with
increments, 4 levels, num_lags = 1, minibatch 50): AUSLAN's shape (46 columns), CMUsubject16's (126 columns, L = 500) and, for the open question of
DESIGN.md section 8, ArabicDigits' (28 columns) with the wide route forced.

    python tools/bench_wide_linear.py > profiles/wide_linear.txt
    python tools/bench_wide_linear.py --ab libgpsig_hip_parent.so >> profiles/wide_linear.txt     # + a process on gpsig_amd/lib/<that library>

One process, alternating blocks: per shape every configuration (base kernel x route) is timed --blocks times in turn, so that drift of the device
hits all of them alike.  Per configuration and quantity one JSON line: the median of the block medians and the block medians themselves (their spread
is the figure a difference has to exceed).  Quantities: Kzz, Kzx (weighted level sum) and the level diagonals, forward and forward + backward, and
one SVGP step (-ELBO forward + backward).  Routes: "auto" what a user gets (beyond 32 columns the wide route), "wide0" with option wide = 0 (the
route of a library without this one: the older mappings up to 64 columns, torch's matrix route beyond), "wide1" the wide route forced (28 columns).
SignatureRBF runs at the same shapes as the yardstick: the same kernels plus the exponential."""
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

import reference_shapes as RS  # noqa: E402

SHAPES = {"AUSLAN": ("auto", "wide0"), "CMUsubject16": ("auto", "wide0"), "ArabicDigits": ("auto", "wide1")}
BASES = ("SignatureLinear", "SignatureCosine", "SignatureRBF")


def build(name, base, device):
    """reference_shapes.build with the base kernel of choice"""
    from gpsig_amd import kernels
    return RS.build(name, device, kernel_cls=getattr(kernels, base))


def set_route(model, route):
    RS.set_route(model, {"auto": "auto", "wide0": "exact", "wide1": "wide"}[route])
    if route == "wide0" and model.kernel._d_cols > 64:      # (no exact-shape kernels there: what such a library's user gets is the matrix route)
        RS.set_route(model, "matrix")


def quantities(model, X, Y):
    import torch
    k = model.kernel
    with torch.no_grad():
        Xs0 = k.scale_sequences(k._seq3(X, False))
        Zs0 = k.scale_tensors(model.Z)
        fac0 = torch.ones((k.kern.num_levels + 1, Xs0.shape[0]), dtype=Xs0.dtype, device=Xs0.device)
    prims = {"kzz": lambda Z_, X_: k._tens_levels(Z_, True), "kzx": lambda Z_, X_: k._tvs_weighted(Z_, X_, fac0, True),
             "kxx_diag": lambda Z_, X_: k._diag_levels(X_)}
    out = {}
    for pn, pf in prims.items():
        def fwd(pf=pf):
            with torch.no_grad():
                pf(Zs0, Xs0)
        Zr, Xr = Zs0.clone().requires_grad_(True), Xs0.clone().requires_grad_(True)

        def fb(pf=pf, Zr=Zr, Xr=Xr):
            Zr.grad = Xr.grad = None
            o = pf(Zr, Xr)
            (o * o).sum().backward()
        out[pn + "_fwd"], out[pn + "_fwd_bwd"] = fwd, fb

    def step():
        model.zero_grad(set_to_none=True)
        (-model.elbo(X, Y)).backward()
    out["svgp_step"] = step
    return out


def block(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def measure(args):
    import torch
    lib = os.path.basename(os.environ.get("GPSIG_LIB") or "libgpsig_hip.so")
    for name in args.shapes:
        s = RS.shape_of(name)
        configs = []
        for base in BASES:
            for route in (SHAPES[name] if base != "SignatureRBF" else ("auto",)):
                if args.routes and route not in args.routes:
                    continue
                _, model, X, Y = build(name, base, "cuda:0")
                model.kernel._auto_matrix_route = model.kernel.matrix_route
                configs.append((base, route, model, X, Y))
        times, iters = {}, {}
        for b in range(args.blocks):
            for base, route, model, X, Y in configs:
                set_route(model, route)
                try:
                    for q, fn in quantities(model, X, Y).items():
                        key = (base, route, q)
                        if key not in iters:             # first visit: warm up and size the block (at most --block-seconds)
                            fn()
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            fn()
                            torch.cuda.synchronize()
                            iters[key] = max(1, min(args.iters, int(args.block_seconds / max(time.perf_counter() - t0, 1e-6))))
                        times.setdefault(key, []).append(block(fn, iters[key]))
                except NotImplementedError as e:     # the library's refusal of a shape (GPSIG_ERR_UNSUPPORTED) is a line of the record; anything else,
                    times[(base, route, "error")] = "%s: %s" % (type(e).__name__, str(e)[:160])      # a device fault included, ends the process
        for (base, route, q), v in times.items():
            row = dict(lib=lib, shape=name, d_eff=s["d_eff"], L=s["L"], N=s["N"], T=s["T"], M=s["M"], base=base, route=route, what=q)
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
    ap.add_argument("--ab", default=None, help="a library under gpsig_amd/lib without this route: its route ('wide0') in a process of its own, after this build's")
    ap.add_argument("--child-timeout", type=int, default=420)
    args = ap.parse_args()
    if not args.ab:
        return measure(args)
    common = ["--shapes"] + args.shapes + ["--blocks", str(args.blocks), "--iters", str(args.iters), "--block-seconds", str(args.block_seconds)]
    # (that library's own route for these families is what option wide = 0 selects here: it has no wide route for them to switch off)
    for lib, extra in ((None, []), (args.ab, ["--routes", "wide0"])):
        env = dict(os.environ)
        env.pop("GPSIG_LIB", None)
        if lib:
            env["GPSIG_LIB"] = os.path.join(ROOT, "gpsig_amd", "lib", lib)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + common + extra, env=env, timeout=args.child_timeout).returncode
        if rc != 0:              # a child that failed ends the run: nothing more is started on the device
            sys.exit(rc)


if __name__ == "__main__":
    main()
