#!/usr/bin/env python3
"""SignatureMix on wide state spaces: the shapes and the protocol of tools/bench_wide_poly.py (columns as features: CMUsubject16's 126 columns, L = 500,
and AUSLAN's 46 columns, L = 136; 500 inducing tensors with increments, 4 levels, minibatch 50).

    python tools/bench_wide_mix.py > profiles/wide_mix.txt

One process, alternating blocks: per shape every configuration (base kernel x route) is timed --blocks times in turn; per configuration and quantity
one JSON line with the median of the block medians, the block medians and their spread (the figure a difference has to exceed).  Quantities: Kzz, Kzx
(weighted level sum), the level diagonals and the minibatch's sequence Gram, forward and forward + backward, and one SVGP step.  Routes: at 126 columns "auto" (the wide route for
Kzx, Kzz, the level diagonals and the sequence Grams) against "matrix" (torch's matrix route: what a user had before); at 46 columns "auto"
(unchanged: the exact-shape kernels) against "wide1" (the wide route forced: evidence for a later rule, none is moved).  SignatureRBF runs at the same
shapes as the yardstick: mix runs RBF's kernels with one more multiply-add per entry and, in the reverse kernels, the sum that is the mixing's
gradient."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import bench_wide_linear as BL  # noqa: E402
import bench_wide_poly as BP  # noqa: E402

BASES = ("SignatureMix", "SignatureRBF")


def quantities(model, X, Y):
    """bench_wide_linear's quantities and the minibatch's sequence Gram K(X) (level array), which SignatureMix's first-order module also sends to the
    library beyond 64 columns"""
    import torch
    out = BL.quantities(model, X, Y)
    k = model.kernel
    with torch.no_grad():
        Xs0 = k.scale_sequences(k._seq3(X, False))
    Xr = Xs0.clone().requires_grad_(True)

    def fwd():
        with torch.no_grad():
            k._seq_levels(Xs0)

    def fb():
        Xr.grad = None
        o = k._seq_levels(Xr)
        (o * o).sum().backward()
    out["kxx_gram_fwd"], out["kxx_gram_fwd_bwd"] = fwd, fb
    return out


def measure(args):
    import torch
    for name in args.shapes:
        configs = []
        for base in BASES:
            for route in (BP.SHAPES[name][4] if base == "SignatureMix" else ("auto",)):
                s, model, X, Y = BP.build(name, base, "cuda:0")
                model.kernel._auto_matrix_route = model.kernel.matrix_route
                configs.append((base, route, model, X, Y, s))
        times, iters, shape = {}, {}, None
        for b in range(args.blocks):
            for base, route, model, X, Y, shape in configs:
                BP.set_route(model, route)
                try:
                    for q, fn in quantities(model, X, Y).items():
                        if args.what and args.what not in q:
                            continue
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
            row = dict(shape=name, **shape, base=base, route=route, what=q)
            if isinstance(v, str):
                row["error"] = v
            else:
                row.update(ms=round(float(np.median(v)), 3), ms_blocks=[round(x, 3) for x in v], spread_ms=round(max(v) - min(v), 3))
            print(json.dumps(row), flush=True)
        del configs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=list(BP.SHAPES))
    ap.add_argument("--what", default=None, help="only the quantities whose name holds this")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--block-seconds", dest="block_seconds", type=float, default=1.5)
    measure(ap.parse_args())


if __name__ == "__main__":
    main()
