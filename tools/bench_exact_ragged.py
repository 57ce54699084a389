#!/usr/bin/env python3
"""Ragged batches in EXACT mode (``kern.exact_ragged``: gpsig_kernel_*_ragged on the wide route) at the reference's production configuration --
SignatureRBF, low_rank=False, increments, 500 inducing tensors, num_levels = 4, tables cut at 500 rows -- for the state spaces of CMUsubject16
(62 features + time, one lag: 126 columns) and NetFlow (10 columns), N = 50 and 1,024 sequences with lengths uniform in --lmin .. L.

Each line times one evaluation on the ragged route against THE SAME KERNEL OBJECT on the same table padded by repetition of each sequence's last
observation through the dense route (what a user runs today; unchanged by the ragged route):
    K_tens_n_seq_covs   Kzz, Kzx and the diagonal Kxx (normalised: Kzx needs every sequence's level diagonals)
    Kdiag               the level diagonals alone (normalization=False for this line: normalised, Kdiag reads no data)
    predict_f           models.SVGP.predict_f (K_tens_n_seq_covs plus the conditional)
  * lag-free (num_lags = 0 on the full width): with difference=True padding by repetition is exact -- the SAME quantity, and the comparison that counts;
  * with the lag (num_lags = 1 on half the width, lag_axis = "sequence"): a DIFFERENT quantity of the same shape (the lagged channels of a padded
    sequence keep moving after it has ended).
Each route runs on a stream, and so a library context, of its own: `scratch_mb` is that context's scratch memory after the route's calls of the line.

    python tools/bench_exact_ragged.py [--shapes cmusubject16,netflow] [--N 50,1024] [--L 500] [--lmin 4] [--T 500] [--warmup 2] [--iters 5] [--reps 3]

The two routes of a line are timed alternately with HIP events, --reps blocks of --iters iterations each after --warmup iterations per block; one
JSON line per (shape, lags, N, what): the median over all timed iterations per route, the spread of the blocks' medians, and the ratio."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

COLUMNS = {"cmusubject16": 126, "netflow": 10}
LAG = 0.137


def timed(fn, stream, warmup, iters, slow_ms=1000.0):
    """iters timed calls after warmup calls; a route whose first call takes more than slow_ms (the dense route's normalisation factors beyond the
    exact-shape kernels' columns: seconds per call) is timed over two calls without further warm-up, so that a run stays within minutes"""
    import time
    import torch
    with torch.cuda.stream(stream):
        t0 = time.perf_counter()
        fn()
        stream.synchronize()
        if (time.perf_counter() - t0) * 1e3 > slow_ms:
            warmup, iters = 0, 2
        for _ in range(warmup - 1):
            fn()
        stream.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in ev:
            a.record(stream)
            fn()
            b.record(stream)
        stream.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def line(args, out, routes):
    """routes: {name: (fn, stream)}, taking turns block by block"""
    import torch
    from gpsig_amd import _lib
    samples = {name: [] for name in routes}
    for _ in range(args.reps):
        for name, (fn, stream) in routes.items():
            torch.cuda.synchronize()
            samples[name].append(timed(fn, stream, args.warmup, args.iters))
    for name, blocks in samples.items():
        med = [float(np.median(b)) for b in blocks]
        out[name + "_ms_median"] = round(float(np.median(np.concatenate(blocks))), 4)
        out[name + "_ms_block_medians_min_max"] = [round(min(med), 4), round(max(med), 4)]
        out[name + "_scratch_mb"] = round(_lib.context(0, routes[name][1].cuda_stream).scratch_bytes() / 2 ** 20, 1)
    out["ragged_over_padded"] = round(out["ragged_ms_median"] / out["padded_ms_median"], 3)
    lo, hi = out["padded_ms_block_medians_min_max"]
    out["padded_block_spread"] = round((hi - lo) / out["padded_ms_median"], 3)
    print(json.dumps(out), flush=True)


def run(args, shape, N, lagged):
    import torch
    from gpsig_amd import _lib, kernels, models, inducing_variables
    cols, L, M, T = COLUMNS[shape], args.L, 4, args.T
    d = cols // 2 if lagged else cols
    rng = np.random.default_rng(1)
    lengths = np.random.default_rng(0).integers(args.lmin, L + 1, size=N)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1)
    for n, l in enumerate(lengths):
        X[n, l:] = X[n, l - 1]                              # padded by repetition (the reference's preprocessing): both routes read this table
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, cols)) * 0.5
    dev = torch.device("cuda", 0)
    Xt, Zt = torch.tensor(X.reshape(N, -1), device=dev), torch.tensor(Z, device=dev)
    lens = torch.tensor(np.asarray(lengths, dtype=np.int32), device=dev)
    lf = lengths.astype(np.float64)
    head = {"shape": shape, "base": "rbf", "N": N, "L": L, "columns": cols, "num_lags": 1 if lagged else 0, "M": M, "T": T,
            "same_quantity": not lagged, "rows_over_NL": round(float(lf.sum()) / (N * L), 4), "cells_over_NL2": round(float((lf * lf).sum()) / (N * L * L), 4)}

    def kernel(normalization=True):
        k = kernels.SignatureRBF(L * d, d, M, lengthscales=np.full(d, np.sqrt(cols)), normalization=normalization, num_lags=1 if lagged else None)
        if lagged:
            k.lags = np.asarray([LAG])
            k.lag_axis = "sequence"
        k.exact_ragged = True
        return k

    streams = {"ragged": torch.cuda.Stream(dev), "padded": torch.cuda.Stream(dev)}
    for s in streams.values():
        _lib.hold(0, s.cuda_stream)
    try:
        k, ku = kernel(), kernel(normalization=False)
        q_mu = rng.standard_normal((T, 1))
        m = models.SVGP(k, inducing_variables.InducingTensors(Zt, M, increments=True), q_diag=True, whiten=True, q_mu=q_mu, q_sqrt=np.ones((T, 1)))
        calls = {"K_tens_n_seq_covs": lambda kw: k.K_tens_n_seq_covs(Zt, Xt, increments=True, **kw),
                 "Kdiag (normalization=False)": lambda kw: ku.Kdiag(Xt, **kw),
                 "predict_f": lambda kw: m.predict_f(Xt, **kw)}
        for what, call in calls.items():
            routes = {"ragged": ((lambda c=call: c({"lengths": lens})), streams["ragged"]), "padded": ((lambda c=call: c({})), streams["padded"])}
            line(args, dict(head, what=what), routes)
    finally:
        for s in streams.values():
            s.synchronize()
            _lib.release(0, s.cuda_stream)
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cmusubject16,netflow")
    ap.add_argument("--N", default="50,1024")
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--lmin", type=int, default=4)
    ap.add_argument("--T", type=int, default=500, help="inducing tensors")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        for lagged in (False, True):
            for N in (int(v) for v in args.N.split(",")):
                run(args, shape, N, lagged)


if __name__ == "__main__":
    main()
