#!/usr/bin/env python3
"""Low-rank SignatureSpectral on long and ragged batches: one SVGP step (ELBO forward + backward of gpsig_amd.models.SVGPModule, N sequences
against T inducing tensors) with the module option lr_spectral_tiled = True (the lengths-aware tiled spectral instances behind
gpsig_lr_seq_features_spectral_ragged_dev / _ragged_grad) against False (the torch route of the same feature map, what these shapes take by
default).  Two grids, c = r = --components, Q = --Q:

    dense    N in --N x L in --L
    ragged   N = --ragged-N sequences in rows of --ragged-L, lengths spread evenly over 4 .. --ragged-L (the shape of profiles/lowrank_ragged.txt)

    python tools/bench_lr_spectral_long.py [--N 50 1024] [--L 100 200 500] [--d 6] [--M 4] [--components 50] [--Q 5] [--T 64]
                                           [--ragged-N 1024] [--ragged-L 93] [--warmup 2] [--iters 5] [--reps 2]

The two routes are timed alternately with HIP events, --reps blocks of --iters iterations each after --warmup iterations per block; one
JSON line per shape: the median over all timed iterations per route, the spread of the blocks' medians, the peak of
torch.cuda.max_memory_allocated over a route's blocks, and tiled / torch.  A route that runs out of memory at a shape is recorded as
"out of memory" and is not tried at the larger L of the same N."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def timed(fn, warmup, iters):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="*", default=[50, 1024])
    ap.add_argument("--L", type=int, nargs="*", default=[100, 200, 500])
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--Q", type=int, default=5)
    ap.add_argument("--T", type=int, default=64, help="inducing tensors of the SVGP step")
    ap.add_argument("--ragged-N", type=int, default=1024, help="0: no ragged shape")
    ap.add_argument("--ragged-L", type=int, default=93)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    for N in args.N:
        skip = set()
        for L in sorted(args.L):
            skip |= run(args, N, L, None, skip)
    if args.ragged_N:
        lengths = np.linspace(4, args.ragged_L, args.ragged_N).round().astype(np.int64)
        run(args, args.ragged_N, args.ragged_L, lengths, set())


def run(args, N, L, lengths, skip):
    """one shape; returns the routes that ran out of memory"""
    import torch
    from gpsig_amd import kernels, models, inducing_variables, likelihoods
    d, M, c, T, Q = args.d, args.M, args.components, args.T, args.Q
    rng = np.random.default_rng(0)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    if lengths is not None:
        for n, l in enumerate(lengths):
            X[n, l:] = np.nan
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    dev = torch.device("cuda", 0)
    Xt = torch.tensor(X.reshape(N, -1), device=dev)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=dev)
    kern = kernels.SignatureSpectral(L * d, d, M, family="rbf", Q=Q, low_rank=True, num_components=c, rank_bound=c)
    kern.alpha, kern.omega, kern.gamma = np.ones(Q), np.full((Q, d), 0.1), np.full((Q, d), 1 / np.sqrt(d))
    kern.rng = np.random.default_rng(3)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)
    mod = m.kernel

    def svgp_step():
        m.zero_grad()
        (-m.elbo(Xt, Yt, lengths=lengths)).backward()

    routes = [r for r in ("tiled", "torch") if r not in skip]
    samples, peak, oom = {r: [] for r in routes}, {r: 0.0 for r in routes}, set()
    for _ in range(args.reps):
        for route in routes:
            if route in oom:
                continue
            mod.lr_spectral_tiled = route == "tiled"
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            try:
                samples[route].append(timed(svgp_step, args.warmup, args.iters))
                peak[route] = max(peak[route], torch.cuda.max_memory_allocated(dev) / 2 ** 20)
            except torch.cuda.OutOfMemoryError:
                oom.add(route)
                m.zero_grad()
                torch.cuda.empty_cache()
    out = {"base": "spectral", "Q": Q, "N": N, "L": L, "d": d, "M": M, "num_components": c, "rank_bound": c, "T": T, "what": "SVGP step"}
    if lengths is not None:
        out["lengths"] = "%d..%d, mean %.1f" % (lengths.min(), lengths.max(), lengths.mean())
    for route in ("tiled", "torch"):
        if route in skip:
            out[route] = "not run: out of memory at a smaller L"
        elif route in oom:
            out[route] = "out of memory"
        else:
            blocks = samples[route]
            med = [float(np.median(b)) for b in blocks]
            out[route + "_ms_median"] = round(float(np.median(np.concatenate(blocks))), 4)
            out[route + "_ms_block_medians_min_max"] = [round(min(med), 4), round(max(med), 4)]
            out[route + "_peak_mb"] = round(peak[route], 1)
    if "tiled_ms_median" in out and "torch_ms_median" in out:
        out["tiled_over_torch"] = round(out["tiled_ms_median"] / out["torch_ms_median"], 3)
    print(json.dumps(out), flush=True)
    del m
    torch.cuda.empty_cache()
    return oom


if __name__ == "__main__":
    main()
