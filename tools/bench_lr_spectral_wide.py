#!/usr/bin/env python3
"""Low-rank SignatureSpectral on a wide state space, at the spectral form of CMUsubject16's shape (63 columns with time, L = 500, 50 components
and rank 50, 500 inducing tensors with increments, 4 levels, Q = 5 components of family rbf): the route through the spectral cross op on the
matrix cores and the feature kernels that take kxs from memory (autodiff._lr_spectral_wide) against the torch route of the same build (module
option lr_hip = False).  Before the cross op served more than 32 columns these shapes raised with lr_hip = True: the torch route is the yardstick.

    python tools/bench_lr_spectral_wide.py [--N 50 1024] > profiles/lowrank_spectral_wide.txt

One process, alternating blocks (the protocol of tools/bench_lr_wide_train.py): per batch size every (quantity, route) is timed --blocks times in
turn, so that drift of the device hits both routes alike.  One JSON line per (N, quantity): per route the median of the block medians, the block
medians themselves, their spread -- the figure a difference has to exceed -- and the peak of torch.cuda.max_memory_allocated; hip / torch.  Where
the torch route runs out of memory at a batch size, a line says so and the batch size is halved until it fits.
Quantities:
    SVGP step             -ELBO forward + backward of gpsig_amd.models.SVGPModule
    cross forward         kappa(points of the sequences, landmarks), n = N L points: autodiff._SpectralCross against autodiff.base_kernel_matrix
    cross forward+backward  ... under a random linear loss, gradients of points, landmarks, alpha, omega, gamma"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


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


def quantities(args, N):
    import torch
    from gpsig_amd import autodiff, kernels, models, inducing_variables, likelihoods
    L, d, M, c, T, Q = args.L, args.d, args.M, args.components, args.T, args.Q
    rng = np.random.default_rng(0)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    dev = torch.device("cuda", 0)
    Xt = torch.tensor(X.reshape(N, -1), device=dev)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=dev)
    kern = kernels.SignatureSpectral(L * d, d, M, family=args.family, Q=Q, low_rank=True, num_components=c, rank_bound=c)
    kern.alpha, kern.omega, kern.gamma = np.ones(Q), np.full((Q, d), 0.1), np.full((Q, d), 1.0 / np.sqrt(d))
    kern.rng = np.random.default_rng(3)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)
    mod = m.kernel
    with torch.no_grad():
        Xs0 = mod.scale_sequences(mod._seq3(Xt, False))
    P = Xs0.reshape(-1, d).clone().requires_grad_(True)
    S = P.detach()[torch.tensor(rng.choice(N * L, c, replace=False), device=dev)].clone().requires_grad_(True)
    par = [autodiff.positive(t).detach().clone().requires_grad_(True) for t in (mod.raw_alpha, mod.raw_omega, mod.raw_sgamma)]
    Gk = torch.tensor(rng.standard_normal((N * L, c)), device=dev)

    def kappa():
        if mod.lr_hip:
            return autodiff._SpectralCross.apply(P, S, *par, args.family)
        return autodiff.base_kernel_matrix("spectral", P, S, spectral=(args.family, *par))

    def cross_forward():
        with torch.no_grad():
            kappa()

    def cross_both():
        for t in [P, S] + par:
            t.grad = None
        (kappa() * Gk).sum().backward()

    def step():
        m.zero_grad(set_to_none=True)
        (-m.elbo(Xt, Yt)).backward()

    return mod, {"SVGP step": step, "cross forward": cross_forward, "cross forward+backward": cross_both}


def measure(args, N):
    """-> the rows of batch size N, or None where the torch route ran out of memory"""
    import torch
    dev = torch.device("cuda", 0)
    mod, fns = quantities(args, N)
    times, iters, peak = {}, {}, {}
    try:
        for b in range(args.blocks):
            for what, fn in fns.items():
                for route in ("hip", "torch"):
                    mod.lr_hip = route == "hip"
                    key = (what, route)
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats(dev)
                    if key not in iters:                 # first visit: warm up and size the block (at most --block-seconds)
                        fn()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        iters[key] = max(1, min(args.iters, int(args.block_seconds / max(time.perf_counter() - t0, 1e-6))))
                    times.setdefault(key, []).append(block(fn, iters[key]))
                    peak[key] = max(peak.get(key, 0.0), torch.cuda.max_memory_allocated(dev) / 2 ** 20)
    except torch.cuda.OutOfMemoryError:
        print(json.dumps(dict(family=args.family, N=N, L=args.L, d=args.d, what=key[0], route=key[1], result="out of memory")), flush=True)
        return None
    finally:
        mod.lr_hip = True
    rows = []
    for what in fns:
        row = dict(family=args.family, Q=args.Q, N=N, L=args.L, d=args.d, M=args.M, num_components=args.components, T=args.T, what=what)
        for route in ("hip", "torch"):
            v = times[(what, route)]
            row[route + "_ms"] = round(float(np.median(v)), 3)
            row[route + "_ms_blocks"] = [round(x, 3) for x in v]
            row[route + "_spread_ms"] = round(max(v) - min(v), 3)
            row[route + "_peak_mb"] = round(peak[(what, route)], 1)
        row["hip_over_torch"] = round(row["hip_ms"] / row["torch_ms"], 4)
        rows.append(row)
    return rows


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[50, 1024])
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--d", type=int, default=63)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--Q", type=int, default=5)
    ap.add_argument("--family", default="rbf")
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--block-seconds", dest="block_seconds", type=float, default=1.5)
    args = ap.parse_args()
    for N in args.N:
        rows = None
        while rows is None and N >= 2:
            rows = measure(args, N)
            torch.cuda.empty_cache()
            if rows is None:
                N //= 2
        for row in rows or ():
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
