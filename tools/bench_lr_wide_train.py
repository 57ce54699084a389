#!/usr/bin/env python3
"""Low-rank training on a wide state space, at CMUsubject16's shape under the reference's run settings (126 columns, L = 500, 50 components and
rank 50, 500 inducing tensors with increments, 4 levels): the route through the cross op on the matrix cores and the feature kernels that take
kxs from memory (autodiff._lr_route: "kx") against what these shapes took before it, the torch route (module option lr_hip = False).

    python tools/bench_lr_wide_train.py [--N 50 1024] > profiles/lowrank_wide_train.txt

One process, alternating blocks (the protocol of tools/bench_wide_linear.py): per batch size every (quantity, route) is timed --blocks times in
turn, so that drift of the device hits both routes alike.  One JSON line per (N, quantity): per route the median of the block medians, the block
medians themselves, their spread -- the figure a difference has to exceed -- and the peak of torch.cuda.max_memory_allocated; kx / torch.
Quantities, each forward + backward under a random linear loss:
    seq features     the feature map of the N sequences given landmarks and whitening (_LowRankScope.seq)
    tens features    ... of the 500 inducing tensors (_LowRankScope.tens)
    cross matrix     kappa(points of the sequences, landmarks) alone: autodiff._LrCross against autodiff.base_kernel_matrix
    SVGP step        -ELBO forward + backward of gpsig_amd.models.SVGPModule"""
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
    L, d, M, c, T = args.L, args.d, args.M, args.components, args.T
    rng = np.random.default_rng(0)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    dev = torch.device("cuda", 0)
    Xt = torch.tensor(X.reshape(N, -1), device=dev)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=dev)
    kern = kernels.SignatureRBF(L * d, d, M, lengthscales=np.full(d, np.sqrt(d)), low_rank=True, num_components=c, rank_bound=c)
    kern.rng = np.random.default_rng(3)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)
    mod = m.kernel
    with torch.no_grad():
        Xs0 = mod.scale_sequences(mod._seq3(Xt, False))
        Zs0 = mod.scale_tensors(m.Z)
    Xs, Zs = Xs0.clone().requires_grad_(True), Zs0.clone().requires_grad_(True)
    pool = torch.cat([Zs0.reshape(-1, d), Xs0.reshape(-1, d)])
    draw = mod.draw_low_rank(pool.shape[0])
    F = 1 + c + (M - 1) * int(draw.sketches[0].r)
    Gx, Gz = torch.tensor(rng.standard_normal((N, F)), device=dev), torch.tensor(rng.standard_normal((T, F)), device=dev)
    Gk = torch.tensor(rng.standard_normal((N * L, c)), device=dev)
    S = pool[draw.on(dev)[0]].clone().requires_grad_(True)

    def seq():
        Xs.grad = None
        (torch.cat(autodiff._LowRankScope(mod, pool, draw).seq(Xs), dim=1) * Gx).sum().backward()

    def tens():
        Zs.grad = None
        (torch.cat(autodiff._LowRankScope(mod, pool, draw).tens(Zs, True), dim=1) * Gz).sum().backward()

    def cross():
        Xs.grad = S.grad = None
        P = Xs.reshape(-1, d)
        K = autodiff._LrCross.apply(P, S, None, mod._spec) if mod.lr_hip else autodiff.base_kernel_matrix("rbf", P, S)
        (K * Gk).sum().backward()

    def step():
        m.zero_grad(set_to_none=True)
        (-m.elbo(Xt, Yt)).backward()

    return mod, {"seq features": seq, "tens features": tens, "cross matrix": cross, "SVGP step": step}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[50, 1024])
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--d", type=int, default=126)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--block-seconds", dest="block_seconds", type=float, default=1.5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for N in args.N:
        mod, fns = quantities(args, N)
        times, iters, peak = {}, {}, {}
        for b in range(args.blocks):
            for what, fn in fns.items():
                for route in ("kx", "torch"):
                    mod.lr_hip = route == "kx"
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
        mod.lr_hip = True
        for what in fns:
            row = dict(base="rbf", N=N, L=args.L, d=args.d, M=args.M, num_components=args.components, T=args.T, what=what)
            for route in ("kx", "torch"):
                v = times[(what, route)]
                row[route + "_ms"] = round(float(np.median(v)), 3)
                row[route + "_ms_blocks"] = [round(x, 3) for x in v]
                row[route + "_spread_ms"] = round(max(v) - min(v), 3)
                row[route + "_peak_mb"] = round(peak[(what, route)], 1)
            row["kx_over_torch"] = round(row["kx_ms"] / row["torch_ms"], 4)
            print(json.dumps(row), flush=True)
        del mod, fns
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
