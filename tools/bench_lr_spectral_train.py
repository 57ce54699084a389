#!/usr/bin/env python3
"""One SVGP ELBO forward + backward of a low-rank SignatureSpectral (gpsig_amd.models.SVGPModule, inducing tensors): the Nystrom cross
matrix of the landmarks and the sequence features through the HIP ops (module option lr_hip = True: _SpectralCross and
_LrSeqFeaturesSpectral, gpsig_lr_seq_features_spectral_dev / _grad) or through torch ops (lr_hip = False: autodiff._LowRankScope._seq_torch).

    python tools/bench_lr_spectral_train.py [--N 1024 [16384 ...]] [--L 50] [--d 6] [--M 4] [--T 64] [--components 50] [--Q 5] [--family rbf]
                                            [--steps 10] [--routes hip,torch] [--torch-max-N 4096]

Prints one JSON line per (N, route): ms per step (median of --steps after two warm-up steps) and torch.cuda.max_memory_allocated.  The torch
route keeps N L nnz products per level in memory (about 9 GB at N = 1,024 with the defaults): it is skipped above --torch-max-N sequences.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[1024])
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--Q", type=int, default=5)
    ap.add_argument("--family", default="rbf", choices=["rbf", "exp", "mixed"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--routes", default="hip,torch", help="comma-separated: hip (lr_hip = True), torch (lr_hip = False)")
    ap.add_argument("--torch-max-N", type=int, default=4096, help="skip the torch route for larger N (it would not fit)")
    args = ap.parse_args()
    for N in args.N:
        for route in args.routes.split(","):
            if route == "torch" and N > args.torch_max_N:
                print(json.dumps({"N": N, "lr_hip": False, "skipped": f"torch route above --torch-max-N {args.torch_max_N}"}))
                continue
            run(args, N, route == "hip")


def run(args, N, lr_hip):
    import torch
    from gpsig_amd import kernels, models, inducing_variables, likelihoods
    L, d, M, T = args.L, args.d, args.M, args.T
    rng = np.random.default_rng(0)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    dev = torch.device("cuda", 0)
    Xt = torch.tensor(X.reshape(N, -1), device=dev)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=dev)
    kern = kernels.SignatureSpectral(L * d, d, M, family=args.family, Q=args.Q, low_rank=True, num_components=args.components,
                                     rank_bound=args.components)
    kern.alpha, kern.omega, kern.gamma = np.ones(args.Q), np.full((args.Q, d), 0.1), np.full((args.Q, d), 1 / np.sqrt(d))
    kern.rng = np.random.default_rng(3)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)
    m.kernel.lr_hip = lr_hip

    def step():
        m.zero_grad()
        loss = -m.elbo(Xt, Yt)
        loss.backward()
        return loss

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        loss = step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"what": f"low-rank SignatureSpectral ({args.family}, Q={args.Q}) SVGP ELBO forward + backward, N={N}, L={L}, d={d}, "
                              f"M={M}, T={T} inducing tensors (increments), num_components=rank_bound={args.components}",
                      "N": N, "lr_hip": lr_hip, "ms_per_step_median": float(np.median(times)), "ms_per_step_min": float(np.min(times)),
                      "peak_mem_MB": torch.cuda.max_memory_allocated(dev) / 2 ** 20, "loss": float(loss.detach().cpu())}))


if __name__ == "__main__":
    main()
