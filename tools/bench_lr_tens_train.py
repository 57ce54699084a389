#!/usr/bin/env python3
"""Low-rank training with the inducing tensors' feature map through the fused HIP kernels (_LrTensFeatures / _LrTensFeaturesSpectral:
gpsig_lr_tens_features[_spectral]_dev / _grad, csrc/lr_tens_grad_kernel.hpp) or through torch ops (module option lr_tens_hip = False:
autodiff._LowRankScope._tens_torch, the route of every earlier revision).  The sequences take the HIP ops in both routes.  In one process:

    K_tens      forward + backward of K_tens(Z) under a random linear loss, HIP events around the pair
    SVGP step   ELBO forward + backward of gpsig_amd.models.SVGPModule, N sequences against the T inducing tensors, HIP events

    python tools/bench_lr_tens_train.py [--T 500 64] [--d 6 10 28] [--bases rbf spectral] [--M 4] [--components 50] [--Q 5] [--N 50] [--L 50]
                                        [--warmup 5] [--iters 30] [--reps 3]

The two routes are timed alternately, --reps blocks of --iters iterations each after --warmup iterations per block; one JSON line per
(base, T, d, what): the median over all timed iterations per route, the spread of the blocks' medians, and hip / torch."""
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
    ap.add_argument("--T", type=int, nargs="+", default=[500, 64])
    ap.add_argument("--d", type=int, nargs="+", default=[6, 10, 28])
    ap.add_argument("--bases", nargs="+", default=["rbf", "spectral"], choices=["rbf", "spectral"])
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--Q", type=int, default=5)
    ap.add_argument("--N", type=int, default=50, help="sequences of the SVGP step (the reference's minibatch)")
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for base in args.bases:
        for T in args.T:
            for d in args.d:
                run(args, base, T, d)


def run(args, base, T, d):
    import torch
    from gpsig_amd import kernels, models, inducing_variables, likelihoods
    N, L, M, c = args.N, args.L, args.M, args.components
    rng = np.random.default_rng(0)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    lt = M * (M + 1) // 2
    Z = rng.standard_normal((lt, T, 2, d)) * 0.5
    dev = torch.device("cuda", 0)
    Xt = torch.tensor(X.reshape(N, -1), device=dev)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=dev)
    if base == "spectral":
        kern = kernels.SignatureSpectral(L * d, d, M, family="rbf", Q=args.Q, low_rank=True, num_components=c, rank_bound=c)
        kern.alpha, kern.omega, kern.gamma = np.ones(args.Q), np.full((args.Q, d), 0.1), np.full((args.Q, d), 1 / np.sqrt(d))
    else:
        kern = kernels.SignatureRBF(L * d, d, M, low_rank=True, num_components=c, rank_bound=c)
    kern.rng = np.random.default_rng(3)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)
    mod = m.kernel
    Zt = torch.tensor(Z, device=dev, requires_grad=True)
    W = torch.tensor(rng.standard_normal((T, T)), device=dev)
    draw = mod.draw_low_rank(lt * T * 2)

    def k_tens():
        mod.zero_grad()
        Zt.grad = None
        (mod.K_tens(Zt, increments=True, lr=draw) * W).sum().backward()

    def svgp_step():
        m.zero_grad()
        (-m.elbo(Xt, Yt)).backward()

    for what, fn in (("K_tens forward + backward", k_tens), ("SVGP step", svgp_step)):
        samples = {"hip": [], "torch": []}
        for _ in range(args.reps):
            for route in ("hip", "torch"):
                mod.lr_tens_hip = route == "hip"
                samples[route].append(timed(fn, args.warmup, args.iters))
        mod.lr_tens_hip = True
        out = {"base": base + (f" (rbf family, Q={args.Q})" if base == "spectral" else ""), "T": T, "d": d, "M": M, "increments": True,
               "num_components": c, "rank_bound": c, "what": what}
        if what == "SVGP step":
            out["N"], out["L"] = N, L
        for route, blocks in samples.items():
            med = [float(np.median(b)) for b in blocks]
            out[route + "_ms_median"] = round(float(np.median(np.concatenate(blocks))), 4)
            out[route + "_ms_block_medians_min_max"] = [round(min(med), 4), round(max(med), 4)]
        out["hip_over_torch"] = round(out["hip_ms_median"] / out["torch_ms_median"], 3)
        print(json.dumps(out), flush=True)
    del m
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
