#!/usr/bin/env python3
"""Low-rank training on sequences longer than the whole-sequence feature kernels hold in LDS: the time-tiled HIP kernels
(csrc/lr_tiled_kernel.hpp behind gpsig_lr_seq_features_dev / _grad) against the torch route of the same feature map (module option
lr_hip = False: autodiff._LowRankScope._seq_torch, what these shapes took before the tiled kernels).  In one process:

    K(X)        forward + backward of the sequences' low-rank Gram K(X) (features, then one product) under a random linear loss
    SVGP step   ELBO forward + backward of gpsig_amd.models.SVGPModule, N sequences against T inducing tensors

    python tools/bench_lr_long_train.py [--N 50 1024] [--L 100 200 500] [--d 6 10] [--M 4] [--components 50] [--T 64]
                                        [--warmup 2] [--iters 6] [--reps 2]

The two routes are timed alternately with HIP events, --reps blocks of --iters iterations each after --warmup iterations per block; one
JSON line per (N, L, d, what): the median over all timed iterations per route, the spread of the blocks' medians, the peak of
torch.cuda.max_memory_allocated over a route's blocks, and hip / torch."""
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
    ap.add_argument("--N", type=int, nargs="+", default=[50, 1024])
    ap.add_argument("--L", type=int, nargs="+", default=[100, 200, 500])
    ap.add_argument("--d", type=int, nargs="+", default=[6, 10])
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--T", type=int, default=64, help="inducing tensors of the SVGP step")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    for N in args.N:
        for L in args.L:
            for d in args.d:
                run(args, N, L, d)


def run(args, N, L, d):
    import torch
    from gpsig_amd import kernels, models, inducing_variables, likelihoods
    M, c, T = args.M, args.components, args.T
    rng = np.random.default_rng(0)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    dev = torch.device("cuda", 0)
    Xt = torch.tensor(X.reshape(N, -1), device=dev)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=dev)
    kern = kernels.SignatureRBF(L * d, d, M, low_rank=True, num_components=c, rank_bound=c)
    kern.rng = np.random.default_rng(3)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)
    mod = m.kernel
    Xg = Xt.clone().requires_grad_(True)
    W = torch.tensor(rng.standard_normal((N, N)), device=dev)
    draw = mod.draw_low_rank(N * L)

    def gram():
        mod.zero_grad()
        Xg.grad = None
        (mod.K(Xg, lr=draw) * W).sum().backward()

    def svgp_step():
        m.zero_grad()
        (-m.elbo(Xt, Yt)).backward()

    for what, fn in (("K(X) forward + backward", gram), ("SVGP step", svgp_step)):
        samples, peak = {"hip": [], "torch": []}, {"hip": 0.0, "torch": 0.0}
        for _ in range(args.reps):
            for route in ("hip", "torch"):
                mod.lr_hip = route == "hip"
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats(dev)
                samples[route].append(timed(fn, args.warmup, args.iters))
                peak[route] = max(peak[route], torch.cuda.max_memory_allocated(dev) / 2 ** 20)
        mod.lr_hip = True
        out = {"base": "rbf", "N": N, "L": L, "d": d, "M": M, "num_components": c, "rank_bound": c, "what": what}
        if what == "SVGP step":
            out["T"] = T
        for route, blocks in samples.items():
            med = [float(np.median(b)) for b in blocks]
            out[route + "_ms_median"] = round(float(np.median(np.concatenate(blocks))), 4)
            out[route + "_ms_block_medians_min_max"] = [round(min(med), 4), round(max(med), 4)]
            out[route + "_peak_mb"] = round(peak[route], 1)
        out["hip_over_torch"] = round(out["hip_ms_median"] / out["torch_ms_median"], 3)
        print(json.dumps(out), flush=True)
    del m
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
