#!/usr/bin/env python3
"""Ragged batches in low-rank mode: the ragged instances of the sequence feature kernels (``lengths=``: gpsig_lr_seq_features_ragged_dev /
_ragged_grad) against the same table padded by repetition of each sequence's last observation through the existing kernels (what a ragged
data set took before: with the time difference the repeated points give zero increments).  In one process:

    K(X)        forward + backward of the sequences' low-rank Gram K(X) (features, then one product) under a random linear loss
    SVGP step   ELBO forward + backward of gpsig_amd.models.SVGPModule, N sequences against T inducing tensors

for two batches in a table of L rows per sequence: lengths drawn uniformly from --lmin .. L ("ragged": the yardstick of the ratio is
mean(lengths) / L, the work that is linear in a sequence's length), and all lengths = L ("full": the ragged instances against the existing
ones on the same work; the yardstick is 1 within the spread of the existing route's own block medians).

    python tools/bench_lr_ragged.py [--N 1024] [--L 93] [--lmin 4] [--d 6] [--M 4] [--components 50] [--T 64] [--warmup 3] [--iters 10] [--reps 3]

The two routes are timed alternately with HIP events, --reps blocks of --iters iterations each after --warmup iterations per block; one
JSON line per (batch, what): the median over all timed iterations per route, the spread of the blocks' medians, and ragged / padded."""
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
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--L", type=int, default=93)
    ap.add_argument("--lmin", type=int, default=4)
    ap.add_argument("--d", type=int, default=6)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--components", type=int, default=50)
    ap.add_argument("--T", type=int, default=64, help="inducing tensors of the SVGP step")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    run(args, "ragged", rng.integers(args.lmin, args.L + 1, size=args.N))
    run(args, "full", np.full(args.N, args.L))


def run(args, batch, lengths):
    import torch
    from gpsig_amd import kernels, models, inducing_variables, likelihoods
    N, L, d, M, c, T = args.N, args.L, args.d, args.M, args.components, args.T
    rng = np.random.default_rng(1)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    for n, l in enumerate(lengths):
        X[n, l:] = X[n, l - 1]                              # padded by repetition (preprocessing of the reference's benchmarks): both routes read this table
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    dev = torch.device("cuda", 0)
    Xt = torch.tensor(X.reshape(N, -1), device=dev)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=dev)
    lens = torch.tensor(np.asarray(lengths, dtype=np.int32), device=dev)
    kern = kernels.SignatureRBF(L * d, d, M, low_rank=True, num_components=c, rank_bound=c)
    kern.rng = np.random.default_rng(3)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)
    mod = m.kernel
    Xg = Xt.clone().requires_grad_(True)
    W = torch.tensor(rng.standard_normal((N, N)), device=dev)
    draw = mod.draw_low_rank(N * L)
    route = {"lengths": None}

    def gram():
        mod.zero_grad()
        Xg.grad = None
        (mod.K(Xg, lr=draw, lengths=route["lengths"]) * W).sum().backward()

    def svgp_step():
        m.zero_grad()
        (-m.elbo(Xt, Yt, lengths=route["lengths"])).backward()

    for what, fn in (("K(X) forward + backward", gram), ("SVGP step", svgp_step)):
        samples = {"ragged": [], "padded": []}
        for _ in range(args.reps):
            for name in ("ragged", "padded"):
                route["lengths"] = lens if name == "ragged" else None
                torch.cuda.synchronize()
                samples[name].append(timed(fn, args.warmup, args.iters))
        out = {"batch": batch, "base": "rbf", "N": N, "L": L, "d": d, "M": M, "num_components": c, "rank_bound": c, "what": what,
               "mean_length_over_L": round(float(np.mean(lengths)) / L, 4), "max_length": int(np.max(lengths))}
        if what == "SVGP step":
            out["T"] = T
        for name, blocks in samples.items():
            med = [float(np.median(b)) for b in blocks]
            out[name + "_ms_median"] = round(float(np.median(np.concatenate(blocks))), 4)
            out[name + "_ms_block_medians_min_max"] = [round(min(med), 4), round(max(med), 4)]
        out["ragged_over_padded"] = round(out["ragged_ms_median"] / out["padded_ms_median"], 3)
        lo, hi = out["padded_ms_block_medians_min_max"]
        out["padded_block_spread"] = round((hi - lo) / out["padded_ms_median"], 3)
        print(json.dumps(out), flush=True)
    del m
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
