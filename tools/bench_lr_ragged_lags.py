#!/usr/bin/env python3
"""Ragged batches WITH LAGS in low-rank mode (``lag_axis = "sequence"``: each sequence on its own time axis) at the reference's run
configuration -- num_lags = 1, increments, 500 inducing tensors, num_levels = 4, c = r = 50, tables cut at 500 rows -- for the shapes of
CMUsubject16 (62 features) and NetFlow (4), N = 50 and 1,024 sequences with lengths uniform in --lmin .. L.  In one process:

  (a) SVGP step           ELBO forward + backward of gpsig_amd.models.SVGPModule                      ragged, per-sequence axes
      K_tens_n_seq_covs   gpsig_amd.kernels.SignatureKernel.K_tens_n_seq_covs on CUDA tensors         against
                          the same table padded by repetition of each sequence's last observation on the existing dense route: what a user runs
                          today.  A DIFFERENT quantity (the lagged channels of a padded sequence keep moving after it has ended) of the same
                          shape; the ragged route does mean(lengths) / L of the length-proportional work.
  (b) lag op              autodiff._SeqLagsRagged (gpsig_seq_lags_ragged_dev / _grad), forward and forward + backward, against its torch
                          restatement autodiff._add_lags_ragged on the GPU, with the peak memory of one forward + backward of each.

    python tools/bench_lr_ragged_lags.py [--shapes cmusubject16,netflow] [--N 50,1024] [--L 500] [--lmin 4] [--T 500] [--warmup 3] [--iters 10] [--reps 3]

The two routes of a line are timed alternately with HIP events, --reps blocks of --iters iterations each after --warmup iterations per block;
one JSON line per (shape, N, what): the median over all timed iterations per route, the spread of the blocks' medians, and the ratio."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FEATURES = {"cmusubject16": 62, "netflow": 4}
LAG = 0.137


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


def alternate(args, routes):
    """{name: fn} -> {name: blocks of samples}, the routes taking turns block by block"""
    import torch
    samples = {name: [] for name in routes}
    for _ in range(args.reps):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            samples[name].append(timed(fn, args.warmup, args.iters))
    return samples


def line(out, samples, new, old):
    for name, blocks in samples.items():
        med = [float(np.median(b)) for b in blocks]
        out[name + "_ms_median"] = round(float(np.median(np.concatenate(blocks))), 4)
        out[name + "_ms_block_medians_min_max"] = [round(min(med), 4), round(max(med), 4)]
    out["%s_over_%s" % (new, old)] = round(out[new + "_ms_median"] / out[old + "_ms_median"], 3)
    lo, hi = out[old + "_ms_block_medians_min_max"]
    out[old + "_block_spread"] = round((hi - lo) / out[old + "_ms_median"], 3)
    print(json.dumps(out), flush=True)


def peak_mb(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def run(args, shape, N):
    import torch
    from gpsig_amd import autodiff, kernels, models, inducing_variables, likelihoods
    d, L, M, c, T = FEATURES[shape], args.L, 4, 50, args.T
    rng = np.random.default_rng(1)
    lengths = np.random.default_rng(0).integers(args.lmin, L + 1, size=N)
    lab = np.repeat([0, 1], N // 2)
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    for n, l in enumerate(lengths):
        X[n, l:] = X[n, l - 1]                              # padded by repetition (the reference's preprocessing): both routes read this table
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, 2 * d)) * 0.5
    dev = torch.device("cuda", 0)
    Xt = torch.tensor(X.reshape(N, -1), device=dev)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=dev)
    Zt = torch.tensor(Z, device=dev)
    lens = torch.tensor(np.asarray(lengths, dtype=np.int32), device=dev)
    head = {"shape": shape, "base": "rbf", "N": N, "L": L, "num_features": d, "num_lags": 1, "M": M, "num_components": c, "rank_bound": c, "T": T,
            "mean_length_over_L": round(float(np.mean(lengths)) / L, 4)}

    def kernel():
        k = kernels.SignatureRBF(L * d, d, M, lengthscales=np.full(d, np.sqrt(d)), low_rank=True, num_components=c, rank_bound=c, num_lags=1)
        k.lags = np.asarray([LAG])
        k.lag_axis = "sequence"
        k.rng = np.random.default_rng(3)
        return k

    # ---- (a) ragged on per-sequence axes against padded by repetition on the dense route
    m = models.SVGPModule(kernel(), inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)

    def step(lengths_):
        def fn():
            m.zero_grad()
            (-m.elbo(Xt, Yt, lengths=lengths_)).backward()
        return fn

    line(dict(head, what="SVGP step"), alternate(args, {"ragged": step(lens), "padded": step(None)}), "ragged", "padded")
    del m
    k = kernel()
    line(dict(head, what="K_tens_n_seq_covs (evaluation)"),
         alternate(args, {"ragged": lambda: k.K_tens_n_seq_covs(Zt, Xt, increments=True, lengths=lens),
                          "padded": lambda: k.K_tens_n_seq_covs(Zt, Xt, increments=True)}), "ragged", "padded")

    # ---- (b) the lag op against its torch restatement
    X3 = Xt.reshape(N, L, d).clone().requires_grad_(True)
    lags = torch.tensor([LAG], dtype=torch.float64, device=dev, requires_grad=True)
    G = torch.tensor(rng.standard_normal((N, L, 2, d)), device=dev)
    ops = {"hip": lambda: autodiff._SeqLagsRagged.apply(X3, lags, lens), "torch": lambda: autodiff._add_lags_ragged(X3, lags, lens)}

    def fwd(op):
        def fn():
            with torch.no_grad():
                op()
        return fn

    def both(op):
        def fn():
            X3.grad = lags.grad = None
            (op() * G).sum().backward()
        return fn

    line(dict(head, what="lag op forward"), alternate(args, {n: fwd(op) for n, op in ops.items()}), "hip", "torch")
    out = dict(head, what="lag op forward + backward")
    for n, op in ops.items():
        out[n + "_peak_mb"] = peak_mb(both(op))
    line(out, alternate(args, {n: both(op) for n, op in ops.items()}), "hip", "torch")
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cmusubject16,netflow")
    ap.add_argument("--N", default="50,1024")
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--lmin", type=int, default=4)
    ap.add_argument("--T", type=int, default=500, help="inducing tensors")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        for N in (int(v) for v in args.N.split(",")):
            run(args, shape, N)


if __name__ == "__main__":
    main()
