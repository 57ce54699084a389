#!/usr/bin/env python3
"""Exact-mode SignatureSpectral EVALUATION on a wide state space, at the spectral form of CMUsubject16's shape (63 columns with time, L = 500, 500
inducing tensors with increments, 4 levels, Q = 5 components of family rbf): the library's own surface with the kernel object's opt-in
``spectral_wide`` (the wide route with the spectral argument kernel, csrc/wide_spectral_kernel.hpp) against what a user had for these evaluations
before the opt-in -- the library refused them --: autodiff.SignatureKernelModule under torch.no_grad(), the torch matrix route.

    python tools/bench_spectral_wide_exact.py [--N 50 1024] > profiles/spectral_wide_exact.txt

One process, alternating blocks (the protocol of tools/bench_lr_spectral_eval_wide.py): per batch size every (quantity, side) is timed --blocks
times in turn, so that drift of the device hits both sides alike.  One JSON line per (N, quantity): per side the median of the block medians of the
HIP-event times, the block medians themselves and their spread -- the figure a difference has to exceed --; new / old.  Memory per side: the peak of
torch's allocator during one call (the torch route's intermediates, the outputs) and the growth of the device's memory in use across the side's
first call as the driver reports it (the library's scratch buffers live outside torch's allocator and stay with the context).  A side that fails
(the torch route's (lt, 2 T, N L) matrices at N = 1,024 may not fit) is reported with its error instead of a time.
Quantities:
    (a) K_tens_n_seq_covs     Kzz, Kzx and the level diagonals of the sequences: what models.SVGP.predict_f evaluates
    (b) K_tens_vs_seq         Kzx alone"""
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
    from gpsig_amd import autodiff, kernels
    L, d, M, T, Q = args.L, args.d, args.M, args.T, args.Q
    rng = np.random.default_rng(0)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(N)
    Xt = torch.cumsum(0.2 * torch.randn((N, L, d), device=dev, dtype=torch.float64, generator=gen), dim=1).reshape(N, L * d)
    Zt = torch.tensor(rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5, device=dev)
    kern = kernels.SignatureSpectral(L * d, d, M, family=args.family, Q=Q)
    kern.alpha, kern.omega, kern.gamma = np.ones(Q), np.full((Q, d), 0.1), np.full((Q, d), 1.0 / np.sqrt(d))
    mod = autodiff.SignatureKernelModule(kern, device=dev)
    kern.spectral_wide = True

    def new_covs():
        kern.K_tens_n_seq_covs(Zt, Xt, increments=True)

    def old_covs():
        with torch.no_grad():
            mod.K_tens_n_seq_covs(Zt, Xt, increments=True)

    def new_kzx():
        kern.K_tens_vs_seq(Zt, Xt, increments=True)

    def old_kzx():
        with torch.no_grad():
            mod.K_tens_vs_seq(Zt, Xt, increments=True)

    return {"(a) K_tens_n_seq_covs": (new_covs, old_covs), "(b) K_tens_vs_seq": (new_kzx, old_kzx)}


def used_mb():
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free) / 2.0 ** 20


def measure(args, N):
    import torch
    fns = quantities(args, N)
    times, iters, mem, failed = {}, {}, {}, {}
    for b in range(args.blocks):
        for what, pair in fns.items():
            for side, fn in zip(("new", "old"), pair):
                key = (what, side)
                if key in failed:
                    continue
                torch.cuda.synchronize()
                try:
                    if key not in iters:                 # first visit: memory, warm-up, and the size of a block (at most --block-seconds)
                        torch.cuda.empty_cache()
                        torch.cuda.reset_peak_memory_stats()
                        before, base = used_mb(), torch.cuda.memory_allocated()
                        fn()
                        torch.cuda.synchronize()
                        mem[key] = (round((torch.cuda.max_memory_allocated() - base) / 2.0 ** 20, 1), round(used_mb() - before, 1))
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        iters[key] = max(1, min(args.iters, int(args.block_seconds / max(time.perf_counter() - t0, 1e-6))))
                    times.setdefault(key, []).append(block(fn, iters[key]))
                except (RuntimeError, MemoryError, NotImplementedError) as e:
                    failed[key] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:160])
                    torch.cuda.empty_cache()
    for what in fns:
        row = dict(family=args.family, Q=args.Q, N=N, L=args.L, d=args.d, M=args.M, T=args.T, what=what)
        for side in ("new", "old"):
            if (what, side) in failed:
                row[side + "_failed"] = failed[(what, side)]
                continue
            v = times[(what, side)]
            row[side + "_ms"] = round(float(np.median(v)), 3)
            row[side + "_ms_blocks"] = [round(x, 3) for x in v]
            row[side + "_spread_ms"] = round(max(v) - min(v), 3)
            row[side + "_peak_torch_mb"], row[side + "_device_growth_mb"] = mem[(what, side)]
        if "new_ms" in row and "old_ms" in row:
            row["new_over_old"] = round(row["new_ms"] / row["old_ms"], 4)
        print(json.dumps(row), flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[50, 1024])
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--d", type=int, default=63)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--Q", type=int, default=5)
    ap.add_argument("--family", default="rbf")
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--block-seconds", dest="block_seconds", type=float, default=1.5)
    args = ap.parse_args()
    for N in args.N:
        measure(args, N)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
