#!/usr/bin/env python3
"""Exact-mode SignatureSpectral training at the spectral form of CMUsubject16's shape (63 columns with time, L = 500, 500 inducing tensors with
increments, 4 levels, Q = 5): the matrix route with kappa by the batched HIP op (SignatureKernelModule.spectral_kappa = "hip", autodiff._SpectralKappa)
against kappa by torch ops on the difference tensor ("torch").

    python tools/bench_spectral_kappa.py [--both 5] [--hip 50 1024] > profiles/spectral_kappa.txt

--both N ...: one SVGP step (-ELBO forward + backward) on BOTH routes, alternating blocks in one process (the protocol of tools/bench_lr_spectral_wide.py):
    per route the median of the block medians, the block medians, their spread and the peak of torch's allocator; hip / torch.  N = 5 by default: Kzx's
    difference tensor is 10,000 x 2,500 x 63 x 8 B = 12.6 GB there, chosen from the byte count (torch keeps one scaled copy per component for autograd).
--hip N ...:  the step on the "hip" route alone, and the op alone at Kzx's shape (10,000 tensor rows against N L points): forward, and forward + backward
    under a random linear loss.  The torch route is not run at these sizes: profiles/spectral_wide_exact.txt records it out of memory at N = 50.  A
    quantity that does not fit prints a line saying so.
Every line also carries the library's scratch (gpsig_scratch_bytes of the stream's context), which torch's allocator does not see."""
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
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def scratch_mb():
    import torch
    from gpsig_amd import _lib
    c = _lib.context(0, torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    return round(c._lib.gpsig_scratch_bytes(c._h) / 2 ** 20, 1)


def model(args, N):
    import torch
    from gpsig_amd import kernels, models, inducing_variables, likelihoods
    L, d, M, T, Q = args.L, args.d, args.M, args.T, args.Q
    rng = np.random.default_rng(0)
    lab = np.arange(N) % 2
    X = np.cumsum(rng.standard_normal((N, L, d)) * 0.2, axis=1) + lab[:, None, None] * np.linspace(0, 1, L)[None, :, None]
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    dev = torch.device("cuda", 0)
    kern = kernels.SignatureSpectral(L * d, d, M, family=args.family, Q=Q)
    kern.alpha, kern.omega, kern.gamma = np.ones(Q), np.full((Q, d), 0.1), np.full((Q, d), 1.0 / np.sqrt(d))
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)
    Xt = torch.tensor(X.reshape(N, -1), device=dev)
    Yt = torch.tensor(lab[:, None].astype(np.float64), device=dev)

    def step():
        m.zero_grad(set_to_none=True)
        (-m.elbo(Xt, Yt)).backward()
    return m, step


def timed(fns, routes, set_route, args, base):
    """alternating blocks over (quantity, route) -> rows"""
    import torch
    dev = torch.device("cuda", 0)
    times, iters, peak, failed = {}, {}, {}, set()
    for b in range(args.blocks):
        for what, fn in fns.items():
            for route in routes:
                if what in failed:
                    continue
                set_route(route)
                key = (what, route)
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats(dev)
                try:
                    if key not in iters:                 # first visit: warm up and size the block (at most --block-seconds)
                        fn()
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        iters[key] = max(1, min(args.iters, int(args.block_seconds / max(time.perf_counter() - t0, 1e-6))))
                    times.setdefault(key, []).append(block(fn, iters[key]))
                except (torch.cuda.OutOfMemoryError, MemoryError) as e:
                    print(json.dumps(dict(base, what=what, route=route, result="out of memory", error=str(e)[:120])), flush=True)
                    failed.add(what)                     # (the other quantities go on)
                    continue
                peak[key] = max(peak.get(key, 0.0), torch.cuda.max_memory_allocated(dev) / 2 ** 20)
    rows = []
    for what in fns:
        if what in failed:
            continue
        row = dict(base, what=what)
        for route in routes:
            v = times[(what, route)]
            row[route + "_ms"] = round(float(np.median(v)), 3)
            row[route + "_ms_blocks"] = [round(x, 3) for x in v]
            row[route + "_spread_ms"] = round(max(v) - min(v), 3)
            row[route + "_peak_mb"] = round(peak[(what, route)], 1)
        if len(routes) == 2:
            row["hip_over_torch"] = round(row["hip_ms"] / row["torch_ms"], 4)
        row["library_scratch_mb"] = scratch_mb()
        rows.append(row)
    return rows


def main():
    import torch
    from gpsig_amd import autodiff
    ap = argparse.ArgumentParser()
    ap.add_argument("--both", type=int, nargs="*", default=[5])
    ap.add_argument("--hip", type=int, nargs="*", default=[50, 1024])
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--d", type=int, default=63)
    ap.add_argument("--M", type=int, default=4)
    ap.add_argument("--Q", type=int, default=5)
    ap.add_argument("--T", type=int, default=500)
    ap.add_argument("--family", default="rbf")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--block-seconds", dest="block_seconds", type=float, default=1.5)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    shape = dict(family=args.family, Q=args.Q, L=args.L, d=args.d, M=args.M, T=args.T)
    for N in args.both:
        m, step = model(args, N)
        base = dict(shape, N=N, difference_tensor_gb=round(args.M * (args.M + 1) * args.T * N * args.L * args.d * 8 / 1e9, 1))
        for row in timed({"SVGP step": step}, ("hip", "torch"), lambda r: setattr(m.kernel, "spectral_kappa", r), args, base):
            print(json.dumps(row), flush=True)
        del m, step
        torch.cuda.empty_cache()
    for N in args.hip:
        m, step = model(args, N)
        m.kernel.spectral_kappa = "hip"
        rng = np.random.default_rng(1)
        rows_z = args.M * (args.M + 1) * args.T
        base = dict(shape, N=N, kzx_rows=rows_z, kzx_columns=N * args.L)
        try:
            A = torch.tensor(rng.standard_normal((rows_z, args.d)) * 0.5, device=dev, requires_grad=True)
            B = torch.tensor(rng.standard_normal((N * args.L, args.d)) * 0.5, device=dev, requires_grad=True)
            par = [autodiff.positive(t).detach().clone().requires_grad_(True) for t in (m.kernel.raw_alpha, m.kernel.raw_omega, m.kernel.raw_sgamma)]
            G = torch.randn(rows_z, N * args.L, dtype=torch.float64, device=dev)
        except torch.cuda.OutOfMemoryError:
            print(json.dumps(dict(base, what="op alone", route="hip", result="out of memory (its operands)")), flush=True)
            continue

        def forward():
            with torch.no_grad():
                autodiff._SpectralKappa.apply(A, B, *par, args.family)

        def both():
            for t in [A, B] + par:
                t.grad = None
            (autodiff._SpectralKappa.apply(A, B, *par, args.family) * G).sum().backward()

        for row in timed({"kappa forward": forward, "kappa forward+backward": both, "SVGP step": step}, ("hip",), lambda r: None, args, base):
            print(json.dumps(row), flush=True)
        del m, step, A, B, G
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
