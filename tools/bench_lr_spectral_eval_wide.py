#!/usr/bin/env python3
"""Low-rank SignatureSpectral EVALUATION on a wide state space, at the spectral form of CMUsubject16's shape (63 columns with time, L = 500, 50
components and rank 50, 500 inducing tensors with increments, 4 levels, Q = 5 components of family rbf): the library's own surface with the kernel
object's opt-in ``lr_spectral_wide`` (the evaluation form of the spectral cross kernel, csrc/lr_eval_spectral_wide_inst.hip, then the feature
kernels that take kxs / kzs from memory) against what the same build -- and the commit before the opt-in -- offers for these evaluations.

    python tools/bench_lr_spectral_eval_wide.py [--N 1024 16384] > profiles/lowrank_spectral_eval_wide.txt

One process, alternating blocks (the protocol of tools/bench_lr_eval_wide.py and tools/bench_lr_spectral_wide.py): per batch size every (quantity,
side) is timed --blocks times in turn, so that drift of the device hits both sides alike.  One JSON line per (N, quantity): per side the median of
the block medians of the HIP-event times, the block medians themselves and their spread -- the figure a difference has to exceed --; new / old.
Quantities:
    (a) K_tens_n_seq_covs     new: kernels.SignatureSpectral.K_tens_n_seq_covs with the flag (what models.SVGP.predict_f evaluates), one shared
                              draw per evaluation; old: SignatureKernelModule.K_tens_n_seq_covs of SVGPModule under torch.no_grad()
                              (gpsig_spectral_cross + the kx training instances), the code a user of the commit before has for it
    (b) sequence features     on a fixed state and the same points.  new: gpsig_lr_seq_features (cross kernel with the phases in its walk + kx
                              feature kernel); old: gpsig_spectral_cross forward (phase kernel, (Q, n) round trip, cross kernel) followed by
                              gpsig_lr_seq_features_kx_dev -- the same feature kernel, so the difference is the cross kernels'.  A second line
                              times the old cross op alone.  The new cross kernel has no entry point of its own: kernel against kernel is read
                              from a kernel trace of this tool (rocprofv3 --kernel-trace --stats, a run of its own), lr_spx_eval_kernel against
                              lr_spx_phase_kernel + lr_spx_kernel<false>
    (c) ragged                new only: K_tens_n_seq_covs with lengths uniform in 4 .. L against the same call at full lengths"""
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
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(N)
    Xt = torch.cumsum(0.2 * torch.randn((N, L, d), device=dev, dtype=torch.float64, generator=gen), dim=1).reshape(N, L * d)
    Z = rng.standard_normal((M * (M + 1) // 2, T, 2, d)) * 0.5
    Zt = torch.tensor(Z, device=dev)
    kern = kernels.SignatureSpectral(L * d, d, M, family=args.family, Q=Q, low_rank=True, num_components=c, rank_bound=c)
    kern.alpha, kern.omega, kern.gamma = np.ones(Q), np.full((Q, d), 0.1), np.full((Q, d), 1.0 / np.sqrt(d))
    kern.rng = np.random.default_rng(3)
    m = models.SVGPModule(kern, inducing_variables.InducingTensors(Z, M, increments=True), likelihoods.Bernoulli(), num_data=N, device=dev)
    mod = m.kernel
    kern.lr_spectral_wide = True
    lengths = torch.as_tensor(rng.integers(4, L + 1, size=N).astype(np.int32), device=dev)

    h = st = kern.draw_low_rank(X=Xt[:64].cpu().numpy(), Z=Z, increments=True)        # (b)'s fixed state: drawn on the host, handed to both sides
    S, Wh = torch.tensor(h.landmarks, device=dev), torch.tensor(h.whitening, device=dev)
    par = [torch.tensor(np.ascontiguousarray(v), device=dev) for v in (kern.alpha, kern.omega, kern.gamma)]
    P = Xt.reshape(N * L, d)
    keep = []
    aux = kernels.SignatureRBF(c, c, M, lengthscales=None, low_rank=True, num_components=c, rank_bound=c)
    p_kx = aux._params(keep)
    arr = autodiff._sketch_array(h.sketches, keep)
    kxs = torch.empty((N * L, c), dtype=torch.float64, device=dev)
    out = torch.empty((N, 1 + c + (M - 1) * c), dtype=torch.float64, device=dev)
    ptr = autodiff._ptr

    def old_cross():
        lc = autodiff._ctx_for(P)
        lc.check(lc._lib.gpsig_spectral_cross(lc._h, Q, autodiff._SPECTRAL_FAMILY[args.family], d, ptr(P), N * L, ptr(S), c, *(ptr(t) for t in par),
                                              ptr(kxs)))

    def old_features():
        old_cross()
        autodiff._ctx_for(P).call("gpsig_lr_seq_features_kx_dev", p_kx, c, c, M - 1, arr, ptr(kxs), N, L, None, ptr(Wh), ptr(out))

    def new_features():
        L_ = kernels._Launch(Xt)
        kern._lr_features(L_, kern._params(L_.keep, L_.dtype_id), st.as_c(L_.keep), Xt)

    def new_covs():
        kern.K_tens_n_seq_covs(Zt, Xt, increments=True)

    def old_covs():
        with torch.no_grad():
            mod.K_tens_n_seq_covs(Zt, Xt, increments=True)

    def new_ragged():
        kern.K_tens_n_seq_covs(Zt, Xt, increments=True, lengths=lengths)

    return {"(a) K_tens_n_seq_covs": (new_covs, old_covs),
            "(b) seq features: gpsig_lr_seq_features against gpsig_spectral_cross + kx_dev": (new_features, old_features),
            "(b) the old composition's cross op alone (new side: the whole new call again)": (new_features, old_cross),
            "(c) ragged K_tens_n_seq_covs, lengths 4..%d (mean %.0f), against full lengths" % (L, float(lengths.double().mean())): (new_ragged, new_covs)}


def measure(args, N):
    import torch
    fns = quantities(args, N)
    times, iters = {}, {}
    for b in range(args.blocks):
        for what, pair in fns.items():
            for side, fn in zip(("new", "old"), pair):
                key = (what, side)
                torch.cuda.synchronize()
                if key not in iters:                 # first visit: warm up and size the block (at most --block-seconds)
                    fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    iters[key] = max(1, min(args.iters, int(args.block_seconds / max(time.perf_counter() - t0, 1e-6))))
                times.setdefault(key, []).append(block(fn, iters[key]))
    for what in fns:
        row = dict(family=args.family, Q=args.Q, N=N, L=args.L, d=args.d, M=args.M, num_components=args.components, T=args.T, what=what)
        for side in ("new", "old"):
            v = times[(what, side)]
            row[side + "_ms"] = round(float(np.median(v)), 3)
            row[side + "_ms_blocks"] = [round(x, 3) for x in v]
            row[side + "_spread_ms"] = round(max(v) - min(v), 3)
        row["new_over_old"] = round(row["new_ms"] / row["old_ms"], 4)
        print(json.dumps(row), flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[1024, 16384])
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
        measure(args, N)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
