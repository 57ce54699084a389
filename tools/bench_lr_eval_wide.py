#!/usr/bin/env python3
"""The low-rank evaluation path on WIDE state spaces: CMUsubject16's shape (126 columns, L = 500, c = r = 50, M = 4, T = 500 inducing tensors with
increments) and the tensors' map at PEMS' 1,928 columns.  Beyond about 120 columns no sequence tile holds the points in LDS: the library computes
the Nystrom cross matrix on the float64 matrix cores from the raw points and runs the feature kernels that take it from memory (the wide route,
csrc/lr_eval_wide_inst.hip); a library before that route takes the multi-pass route (one thread per cross-matrix entry, five (N, L, c) arrays).

    python tools/bench_lr_eval_wide.py                       # one process, the library in GPSIG_LIB (default: this build's)
    python tools/bench_lr_eval_wide.py --ab libgpsig_hip_parent.so > profiles/lowrank_eval_wide.txt
                                                             # alternating processes: this build, gpsig_amd/lib/<that library> (the parent
                                                             # commit's), and this build with lr_fused = 0 (the multi-pass route), --rounds each

Per line one JSON object: the median and the block medians of the HIP-event times of one call (the protocol of tools/bench_lr_eval_long.py:
alternating blocks of warm-up + timed calls, the spread of the block medians is the noise figure), and the context's scratch bytes after it
(gpsig_scratch_bytes: the peak, the context only grows its buffers).
  K_tens_n_seq_covs      what models.SVGP.predict_f evaluates, CUDA tensors, one shared draw per evaluation
  seq_features           gpsig_lr_seq_features alone on a fixed state (device pointers)
  tens_features          gpsig_lr_tens_features alone
  ragged                 K_tens_n_seq_covs with lengths uniform in 4 .. 500 (this build only: the parent refuses it at this width)
float32 runs with lr_native_f32: the parent computes those calls in float64 and rounds (kernels._f32_upcast); with lr_fused = 0 so does this build."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def timed(fn, warmup, iters, reps):
    import torch
    blocks = []
    for _ in range(reps):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        blocks.append([a.elapsed_time(b) for a, b in ev])
    return blocks


def report(args, row, blocks, ctx):
    meds = [float(np.median(b)) for b in blocks]
    row.update(lib=os.path.basename(os.environ.get("GPSIG_LIB") or "libgpsig_hip.so"), lr_fused=args.lr_fused,
               ms_median=round(float(np.median(np.concatenate(blocks))), 3), ms_block_medians=[round(m, 3) for m in meds],
               block_spread=round((max(meds) - min(meds)) / float(np.median(meds)), 4), scratch_bytes=ctx.scratch_bytes())
    print(json.dumps(row), flush=True)


def features_fn(k, st, A, lengths=None):
    from gpsig_amd import kernels

    def fn():
        L_ = kernels._Launch(A)
        return k._lr_features(L_, k._params(L_.keep, L_.dtype_id), st.as_c(L_.keep), A, lengths=lengths)[0]
    return fn


def measure(args):
    import torch
    from gpsig_amd import _lib, kernels
    dev = torch.device("cuda:0")
    M, d, c, T, L = 4, args.d, 50, 500, args.L
    rng = np.random.default_rng(0)
    Z = torch.as_tensor(rng.standard_normal((M * (M + 1) // 2, T, 2, d)), device=dev)
    ctx = _lib.context(0, torch.cuda.current_stream(dev).cuda_stream)
    if args.lr_fused is not None:
        ctx.set_option("lr_fused", args.lr_fused)

    def kernel(width, dtype):
        k = kernels.SignatureRBF(L * width, width, M, low_rank=True, num_components=c, rank_bound=c, lengthscales=np.full(width, np.sqrt(width)))
        k.rng = np.random.default_rng(1)
        k.lr_native_f32 = dtype == "float32"
        return k

    # float32 is wide from twice the columns on (65 c + 138 max(c, r, d') floats): at --d it runs the tiled float32 kernel in both libraries
    widths = {"float64": [d], "float32": [d] + ([args.d_f32] if args.d_f32 else [])}
    for N in args.N:
        for dtype in args.dtypes:
            for w in widths[dtype]:
                gen = torch.Generator(device=dev).manual_seed(N)         # (on the device: the table has up to 3 * 10^9 entries)
                X64 = torch.cumsum(0.3 * torch.randn((N, L, w), device=dev, dtype=torch.float64, generator=gen), dim=1).reshape(N, L * w)
                Z64 = Z if w == d else torch.as_tensor(np.random.default_rng(2).standard_normal((M * (M + 1) // 2, T, 2, w)), device=dev)
                k = kernel(w, dtype)
                X = X64.float() if dtype == "float32" else X64
                Zt = Z64.float() if dtype == "float32" else Z64
                del X64
                report(args, dict(N=N, L=L, d=w, dtype=dtype, what="K_tens_n_seq_covs"),
                       timed(lambda: k.K_tens_n_seq_covs(Zt, X, increments=True), args.warmup, args.iters, args.reps), ctx)
                if dtype == "float64" or args.lr_fused != 0:          # (the C entry point refuses float32 on the multi-pass route)
                    st = k.draw_low_rank(X=X[:64], Z=Zt, increments=True)
                    try:
                        report(args, dict(N=N, L=L, d=w, dtype=dtype, what="seq_features"),
                               timed(features_fn(k, st, X), args.warmup, args.iters, args.reps), ctx)
                    except NotImplementedError as e:                   # the parent's library in float32 beyond its tiled kernel
                        print(json.dumps(dict(N=N, L=L, d=w, dtype=dtype, what="seq_features", refused=str(e)[:80])), flush=True)
                del X
    if args.ragged:
        N = args.N[0]
        lengths = rng.integers(4, L + 1, size=N)
        full = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1)
        for n, l in enumerate(lengths):
            full[n, l:] = np.nan
        ragged = torch.as_tensor(full.reshape(N, L * d), device=dev)
        lens = torch.as_tensor(lengths.astype(np.int32), device=dev)
        k = kernel(d, "float64")
        report(args, dict(N=N, L=L, d=d, dtype="float64", what="ragged K_tens_n_seq_covs, lengths 4..%d (mean %.0f)" % (L, lengths.mean())),
               timed(lambda: k.K_tens_n_seq_covs(Z, ragged, increments=True, lengths=lens), args.warmup, args.iters, args.reps), ctx)
    # the tensors' map alone at PEMS' width
    dw = args.d_tens
    Zw = torch.as_tensor(rng.standard_normal((M * (M + 1) // 2, T, 2, dw)), device=dev)
    for dtype in args.dtypes:
        if dtype == "float32" and args.lr_fused == 0:
            continue
        k = kernels.SignatureRBF(16 * dw, dw, M, low_rank=True, num_components=c, rank_bound=c, lengthscales=np.full(dw, np.sqrt(dw)))
        k.rng = np.random.default_rng(1)
        k.lr_native_f32 = dtype == "float32"
        Zt = Zw.float() if dtype == "float32" else Zw
        st = k.draw_low_rank(Z=Zt, increments=True)

        def fn():
            L_ = kernels._Launch(Zt)
            return k._lr_features(L_, k._params(L_.keep, L_.dtype_id), st.as_c(L_.keep), Zt, tensors=True, increments=True)[0]
        try:
            report(args, dict(T=T, d=dw, dtype=dtype, what="tens_features"), timed(fn, args.warmup, args.iters, args.reps), ctx)
        except NotImplementedError as e:
            print(json.dumps(dict(T=T, d=dw, dtype=dtype, what="tens_features", refused=str(e)[:80])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--L", type=int, default=500)
    ap.add_argument("--d", type=int, default=126)
    ap.add_argument("--d-f32", dest="d_f32", type=int, default=320, help="a second width for float32, beyond its tiled kernel (0: none)")
    ap.add_argument("--d-tens", dest="d_tens", type=int, default=1928)
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--lr-fused", dest="lr_fused", type=int, default=None)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ab", default=None, help="a library under gpsig_amd/lib to alternate with, in processes of their own")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--child-timeout", type=int, default=400)
    args = ap.parse_args()
    if not args.ab:
        return measure(args)
    common = ["--N"] + [str(n) for n in args.N] + ["--L", str(args.L), "--d", str(args.d), "--d-tens", str(args.d_tens), "--d-f32", str(args.d_f32), "--dtypes"] + args.dtypes + [
        "--warmup", str(args.warmup), "--iters", str(args.iters), "--reps", str(args.reps)]
    runs = [(None, ["--ragged"] if args.ragged else []), (args.ab, []), (None, ["--lr-fused", "0"])]
    for _ in range(args.rounds):
        for lib, extra in runs:
            env = dict(os.environ)
            env.pop("GPSIG_LIB", None)
            if lib:
                env["GPSIG_LIB"] = os.path.join(ROOT, "gpsig_amd", "lib", lib)
            rc = subprocess.run([sys.executable, os.path.abspath(__file__)] + common + extra, env=env, timeout=args.child_timeout).returncode
            if rc != 0:              # a child that failed ends the run: nothing more is started on the device
                sys.exit(rc)


if __name__ == "__main__":
    main()
