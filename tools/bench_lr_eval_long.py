#!/usr/bin/env python3
"""The low-rank evaluation path on long and ragged batches: gpsig_amd.kernels.SignatureKernel.K_tens_n_seq_covs (what models.SVGP.predict_f
evaluates) at T = 500 inducing tensors, M = 4, increments, c = r = 50, d = 6, sequences beyond the whole-sequence kernels' L <= 128.

    python tools/bench_lr_eval_long.py                       # one process, the library in GPSIG_LIB (default: this build's)
    python tools/bench_lr_eval_long.py --ab libgpsig_hip_parent.so > profiles/lowrank_eval_long.txt
                                                             # alternating processes: this build, gpsig_amd/lib/<that library>, and this build
                                                             # with lr_fused = 0 (the multi-pass route), --rounds times each

Per (N, L, dtype) one JSON line: the median and the block medians of the HIP-event times of one evaluation (CUDA tensors, one shared draw per
evaluation, as predict_f does), the context's scratch bytes after it (gpsig_scratch_bytes; a library without that symbol reports null) and the
process's own VRAM as the kernel driver accounts it (/proc/self/fdinfo: drm-memory-vram; not the device-wide figure -- the device is shared).
float32 runs with lr_native_f32.  --ragged adds N = 1,024, L = 500 with lengths uniform in 4 .. 500 (``lengths=``) against the same table
padded by repetition of each sequence's last observation.

A library older than this tool lacks the entry points added since: --legacy drops them from the binding's symbol table before it loads
(--ab passes it for the other library), and the ragged line is skipped there."""
import argparse
import glob
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

NEW_SYMBOLS = ("gpsig_scratch_bytes", "gpsig_lr_seq_features_ragged")


def own_vram_bytes():
    """the process's VRAM by its DRM clients (one entry per client id)"""
    seen, total = set(), 0
    for fn in glob.glob("/proc/self/fdinfo/*"):
        try:
            with open(fn) as f:
                text = f.read()
        except OSError:
            continue
        if "drm-memory-vram" not in text:
            continue
        fields = dict(l.split(":", 1) for l in text.splitlines() if ":" in l)
        cid = fields.get("drm-client-id", "").strip()
        if cid in seen:
            continue
        seen.add(cid)
        v = fields["drm-memory-vram"].split()
        total += int(v[0]) * {"KiB": 1 << 10, "MiB": 1 << 20, "GiB": 1 << 30}.get(v[1] if len(v) > 1 else "", 1)
    return total if seen else None


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


def measure(args):
    import torch
    from gpsig_amd import _lib
    if args.legacy:
        for name in NEW_SYMBOLS:
            _lib._PLAIN.pop(name, None)
            _lib._KERNEL_FUNCS.pop(name, None)
    from gpsig_amd import kernels
    dev = torch.device("cuda:0")
    M, d, c, T = 4, 6, 50, 500
    rng = np.random.default_rng(0)
    Z = torch.as_tensor(rng.standard_normal((M * (M + 1) // 2, T, 2, d)), device=dev)
    shapes = [(N, L) for N in args.N for L in args.L]
    for N, L in shapes:
        X64 = torch.as_tensor(np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1).reshape(N, L * d), device=dev)
        for dtype in args.dtypes:
            k = kernels.SignatureRBF(L * d, d, M, low_rank=True, num_components=c, rank_bound=c, lengthscales=np.ones(d))
            k.rng = np.random.default_rng(1)
            k.lr_native_f32 = dtype == "float32"
            X = X64.float() if dtype == "float32" else X64
            Zt = Z.float() if dtype == "float32" else Z
            ctx = _lib.context(0, torch.cuda.current_stream(dev).cuda_stream)
            if args.lr_fused is not None:
                ctx.set_option("lr_fused", args.lr_fused)
            blocks = timed(lambda: k.K_tens_n_seq_covs(Zt, X, increments=True), args.warmup, args.iters, args.reps)
            report(args, dict(N=N, L=L, dtype=dtype, what="K_tens_n_seq_covs"), blocks, ctx)
    if args.ragged and not args.legacy:
        N, L = 1024, 500
        lengths = rng.integers(4, L + 1, size=N)
        full = np.cumsum(0.3 * rng.standard_normal((N, L, d)), axis=1)
        idx = np.minimum(np.arange(L)[None, :], lengths[:, None] - 1)
        padded = torch.as_tensor(full[np.arange(N)[:, None], idx].reshape(N, L * d), device=dev)
        for n, l in enumerate(lengths):
            full[n, l:] = np.nan
        ragged = torch.as_tensor(full.reshape(N, L * d), device=dev)
        lens = torch.as_tensor(lengths.astype(np.int32), device=dev)
        k = kernels.SignatureRBF(L * d, d, M, low_rank=True, num_components=c, rank_bound=c, lengthscales=np.ones(d))
        k.rng = np.random.default_rng(1)
        ctx = _lib.context(0, torch.cuda.current_stream(dev).cuda_stream)
        for what, fn in (("ragged, lengths 4..500 (mean %.0f)" % lengths.mean(), lambda: k.K_tens_n_seq_covs(Z, ragged, increments=True, lengths=lens)),
                         ("the same table padded by repetition", lambda: k.K_tens_n_seq_covs(Z, padded, increments=True))):
            report(args, dict(N=N, L=L, dtype="float64", what=what), timed(fn, args.warmup, args.iters, args.reps), ctx)


def report(args, row, blocks, ctx):
    meds = [float(np.median(b)) for b in blocks]
    row.update(lib=os.path.basename(os.environ.get("GPSIG_LIB") or "libgpsig_hip.so"), lr_fused=args.lr_fused,
               ms_median=round(float(np.median(np.concatenate(blocks))), 3), ms_block_medians=[round(m, 3) for m in meds],
               scratch_bytes=None if args.legacy else ctx.scratch_bytes(), own_vram_bytes=own_vram_bytes())
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--L", type=int, nargs="+", default=[200, 500])
    ap.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    ap.add_argument("--lr-fused", dest="lr_fused", type=int, default=None)
    ap.add_argument("--ragged", action="store_true")
    ap.add_argument("--legacy", action="store_true", help="the library in GPSIG_LIB predates gpsig_scratch_bytes / gpsig_lr_seq_features_ragged")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ab", default=None, help="a library under gpsig_amd/lib to alternate with, in processes of their own")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--child-timeout", type=int, default=240)
    args = ap.parse_args()
    if not args.ab:
        return measure(args)
    common = ["--N"] + [str(n) for n in args.N] + ["--L"] + [str(l) for l in args.L] + ["--dtypes"] + args.dtypes + [
        "--warmup", str(args.warmup), "--iters", str(args.iters), "--reps", str(args.reps)]
    runs = [(None, ["--ragged"] if args.ragged else []), (args.ab, ["--legacy"]), (None, ["--lr-fused", "0"])]
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
