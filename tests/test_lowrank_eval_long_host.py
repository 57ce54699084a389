"""The low-rank evaluation path on long and ragged batches, without a GPU: the ``lengths=`` checks of gpsig_amd.kernels (they run before any
library call), the new entry point's registration, the tile plan of the time-tiled evaluation kernels (csrc/lr_tile_plan.hpp:
lr_eval_tile_dir) against a recomputation here, and the compiler's report of the new unit (every kernel exists for gfx950 and keeps no
scratch memory)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsig_amd", "csrc")
MAX_LDS = 156 * 1024


def _kern(**kw):
    from gpsig_amd import kernels
    return kernels.SignatureRBF(20, 2, 2, **kw)


X = np.cumsum(np.random.default_rng(0).standard_normal((4, 10, 2)), axis=1).reshape(4, 20)
GOOD = [10, 3, 1, 7]
METHODS = {
    "K": lambda k, l: k.K(X, lengths=l),
    "K lengths2": lambda k, l: k.K(X, X, lengths2=l),
    "Kdiag": lambda k, l: k.Kdiag(X, lengths=l),
    "K_tens_vs_seq": lambda k, l: k.K_tens_vs_seq(np.zeros((3, 2, 2)), X, lengths=l),
    "K_tens_n_seq_covs": lambda k, l: k.K_tens_n_seq_covs(np.zeros((3, 2, 2)), X, lengths=l),
    "K_seq_n_seq_covs": lambda k, l: k.K_seq_n_seq_covs(X[:2], X, lengths2=l),
    "draw_low_rank": lambda k, l: k.draw_low_rank(X=X, lengths=l),
}


@pytest.mark.parametrize("method", sorted(METHODS))
def test_exact_mode_and_lags_refuse_lengths(method):
    with pytest.raises(NotImplementedError, match="repeating its last observation"):
        METHODS[method](_kern(), GOOD)
    with pytest.raises(NotImplementedError, match="num_lags"):
        METHODS[method](_kern(low_rank=True, num_components=6, rank_bound=5, num_lags=1), GOOD)


@pytest.mark.parametrize("method", sorted(METHODS))
@pytest.mark.parametrize("bad", [np.asarray(GOOD, dtype=np.float64), GOOD[:3], [[10, 3, 1, 7]], [0, 3, 1, 7], [11, 3, 1, 7]],
                         ids=["float", "short", "2-d", "zero", "L+1"])
def test_bad_lengths_are_value_errors(method, bad):
    with pytest.raises(ValueError, match="lengths"):
        METHODS[method](_kern(low_rank=True, num_components=6, rank_bound=5), bad)


def test_lengths_are_accepted_as_ints_arrays_and_tensors():
    import torch
    k = _kern(low_rank=True, num_components=6, rank_bound=5)
    for given in (GOOD, np.asarray(GOOD), np.asarray(GOOD, dtype=np.uint8), torch.tensor(GOOD)):
        got = k._ragged_lengths(given, X)
        assert got.dtype == np.int32 and got.tolist() == GOOD
    assert k._ragged_lengths(None, X) is None


def test_real_points_replace_padded_rows_by_the_last_valid_row():
    import torch
    k = _kern(low_rank=True, num_components=6, rank_bound=5)
    Xn = X.reshape(4, 10, 2).copy()
    want = Xn.copy()
    for n, l in enumerate(GOOD):
        Xn[n, l:] = np.nan
        want[n, l:] = want[n, l - 1]
    lens = k._ragged_lengths(GOOD, X)
    assert np.array_equal(k._real_points(Xn.reshape(4, 20), lens), want.reshape(4, 20))
    assert np.array_equal(k._real_points(torch.tensor(Xn.reshape(4, 20)), lens).numpy(), want.reshape(4, 20))
    assert k._real_points(X, None) is X


def test_the_entry_point_is_declared_and_registered():
    from gpsig_amd import _lib
    assert "gpsig_lr_seq_features_ragged" in _lib.ALL_SYMBOLS
    with open(os.path.join(ROOT, "include", "gpsig_hip.h")) as f:
        hdr = f.read()
    assert re.search(r"int gpsig_lr_seq_features_ragged\(gpsig_ctx\* ctx, const gpsig_params\* p, const gpsig_lowrank\* lr, const void\* X, "
                     r"int64_t N, int32_t L,\s*const int32_t\* lengths, void\* Phi\);", hdr)


# ---- the tile plan ------------------------------------------------------------------------------------------------------------------
def footprint(f32, c, r, d, TL, pad):
    """U [c], two work arrays [rows] of row stride TL + max(pad, 1), one carry row for each of 8 levels, in the element type"""
    rows = max(c, r, d)
    return (4 if f32 else 8) * ((TL + max(pad, 1)) * (c + 2 * rows) + 8 * rows)


SHAPES = [(f32, c, r, d, l, pad) for f32 in (0, 1) for (c, r, d, l) in ((64, 64, 3, 385), (50, 50, 6, 499), (12, 7, 3, 514), (4, 3, 9, 899),
                                                                         (16, 12, 3, 69), (120, 100, 3, 100), (400, 300, 3, 100))
          for pad in (0, 1, 3)]


def test_tile_plan_against_a_recomputation(tmp_path):
    exe = str(tmp_path / "lr_eval_plan_print")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "lr_eval_plan_print.cpp")])
    args = [str(v) for s in SHAPES for v in s]
    res = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().split("\n")[:len(SHAPES)]
    tiled = 0
    for (f32, c, r, d, l, pad), line in zip(SHAPES, lines):
        TL, ntiles, lp, lds, whole = (int(v) for v in line.split())
        assert TL % 64 == 0 and TL >= 0
        assert footprint(f32, c, r, d, TL + 64, pad) > MAX_LDS, (f32, c, r, d, TL)
        if TL == 0:                                          # not even one tile: nothing to launch
            assert footprint(f32, c, r, d, 64, pad) > MAX_LDS and ntiles == 0 and lds == 0
            continue
        assert lds == footprint(f32, c, r, d, TL, pad) <= MAX_LDS
        assert lp == TL + max(pad, 1) and ntiles == -(-l // TL)
        rows = max(c, r, d)
        assert whole == (4 if f32 else 8) * (((l + 1 + 63) // 64 * 64 + pad) * (c + 2 * rows))
        tiled += 1
    assert tiled == len(SHAPES) - 9              # no float64 tile at 120 rows, none in either type at 400
    # the figures the documents quote: 64 rows -> tiles of 64 (float64) and 192 (float32) steps
    by = {s: int(line.split()[0]) for s, line in zip(SHAPES, lines)}
    assert by[(0, 64, 64, 3, 385, 1)] == 64 and by[(1, 64, 64, 3, 385, 1)] == 192
    assert by[(1, 50, 50, 6, 499, 1)] >= 2 * by[(0, 50, 50, 6, 499, 1)] - 64


# ---- the compiler's report -----------------------------------------------------------------------------------------------------------
KERNELS = ("lr_seq_features_eval_tiled_kernel", "lr_seq_features_eval_tiled_spectral_kernel", "lr_seq_features_eval_tiled_f32_kernel")


def test_new_kernels_exist_and_keep_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path / "lr_eval_tiled_inst.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(CSRC, "lr_eval_tiled_inst.hip")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        text = f.read()
    for kernel in KERNELS:
        names = re.findall(r"^(_ZN5gpsig\d+%sENS_\w+E):" % kernel, text, re.M)
        assert len(names) == 1, (kernel, names)
        m = re.search(r"; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", text[text.find("\n" + names[0] + ":"):], re.S)
        assert m, kernel
        vgprs, scratch, occupancy = (int(g) for g in m.groups())
        print(kernel, "VGPRs", vgprs, "scratch", scratch, "occupancy", occupancy)
        assert scratch == 0 and vgprs <= 128 and occupancy >= 4, (kernel, vgprs, scratch, occupancy)
    # the out-of-line spectral term as well
    for m in re.finditer(r"; ScratchSize: (\d+)", text):
        assert int(m.group(1)) == 0
