"""Host checks of device headers that are plain C++: gpsig_amd/csrc/fast_exp.hpp (the table-driven float64 exp of the RBF / Matern
envelopes) against the long-double library
exp, on the host: the header's arithmetic is fma / rint / ldexp only, so the device computes the same bits."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fast_exp_within_one_and_a_half_ulp(tmp_path):
    exe = str(tmp_path / "test_fast_exp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "gpsig_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "test_fast_exp.cpp")])
    worst_a, worst_t, worst_1024, worst_2048, worst_2l, edges = subprocess.check_output([exe, "2000000"]).split()
    assert float(worst_a) < 1.5 and float(worst_t) < 1.5, (worst_a, worst_t)
    # the degree-3 variants: 2048 entries lose nothing; 1024 entries (what the Kzx tile kernel takes for incremental tensors) drop a
    # term of 5.5e-16 relative at the ends of the reduction interval: observed 5.8 ulp, nine orders below the 1e-6 parity tolerance
    assert float(worst_2048) < 1.5 and float(worst_1024) < 6.5, (worst_1024, worst_2048)
    # the two-level form of the 1024-entry table (two conflict-free tables of 32 entries): one more rounding, the entries' product
    assert float(worst_2l) < 7.5, worst_2l
    assert int(edges) == 1


def test_tile_kernel_level_partition(tmp_path):
    """gpsig_amd/csrc/tvs_plan.hpp: how the Kzx tile kernel deals the signature levels to the waves of a workgroup."""
    exe = str(tmp_path / "test_tvs_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "gpsig_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "test_tvs_plan.cpp")])
    assert subprocess.check_output([exe]).split() == [b"0"]


def test_contraction_depth_pieces(tmp_path):
    """gpsig_amd/csrc/sig_pieces.hpp: the depth pieces of the feature contraction (equal pieces as in round 3, the last one cut into
    finer ones of halving size in round 4) cover every slab exactly once and depend on the depth and the two counts alone; the model that
    chooses the two counts (sig_piece_counts) stays within its bounds and SigGramArgs::bound over a grid of sizes, and gives the pinned values."""
    exe, max_pieces = sig_pieces_exe(tmp_path)
    assert subprocess.check_output([exe, max_pieces]).split() == [b"0"]


def sig_pieces_exe(tmp_path):
    """tests/emu/test_sig_pieces.cpp, stand-alone, under the address and undefined-behaviour sanitizers; and SG_MAX_PIECES as sig_feat_kernel.hpp has it"""
    exe = str(tmp_path / "test_sig_pieces")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "gpsig_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "emu", "test_sig_pieces.cpp")])
    with open(os.path.join(ROOT, "gpsig_amd", "csrc", "sig_feat_kernel.hpp")) as f:
        return exe, re.search(r"constexpr int SG_MAX_PIECES = (\d+);", f.read()).group(1)


def test_contraction_piece_counts_against_their_restatements(tmp_path):
    """gpsig_amd/csrc/sig_pieces.hpp: sig_piece_counts, which sig_features_K (sig_feat_api.hip) asks for the number of depth pieces, against the
    two Python restatements of the model: planned_pieces of test_gpu_gram_diag_tiles.py over its domain (no graded tail: at most 512 workgroups)
    and bench.py's depth_pieces (the equal pieces of any symmetric Gram)."""
    import importlib.util
    from test_gpu_gram_diag_tiles import planned_pieces
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    exe, max_pieces = sig_pieces_exe(tmp_path)
    rows = [[int(v) for v in line.split()] for line in subprocess.check_output([exe, max_pieces, "plans"]).decode().splitlines()]
    assert len(rows) > 100
    in_domain = 0
    for N, d, M, nslab, nsplit, graded in rows:
        tiles = ((N + 127) // 128) * ((N + 127) // 128 + 1) // 2
        assert bench.depth_pieces(N, nslab) == nsplit, (N, d, M)
        if tiles * nsplit <= 512:
            in_domain += 1
            assert planned_pieces(N, d, M) == (nslab, nsplit) and graded == 1, (N, d, M)
    assert 20 < in_domain < len(rows)
