"""The time-tiled low-rank sequence feature kernels (csrc/lr_tile_plan.hpp, lr_tiled_kernel.hpp) without a GPU: the tile plan on the host
under the address and undefined-behaviour sanitizers, and the compiler's report of the two kernels (both exist for gfx950 and keep no
scratch memory)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsig_amd", "csrc")

KERNELS = ("lr_seq_features_tiled_kernel", "lr_seq_features_grad_tiled_kernel")


def test_tile_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "test_lr_tile_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "test_lr_tile_plan.cpp")])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, (res.stdout.decode(), res.stderr.decode()[-2000:])
    bad, plans = res.stdout.split()[-2:]
    assert int(bad) == 0 and int(plans) > 1000000


def test_python_guard_is_the_plan_of_one_tile():
    """autodiff._LowRankScope.seq restates "one 64-step tile fits" of lr_tile_plan.hpp: the same numbers on both sides."""
    with open(os.path.join(CSRC, "lr_tile_plan.hpp")) as f:
        hdr = f.read()
    assert "LR_FUSED_MAX_LDS = 156 * 1024" in hdr and "LR_TILE_STEP = 64" in hdr and "LR_TILE_LEVELS = 8" in hdr
    with open(os.path.join(ROOT, "gpsig_amd", "autodiff.py")) as f:
        src = f.read()
    assert "8 * (65 * 4 * rows + 17 * rows), 8 * (65 * (cc + 2 * max(cc, r, d)) + 8 * max(cc, r, d))) <= 156 * 1024" in src


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("lr_tiled") / "lr_grad_api.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(CSRC, "lr_grad_api.hip")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


@pytest.mark.parametrize("kernel", KERNELS)
def test_tiled_kernels_keep_no_scratch(report, kernel):
    names = re.findall(r"^(_ZN5gpsig\d+%sILi\d+EEEvNS_11LrTiledArgsE):" % kernel, report, re.M)
    assert names, "kernel %s not in the compiler's output" % kernel
    for name in names:
        m = re.search(r"; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", report[report.find("\n" + name + ":"):], re.S)
        assert m, name
        vgprs, scratch, occupancy = (int(g) for g in m.groups())
        print(name, "VGPRs", vgprs, "scratch", scratch, "occupancy", occupancy)
        assert scratch == 0, (name, scratch)
