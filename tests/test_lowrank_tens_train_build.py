"""The reverse kernels of the inducing tensors' low-rank feature map (csrc/lr_tens_grad_kernel.hpp), from the compiler's report (no GPU
needed): both instances exist in their unit and keep no scratch; and the four entry points around them are declared where the ABI lives."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = ("_ZN5gpsig28lr_tens_features_grad_kernelENS_14LrTensGradArgsE",
           "_ZN5gpsig37lr_tens_features_grad_spectral_kernelENS_22LrTensGradSpectralArgsE")
SYMBOLS = ("gpsig_lr_tens_features_dev", "gpsig_lr_tens_features_grad", "gpsig_lr_tens_features_spectral_dev",
           "gpsig_lr_tens_features_spectral_grad")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "gpsig_amd", "csrc", "lr_grad_api.hip")
    out = str(tmp_path_factory.mktemp("lr_tens") / "lr_grad_api.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, src],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


@pytest.mark.parametrize("name", KERNELS)
def test_reverse_kernels_keep_no_scratch(report, name):
    start = report.find("\n" + name + ":")
    assert start >= 0, "kernel %s not in the compiler's output" % name
    m = re.search(r"; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", report[start:], re.S)
    assert m, name
    vgprs, scratch, occupancy = (int(g) for g in m.groups())
    print(name, "VGPRs", vgprs, "scratch", scratch, "occupancy", occupancy)
    assert scratch == 0, (name, scratch)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_entry_points_are_declared(symbol):
    from gpsig_amd import _lib
    with open(os.path.join(ROOT, "include", "gpsig_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint %s\(gpsig_ctx\* ctx" % symbol, header), symbol
    assert symbol in _lib.ALL_SYMBOLS
    with open(os.path.join(ROOT, "gpsig_amd", "csrc", "lr_grad_api.hip")) as f:
        assert re.search(r"\bint %s\(gpsig_ctx\* c" % symbol, f.read()), symbol
