"""The kernels of the spectral cross op beyond 32 columns (csrc/lr_cross_spectral_kernel.hpp, instances in csrc/lr_cross_spectral_inst.hip), from
the compiler's report (no GPU needed): the unit compiles for gfx950, every kernel is in it and keeps no scratch.  Registers, LDS and occupancy
are printed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = "lr_cross_spectral_inst"
KERNELS = (
    "_ZN5gpsig18lr_spx_prep_kernelEPKdlPd",
    "_ZN5gpsig19lr_spx_norms_kernelEPKdiiS1_Pd",
    "_ZN5gpsig19lr_spx_phase_kernelEPKdliS1_iPd",
    "_ZN5gpsig13lr_spx_kernelILb0EEEvNS_9LrSpxArgsE",
    "_ZN5gpsig13lr_spx_kernelILb1EEEvNS_9LrSpxArgsE",
    "_ZN5gpsig20lr_spx_points_kernelENS_9LrSpxArgsE",
    "_ZN5gpsig23lr_spx_landmarks_kernelENS_9LrSpxArgsE",
    "_ZN5gpsig20lr_spx_reduce_kernelEPKdiliPd",
    "_ZN5gpsig20lr_spx_finish_kernelENS_9LrSpxArgsEPKdS2_PdS3_S3_S3_",
)
FIELDS = (r"codeLenInByte = (\d+)", r"; TotalNumSgprs: (\d+)", r"; NumVgprs: (\d+)", r"; NumAgprs: (\d+)", r"; ScratchSize: (\d+)",
          r"; LDSByteSize: (\d+)", r"; Occupancy: (\d+)")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "gpsig_amd", "csrc", UNIT + ".hip")
    dst = str(tmp_path_factory.mktemp("lr_spectral_wide") / (UNIT + ".s"))
    proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst, src],
                          stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    with open(dst) as f:
        return f.read()


def numbers(report, name):
    start = report.find("\n" + name + ":")
    assert start >= 0, "kernel %s not in the compiler's output" % name
    end = report.find("; Occupancy:", start)
    block = report[start:report.find("\n", end)]
    return tuple(int(re.search(f, block).group(1)) for f in FIELDS)


@pytest.mark.parametrize("name", KERNELS)
def test_kernels_keep_no_scratch(report, name):
    code, sgprs, vgprs, agprs, scratch, lds, occupancy = numbers(report, name)
    print(name, "code", code, "SGPRs", sgprs, "VGPRs", vgprs, "AGPRs", agprs, "scratch", scratch, "LDS", lds, "occupancy", occupancy)
    assert scratch == 0, (name, scratch)


def test_no_other_kernel_in_the_unit(report):
    found = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", report, flags=re.M))
    assert found == set(KERNELS), found ^ set(KERNELS)
