"""The kernels of SignatureSpectral's low-rank evaluation side beyond 32 columns, from the compiler's report (no GPU needed): the evaluation form
of the spectral cross kernel and the landmark Gram with row stride d exist in their own unit (csrc/lr_eval_spectral_wide_inst.hip) and keep no
scratch -- registers, LDS and occupancy are printed --; and the kernels of the units the route shares with the training path
(lr_cross_spectral_inst, lr_cross_inst, lr_kx_inst) are the code they were: the report's numbers equal those of a build of the parent commit
(recorded below from that build), code length included."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

UNIT = "lr_eval_spectral_wide_inst"
NEW = (
    "_ZN5gpsig18lr_spx_eval_kernelILb0EEEvNS_13LrSpxEvalArgsE",
    "_ZN5gpsig18lr_spx_eval_kernelILb1EEEvNS_13LrSpxEvalArgsE",
    "_ZN5gpsig18lr_spx_gram_kernelEPKdS1_lliiiS1_Pd",
)
# (unit, kernel): codeLenInByte, TotalNumSgprs, NumVgprs, NumAgprs, ScratchSize, LDSByteSize, Occupancy of the parent commit's build
PARENT = {
    ("lr_cross_spectral_inst", "_ZN5gpsig18lr_spx_prep_kernelEPKdlPd"): (132, 12, 4, 0, 0, 0, 8),
    ("lr_cross_spectral_inst", "_ZN5gpsig19lr_spx_norms_kernelEPKdiiS1_Pd"): (684, 20, 20, 8, 0, 0, 8),
    ("lr_cross_spectral_inst", "_ZN5gpsig19lr_spx_phase_kernelEPKdliS1_iPd"): (3452, 82, 118, 8, 0, 33280, 4),
    ("lr_cross_spectral_inst", "_ZN5gpsig20lr_spx_points_kernelENS_9LrSpxArgsE"): (24496, 106, 252, 30, 0, 0, 1),
    ("lr_cross_spectral_inst", "_ZN5gpsig23lr_spx_landmarks_kernelENS_9LrSpxArgsE"): (4880, 70, 106, 16, 0, 0, 4),
    ("lr_cross_spectral_inst", "_ZN5gpsig20lr_spx_reduce_kernelEPKdiliPd"): (204, 13, 8, 0, 0, 0, 8),
    ("lr_cross_spectral_inst", "_ZN5gpsig20lr_spx_finish_kernelENS_9LrSpxArgsEPKdS2_PdS3_S3_S3_"): (2744, 44, 32, 0, 0, 0, 8),
    ("lr_cross_spectral_inst", "_ZN5gpsig13lr_spx_kernelILb0EEEvNS_9LrSpxArgsE"): (34472, 106, 235, 40, 0, 33280, 1),
    ("lr_cross_spectral_inst", "_ZN5gpsig13lr_spx_kernelILb1EEEvNS_9LrSpxArgsE"): (65772, 106, 239, 40, 0, 33280, 1),
    ("lr_cross_inst", "_ZN5gpsig21lr_cross_norms_kernelEPKdiiPd"): (552, 18, 16, 8, 0, 0, 8),
    ("lr_cross_inst", "_ZN5gpsig15lr_cross_kernelENS_11LrCrossArgsE"): (32760, 106, 159, 16, 0, 33280, 2),
    ("lr_cross_inst", "_ZN5gpsig27lr_cross_grad_points_kernelENS_11LrCrossArgsE"): (54644, 106, 247, 16, 0, 35360, 1),
    ("lr_cross_inst", "_ZN5gpsig30lr_cross_grad_landmarks_kernelENS_11LrCrossArgsE"): (2744, 48, 48, 8, 0, 0, 8),
    ("lr_cross_inst", "_ZN5gpsig32lr_cross_grad_reduce_cols_kernelEPKdiiPdS2_"): (212, 16, 10, 0, 0, 0, 8),
    ("lr_cross_inst", "_ZN5gpsig27lr_cross_grad_reduce_kernelEPKdiS1_S1_iiPd"): (1064, 28, 15, 0, 0, 0, 8),
    ("lr_kx_inst", "_ZN5gpsig26lr_tens_features_kx_kernelENS_12LrTensKxArgsE"): (3388, 48, 30, 0, 0, 0, 8),
    ("lr_kx_inst", "_ZN5gpsig30lr_tens_features_kx_f32_kernelENS_15LrTensKxArgsF32E"): (4820, 53, 32, 0, 0, 0, 8),
    ("lr_kx_inst", "_ZN5gpsig31lr_tens_features_grad_kx_kernelENS_16LrTensGradKxArgsE"): (10228, 106, 102, 0, 0, 0, 4),
    ("lr_kx_inst", "_ZN5gpsig31lr_seq_features_tiled_kx_kernelILi1024EEEvNS_13LrTiledKxArgsE"): (7084, 106, 66, 0, 0, 0, 7),
    ("lr_kx_inst", "_ZN5gpsig36lr_seq_features_grad_tiled_kx_kernelILi512EEEvNS_13LrTiledKxArgsE"): (17440, 106, 107, 0, 0, 0, 4),
}
FIELDS = (r"codeLenInByte = (\d+)", r"; TotalNumSgprs: (\d+)", r"; NumVgprs: (\d+)", r"; NumAgprs: (\d+)", r"; ScratchSize: (\d+)",
          r"; LDSByteSize: (\d+)", r"; Occupancy: (\d+)")


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = {}
    tmp = tmp_path_factory.mktemp("lr_spectral_eval_wide")
    procs = []
    for unit in sorted({UNIT} | {u for u, _ in PARENT}):
        src = os.path.join(ROOT, "gpsig_amd", "csrc", unit + ".hip")
        dst = str(tmp / (unit + ".s"))
        procs.append((unit, dst, subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst, src],
                                                  stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)))
    for unit, dst, proc in procs:
        assert proc.wait() == 0, unit
        with open(dst) as f:
            out[unit] = f.read()
    return out


def numbers(report, name):
    start = report.find("\n" + name + ":")
    assert start >= 0, "kernel %s not in the compiler's output" % name
    end = report.find("; Occupancy:", start)
    block = report[start:report.find("\n", end)]
    return tuple(int(re.search(f, block).group(1)) for f in FIELDS)


@pytest.mark.parametrize("name", NEW)
def test_new_kernels_keep_no_scratch(reports, name):
    code, sgprs, vgprs, agprs, scratch, lds, occupancy = numbers(reports[UNIT], name)
    print(name, "code", code, "SGPRs", sgprs, "VGPRs", vgprs, "AGPRs", agprs, "scratch", scratch, "LDS", lds, "occupancy", occupancy)
    assert scratch == 0, (name, scratch)


def test_no_other_kernel_in_the_new_unit(reports):
    found = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", reports[UNIT], flags=re.M))
    assert found == set(NEW), found ^ set(NEW)


def test_shared_units_hold_the_kernels_they_held(reports):
    for unit in sorted({u for u, _ in PARENT}):
        found = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", reports[unit], flags=re.M))
        want = {n for u, n in PARENT if u == unit}
        assert found == want, (unit, found ^ want)


@pytest.mark.parametrize("unit,name", sorted(PARENT))
def test_shared_kernels_are_the_code_they_were(reports, unit, name):
    got = numbers(reports[unit], name)
    print(name, got)
    assert got == PARENT[(unit, name)], (name, got, PARENT[(unit, name)])
