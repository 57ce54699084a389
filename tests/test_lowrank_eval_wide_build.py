"""The kernels of the low-rank evaluation path's wide route, from the compiler's report (no GPU needed): the evaluation form of the Nystrom cross
kernel (csrc/lr_eval_wide_inst.hip) and the float32 feature kernels that take kxs / kzs from memory exist in their units and keep no scratch;
and the kernels the route shares with the training path -- lr_cross_kernel, lr_seq_features_tiled_kx_kernel -- are the code they were: the
report's numbers equal those of a build of the parent commit (recorded below), code length included."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = {
    "lr_eval_wide_inst": ("_ZN5gpsig20lr_cross_eval_kernelIdLb0EEEvNS_15LrCrossEvalArgsIT_EE", "_ZN5gpsig20lr_cross_eval_kernelIfLb0EEEvNS_15LrCrossEvalArgsIT_EE",
                          "_ZN5gpsig20lr_cross_eval_kernelIdLb1EEEvNS_15LrCrossEvalArgsIT_EE", "_ZN5gpsig20lr_cross_eval_kernelIfLb1EEEvNS_15LrCrossEvalArgsIT_EE"),
    "lr_eval_tiled_inst": ("_ZN5gpsig40lr_seq_features_eval_tiled_kx_f32_kernelENS_20LrEvalTiledKxArgsF32E",),
    "lr_kx_inst": ("_ZN5gpsig30lr_tens_features_kx_f32_kernelENS_15LrTensKxArgsF32E",),
}
# (unit, kernel): codeLenInByte, TotalNumSgprs, NumVgprs, NumAgprs, ScratchSize, LDSByteSize, Occupancy of the parent commit's build
PARENT = {
    ("lr_cross_inst", "_ZN5gpsig15lr_cross_kernelENS_11LrCrossArgsE"): (32760, 106, 159, 16, 0, 33280, 2),
    ("lr_kx_inst", "_ZN5gpsig31lr_seq_features_tiled_kx_kernelILi1024EEEvNS_13LrTiledKxArgsE"): (7084, 106, 66, 0, 0, 0, 7),
}
FIELDS = (r"codeLenInByte = (\d+)", r"; TotalNumSgprs: (\d+)", r"; NumVgprs: (\d+)", r"; NumAgprs: (\d+)", r"; ScratchSize: (\d+)",
          r"; LDSByteSize: (\d+)", r"; Occupancy: (\d+)")


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = {}
    tmp = tmp_path_factory.mktemp("lr_eval_wide")
    procs = []
    for unit in sorted(set(NEW) | {u for u, _ in PARENT}):
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


@pytest.mark.parametrize("unit,name", [(u, n) for u, names in sorted(NEW.items()) for n in names])
def test_new_kernels_keep_no_scratch(reports, unit, name):
    code, sgprs, vgprs, agprs, scratch, lds, occupancy = numbers(reports[unit], name)
    print(name, "code", code, "SGPRs", sgprs, "VGPRs", vgprs, "AGPRs", agprs, "scratch", scratch, "LDS", lds, "occupancy", occupancy)
    assert scratch == 0, (name, scratch)


@pytest.mark.parametrize("unit,name", sorted(PARENT))
def test_shared_kernels_are_the_code_they_were(reports, unit, name):
    got = numbers(reports[unit], name)
    print(name, got)
    assert got == PARENT[(unit, name)], (name, got, PARENT[(unit, name)])
