"""The spectral instances of the low-rank reverse kernel (csrc/lr_grad_kernel.hpp, lr_seq_features_grad_spectral_kernel), from the
compiler's report (no GPU needed): both workgroup sizes exist, the 512-thread one keeps no scratch, and the 1024-thread one keeps no more
scratch and reaches no lower occupancy than its twin of the other families."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPECTRAL = "_ZN5gpsig36lr_seq_features_grad_spectral_kernelILi{t}EEEvNS_18LrGradSpectralArgsE"
TWIN = "_ZN5gpsig27lr_seq_features_grad_kernelILi{t}EEEvNS_10LrGradArgsE"


def _compile(tmp_path, unit):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "gpsig_amd", "csrc", unit)
    out = str(tmp_path / (unit + ".s"))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, src],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def _report(text, name):
    start = text.find("\n" + name + ":")
    assert start >= 0, "kernel %s not in the compiler's output" % name
    m = re.search(r"; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", text[start:], re.S)
    assert m, name
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def test_spectral_reverse_instances_meet_the_scratch_targets(tmp_path):
    text = _compile(tmp_path, "lr_grad_api.hip")
    _, scratch512, occ512 = _report(text, SPECTRAL.format(t=512))
    _, _, twin_occ512 = _report(text, TWIN.format(t=512))
    assert scratch512 == 0 and occ512 >= twin_occ512, (scratch512, occ512, twin_occ512)
    _, scratch1024, occ1024 = _report(text, SPECTRAL.format(t=1024))
    _, twin_scratch1024, twin_occ1024 = _report(text, TWIN.format(t=1024))
    assert scratch1024 <= twin_scratch1024 and occ1024 >= twin_occ1024, (scratch1024, twin_scratch1024, occ1024, twin_occ1024)
