"""Exact-mode SignatureSpectral beyond 32 columns, what can be checked without a GPU: the spectral argument kernel's unit
(csrc/wide_spectral_inst.hip) compiles for gfx950, holds its three kernels and keeps no scratch (registers, LDS and occupancy are printed); the
Makefile picks the unit up; the library exports the C entry points it exported before -- the feature adds none --; and SignatureSpectral._params
carries the two opt-in switches in base_params[2] / [3] independently."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsig_amd", "csrc")
UNIT = "wide_spectral_inst"
KERNELS = (
    "_ZN5gpsig20wide_spx_prep_kernelEPKdlPd",
    "_ZN5gpsig20wide_spx_side_kernelEPKdlliiS1_S1_PdS2_",
    "_ZN5gpsig15wide_spx_kernelENS_11WideSpxArgsE",
)
FIELDS = (r"codeLenInByte = (\d+)", r"; TotalNumSgprs: (\d+)", r"; NumVgprs: (\d+)", r"; NumAgprs: (\d+)", r"; ScratchSize: (\d+)",
          r"; LDSByteSize: (\d+)", r"; Occupancy: (\d+)")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("wide_spectral") / (UNIT + ".s"))
    proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst, os.path.join(CSRC, UNIT + ".hip")],
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


def test_the_contractions_run_on_the_float64_matrix_cores(report):
    for name in KERNELS[1:]:
        start = report.find("\n" + name + ":")
        assert "v_mfma_f64_16x16x4" in report[start:report.find("; Occupancy:", start)], name


def test_the_unit_is_part_of_the_build():
    """the Makefile compiles every *.hip of the directory; the launchers are declared once, in launchers.hpp, and called from wide_api.hip"""
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "$(wildcard *.hip)" in f.read()
    assert os.path.exists(os.path.join(CSRC, UNIT + ".hip"))
    with open(os.path.join(CSRC, "launchers.hpp")) as f:
        decl = f.read()
    with open(os.path.join(CSRC, "wide_api.hip")) as f:
        host = f.read()
    for fn in ("wide_spx_prep_launch", "wide_spx_side_launch", "wide_spx_launch"):
        assert len(re.findall(r"\bint %s\(" % fn, decl)) == 1, fn
        assert re.search(r"\b%s\(" % fn, host), fn
    from gpsig_amd import _lib
    if os.path.exists(_lib.LIB_PATH):
        nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
        assert "wide_spx_launch" in nm


def test_the_library_exports_what_it_exported_before():
    """no new C entry point: the header's list and the Python loader's still agree, and the built library exports exactly those gpsig_* names"""
    from gpsig_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    with open(os.path.join(ROOT, "include", "gpsig_hip.h")) as f:
        declared = set(re.findall(r"\b(gpsig_[a-z_A-Z0-9]+)\s*\(", f.read())) - {"gpsig_ctx"}
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = set(re.findall(r" T (gpsig_\w+)", nm))
    assert exported == declared == set(_lib.ALL_SYMBOLS), exported ^ declared
    assert not [s for s in exported if "wide_spectral" in s or "spectral_wide" in s]


def test_params_carry_the_two_switches_independently():
    from gpsig_amd import kernels
    k = kernels.SignatureSpectral(40 * 5, 40, 3, family="exp", Q=4)
    assert k.spectral_wide is False and k.lr_spectral_wide is False
    for lr, ex in ((False, False), (True, False), (False, True), (True, True)):
        k.lr_spectral_wide, k.spectral_wide = lr, ex
        keep = []
        p = k._params(keep)
        assert (p.base_params[0], p.base_params[1]) == (4.0, 1.0)
        assert (p.base_params[2], p.base_params[3]) == (1.0 if lr else 0.0, 1.0 if ex else 0.0), (lr, ex)
