"""The batched SignatureSpectral kappa op, what can be checked without a GPU: the route function (autodiff.spectral_kappa_route) and the module
attribute behind it; the two entry points in the header and in the loader; and the compiler's report of the reverse pass's unit
(csrc/spectral_kappa_inst.hip) for gfx950 -- exactly its seven kernels, the weights kernel on the float64 matrix cores, no scratch (registers, LDS
and occupancy are printed)."""
import os
import re
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsig_amd", "csrc")
UNIT = "spectral_kappa_inst"
WEIGHTS = "_ZN5gpsig18spk_weights_kernelENS_13SpecKappaArgsE"
KERNELS = (
    WEIGHTS,
    "_ZN5gpsig17spk_reduce_kernelEPKdlliPd",
    "_ZN5gpsig16spk_scale_kernelENS_13SpecKappaArgsE",
    "_ZN5gpsig15spk_rows_kernelENS_13SpecKappaArgsE",
    "_ZN5gpsig15spk_cols_kernelENS_13SpecKappaArgsE",
    "_ZN5gpsig16spk_param_kernelENS_13SpecKappaArgsEi",
    "_ZN5gpsig17spk_finish_kernelENS_13SpecKappaArgsEPdS1_S1_",
)
FIELDS = (r"codeLenInByte = (\d+)", r"; TotalNumSgprs: (\d+)", r"; NumVgprs: (\d+)", r"; NumAgprs: (\d+)", r"; ScratchSize: (\d+)",
          r"; LDSByteSize: (\d+)", r"; Occupancy: (\d+)")
ENTRY_POINTS = ("gpsig_spectral_kappa", "gpsig_spectral_kappa_grad")


# ---- the route ------------------------------------------------------------------------------------------------------------------------------
def route(mode, is_cuda=True, dtype=torch.float64, batch=1, m=2 ** 14, n=2 ** 13, d=64, Q=5):
    from gpsig_amd.autodiff import spectral_kappa_route
    return spectral_kappa_route(mode, is_cuda, dtype, batch, m, n, d, Q)


def test_torch_is_torch_and_cpu_or_float32_never_reach_the_op():
    assert route("torch") == "torch"
    assert route("auto") == "hip"                               # (2^33 bytes of differences on the device, float64)
    assert route("auto", is_cuda=False) == "torch"
    assert route("auto", dtype=torch.float32) == "torch"
    assert route("auto", dtype=None) == "torch"                 # (operands of two dtypes)
    assert route("auto", d=4097) == "torch"
    assert route("auto", Q=65) == "torch"


def test_auto_is_the_memory_condition():
    from gpsig_amd import autodiff
    assert autodiff.SPECTRAL_KAPPA_MIN_BYTES == 2 ** 30
    # batch * m * n * d * 8 = 2^30 - 8 (2^27 - 1 = 7 * 73 * 262657) and 2^30
    assert route("auto", batch=262657, m=7, n=73, d=1) == "torch"
    assert route("auto", batch=1, m=2 ** 10, n=2 ** 10, d=2 ** 7) == "hip"
    assert route("auto", batch=2 ** 5, m=2 ** 8, n=2 ** 8, d=2 ** 6) == "hip"
    assert route("auto", batch=0, m=2 ** 20, n=2 ** 20, d=64) == "torch"
    # the shapes of the existing suites stay on the torch ops: the largest there is far below
    assert route("auto", batch=1, m=300, n=300, d=126) == "torch"


def test_hip_raises_by_name():
    assert route("hip", batch=1, m=1, n=1, d=1, Q=1) == "hip"           # (no size condition)
    assert route("hip", d=4096, Q=64) == "hip"
    for kw, text in ((dict(is_cuda=False), "CUDA"), (dict(dtype=torch.float32), "float64"), (dict(d=4097), "4096"), (dict(Q=65), "64")):
        with pytest.raises(NotImplementedError, match=text):
            route("hip", **kw)
    with pytest.raises(ValueError):
        route("rocblas")


def test_the_module_asks_the_route_function():
    """the attribute and its default; on CPU tensors "auto" and "torch" are the torch ops, bit for bit, and "hip" raises"""
    from gpsig_amd import autodiff, kernels
    k = kernels.SignatureSpectral(4 * 3, 3, 2, family="exp", Q=2)
    mod = autodiff.SignatureKernelModule(k, device="cpu")
    assert mod.spectral_kappa == "auto"
    g = torch.Generator().manual_seed(0)
    A, B = torch.randn(5, 3, generator=g, dtype=torch.float64), torch.randn(4, 3, generator=g, dtype=torch.float64)
    want = autodiff.base_kernel_matrix("spectral", A, B, spectral=(k.family, autodiff.positive(mod.raw_alpha), autodiff.positive(mod.raw_omega),
                                                                   autodiff.positive(mod.raw_sgamma)))
    for mode in ("auto", "torch"):
        mod.spectral_kappa = mode
        assert torch.equal(mod._mx_kappa(A, B), want)
    mod.spectral_kappa = "hip"
    with pytest.raises(NotImplementedError, match="CUDA"):
        mod._mx_kappa(A, B)
    assert torch.equal(mod._kappa(A, B), want)                  # (_kappa itself is torch ops whatever the attribute says)


def test_low_rank_mode_never_asks(monkeypatch):
    """the route belongs to the exact matrix route's primitives alone: the low-rank scope's torch fallback (_LowRankScope._cross -> _kappa: CPU tensors,
    lr_hip = False, shapes its HIP ops refuse) stays base_kernel_matrix at ANY size and under any value of the attribute -- the route function is
    not even called (a whole low-rank evaluation on the device: tests/test_gpu_spectral_kappa_module.py)"""
    import types
    from gpsig_amd import autodiff, kernels

    def never(*a, **k):
        raise AssertionError("spectral_kappa_route asked outside the exact matrix route")
    monkeypatch.setattr(autodiff, "spectral_kappa_route", never)
    monkeypatch.setattr(autodiff, "SPECTRAL_KAPPA_MIN_BYTES", 0)
    k = kernels.SignatureSpectral(6 * 3, 3, 2, family="mixed", Q=2, low_rank=True, num_components=4, rank_bound=4)
    mod = autodiff.SignatureKernelModule(k, device="cpu")
    g = torch.Generator().manual_seed(1)
    pts, S = torch.randn(7, 3, generator=g, dtype=torch.float64), torch.randn(4, 3, generator=g, dtype=torch.float64)
    want = autodiff.base_kernel_matrix("spectral", pts, S, spectral=(k.family, autodiff.positive(mod.raw_alpha), autodiff.positive(mod.raw_omega),
                                                                     autodiff.positive(mod.raw_sgamma)))
    for mode in ("auto", "hip", "torch"):
        mod.spectral_kappa = mode
        got = autodiff._LowRankScope._cross(types.SimpleNamespace(mod=mod, S=S), pts)
        assert torch.equal(got, want), mode


# ---- the bindings ---------------------------------------------------------------------------------------------------------------------------
def test_bindings_in_header_and_loader():
    from gpsig_amd import _lib
    with open(os.path.join(ROOT, "include", "gpsig_hip.h")) as f:
        header = f.read()
    for name in ENTRY_POINTS:
        assert len(re.findall(r"\bint %s\(" % name, header)) == 1, name
        assert name in _lib.ALL_SYMBOLS and name in _lib._PLAIN, name
        assert "wide_spectral" not in name and "spectral_wide" not in name
    # the argument lists: 13 and 18 arguments with the context
    assert len(_lib._PLAIN["gpsig_spectral_kappa"][0]) == 13 and len(_lib._PLAIN["gpsig_spectral_kappa_grad"][0]) == 18
    if os.path.exists(_lib.LIB_PATH):
        nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
        for name in ENTRY_POINTS:
            assert re.search(r" T %s$" % name, nm, flags=re.M), name


def test_launchers_are_declared_once():
    with open(os.path.join(CSRC, "launchers.hpp")) as f:
        decl = f.read()
    with open(os.path.join(CSRC, "spectral_kappa_api.hip")) as f:
        host = f.read()
    for fn in ("spk_weights_launch", "spk_reduce_launch", "spk_scale_launch", "spk_rows_launch", "spk_cols_launch", "spk_param_launch", "spk_finish_launch"):
        assert len(re.findall(r"\bint %s\(" % fn, decl)) == 1, fn
        assert re.search(r"\b%s\(" % fn, host), fn
    for fn in ("wide_spx_prep_launch", "wide_spx_side_launch", "wide_spx_launch"):          # the forward pass is the existing kernels
        assert re.search(r"\b%s\(" % fn, host), fn


# ---- the compiler's report ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("spectral_kappa") / (UNIT + ".s"))
    proc = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", dst, os.path.join(CSRC, UNIT + ".hip")],
                          stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    with open(dst) as f:
        return f.read()


def block(report, name):
    start = report.find("\n" + name + ":")
    assert start >= 0, "kernel %s not in the compiler's output" % name
    end = report.find("; Occupancy:", start)
    return report[start:report.find("\n", end)]


@pytest.mark.parametrize("name", KERNELS)
def test_kernels_keep_no_scratch(report, name):
    code, sgprs, vgprs, agprs, scratch, lds, occupancy = (int(re.search(f, block(report, name)).group(1)) for f in FIELDS)
    print(name, "code", code, "SGPRs", sgprs, "VGPRs", vgprs, "AGPRs", agprs, "scratch", scratch, "LDS", lds, "occupancy", occupancy)
    assert scratch == 0, (name, scratch)


def test_no_other_kernel_in_the_unit(report):
    found = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", report, flags=re.M))
    assert found == set(KERNELS), found ^ set(KERNELS)


def test_the_weights_kernel_runs_on_the_float64_matrix_cores(report):
    assert "v_mfma_f64_16x16x4" in block(report, WEIGHTS)
