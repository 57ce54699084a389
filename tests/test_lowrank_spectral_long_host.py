"""Low-rank SignatureSpectral on long and ragged batches, the part that needs no GPU: the C ABI's two entry points as the header declares
and gpsig_amd._lib binds them, and the new instances (csrc/lr_spectral_tiled_inst.hip) from the compiler's own resource report: none keeps
scratch memory, and none reaches a lower occupancy than its twin of the other families in csrc/lr_ragged_inst.hip.

Figures of the report (registers, scratch bytes, occupancy in wavefronts per SIMD):
    forward, whole sequence    64, 0, 7   twin  82, 0, 5
    forward, tiled (1024)      70, 0, 7   twin  94, 0, 5
    reverse, whole sequence   153, 0, 3   twin 189, 0, 2
    reverse, tiled (512)      115, 0, 4   twin 190, 0, 2
The forward and the tiled instances evaluate a component's exponential and cosine out of line (lr_spectral_term_val, 30 registers): inlined,
their float64 coefficients are hoisted into registers for the whole kernel and the forward instances take 102 / 108 registers, occupancy 4."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gpsig_lr_seq_features_spectral_ragged_dev", "gpsig_lr_seq_features_spectral_ragged_grad")
BASES = ("gpsig_lr_seq_features_spectral_dev", "gpsig_lr_seq_features_spectral_grad")

# (new instance, its twin of the other families)
PAIRS = [
    ("_ZN5gpsig35lr_seq_features_spectral_len_kernelENS_22LrFusedSpectralLenArgsE", "_ZN5gpsig29lr_seq_features_ragged_kernelENS_17LrFusedRaggedArgsE"),
    ("_ZN5gpsig40lr_seq_features_grad_spectral_len_kernelENS_21LrGradSpectralLenArgsE", "_ZN5gpsig34lr_seq_features_grad_ragged_kernelENS_16LrGradRaggedArgsE"),
    ("_ZN5gpsig37lr_seq_features_tiled_spectral_kernelILi1024EEEvNS_19LrTiledSpectralArgsE",
     "_ZN5gpsig35lr_seq_features_tiled_ragged_kernelILi1024EEEvNS_17LrTiledRaggedArgsE"),
    ("_ZN5gpsig42lr_seq_features_grad_tiled_spectral_kernelILi512EEEvNS_19LrTiledSpectralArgsE",
     "_ZN5gpsig40lr_seq_features_grad_tiled_ragged_kernelILi512EEEvNS_17LrTiledRaggedArgsE"),
]


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "gpsig_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert m, "%s is not declared in include/gpsig_hip.h" % name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_and_lib_binds_the_entry_points():
    from gpsig_amd import _lib
    for name, base in zip(NAMES, BASES):
        args, plain = _header_args(name), _header_args(base)
        # the arguments of the existing spectral entry point plus `lengths`, directly after L
        assert len(args) == len(plain) + 1
        at = [i for i, a in enumerate(args) if re.search(r"\bL$", a)][0]
        assert re.fullmatch(r"const\s+int32_t\s*\*\s*lengths", args[at + 1]), args[at + 1]
        assert [a.split()[-1] for a in args[:at + 1] + args[at + 2:]] == [a.split()[-1] for a in plain]
        assert name in _lib._KERNEL_FUNCS, name
        assert len(_lib._KERNEL_FUNCS[name]) + 2 == len(args)               # (ctx, params) + the bound argument types
        assert len(_lib._KERNEL_FUNCS[name]) == len(_lib._KERNEL_FUNCS[base]) + 1


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


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lr_spectral_long")
    new, twin = _compile(tmp, "lr_spectral_tiled_inst.hip"), _compile(tmp, "lr_ragged_inst.hip")
    return [(_report(new, a), _report(twin, b)) for a, b in PAIRS]


def test_new_instances_keep_no_scratch(reports):
    for (name, _), (got, _) in zip(PAIRS, reports):
        print(name, got)
        assert got[1] == 0, (name, got)


def test_new_instances_reach_their_twins_occupancy(reports):
    for (name, _), (got, twin) in zip(PAIRS, reports):
        print(name, got, twin)
    for (name, _), (got, twin) in zip(PAIRS, reports):
        assert got[2] >= twin[2], (name, got, twin)
