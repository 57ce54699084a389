"""Low-rank mode's float32 kernels, from the compiler's report (no GPU needed): every float32 feature kernel and the float32 Gram GEMM exist,
keep no scratch, and reach the occupancy they are designed for -- at least that of their float64 twins."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# float32 kernel -> (its float64 twin, the occupancy it is designed for: wavefronts per SIMD)
FEATURE_KERNELS = {
    "_ZN5gpsig33lr_seq_features_fused2_f32_kernelILi512ELi8EEEvNS_14LrFusedArgsF32E":
        ("_ZN5gpsig29lr_seq_features_fused2_kernelILi512ELi8EEEvNS_11LrFusedArgsE", 6),
    "_ZN5gpsig42lr_seq_features_fused2_spectral_f32_kernelILi512ELi8EEEvNS_14LrFusedArgsF32E":
        ("_ZN5gpsig38lr_seq_features_fused2_spectral_kernelILi512ELi8EEEvNS_11LrFusedArgsE", 6),
    "_ZN5gpsig32lr_seq_features_fused_f32_kernelILi512ELi8EEEvNS_14LrFusedArgsF32E":
        ("_ZN5gpsig28lr_seq_features_fused_kernelILi512ELi8EEEvNS_11LrFusedArgsE", 6),
    "_ZN5gpsig41lr_seq_features_fused_spectral_f32_kernelILi512ELi8EEEvNS_14LrFusedArgsF32E":
        ("_ZN5gpsig37lr_seq_features_fused_spectral_kernelILi512ELi8EEEvNS_11LrFusedArgsE", 6),
    "_ZN5gpsig33lr_tens_features_fused_f32_kernelENS_18LrTensFusedArgsF32E":
        ("_ZN5gpsig29lr_tens_features_fused_kernelENS_15LrTensFusedArgsE", 8),
    "_ZN5gpsig42lr_tens_features_fused_spectral_f32_kernelENS_18LrTensFusedArgsF32E":
        ("_ZN5gpsig38lr_tens_features_fused_spectral_kernelENS_15LrTensFusedArgsE", 8),
}
GEMM_F32 = "_ZN5gpsig25gemm_abt_f32_tiled_kernelEPKfS1_llillPfl"
GEMM_F64 = "_ZN5gpsig25gemm_abt_f64_tiled_kernelEPKdS1_llillPdl"


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


def test_float32_feature_kernels_exist_without_scratch_at_their_occupancy(tmp_path):
    text = _compile(tmp_path, "lr_fused_inst.hip")
    for name, (twin, designed) in FEATURE_KERNELS.items():
        vgprs, scratch, occ = _report(text, name)
        _, _, occ64 = _report(text, twin)
        assert scratch == 0, (name, scratch)
        assert occ >= designed and occ >= occ64, (name, vgprs, occ, occ64)


def test_float32_gram_gemm_exists_without_scratch(tmp_path):
    text = _compile(tmp_path, "lr_api.hip")
    vgprs, scratch, occ = _report(text, GEMM_F32)
    _, _, occ64 = _report(text, GEMM_F64)
    assert scratch == 0 and occ >= occ64 and occ >= 2, (vgprs, scratch, occ, occ64)
    # the float32 MFMA, not a float64 one or the VALU
    body = text[text.find("\n" + GEMM_F32 + ":"):]
    body = body[:body.find(".Lfunc_end")]
    assert "v_mfma_f32_16x16x4_f32" in body or "v_mfma_f32_16x16x4f32" in body
