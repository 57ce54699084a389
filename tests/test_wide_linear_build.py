"""The identity kind of the wide-state-space kernels (SignatureLinear / SignatureCosine on the wide route), from the compiler's report (no GPU
needed): every identity instance that the host side dispatches exists, keeps no more scratch than its RBF twin and reaches at least its occupancy --
it is the same instruction stream minus the exponential and its table."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RBF, IDENTITY = 1, 2                  # WIDE_KD_RBF, WIDE_KD_ID (csrc/wide_kernels.hpp)


def _instances(kd):
    """Mangled names of the kind-dependent wide kernels, as wide_api.hip dispatches them (lat_kernel_of: one wavefront per lattice with 1 / 2 / 4 / 8
    columns per lane, or 2 / 4 / 8 wavefronts of one column per lane; 3 or 7 levels kept per lane)."""
    out = []
    for E in (1, 2):
        out += ["_ZN5gpsig19wide_tvs_%s_kernelILi%dELi%dEEEvNS_11WideTvsArgsE" % (w, E, kd) for w in ("fwd", "bwd")]
    for LQ in (3, 7):
        for C, NW in ((1, 1), (2, 1), (4, 1), (8, 1), (1, 2), (1, 4), (1, 8)):
            out += ["_ZN5gpsig23wide_lattice_%s_kernelILi%dELi%dELi%dELi%dEEEvNS_11WideLatArgsE" % (w, C, LQ, kd, NW) for w in ("fwd", "bwd")]
    out += ["_ZN5gpsig22wide_lattice_dm_kernelILi%dEEEvNS_11WideLatArgsEPd" % kd, "_ZN5gpsig27wide_lattice_adjoint_kernelILi%dEEEvNS_11WideLatArgsEPd" % kd]
    out += ["_ZN5gpsig20wide_tens_%s_kernelILi%dEEEvNS_12WideTensArgsE" % (w, kd) for w in ("fwd", "bwd")]
    return out


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "gpsig_amd", "csrc", "wide_api.hip")
    out = str(tmp_path_factory.mktemp("wide") / "wide_api.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out, src],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def _report(text, name):
    start = text.find("\n" + name + ":")
    assert start >= 0, "kernel %s not in the compiler's output" % name
    m = re.search(r"; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", text[start:], re.S)
    assert m, name
    lds = re.search(r"; LDSByteSize: (\d+)", text[start + m.start():start + m.end()])
    assert lds, name
    return int(m.group(1)), int(m.group(2)), int(m.group(3)), int(lds.group(1))


def test_identity_instances_exist_with_no_more_scratch_and_no_lower_occupancy_than_rbf(assembly):
    for name, twin in zip(_instances(IDENTITY), _instances(RBF)):
        vgprs, scratch, occ, _ = _report(assembly, name)
        tv, ts, to, _ = _report(assembly, twin)
        print(name, (vgprs, scratch, occ), "rbf", (tv, ts, to))
        assert scratch <= ts, (name, scratch, ts)
        assert occ >= to, (name, vgprs, occ, to)


def test_identity_instances_have_no_exp_table(assembly):
    """The RBF instances keep the 64-entry exp table (512 bytes) in LDS; the identity instances neither fill nor read one: those with one wavefront per
    workgroup use no LDS at all, the others only the hand-over buffers between wavefronts (512 bytes less than their twins)."""
    for name, twin in zip(_instances(IDENTITY), _instances(RBF)):
        lds, lds_rbf = _report(assembly, name)[3], _report(assembly, twin)[3]
        assert lds == lds_rbf - 512, (name, lds, lds_rbf)
