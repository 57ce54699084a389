"""The polynomial kind of the wide-state-space kernels (SignaturePoly on the wide route), from the compiler's report (no GPU needed): every
polynomial instance that the host side dispatches exists, keeps no more scratch than its RBF twin, reaches at least the occupancy of its Matern twin
and keeps no exp table in LDS -- repeated squaring in place of the exponential, and in the reverse kernels the sum of the adjoint entries they
store."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATERN, RBF, POLY = 0, 1, 3                  # WIDE_KD_MATERN, WIDE_KD_RBF, WIDE_KD_POLY (csrc/wide_kernels.hpp)


def _instances(kd):
    """Mangled names of the kind-dependent wide kernels, as wide_api.hip dispatches them (lat_kernel_of: one wavefront per lattice with 1 / 2 / 4 / 8
    columns per lane, or 2 / 4 / 8 wavefronts of one column per lane; 3 or 7 levels kept per lane)."""
    out = []
    for E in (1, 2):
        out += ["_ZN5gpsig19wide_tvs_%s_kernelILi%dELi%dEEEvNS_11WideTvsArgsE" % (w, E, kd) for w in ("fwd", "bwd")]
    for LQ in (3, 7):
        for C, NW in ((1, 1), (2, 1), (4, 1), (8, 1), (1, 2), (1, 4), (1, 8)):
            out += ["_ZN5gpsig23wide_lattice_%s_kernelILi%dELi%dELi%dELi%dEEEvNS_11WideLatArgsE" % (w, C, LQ, kd, NW) for w in ("fwd", "bwd")]
    out += ["_ZN5gpsig22wide_lattice_dm_kernelILi%dEEEvNS_11WideLatArgsEPd" % kd, ("_ZN5gpsig32wide_lattice_adjoint_poly_kernelENS_11WideLatArgsEPd" if kd == POLY      # (the polynomial adjoint is a kernel of its own)
                                                                                  else "_ZN5gpsig27wide_lattice_adjoint_kernelILi%dEEEvNS_11WideLatArgsEPd" % kd)]
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


def test_poly_instances_exist_with_no_more_scratch_than_rbf_and_no_lower_occupancy_than_matern(assembly):
    for name, rbf, mat in zip(_instances(POLY), _instances(RBF), _instances(MATERN)):
        vgprs, scratch, occ, _ = _report(assembly, name)
        rs, mo = _report(assembly, rbf)[1], _report(assembly, mat)[2]
        print(name, (vgprs, scratch, occ), "rbf scratch", rs, "matern occupancy", mo)
        assert scratch <= rs, (name, scratch, rs)
        assert occ >= mo, (name, vgprs, occ, mo)


def test_poly_instances_have_no_exp_table(assembly):
    """The RBF instances keep the 64-entry exp table (512 bytes) in LDS; the polynomial instances neither fill nor read one: those with one wavefront
    per workgroup use no LDS at all, the others only the hand-over buffers between wavefronts (512 bytes less than their twins)."""
    for name, twin in zip(_instances(POLY), _instances(RBF)):
        lds, lds_rbf = _report(assembly, name)[3], _report(assembly, twin)[3]
        assert lds == lds_rbf - 512, (name, lds, lds_rbf)
