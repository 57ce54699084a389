"""Ragged batches in exact mode (``kern.exact_ragged``, csrc/wide_ragged_api.hip), the part that needs no GPU: the host-side plan
(csrc/ragged_plan.hpp) as a stand-alone program under the address and undefined-behaviour sanitizers, the four entry points as the header declares
and gpsig_amd._lib binds them, the compiler's report of the new unit's kernels (gfx950, no scratch, the block-diagonal kernel on the float64 matrix
cores) and the switch's defaults: without it every refusal is what it was."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsig_amd", "csrc")

# the new entry point -> its dense twin
TWINS = {"gpsig_kernel_Kdiag_ragged": "gpsig_kernel_Kdiag", "gpsig_kernel_K_tens_vs_seq_ragged": "gpsig_kernel_K_tens_vs_seq",
         "gpsig_kernel_K_tens_n_seq_covs_ragged": "gpsig_kernel_K_tens_n_seq_covs", "gpsig_kernel_K_ragged": "gpsig_kernel_K"}


def test_ragged_plan_on_the_host(tmp_path):
    exe = str(tmp_path / "test_ragged_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "test_ragged_plan.cpp")])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, (res.stdout.decode(), res.stderr.decode()[-2000:])
    bad, plans = res.stdout.split()[-2:]
    assert int(bad) == 0 and int(plans) > 100000


def test_plan_header_has_no_hip_in_it():
    with open(os.path.join(CSRC, "ragged_plan.hpp")) as f:
        text = f.read()
    assert "hip" not in "".join(ln for ln in text.splitlines(True) if ln.lstrip().startswith("#include")).lower()
    assert "__global__" not in text and "__device__" not in text


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "gpsig_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert m, "%s is not declared in include/gpsig_hip.h" % name
    return [a.strip() for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(TWINS))
def test_header_declares_and_lib_binds_the_entry_points(name):
    """The dense twin's arguments plus `const int32_t* lengths` directly after each L (L; L1 and L2 of K), nothing else moved."""
    from gpsig_amd import _lib
    args, plain = _header_args(name), _header_args(TWINS[name])
    at = [i for i, a in enumerate(args) if re.search(r"\bL[12]?$", a)]
    assert len(at) == (2 if name == "gpsig_kernel_K_ragged" else 1)
    for i in at:
        assert re.fullmatch(r"const\s+int32_t\s*\*\s*lengths2?", args[i + 1]), args[i + 1]
    rest = [a for i, a in enumerate(args) if i - 1 not in at]
    assert [a.split()[-1] for a in rest] == [a.split()[-1] for a in plain]
    assert name in _lib._KERNEL_FUNCS and name in _lib.ALL_SYMBOLS
    assert len(_lib._KERNEL_FUNCS[name]) + 2 == len(args)               # (ctx, params) + the bound argument types
    assert len(_lib._KERNEL_FUNCS[name]) == len(_lib._KERNEL_FUNCS[TWINS[name]]) + len(at)
    for i in at:                                                           # a pointer where the lengths go
        assert _lib._KERNEL_FUNCS[name][i + 1 - 2] is _lib._vp


def test_abi_version_and_option_list_are_untouched():
    text = open(os.path.join(ROOT, "include", "gpsig_hip.h")).read()
    assert re.search(r"#define\s+GPSIG_ABI_VERSION\s+1\b", text)
    src = open(os.path.join(CSRC, "wide_ragged_api.hip")).read()
    assert "gpsig_set_option" not in src and "wide_chunk_bytes" in src     # no option of its own: the chunks follow wide_chunk_mb


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("exact_ragged") / "wide_ragged_api.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", out,
                           os.path.join(CSRC, "wide_ragged_api.hip")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def _kernels(report, pattern):
    return re.findall(r"^(%s):" % pattern, report, re.M)


def _body(report, name):
    at = report.find("\n" + name + ":")
    return report[at:report.find(".Lfunc_end", at)]


# the unit's kernels by their mangled names: the block-diagonal argument kernel, the ragged forms of the chain and lattice kernels, and the lengths-aware
# overload of prep_seq_scaled_kernel (the one that takes the two extra pointers)
KINDS = {"block diagonal": r"_ZN5gpsig28wide_ragged_diag_args_kernelENS_18WideRaggedDiagArgsE",
         "chains": r"_ZN5gpsig\d+wide_tvs_fwd_ragged_kernelILi\dELi\dEEEvNS_17WideTvsRaggedArgsE",
         "lattices": r"_ZN5gpsig\d+wide_lattice_fwd_ragged_kernelILi\dELi\dELi\dELi\dEEEvNS_17WideLatRaggedArgsE",
         "packed rows": r"_ZN5gpsig22prep_seq_scaled_kernelIdEEvPKT_li\w*PKiPKlPS1_"}
COUNTS = {"block diagonal": 1, "chains": 4, "lattices": 28, "packed rows": 1}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_kernels_compile_for_gfx950_without_scratch(report, kind):
    names = _kernels(report, KINDS[kind])
    assert len(names) == COUNTS[kind], (kind, names)              # only the kinds served are instantiated
    for name in names:
        tail = report[report.find("\n" + name + ":"):]
        m = re.search(r"; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; LDSByteSize: (\d+).*?; Occupancy: (\d+)", tail, re.S)
        assert m, name
        vgprs, scratch, lds, occupancy = (int(g) for g in m.groups())
        print(name, "VGPRs", vgprs, "LDS", lds, "scratch", scratch, "occupancy", occupancy)
        assert scratch == 0, (name, scratch)


def test_dense_forms_are_not_instantiated_again(report):
    """The unit instantiates the ragged forms only; of the wide route's kernels that are no templates it holds copies of the two it launches."""
    assert not _kernels(report, r"_ZN5gpsig\d+wide_tvs_fwd_kernelI\w+") and not _kernels(report, r"_ZN5gpsig\d+wide_lattice_fwd_kernelI\w+")
    assert not _kernels(report, r"\w*wide_tvs_bwd_kernel\w*") and not _kernels(report, r"\w*wide_lattice_bwd_kernel\w*")
    shared = sorted(n for n in _kernels(report, r"_ZN5gpsig\d+wide_\w+_kernel\w*") if "ragged" not in n)
    assert [n.split("kernel")[0] for n in shared] == ["_ZN5gpsig20wide_aug_rows_", "_ZN5gpsig24wide_tvs_epilogue_"], shared


def test_block_diagonal_kernel_runs_on_the_float64_matrix_cores(report):
    name, = _kernels(report, KINDS["block diagonal"])
    body = _body(report, name)
    assert "v_mfma_f64_16x16x4" in body
    assert "atomic" not in body                                   # every entry is one accumulation chain in one workgroup


def _kern(**kw):
    from gpsig_amd import kernels
    return kernels.SignatureRBF(9 * 2, 2, 3, **kw)


def test_without_the_switch_every_refusal_is_what_it_was():
    X = np.zeros((4, 18))
    k = _kern()
    assert k.exact_ragged is False
    for call in (lambda: k.K(X, lengths=[9, 4, 2, 1]), lambda: k.K(X, X, lengths2=[9, 4, 2, 1]), lambda: k.Kdiag(X, lengths=[9, 4, 2, 1]),
                 lambda: k.K_tens_vs_seq(np.zeros((6, 3, 2)), X, lengths=[9, 4, 2, 1]),
                 lambda: k.K_tens_n_seq_covs(np.zeros((6, 3, 2)), X, lengths=[9, 4, 2, 1]),
                 lambda: k.K_seq_n_seq_covs(np.zeros((2, 5, 2)), X, lengths2=[9, 4, 2, 1])):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == ("lengths= is built for low-rank mode only: in exact mode pad each sequence by repeating its last "
                                "observation, which is exact there with difference=True (zero increments add nothing)")
    del k.exact_ragged                                               # read with getattr: an object from before the attribute refuses too
    with pytest.raises(NotImplementedError, match="repeating its last"):
        k.K(X, lengths=[9, 4, 2, 1])


def test_with_the_switch_lags_still_need_the_sequence_axis():
    X = np.zeros((4, 18))
    k = _kern(num_lags=1)
    k.exact_ragged = True
    assert k.lag_axis == "table"
    with pytest.raises(NotImplementedError) as e:
        k.K(X, lengths=[9, 4, 2, 1])
    assert str(e.value) == "lengths= is not built for num_lags > 0: the lag interpolation runs on the table's own time axis"
    with pytest.raises(NotImplementedError, match="time axis"):
        k.Kdiag(X, lengths=[9, 4, 2, 1])


@pytest.mark.parametrize("bad", [[9, 4, 0, 1], [9, 4, 10, 1], [9, 4, 2], [[9, 4, 2, 1]], np.array([9.0, 4.0, 2.0, 1.0])],
                         ids=["zero", "L+1", "short", "2-d", "float"])
def test_with_the_switch_bad_lengths_are_value_errors(bad):
    X = np.zeros((4, 18))
    k = _kern()
    k.exact_ragged = True
    for call in (lambda: k.K(X, lengths=bad), lambda: k.K(X, X, lengths2=bad), lambda: k.Kdiag(X, lengths=bad),
                 lambda: k.K_tens_vs_seq(np.zeros((6, 3, 2)), X, lengths=bad)):
        with pytest.raises(ValueError):
            call()


def test_module_keeps_refusing_lengths_in_exact_mode():
    """Gradients are out of scope: autodiff.SignatureKernelModule refuses `lengths=` in exact mode whatever the kernel object's switch says."""
    import torch
    from gpsig_amd import autodiff
    k = _kern()
    k.exact_ragged = True
    mod = autodiff.SignatureKernelModule(k, device=torch.device("cpu"))
    with pytest.raises(NotImplementedError):
        mod.K(torch.zeros((4, 18), dtype=torch.float64), lengths=[9, 4, 2, 1])
