"""The predicates that send SignatureSpectral's low-rank evaluation calls beyond 32 columns to the wide route (csrc/lr_tile_plan.hpp:
lr_spectral_eval_wide, lr_spectral_eval_tens_wide) on the host (no GPU needed): tests/emu/test_lr_spectral_eval_route.cpp restates the bounds --
float64, c <= 64, M <= 8, d <= 4096, one 64-step tile of max(c, r) rows (a tensor's kzs arrays within 64 KB, T <= 2^31 - 1) -- and checks over the
grid of tests/emu/test_lr_eval_route.cpp that the predicates answer "wide" exactly there and name the failing bound elsewhere, and that
lr_eval_route / lr_eval_tens_route answer for a spectral kernel what they answered before: they serve every call without the opt-in."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsig_amd", "csrc")


def test_spectral_route_predicates_on_the_host(tmp_path):
    exe = str(tmp_path / "test_lr_spectral_eval_route")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "test_lr_spectral_eval_route.cpp")])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, (res.stdout.decode(), res.stderr.decode()[-2000:])
    bad, cases, wides = (int(v) for v in res.stdout.split()[-3:])
    print("cases", cases, "of them wide", wides)
    assert bad == 0 and cases > 10000 and wides > 1000


def test_api_asks_the_predicates_behind_the_opt_in():
    """both host paths of lr_api.hip ask the new predicates, only for a kernel object that opts in (base_params[2]); the opt-in is no option name
    (tests/kernel_forms.py pins that set: neither lr_api.hip nor api.hip, which holds the option setter, names one), and the exact entry points'
    parameter check (the ENTER macro, api_common.hpp) does not read it"""
    with open(os.path.join(CSRC, "lr_api.hip")) as f:
        lr_api = f.read()
    with open(os.path.join(CSRC, "api.hip")) as f:
        api = f.read()
    with open(os.path.join(CSRC, "api_common.hpp")) as f:
        common = f.read()
    assert "lr_spectral_eval_wide(" in lr_api and "lr_spectral_eval_tens_wide(" in lr_api and "base_params[2]" in lr_api
    assert "lr_eval_route(" in lr_api and "lr_eval_tens_route(" in lr_api
    assert '"lr_spectral_wide"' not in lr_api and '"lr_spectral_wide"' not in api
    enter = common[common.index("#define ENTER(c, p)"):common.index("#define ENTER_LR(c, p)")]
    assert "check_params((c), (p))" in enter
