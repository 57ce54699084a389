"""The route predicates of the low-rank evaluation entry points (csrc/lr_tile_plan.hpp: lr_eval_route, lr_eval_tens_route) on the host (no
GPU needed): tests/emu/test_lr_eval_route.cpp restates the conditions under which gpsig_lr_seq_features / _ragged / gpsig_lr_tens_features picked
the fused kernels, the tiled kernels, the multi-pass route or a refusal before the wide route existed, and checks over a grid of (float type, c,
r, d', L, M, ragged, lr_fused, spectral) that the predicate agrees with them wherever it does not answer "wide", that "wide" only ever replaces
"passes" or "refuse", and that the named shapes (CMUsubject16's 126 columns, PEMS' 1,928, the smallest shapes beyond the tiled kernels) are wide."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsig_amd", "csrc")


def test_route_predicates_on_the_host(tmp_path):
    exe = str(tmp_path / "test_lr_eval_route")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "emu", "test_lr_eval_route.cpp")])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert res.returncode == 0, (res.stdout.decode(), res.stderr.decode()[-2000:])
    bad, cases, wides = (int(v) for v in res.stdout.split()[-3:])
    print("cases", cases, "of them wide", wides)
    assert bad == 0 and cases > 100000 and wides > 1000


def test_api_calls_the_predicates():
    """both host paths of lr_api.hip ask the predicate, and no option name was added for the route (tests/kernel_forms.py pins the set)"""
    with open(os.path.join(CSRC, "lr_api.hip")) as f:
        api = f.read()
    assert "lr_eval_route(" in api and "lr_eval_tens_route(" in api
