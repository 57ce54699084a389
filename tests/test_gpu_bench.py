"""bench.py on the GPU: a plain run does what its headline needs and nothing else; with --full the N > 1 line is produced by N ranks
bench.py starts itself, and the default line carries the measurement (clock, what binds, measured traffic)."""
import json
import os
import subprocess
import sys
import tempfile
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, env_extra=None, timeout=1500, full=True):
    """The full record bench.py --full writes with --record (full=False: a plain run's), after checking the one line it prints: the
    last line of stdout, strict JSON, under 2 KB, the record's headline."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    with tempfile.TemporaryDirectory() as tmp:
        rec = os.path.join(tmp, "record.json")
        pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + (["--full"] if full else []) + ["--record", rec], env=env, capture_output=True, text=True,
                            timeout=timeout)
        assert pr.returncode == 0, pr.stderr[-3000:]
        with open(rec) as f:
            record = json.load(f, parse_constant=_no_constant)
    out = pr.stdout.splitlines()
    assert [ln for ln in out if ln.startswith("{")] == out[-1:] and len(out[-1]) < 2048, pr.stdout[-3000:]
    line = json.loads(out[-1], parse_constant=_no_constant)
    for k in ("value", "ms_per_step", "steps", "warmup", "n_gpus") + (("rel_err",) if full else ()):
        assert line[k] == record[k], k
    assert line["roofline"]["bound"] == record["roofline"]["bound"]
    return record


def _no_constant(name):
    raise ValueError("not strict JSON: " + name)


def test_two_ranks_started_by_bench_itself():
    """`python bench.py --gpus 2 --steps 1` WITHOUT torchrun (gloo: both ranks on the one GPU of this box): n_gpus is the number of
    ranks that computed the line, and the gathered Gram equals single-rank evaluations."""
    line = _bench(["--gpus", "2", "--steps", "1", "--warmup", "1", "--weak", "--no-cpu-baseline"], {"GPSIG_BENCH_BACKEND": "gloo"})
    assert line["n_gpus"] == 2
    seen = line["ranks_seen"]
    assert seen["world_size"] == 2 and seen["backend"] == "gloo" and seen["launched_by"] == "bench.py itself"
    assert sorted(r["rank"] for r in seen["ranks"]) == [0, 1] and all(r["arch"].startswith("gfx950") for r in seen["ranks"])
    assert line["verify_max_abs_diff_vs_single_rank"] <= 1e-12
    assert line["rel_err"] <= 1e-6
    # where each rank's time went (round 5): the row-block kernels, the gathers, rank 0's symmetrisation
    pr = line["per_rank"]
    assert [t["rank"] for t in pr["ranks"]] == [0, 1] and all(t["compute_ms"] > 0 and t["chunks"] == 4 for t in pr["ranks"])
    assert pr["compute_max_over_min"] >= 1.0 and pr["symmetrise_ms_rank0"] > 0 and pr["ranks"][1]["symmetrise_ms"] == 0.0


@pytest.mark.parametrize("cfg", ["c2", "c3"])
def test_dump_outputs_is_the_timed_result(cfg):
    """--dump-outputs DIR after --steps 3: the line counts three timed steps, and DIR holds the last step's arrays (c2's Gram as a seeded
    sample of its rows; c3's Kzz, Kzx sampled, Kxx-diag) under 64 MB, equal to the library's evaluation of the same seeded inputs."""
    import importlib.util
    import numpy as np
    import torch
    from gpsig_amd import kernels
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    with tempfile.TemporaryDirectory() as tmp:
        line = _bench(["--config", cfg, "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-traffic", "--dump-outputs", tmp])
        assert sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp)) < 64e6
        got = {f[:-4]: np.load(os.path.join(tmp, f)) for f in os.listdir(tmp)}
    assert line["steps"] == 3 and line["warmup"] == 1
    w = bench.WORKLOADS[cfg]
    dev = torch.device("cuda:0")
    X = torch.as_tensor(bench.make_inputs(w), device=dev)
    kern = (kernels.SignatureLinear if w["base"] == "linear" else kernels.SignatureRBF)(w["L"] * w["d"], w["d"], w["M"], lengthscales=bench.lengthscales(w))
    if w["T"]:
        Z = torch.as_tensor(bench.make_tensors(w, False), device=dev)
        want = dict(zip(("Kzz", "Kzx", "Kxx_diag"), (a.cpu().numpy() for a in kern.K_tens_n_seq_covs(Z, X))))
    else:
        want = {"K": kern.K(X).cpu().numpy()}
    assert sorted(got) == sorted(list(want) + [k + "_rows" for k in want if want[k].nbytes > 32e6])
    for k, a in want.items():
        if k + "_rows" in got:
            a = a[got[k + "_rows"].astype(np.int64)]
        assert got[k].dtype == np.float64 and got[k].shape == a.shape
        assert np.abs(got[k] - a).max() <= 1e-12 * np.abs(a).max(), k


def test_plain_run_is_the_headline_and_nothing_else(tmp_path):
    """Without --full: the line's contract fields and the timed region's own figures, the dump of the last timed step (equal to the
    library's evaluation of the same seeded inputs), and none of what takes time of its own -- no CPU baseline, no comparison with the
    oracle, no host-pointer evaluation, no rocprofv3 pass, no secondary configurations.  --full --timed-loop-only is the same run."""
    import importlib.util
    import numpy as np
    import torch
    from gpsig_amd import kernels
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    t0 = time.perf_counter()
    rec = _bench(["--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path)], full=False)
    wall = time.perf_counter() - t0
    assert rec["metric"] == bench.METRIC and rec["unit"] == "sequence-pairs/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["n_gpus"] == 1 and rec["steps"] == 5 and rec["warmup"] == 2 and rec["config"]["name"] == "c2"
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - 4096.0 * 4096.0 / (rec["ms_per_step"] * 1e-3)) <= 1e-9 * rec["value"]
    rf = rec["roofline"]
    assert rf["bound"] == "mfma" and 0.5 < rf["frac"] < 1.0 and rf["kernel_ms_per_launch"] > 0 and 1.0 < rec["clock_ghz"] < 2.6
    for k in ("cpu_baseline", "rel_err", "end_to_end_ms_host_pointers", "secondary"):
        assert k not in rec, k
    assert rf["traffic"] is None and rf["traffic_source"] is None and rf["issue_frac"] is None
    # 30 s outside the steps is the budget of such a run; the steps themselves are 7 x ~10 ms here
    assert wall - 7 * rec["ms_per_step"] * 1e-3 < 30.0, wall
    w = bench.WORKLOADS["c2"]
    kern = kernels.SignatureLinear(w["L"] * w["d"], w["d"], w["M"], lengthscales=bench.lengthscales(w))
    want = kern.K(torch.as_tensor(bench.make_inputs(w), device="cuda:0")).cpu().numpy()
    got = {f[:-4]: np.load(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))}
    assert sorted(got) == ["K", "K_rows"]
    a = want[got["K_rows"].astype(np.int64)]
    assert got["K"].dtype == np.float64 and got["K"].shape == a.shape and np.abs(got["K"] - a).max() <= 1e-12 * np.abs(a).max()
    same = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--timed-loop-only"], full=False)
    assert "rel_err" not in same and "cpu_baseline" not in same and same["roofline"]["traffic"] is None


def test_clock_probe_reads_a_plausible_shader_clock():
    import torch
    from gpsig_amd import _lib, kernels
    dev = torch.device("cuda:0")
    ctx = _lib.context(0, torch.cuda.current_stream(dev).cuda_stream)
    kern = kernels.SignatureLinear(64 * 8, 8, 5)
    X = torch.randn(1024, 64 * 8, dtype=torch.float64, device=dev)
    kern.K(X)
    torch.cuda.synchronize()
    ctx.clock_probe_start(200.0, 64)                        # far longer than the work: the read below ends it
    t0 = time.perf_counter()
    for _ in range(6):
        kern.K(X)
    torch.cuda.current_stream(dev).synchronize()
    busy_ms = (time.perf_counter() - t0) * 1e3
    mean, lo, hi, window = ctx.clock_probe_read()
    assert 1.0 < lo <= mean <= hi < 2.6, (mean, lo, hi)      # MI355X: 2.4 GHz peak engine clock, lower under float64 load
    assert 0.5 * busy_ms < window < busy_ms + 5.0, (window, busy_ms)
    with pytest.raises(ValueError):
        ctx.clock_probe_read()                               # one read per start
    ctx.clock_probe_start(2.0, 8)                            # a probe nobody reads leaves by itself
    torch.cuda.synchronize()


def test_default_line_carries_the_measurement():
    line = _bench(["--steps", "5", "--warmup", "2"])
    assert line["n_gpus"] == 1 and line["config"]["name"] == "c2" and line["rel_err"] <= 1e-6
    rf = line["roofline"]
    # the headline Gram is the feature contraction on the float64 matrix cores: priced in TFLOP/s against their peak
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == 78.6
    assert 0.5 < rf["frac"] < 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert rf["mfma"]["depth"] == 37456 and 0.7 < rf["mfma"]["kernel_share_of_step"] <= 1.0
    assert rf["issue_frac"] is None and rf["stream_frac"] > 0
    assert 1.0 < line["clock_ghz"] < 2.6
    assert rf["traffic"] and rf["traffic_source"]["how"].startswith("measured by this run")
    assert "sig_gram_dma_kernel" in rf["traffic_source"]["kernel"]
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["cores"] >= 1
    names = [s["name"] for s in line["secondary"]]
    assert names == ["c2-linear-lattice", "c2-linear-order5", "c2-rbf", "c3-rbf", "c3-rbf-increments", "c3-linear", "c5-rbf", "c4-single-gpu",
                     "grad-c2shape-n1024-linear", "grad-c2shape-n1024-linear-level-primitives", "grad-c2shape-n1024-linear-pair-kernels",
                     "grad-c2shape-n1024-rbf", "grad-c2shape-n1024-matern32", "grad-n512-l128-rbf", "c2-matern32", "grad-n512-rbf-order2", "grad-c3-rbf-order2",
                     "svgp-step-charactertrajectories", "svgp-step-netflow", "svgp-step-arabicdigits", "svgp-step-cmusubject16", "c3-svgp-predict",
                     "c2-rbf-order2", "c3-rbf-order2"]
    ho = line["secondary"][1]                           # the higher-order algorithm at order = num_levels: the same contraction, the same time
    assert ho["bound"] == "mfma" and ho["ms_per_step"] < 1.3 * line["ms_per_step"]
    lat = line["secondary"][0]                          # the same Gram through the pair recursion: vector-issue bound, about twice the time
    assert lat["bound"] == "valu-issue" and 0.3 < lat["issue_frac"] <= 1.05 and lat["ms_per_step"] > line["ms_per_step"]
    # the instruction counts behind issue_frac are measured by the run itself (one rocprofv3 --pmc SQ_INSTS_VALU pass per record), not typed in
    for i in (0, 2, 3, 4, 6):
        assert line["secondary"][i]["issue_source"].startswith("measured by this run"), line["secondary"][i]
    c4 = line["secondary"][7]                           # configs[3] on one GPU: the N = 1 point of the scaling series' own workload
    assert c4["name"] == "c4-single-gpu" and c4["rel_err"] <= 1e-6 and "N=32768" in c4["workload"] and c4["ms_per_step"] > 100
    for s in line["secondary"]:
        assert not s.get("error"), s
        assert s["ms_per_step"] > 0
        if not s["name"].startswith(("grad-", "svgp-step-", "c3-svgp")) and s["name"] != "c2-matern32":
            assert s["rel_err"] <= (1e-4 if s["dtype"] == "f32" else 1e-6) and s["clock_ghz"] > 1.0
    c3l = line["secondary"][5]                          # configs[2] with SignatureLinear: Kzx as one product of level features (round 4)
    assert c3l["bound"] == "mfma" and c3l["ms_per_step"] < line["secondary"][3]["ms_per_step"]
    c5 = line["secondary"][6]                           # configs[4]: priced as issue-bound from its counters (round 4)
    assert c5["bound"] == "valu-issue" and 0.5 < c5["issue_frac"] <= 1.1
    # round 6: one SVGP step at the reference's own run settings (benchmarks/run_gpsig_benchmarks.py:32) -- the wide shapes (10, 28, 126 columns) cost
    # no more per column-FMA than the 8-column shape the tile kernels serve -- and configs[2] end to end
    sv = {s["name"]: s for s in line["secondary"] if s["name"].startswith("svgp-step-")}
    base = sv["svgp-step-charactertrajectories"]["column_fma_per_s"]
    for name in ("svgp-step-netflow", "svgp-step-arabicdigits", "svgp-step-cmusubject16"):
        assert sv[name]["column_fma_per_s"] > base / 3.0, (name, sv[name]["column_fma_per_s"], base)
        assert sv[name]["ms_per_step"] < 40.0
    pr = [s_ for s_ in line["secondary"] if s_["name"] == "c3-svgp-predict"][0]
    assert pr["name"] == "c3-svgp-predict" and pr["finite"] and 0 < pr["covariances_ms"] < pr["ms_per_step"] < 30.0
    g = {s["name"]: s["ms_per_step"] for s in line["secondary"] if s["name"].startswith("grad-")}
    # the linear kernel's reverse pass through the feature contraction: several times faster than through the pair kernels
    assert g["grad-c2shape-n1024-linear"] * 3 < g["grad-c2shape-n1024-linear-pair-kernels"]
    assert g["grad-c2shape-n1024-linear"] < 1.1 * g["grad-c2shape-n1024-linear-level-primitives"]     # the level sum as one op is not slower
    # round 5's fused reverse kernel is what runs (the Lam-through-HBM route took 48 / 106 / 55 ms for these three)
    assert g["grad-c2shape-n1024-rbf"] < 25 and g["grad-c2shape-n1024-matern32"] < 35 and g["grad-n512-l128-rbf"] < 32
    assert [s_ for s_ in line["secondary"] if s_["name"] == "c2-matern32"][0]["ms_per_step"] < 75       # (run-time-kind instances: 77-84 ms)
    assert line["secondary"][3]["stream_frac"] > 0     # printed as stream_frac, never as an HBM fraction above 1
    # round 6: order 2 of SignatureRBF -- exact instances (K(X): 2.5 x order 1, was 9 x), higher-order chains in the tile kernel (Kzx: 1.15 x), fused reverse passes
    by = {s_["name"]: s_ for s_ in line["secondary"]}
    assert by["c2-rbf-order2"]["ms_per_step"] < 4.5 * by["c2-rbf"]["ms_per_step"] and by["c2-rbf-order2"]["rel_err"] <= 1e-6
    assert by["c3-rbf-order2"]["ms_per_step"] < 2.0 * by["c3-rbf"]["ms_per_step"] and by["c3-rbf-order2"]["rel_err"] <= 1e-6
    assert g["grad-n512-rbf-order2"] < 120 and g["grad-c3-rbf-order2"] < 6 * by["c3-rbf-order2"]["ms_per_step"] + 6
