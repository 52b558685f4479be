"""CPU: bench.py's launcher half (no GPU touched) and the CPU-baseline harness of oracle/cpu_baseline.py."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_n_without_a_distributed_env_launches_n_ranks(monkeypatch, capsys):
    """`python bench.py --gpus 4` must start 4 ranks under torch.distributed.run itself and relay rank 0's line."""
    bench = _load_bench()
    seen = {}

    def fake_run(cmd, env=None, stdout=None, text=None):
        seen["cmd"], seen["env"] = cmd, env
        line = json.dumps({"metric": "rows/sec through X'WX kernel at p=500", "value": 1.0, "n_gpus": 4})
        return types.SimpleNamespace(returncode=0, stdout="[rank1] noise\n" + line + "\n")

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "2"])
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(v, raising=False)
    assert bench.main() == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nnodes=1" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4" and cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "7", "--warmup", "2"] and cmd[-7].endswith("bench.py")
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and json.loads(out[0])["n_gpus"] == 4
    assert "torch" not in bench.__dict__           # the launcher never imported torch, let alone touched the GPU


def test_launcher_fails_when_rank0_reports_another_world(monkeypatch):
    bench = _load_bench()
    monkeypatch.setattr(bench.subprocess, "run", lambda *a, **k: types.SimpleNamespace(
        returncode=0, stdout=json.dumps({"metric": "m", "n_gpus": 1}) + "\n"))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.main() != 0


def test_worker_refuses_world_size_mismatch(monkeypatch):
    bench = _load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert "WORLD_SIZE" in str(e.value)


def test_traffic_is_null_for_a_profile_of_another_kernel_source(monkeypatch, tmp_path):
    bench = _load_bench()
    t, src = bench.traffic_from_profile(500, 1000)
    prof = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))
    have = bench.gram_sources_sha16()
    if prof.get("gram_hip_sha16") == have:
        assert t is not None and t > 0 and have in src
    else:
        assert t is None and "stale" in src
    assert bench.traffic_from_profile(100, 1000)[0] is None


def test_fast_synth_matches_the_numpy_generator():
    from oracle import dlsa_oracle as orc, fast_synth
    fast_synth.build()
    assert fast_synth.load() is not None
    for row0 in (0, 12345678901):
        A = fast_synth.synth_features(7, row0, 300, 33, orc.SYNTH_UNIFORM)
        assert np.array_equal(A, orc.synth_features(7, row0, 300, 33, orc.SYNTH_UNIFORM))      # bit-identical
        G = fast_synth.synth_features(7, row0, 300, 8, orc.SYNTH_GAUSSIAN)
        assert np.max(np.abs(G - orc.synth_features(7, row0, 300, 8, orc.SYNTH_GAUSSIAN))) < 1e-15   # libm last ulp
        assert np.array_equal(fast_synth.synth_label_uniforms(7, row0, 500), orc.synth_label_uniforms(7, row0, 500))


def test_cpu_baseline_harness_small():
    """The section-8(d) harness on a toy size: pools of single-threaded workers (a sweep over worker counts: `value` is the fastest
    pool's map rate, `cores` the workers it used) + single process + bare Gram."""
    from oracle import cpu_baseline
    ncpu = os.cpu_count()
    r = cpu_baseline.run(12, 5, rows_per_partition=3000, gram_rows=20000, single_partitions=2, workers_sweep=(2, ncpu))
    assert r["kind"] == "port" and r["unit"] == "rows/s" and r["host_cores"] == ncpu
    assert [s["workers"] for s in r["pool_sweep"]] == sorted({2, ncpu})
    pool = r["pool"]
    assert pool in r["pool_sweep"] and r["cores"] == pool["workers"] and pool["threads_per_worker"] == 1
    assert abs(r["value"] - max(s["map_rows_per_s"] for s in r["pool_sweep"])) < 1e-9 and abs(r["value"] - pool["map_rows_per_s"]) < 1e-9
    for s in r["pool_sweep"]:
        assert s["rows"] == s["workers"] * 3000 and s["map_wall_s"] > 0 and s["lars_wall_s"] > 0
        assert s["theta_err_vs_truth_linf"] < 0.8          # the combined estimate is near beta* (first 4 ones, rest 0)
    assert r["single_process"]["partitions"] == 2 and r["gram"]["rows_per_s"] > 0
    assert "%d workers" % pool["workers"] in r["sample"]
    # the default sweep on a host with fewer than 32 cores is the one pool that uses them all
    if ncpu < 32:
        d = cpu_baseline.run(12, 5, rows_per_partition=3000, gram_rows=20000, single_partitions=1)
        assert [s["workers"] for s in d["pool_sweep"]] == [ncpu] and d["cores"] == ncpu


def test_bench_arguments_round3():
    """--scaling / --e2e-partitions parse; the defaults are the contract's (N = 1, K = 10, W = 2: minutes, not hours)."""
    bench = _load_bench()
    a = bench.parse([])
    assert (a.gpus, a.steps, a.warmup, a.scaling, a.e2e_partitions) == (1, 10, 2, "both", 25)
    assert bench.parse(["--gpus", "8", "--scaling", "strong"]).scaling == "strong"
    with pytest.raises(SystemExit):
        bench.parse(["--scaling", "sideways"])


def test_committed_traffic_profile_matches_the_tree():
    """profiles/pmc_latest.json must have been taken from the Gram sources in the tree, or `roofline.traffic` is null in the
    driver's bench line: a reminder to re-run bench/profile_round.sh after touching gram.hip / gram_cyclic.hip / common.h."""
    bench = _load_bench()
    prof = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))
    assert prof.get("gram_hip_sha16") == bench.gram_sources_sha16(), "stale profiles/pmc_latest.json"
    t, _ = bench.traffic_from_profile(500, 25_000_000)
    assert 0.99 * 25e6 * 4008 < t < 1.05 * 25e6 * 4008          # fabric traffic ~ the algorithmic bytes of the launch


def test_rank_threads_never_oversubscribe_the_host():
    """N ranks x (OpenMP / torch intra-op threads) stay within the node's cores; the launcher exports it."""
    bench = _load_bench()
    for ncpu in (8, 64, 128, 256):
        for n in (1, 2, 4, 8):
            t = bench.rank_threads(ncpu, n)
            assert 1 <= t <= 8 and t * n <= max(ncpu, n)
    assert bench.rank_threads(8, 8) == 1 and bench.rank_threads(256, 8) == 8 and bench.rank_threads(4, 8) == 1


def test_launcher_exports_the_per_rank_thread_count(monkeypatch):
    bench = _load_bench()
    seen = {}

    def fake_run(cmd, env=None, stdout=None, text=None):
        seen["env"] = env
        return types.SimpleNamespace(returncode=0, stdout=json.dumps({"metric": "m", "n_gpus": 8}) + "\n")

    monkeypatch.setattr(bench.subprocess, "run", fake_run)
    monkeypatch.setattr(bench.os, "cpu_count", lambda: 16)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8"])
    for v in ("WORLD_SIZE", "OMP_NUM_THREADS"):
        monkeypatch.delenv(v, raising=False)
    assert bench.main() == 0
    assert seen["env"]["OMP_NUM_THREADS"] == "2"


def test_bench_arguments_round6():
    """the end-to-end fit legs are part of the --full line (--no-e2e leaves them out; --e2e still parses), and the warm-up is
    extended until two launches agree, for at most --warmup-cap-seconds"""
    bench = _load_bench()
    a = bench.parse([])
    assert a.no_e2e is False and a.warmup_cap_seconds == 5.0
    assert bench.parse(["--no-e2e"]).no_e2e is True and bench.parse(["--e2e"]).no_e2e is False
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ("first_over_median", "warmup_extra_steps", "first_step_ms_over_ranks", '"k1"', '"lock_step"', "passes_per_partition"):
        assert key in src, key


def test_bench_arguments_full_and_dump():
    """A plain run is the headline figure alone: the other legs need --full; --dump-outputs takes a directory."""
    bench = _load_bench()
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_float64_and_samples_beyond_the_cap(monkeypatch, tmp_path):
    bench = _load_bench()
    H = np.arange(30.0).reshape(5, 6)
    bench.dump_outputs(str(tmp_path / "all"), {"H": H})
    assert np.array_equal(np.load(str(tmp_path / "all" / "H.npy")), H)
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 8 * 20)
    big = {"H": H, "v": np.arange(10, dtype=np.float32)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in big}
    assert sum(g.nbytes for g in got.values()) <= 8 * 20 and all(g.dtype == np.float64 for g in got.values())
    assert set(got["H"]) <= set(H.ravel()) and list(got["H"]) == sorted(got["H"]) and got["H"].size == 30 * 20 // 40
    for k in big:                                    # the sample is fixed: the same entries every time
        assert np.array_equal(got[k], np.load(str(tmp_path / "b" / (k + ".npy"))))


def test_bench_arguments_round4():
    bench = _load_bench()
    a = bench.parse([])
    assert a.preflight is False and a.sustain_seconds == 12.0
    assert bench.parse(["--preflight", "--gpus", "8"]).preflight is True


def test_preflight_only_run_needs_no_json_line(monkeypatch):
    bench = _load_bench()
    monkeypatch.setattr(bench.subprocess, "run", lambda *a, **k: types.SimpleNamespace(returncode=0, stdout="[bench] preflight ok\n"))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--preflight"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert bench.main() == 0
    monkeypatch.setattr(bench.subprocess, "run", lambda *a, **k: types.SimpleNamespace(returncode=3, stdout=""))
    assert bench.main() == 3


def test_committed_kernel_evidence_matches_the_tree():
    """profiles/r0N_pmc_<kernel>.json (bench/pmc_evidence.py; the newest round's file per kernel) carry the hash of the sources they
    were taken from: a kernel whose sources changed since needs its counters taken again (python3 bench/pmc_evidence.py r05 <tag> on
    the GPU box)."""
    sys.path.insert(0, os.path.join(ROOT, "bench"))
    import pmc_evidence as ev
    stale = []
    for tag, k in ev.KERNELS.items():
        path = ev.latest_evidence_path(tag)
        assert os.path.exists(path), "missing " + path
        doc = json.load(open(path))
        if doc["sources_sha16"] != ev.sources_sha16(k["src"]):
            stale.append(tag)
        assert doc["kernels"], tag
        kk = next(iter(doc["kernels"].values()))
        assert kk.get("duration_ms_under_pmc", 0) > 0 and "GRBM_GUI_ACTIVE" in kk and "FETCH_SIZE" in kk, tag
    assert not stale, "stale evidence for: " + ", ".join(stale)


def test_committed_eight_rank_dry_run_line_is_consistent_with_the_one_rank_line():
    """profiles/r06_bench_gloo8_dryrun.json: `DLSA_BENCH_BACKEND=gloo python bench.py --gpus 8 --rows-per-gpu 2000000` (eight ranks
    SHARING one GPU over gloo: the N > 1 code path of the line, rates meaningless) against profiles/r06_bench_rows2e6_n1.json, the N = 1
    line at the same rows per GPU: same metric / dtype / unit / rows per GPU / workload kernel, value = N x value_per_gpu, the ranks
    counted from the communicator, a strong-scaling leg that kept the metric's kernel."""
    n8 = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_gloo8_dryrun.json")))
    n1 = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_rows2e6_n1.json")))
    assert n8["n_gpus"] == 8 and n1["n_gpus"] == 1
    for key in ("metric", "unit", "dtype", "higher_is_better", "scaling", "data", "steps", "warmup"):
        assert n8[key] == n1[key], key
    assert n8["config"]["rows_per_gpu"] == n1["config"]["rows_per_gpu"] == 2_000_000 and n8["config"]["p"] == n1["config"]["p"] == 500
    assert n8["config"]["parallelism"] == "row-shards x8" and n1["config"]["parallelism"] == "row-shards x1"
    assert abs(n8["value_per_gpu"] * 8 - n8["value"]) <= 1e-9 * n8["value"] and abs(n1["value_per_gpu"] - n1["value"]) <= 1e-9 * n1["value"]
    assert n8["comm_ranks"] == 8 and n8["rccl_ranks"] == 0 and n1["comm_ranks"] == 1          # (gloo dry run: no RCCL rank claimed)
    assert n8["allreduce"]["ranks"] == 8 and n8["allreduce"]["payload_bytes"] == (500 * 500 + 2 * 500) * 8
    assert "gram_cyclic_kernel" in n8["roofline"]["kernel"] and "gram_cyclic_kernel" in n1["roofline"]["kernel"]
    ss = n8["strong_scaling"]
    assert ss and "skipped" not in ss and ss["rows_per_gpu"] == 250_000 and "gram_cyclic_kernel" in ss["kernel"]
    assert n8["roofline"]["algorithmic_bytes_per_row"] == n1["roofline"]["algorithmic_bytes_per_row"] == 4008


def test_strong_scaling_leg_is_refused_below_the_kernel_floor():
    bench = _load_bench()
    assert bench.STRONG_MIN_ROWS == 65536
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "strong-scaling leg skipped" in src and "R // world < STRONG_MIN_ROWS" in src


def _newest_round_with(suffixes):
    import glob
    import re
    rounds = sorted({int(re.match(r"r(\d+)_", os.path.basename(f)).group(1)) for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_kernel_stats.csv"))},
                    reverse=True)
    for r in rounds:
        paths = [os.path.join(ROOT, "profiles", "r%02d_%s" % (r, s)) for s in suffixes]
        if all(os.path.exists(p) for p in paths):
            return r, paths
    return None, None


def test_committed_rocprof_summary_reproduces_the_committed_default_line():
    """round 5's rocprofv3 CSV (98.9 ms for the dispatched kernel) was committed beside a default line of 91.0 ms --
    a kernel cannot take longer than the step that holds it.  From round 6 on bench/profile_round.sh makes the unprofiled default run
    and the profiled run in ONE gpurun call; the committed CSV's average for the kernel the line names must be within 3 % of the
    line's HIP-event kernel_ms, and pmc_latest.json carries the same-call record."""
    import csv
    r, paths = _newest_round_with(("bench_kernel_stats.csv", "bench_default.json"))
    assert r is not None
    if r < 6:
        pytest.skip("no round-6 profile committed yet (round 5's pair is the one the guard was written for)")
    line = json.loads([l for l in open(paths[1]) if l.startswith("{")][-1])
    kname = line["roofline"]["kernel"].split("dlsa::")[1].split(" ")[0]
    rows = [row for row in csv.DictReader(open(paths[0])) if kname.replace(",", ", ") in row["Name"] or kname in row["Name"].replace(" ", "")]
    assert len(rows) == 1, (kname, [row["Name"] for row in rows])
    avg_ms = float(rows[0]["AverageNs"]) / 1e6
    assert abs(avg_ms / line["roofline"]["kernel_ms"] - 1.0) < 0.03, (avg_ms, line["roofline"]["kernel_ms"])
    assert avg_ms <= line["ms_per_step"] * 1.03
    prof = json.load(open(os.path.join(ROOT, "profiles", "pmc_latest.json")))
    sc = prof["same_call"]
    assert kname.replace(" ", "") in sc["kernel"].replace(" ", "") and abs(sc["rocprof_over_unprofiled"] - 1.0) < 0.03
    assert abs(sc["unprofiled_kernel_ms"] - line["roofline"]["kernel_ms"]) < 1e-9          # the committed line IS that call's unprofiled run
    # the fit legs are in the committed default line (driver-visible numbers for the fit, VERDICT r5 missing 2)
    e2e = line["extra"]["end_to_end_fit"]
    assert e2e["status_ok"] and e2e["k1"]["status_ok"] and e2e["lock_step"]["status_ok"]
    assert line["cpu_baseline"]["value"] >= max(s["map_rows_per_s"] for s in line["cpu_baseline"]["pool_sweep"]) * (1 - 1e-12)
