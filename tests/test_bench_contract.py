"""The driver's contract with bench.py (one JSON line on stdout; keys, types, roofline and cpu_baseline objects),
checked on a small run -- `-m gpu`."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_contract_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "128", "--warmup", "64",
                          "--envs", "8192", "--cpu-seconds", "2", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    with open(os.path.join(ROOT, "BASELINE.json")) as fh:
        base = json.load(fh)
    assert d["metric"] in base["metric"] and d["unit"] == "env-steps/s"
    assert d["n_gpus"] == 1 and d["steps"] == 128 and d["warmup"] == 64
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 1e6 and abs(d["value"] - 8192 * 128 / (d["ms_per_step"] * 1e-3 * 128)) < 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and r["achieved"] > 0
    assert r["traffic"] is None or r["traffic"] > 0            # PMC profile on file only for the 65 536-env shapes
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "env-steps/s" and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    for sec in ("fused_rollout", "graph_replay", "steady_state_no_reset"):
        assert "error" not in d[sec], d[sec]
    assert d["repeats"] >= 1 and d["timed_step_indices_after_reset"][0] == 0 and d["us_per_step"]["min"] <= d["us_per_step"]["max"]
    assert r["frac"] <= 1.0 or "frac_above_one_because" in r
    assert r["min_bytes_per_env_step"] == 125 and r["frac_min_bytes"] > 0
    assert c["by_devices"]["4"]["value"] == c["value"] and c["nproc"] >= c["cores"]


@pytest.mark.gpu
def test_bench_config4_prints_a_contract_line_with_one_launch_per_step():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "4", "--steps", "20", "--warmup", "5",
                          "--envs", "4096", "--repeats", "20", "--cpu-seconds", "2", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["unit"] == "env-steps/s" and d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["repeats"] == 20
    assert "InvertedPendulum" in d["config"]["workload"] and d["dtype"] == "f64" and d["vs_baseline"] is None
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["launches_per_step"] == 1 and r["kernel"] == "pend_step_kernel"
    assert r["mfma"]["instruction"] == "v_mfma_f64_16x16x4_f64" and 5 < r["mfma"]["plant_substeps_per_env_step"] < 15
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["value"] > 0


@pytest.mark.gpu
def test_bench_multi_gpu_code_path_runs_on_rccl_with_one_rank():
    """GW_BENCH_FORCE_GATHER=1: the N > 1 path of bench.py (process group on RCCL, chunked feedback gather every 16 steps with
    the warm-up flush and the end-of-region drain, the per-step observation gather) with a single rank -- every collective call
    the driver's multi-GPU runs make, on the one GPU this box has."""
    env = dict(os.environ, GW_BENCH_FORCE_GATHER="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                          "--envs", "8192", "--repeats", "30", "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=600,
                         cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-1000:]                  # ONE line on stdout although RCCL prints a banner to fd 1
    d = json.loads(lines[0])
    assert d["config"]["obs_gather"] == "per-step" and "after EVERY env.step()" in d["config"]["parallelism"]
    g = d["gather_forms"]
    for form, late in (("no_gather", None), ("pipelined_gather", 1), ("chunked_gather", 16)):
        assert "error" not in g[form], g[form]
        assert g[form]["observations_late_by_steps"] == late and g[form]["env_steps_per_s"] > 1e6
    assert g["pipelined_gather"]["bytes_per_rank_per_step"] == 9 * 8192 and g["chunked_gather"]["bytes_per_rank_per_step"] == 8192
    assert d["value"] > 1e6 and d["value"] <= g["no_gather"]["env_steps_per_s"] * 1.5
    r = d["ranks"]
    assert r["world_size"] == 1 and r["backend"] == "nccl" and len(r["devices"]) == 1 and r["devices"][0] and r["rccl_version"]
    assert "without the per-step gather" in d["roofline"]["how"].lower()


@pytest.mark.gpu
def test_plain_bench_gpus_2_starts_its_own_ranks():
    """`python3 bench.py --gpus 2` with NO launcher: the parent starts two fresh rank processes before touching HIP, relays
    rank 0's one line and exits 0.  Two RCCL ranks cannot share the one GPU of this box, so the collectives run on gloo
    (GW_BENCH_BACKEND=gloo: the rehearsal mode) -- launcher, rendezvous, sharded action stream, per-step gather protocol,
    max-over-ranks timing and the `ranks` evidence are the code the driver's N-GPU command runs."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["GW_BENCH_BACKEND"] = "gloo"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "20", "--warmup", "5",
                          "--envs", "8192", "--repeats", "10", "--full"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-1000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_envs"] == 2 * 8192 and d["config"]["obs_gather"] == "per-step"
    assert "cpu_baseline" not in d and d["scaling"] == "weak" and d["value"] > 1e5
    r = d["ranks"]
    assert r["world_size"] == 2 and r["backend"] == "gloo" and len(r["devices"]) == 2 and "launch_ranks" in r["launcher"]
    assert sorted(e["rank"] for e in r["per_rank"]) == [0, 1] and len({e["pid"] for e in r["per_rank"]}) == 2
    for form in ("no_gather", "pipelined_gather", "chunked_gather"):
        assert "error" not in d["gather_forms"][form], d["gather_forms"][form]


def _one_line(out):
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_times_exactly_its_steps_and_dumps_what_the_last_step_returned(tmp_path):
    """A plain run (no --full) times --steps steps once, reports the headline only, and --dump-outputs writes the outputs of
    the last timed step: the oracle's after the same windows (two untimed warm-up windows + `repeats` timed ones; a reset
    does not rewind the env clock, so every window counts) of the same action stream."""
    import numpy as np
    from gymwipe_amd.actions import actions_numpy
    from oracle.ct_oracle import CtOracle
    N, D, K, W = 1024, 4, 59, 5
    runs = []
    for repeats in ("1", "3"):
        out_dir = tmp_path / ("r" + repeats)
        d = _one_line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                                      "--warmup", str(W), "--envs", str(N), "--repeats", repeats, "--dump-outputs", str(out_dir)],
                                     capture_output=True, text=True, timeout=600, cwd=ROOT))
        assert d["steps"] == K and d["warmup"] == W and d["repeats"] == int(repeats) and d["ms_per_step"] > 0
        assert d["metric"] and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
        assert abs(d["value"] - N / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
        for sec in ("cpu_baseline", "fused_rollout", "graph_replay", "steady_state_no_reset", "gather_forms"):
            assert sec not in d, sec
        dumped = {k: np.load(str(out_dir / (k + ".npy"))) for k in ("obs", "reward", "done")}
        assert sorted(p.name for p in out_dir.iterdir()) == ["done.npy", "obs.npy", "reward.npy"]
        for a in dumped.values():
            assert a.shape == (N,) and a.dtype in (np.float32, np.float64)
        runs.append((2 + int(repeats), dumped))
    orc = CtOracle(N, D, nthreads=8)
    dev, dur = actions_numpy(1234, 0, N, 0, W + K, D)
    windows = 0
    for n_windows, got in runs:
        while windows < n_windows:
            for i in range(W + K):
                if i % 64 == 0:
                    orc.reset()
                o, r, dn = orc.step(dev[i], dur[i])
            windows += 1
        assert (got["obs"] == o).all() and (got["reward"] == r).all() and (got["done"] == dn).all()


@pytest.mark.gpu
def test_plain_bench_config4_dumps_the_pendulum_outputs(tmp_path):
    d = _one_line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "4", "--steps", "20", "--warmup", "5",
                                  "--envs", "4096", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600,
                                 cwd=ROOT))
    assert d["steps"] == 20 and d["repeats"] == 1 and "cpu_baseline" not in d
    import numpy as np
    for k in ("obs", "reward", "done", "sensor_angle"):
        a = np.load(str(tmp_path / (k + ".npy")))
        assert a.shape == (4096,) and a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
