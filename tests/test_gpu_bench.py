"""bench.py's JSON contract on the GPU (a short run of the default workload in a child process): one JSON line with
the BASELINE.json metric, and the roofline / throughput fields consistent with each other."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_bench_json_line_is_self_consistent():
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "5", "--warmup", "2", "--full",
                        "--no-cpu-baseline", "--no-pmc"], cwd=REPO, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    with open(os.path.join(REPO, "BASELINE.json")) as f:
        assert out["metric"] == json.load(f)["metric"]
    assert out["n_gpus"] == 1 and out["steps"] == 5 and out["warmup"] == 2 and out["higher_is_better"] is True
    cfg = out["config"]
    # the default entry is the reference trainer's COO wiring (bench.py --entry coo)
    assert cfg["entry"].startswith("trainer COO"), cfg["entry"]
    assert cfg["num_nodes"] == 160_000 and cfg["nnz_per_adjacency"] == 6_559_580 and cfg["feat_dim"] == 128
    edges = 3 * cfg["nnz_per_adjacency"] * cfg["layers"]
    assert abs(out["value"] - edges / (out["ms_per_step"] * 1e-3)) <= 2e-3 * out["value"]
    rf = out["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    # bench.py derives achieved / frac from the avg_launch_ms it emits: recomputing them from the line differs only
    # by the 0.1 GB/s rounding of achieved (no dependence on the measured time's digits)
    achieved = rf["algorithmic_bytes_per_launch"] / (rf["avg_launch_ms"] * 1e-3) / 1e9
    assert abs(rf["achieved"] - achieved) <= 0.051 + 1e-9 * achieved
    assert abs(rf["frac"] - achieved / rf["peak"]) <= 1e-5
    assert 0.0 < rf["frac"] < 1.0  # compulsory bytes: physically below peak
    # the dominant kernel is one of the step's kernels: its launches take less than the whole step
    assert rf["avg_launch_ms"] < out["ms_per_step"]
    # one entry per hot-path kernel, each self-consistent; the dominant one has the largest measured time per step,
    # and together they fit inside the step
    ks = rf["kernels"]
    assert set(ks) == {"propagation", "dense", "head"}
    for k, e in ks.items():
        a = e["algorithmic_bytes_per_launch"] / (e["avg_launch_ms"] * 1e-3) / 1e9
        assert abs(e["achieved"] - a) <= 0.051 + 1e-9 * a, k
        assert 0.0 < e["frac"] < 1.0 and e["launches_timed"] >= e["launches_per_step"], k
    assert rf["kernel"] == max(ks.values(), key=lambda e: e["ms_per_step"])["kernel"]
    # per-kernel times come from eager steps after the timed (graph-replay) region, bracketed themselves by events on
    # the same stream: the kernels of one step run one after another there, so their sum fits inside that step (2 %
    # for event resolution); and the eager step is the graph-replayed step plus launch gaps, not a different workload
    ek = rf["eager_ms_per_step"]
    assert sum(e["ms_per_step"] for e in ks.values()) <= ek * 1.02 + 2e-3, (ks, ek)
    assert out["ms_per_step"] * 0.9 <= ek <= out["ms_per_step"] * 1.6 + 0.05, (out["ms_per_step"], ek)
    assert ks["propagation"]["algorithmic_bytes_per_launch"] == 411_520_000  # SURVEY 8(d) / DESIGN §4 at B(20,4)
    assert abs(ks["dense"]["algorithmic_bytes_per_launch"] - 494.7e6) < 0.5e6


@pytest.mark.timeout(120)
def test_bench_plain_run_dumps_last_step_outputs(tmp_path):
    """A plain run (no --full) measures the headline figure only ('roofline' and 'cpu_baseline' null) and
    --dump-outputs writes the last timed step's log-probs and embeddings as float32 .npy files. On B(20,3) (8,000
    nodes: every row fits the size budget, so no sample file)."""
    import numpy as np
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--ngram", "3", "--clock-warmup-s", "0", "--dump-outputs", str(d)], cwd=REPO,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["dtype"] == "f32" and out["unit"] == "edges/s"
    assert out["roofline"] is None and out["cpu_baseline"] is None and "extra" not in out
    edges = 3 * out["config"]["nnz_per_adjacency"] * out["config"]["layers"]
    assert abs(out["value"] - edges / (out["ms_per_step"] * 1e-3)) <= 2e-3 * out["value"]
    assert sorted(p.name for p in d.iterdir()) == ["embeddings.npy", "log_probs.npy"]
    lp, emb = np.load(d / "log_probs.npy"), np.load(d / "embeddings.npy")
    assert lp.dtype == np.float32 and lp.shape == (8000, 20) and emb.dtype == np.float32 and emb.shape == (8000, 128)
    # what the model's head returns: log_softmax rows (probabilities sum to 1) and L2-normalised embedding rows
    assert np.abs(np.exp(lp.astype(np.float64)).sum(1) - 1.0).max() < 1e-5
    assert np.abs(np.linalg.norm(emb.astype(np.float64), axis=1) - 1.0).max() < 1e-5


@pytest.mark.timeout(300)
@pytest.mark.parametrize("gpus,partition,label", [(2, "auto", "replicate_then_middle_x2"),
                                                   (2, "middle", "middle_ghost_a2a_x2"),
                                                   (3, "halo", "halo_recompute_x3"),
                                                   (4, "middle", "middle_ghost_a2a_x4")])
def test_bench_multi_rank_rehearsal(gpus, partition, label):
    """bench.py --gpus N with N gloo ranks sharing this GPU (the driver's N > 1 launch shape, RCCL replaced by gloo):
    each partition runs its timed loop and rank 0 prints one JSON line with the whole job's numbers."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", str(gpus), "--dist-backend", "gloo",
                        "--one-device", "--steps", "3", "--warmup", "1", "--no-pmc", "--clock-warmup-s", "0",
                        "--partition", partition], cwd=REPO, capture_output=True, text=True, timeout=280, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == gpus and out["config"]["parallelism"] == label and out["value"] > 0
