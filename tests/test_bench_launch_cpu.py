"""bench.py --gpus N outside a torch.distributed launch starts N ranks itself
(VERDICT r03 missing #2): one process per rank through torch.distributed.run,
started before anything touches the GPU, rank 0 printing the one JSON line
with n_gpus = N and every rank's time.  --dry-run runs exactly that rank /
barrier / max-over-ranks path over gloo with a no-op step (no device here)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env,
                       capture_output=True, text=True, timeout=240, cwd="/tmp")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return lines


def test_bench_gpus2_launches_two_ranks_one_line():
    lines = _run(["--gpus", "2", "--dry-run", "--steps", "2", "--warmup", "1"])
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and len(d["rank_ms_per_step"]) == 2
    ranks = sorted(r for r, _ in d["rank_pids"])
    pids = {p for _, p in d["rank_pids"]}
    assert ranks == [0, 1] and len(pids) == 2
    assert d["ms_per_step"] == max(d["rank_ms_per_step"])


def test_bench_extras_need_full():
    """--cpu-sample / --host-stream ask for what only --full measures."""
    bench = os.path.join(ROOT, "bench.py")
    for extra in (["--cpu-sample", "5"], ["--host-stream", "100"]):
        p = subprocess.run([sys.executable, bench, "--dry-run"] + extra, capture_output=True,
                           text=True, timeout=60)
        assert p.returncode == 2 and "--full" in p.stderr
    d = json.loads(_run(["--dry-run", "--full", "--cpu-sample", "5", "--steps", "1"])[0])
    assert d["steps"] == 1


def test_dump_outputs_float64_and_seeded_sample(tmp_path, monkeypatch):
    """--dump-outputs writes float64 .npy; over the byte limit the per-subint
    arrays keep the same seeded rows, the same from call to call."""
    import numpy as np
    import bench
    n = 1000
    arrays = {"params": np.arange(n * 5.0).reshape(n, 5), "status": np.arange(n, dtype=np.int32),
              "template": np.ones(7, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "all"), arrays, n)
    for k, a in arrays.items():
        got = np.load(str(tmp_path / "all" / (k + ".npy")))
        assert got.dtype == np.float64 and np.array_equal(got, a)
    monkeypatch.setattr(bench, "DUMP_LIMIT", 10000)
    for name in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / name), arrays, n)
    got = {f[:-4]: np.load(str(tmp_path / "s1" / f)) for f in os.listdir(str(tmp_path / "s1"))}
    assert sorted(got) == ["params", "sample_rows", "status", "template"]
    rows = got["sample_rows"].astype(int)
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0)
    assert np.array_equal(got["params"], arrays["params"][rows])
    assert np.array_equal(got["status"], arrays["status"][rows])
    assert np.array_equal(got["template"], arrays["template"])
    assert sum(a.nbytes for a in got.values()) <= 10000
    for k, a in got.items():
        assert np.array_equal(a, np.load(str(tmp_path / "s2" / (k + ".npy")))), k


def test_bench_gpus1_stays_in_process():
    d = json.loads(_run(["--dry-run", "--steps", "1", "--warmup", "0"])[0])
    assert d["n_gpus"] == 1 and len(d["rank_pids"]) == 1
