"""bench.py as a command: a plain run times --steps steps and prints the line
without the --full legs, and --dump-outputs DIR holds what the last timed
step's fit_batch returned -- here against the same call made in-process on
the same synthetic inputs (the fits are bitwise reproducible)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSUB = 96  # subints of the headline shape (64 chan x 2048 bin): one small batch


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from pulseportraiture_amd.engine import get_engine
    return get_engine(0)


def test_plain_run_dumps_last_step(gpu, tmp_path):
    import bench
    from pulseportraiture_amd.engine import results_to_host
    d = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "2", "--warmup", "1", "--nsub", str(NSUB), "--dump-outputs", d],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "TOAs/s" and line["dtype"] == "f64" and line["higher_is_better"]
    # ms_per_step is rounded to 1 us
    assert line["value"] == pytest.approx(NSUB / line["ms_per_step"] * 1e3, rel=1e-2)
    for k in ("legs", "cpu_baseline", "parity_sample", "host_stream"):
        assert line[k] is None, k

    _, _, _, flags, _, log10_tau, _, _ = bench.CONFIGS["headline"]
    w, data, kw, _ = bench.synth_inputs(gpu, "headline", NSUB, 20240917, 0)
    out = gpu.fit_batch(data, kw["model"], kw["freqs"], kw["P"], kw["init"], flags,
                        nu_fit=kw["nu"], log10_tau=log10_tau, guess=True, guess_Ns=100,
                        guess_tau=kw["gtau"])
    ref = results_to_host(out, None, gpu.stream)
    torch.cuda.synchronize()
    names = sorted(f[:-4] for f in os.listdir(d))
    assert names == sorted(ref)
    total = 0
    for k in names:
        got = np.load(os.path.join(d, k + ".npy"))
        total += got.nbytes
        assert got.dtype == np.float64 and got.shape == ref[k].shape, k
        assert np.array_equal(got, ref[k].astype(np.float64), equal_nan=True), k
    assert np.load(os.path.join(d, "params.npy")).shape == (NSUB, 5)
    assert total <= 64e6
