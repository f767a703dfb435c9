"""A plain bench.py run: the headline line only (no oracle check, no side legs, no CPU baseline), --steps timed steps, and
--dump-outputs writing the same sample of the last timed step's audio from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_plain(out_dir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "PBSO_BENCH_BACKEND", "PBSO_BENCH_GATHER_SELF"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--objects", "64", "--buffers", "86",
                        "--steps", "5", "--warmup", "1", "--settle", "4", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    d = run_plain(tmp_path / "a")
    for k, t in dict(metric=str, value=float, unit=str, higher_is_better=bool, dtype=str, ms_per_step=float).items():
        assert isinstance(d[k], t), k
    assert d["steps"] == 5 and d["warmup"] == 1 and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert abs(d["value"] - 64 * 86 * 513 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for k in ("parity", "cpu_baseline", "strong_share", "steps_of_one_second", "exact_f32_projection",
              "mixed_precision_projection", "host_delivered"):
        assert k not in d, k
    e = run_plain(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["audio_row_ids.npy", "audio_rows.npy", "audio_samples.npy"] == sorted(os.listdir(tmp_path / "b"))
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all()
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    rows = np.load(tmp_path / "a" / "audio_rows.npy")
    assert rows.shape == (16, 86 * 513) and np.abs(rows).max() > 0
