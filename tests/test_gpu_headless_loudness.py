"""pbso_headless --loudness FILE [--loudness-target T]: the loudness bus on what the tool writes.  The report of a --channels 2 --pan
run against the model of tests/loudness_model.py fed the samples of the WAV the tool wrote: the energies and the peaks bit for bit
(through %.17g), integrated within 1e-9 LU, gain_to_target by its formula; the WAV itself is the run's without --loudness."""
import math
import subprocess

import numpy as np
import pytest
import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

from tests import loudness_model as lm
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def _report(path):
    return {k: float(v) for k, v in (line.split() for line in open(path).read().splitlines())}


@pytest.mark.parametrize("mixed", [True, False], ids=["pan", "mono"])
def test_headless_loudness_is_the_model_on_the_samples_of_the_wav(tmp_path, mixed):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, target = 45, (2 if mixed else 1), -16.0
    hits = [(b, 1 + (3 * b) % 7, (0.2 + 0.01 * b, -0.5, 1.0)) for b in range(0, nb, 2)]
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    # two cuts: the stage is stepped in pieces of 20, 10 and 15 buffers.  The data set's object is quiet (a peak of 3e-4 in the WAV);
    # the pan gains bring the mix above the absolute gate, the mono run stays below it and has no integrated loudness
    pan = [(0, (2000.0, 0.0, 500.0, 30.5)), (20, (1000.0, 40.0, 1500.0, 70.25)), (30, (1600.0, 0.0, 1200.0, 10.0))]
    (tmp_path / "pan.txt").write_text("".join(f"{b} 0 " + " ".join(repr(x) for x in gd) + "\n" for b, gd in pan))
    base = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb)]
    if mixed:
        base += ["--channels", str(C), "--ramp", "300", "--pan", str(tmp_path / "pan.txt")]
    _run(base + ["--out", str(tmp_path / "plain.wav")])
    _run(base + ["--out", str(tmp_path / "loud.wav"), "--loudness", str(tmp_path / "loud.txt"), "--loudness-target", repr(target)])
    assert open(tmp_path / "loud.wav", "rb").read() == open(tmp_path / "plain.wav", "rb").read()
    ch, x = _wav(tmp_path / "loud.wav")
    x = np.ascontiguousarray(x).reshape(C, -1)
    assert ch == C and x.shape == (C, nb * B) and np.abs(x).max() > 0

    model = lm.Model(44100, C, true_peak=True)
    model.process(x)
    want, got = model.report(), _report(tmp_path / "loud.txt")
    n = nb * B // 4410
    assert got["n_blocks"] == want["n_blocks"] == n == 5 and got["n_gated"] == want["n_gated"]
    for j in range(n):
        for c in range(C):
            assert np.float64(got[f"energy.{j}.{c}"]).view(np.uint64) == model.records["energy"][j, c].view(np.uint64), (j, c)
            assert np.float32(got[f"true_peak.{j}.{c}"]) == model.records["true_peak"][j, c] > 0, (j, c)
            assert np.float32(got[f"sample_peak.{j}.{c}"]) == model.records["sample_peak"][j, c] > 0, (j, c)
    print(f"integrated {got['integrated']} LUFS, true peak {got['true_peak']}, gain to {target}: {got['gain_to_target']}")
    assert math.isfinite(want["momentary"]) and math.isfinite(want["integrated"]) == mixed
    for k in ("integrated", "momentary", "max_momentary", "relative_threshold"):
        assert abs(got[k] - want[k]) < 1e-9 if math.isfinite(want[k]) else got[k] == want[k], (k, got[k], want[k])
    assert got["short_term"] == got["max_short_term"] == -math.inf                  # fewer than 30 sub-blocks
    assert got["true_peak"] == want["true_peak"] and got["sample_peak"] == want["sample_peak"] == float(np.abs(x[:, :n * 4410]).max())
    assert got["target"] == target
    if mixed:
        assert got["gain_to_target"] == pytest.approx(10.0 ** ((target - got["integrated"]) / 20.0), rel=1e-15)
    else:
        assert got["gain_to_target"] == math.inf
