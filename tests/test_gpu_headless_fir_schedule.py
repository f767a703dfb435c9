"""pbso_headless --fir-schedule: the --fir and --fir-delay lines scheduled up front (pbso_scene_fir_set_at / _set_delay_at at
<buffer> * frames; with --devices the group's calls) instead of cutting the run at every change point.  The WAV is BYTE-IDENTICAL
to the one the same command writes without the flag, for a single engine and through a device group.  Both commands carry
--time-chunks 1: under the engine's own launch policy the oscillator bank's rows -- not the mix -- differ in their last bit between
one step of nine buffers and the cut steps, and the mixer promises the same output for the same rows only."""
import subprocess

import numpy as np
import pytest

from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("devices", [None, "0"])
def test_fir_schedule_writes_the_same_wav(tmp_path, devices):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, K, xfade, ramp = 9, 2, 40, 300, 700
    copies = 1 if devices is None else 2
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    rng = np.random.default_rng(13)
    for name in ("near.f32", "far.f32"):
        (rng.standard_normal((C, K)) * np.exp(-np.arange(K) / 9.0)).astype("<f4").tofile(tmp_path / name)
    script = [(0, 0, 30, "near.f32"), (3, 0, 700, "far.f32"), (7, 0, 5, "near.f32")]
    # <buffer> <copy> <delay>: at a filter change point, between two of them, one buffer into a ramp of 700
    dscript = [(0, 0, 120.25), (3, 0, 640.5), (5, 0, 12.0), (6, 0, 333.125)]
    if copies == 2:
        script += [(0, 1, 100, "far.f32"), (7, 1, 0, "near.f32")]
        dscript += [(0, 1, 0.0), (5, 1, 512.75)]
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    (tmp_path / "fir.txt").write_text("".join(f"{b} {cp} {on} {tmp_path / name}\n" for b, cp, on, name in script))
    (tmp_path / "delay.txt").write_text("# buffer copy delay\n" + "".join(f"{b} {cp} {dl!r}\n" for b, cp, dl in dscript))
    wavs = []
    for flag in ([], ["--fir-schedule"]):
        out = tmp_path / ("scheduled.wav" if flag else "cut.wav")
        cmd = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--fir",
               str(tmp_path / "fir.txt"), "--xfade", str(xfade), "--fir-delay", str(tmp_path / "delay.txt"), "--delay-ramp", str(ramp),
               "--time-chunks", "1", "--out", str(out)] + flag
        if devices is not None:
            cmd += ["--devices", devices, "--copies", str(copies)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        wavs.append(open(out, "rb").read())
    assert len(wavs[0]) == 44 + 4 * C * nb * 513 and any(wavs[0][44:])
    assert wavs[0] == wavs[1]


def test_fir_schedule_needs_a_fir_script(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    r = subprocess.run([EXE, "-d", str(d), "--buffers", "1", "--out", str(tmp_path / "o.wav"), "--fir-schedule"], capture_output=True, text=True)
    assert r.returncode != 0 and "--fir-schedule needs --fir" in r.stderr, r.stderr
