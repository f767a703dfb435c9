"""pbso_headless --pan-schedule: the pan script's lines scheduled up front (pbso_scene_mix_set_at at <buffer> * frames; with --devices
pbso_group_scene_mix_set_at) instead of cutting the run at every change point.  The WAV is BYTE-IDENTICAL to the one the same
command writes without the flag, for a single engine and through a device group.  Both commands carry --time-chunks 1: under the
engine's own launch policy the oscillator bank's rows -- not the mix -- differ in their last bit between one step of nine buffers
and steps of 3, 1, 3 and 2, and the mixer promises the same output for the same rows only."""
import subprocess

import pytest

from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("devices", [None, "0"])
def test_pan_schedule_writes_the_same_wav(tmp_path, devices):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, ramp = 9, 2, 300
    copies = 1 if devices is None else 2
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    # <buffer> <copy> g_0 d_0 g_1 d_1: the set at buffer 4 lands during the ramp of the one at buffer 3
    pan = [(0, 0, (1.0, 0.0, 0.25, 30.5)), (3, 0, (0.5, 400.0, 0.75, 700.25)), (4, 0, (0.9, 3.5, 0.1, 650.0)), (7, 0, (-0.3, 12.75, 1.0, 0.0))]
    if copies == 2:
        pan += [(0, 1, (0.2, 100.0, 0.9, 3.0)), (4, 1, (0.6, 1.5, 0.1, 520.0)), (8, 1, (0.3, 0.0, 0.3, 0.0))]
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    (tmp_path / "pan.txt").write_text("# buffer copy g0 d0 g1 d1\n" + "".join(f"{b} {cp} " + " ".join(repr(x) for x in gd) + "\n"
                                                                             for b, cp, gd in pan))
    wavs = []
    for flag in ([], ["--pan-schedule"]):
        out = tmp_path / ("scheduled.wav" if flag else "cut.wav")
        cmd = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--pan",
               str(tmp_path / "pan.txt"), "--ramp", str(ramp), "--time-chunks", "1", "--out", str(out)] + flag
        if devices is not None:
            cmd += ["--devices", devices, "--copies", str(copies)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        wavs.append(open(out, "rb").read())
    assert len(wavs[0]) == 44 + 4 * C * nb * 513 and any(wavs[0][44:])
    assert wavs[0] == wavs[1]


def test_pan_schedule_needs_a_pan_script(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    r = subprocess.run([EXE, "-d", str(d), "--buffers", "1", "--out", str(tmp_path / "o.wav"), "--pan-schedule"], capture_output=True, text=True)
    assert r.returncode != 0 and "--pan-schedule needs --pan" in r.stderr, r.stderr
