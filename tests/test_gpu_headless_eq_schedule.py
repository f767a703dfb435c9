"""pbso_headless --eq FILE --eq-schedule: the EQ script's lines scheduled up front (pbso_eq_set_at at <buffer> * frames) instead of
cutting the run at every change point.  The WAV is BYTE-IDENTICAL to the one the same command writes without the flag: plain, with
--limit behind the EQ, and with --out-rate 48000 behind it.  Both commands carry --time-chunks 1: under the engine's own launch policy
the oscillator bank's rows -- not the EQ -- may differ in their last bit between one step of six buffers and steps of 1, 2, 2 and 1,
and the EQ promises the same output for the same input only."""
import subprocess

import pytest

from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("behind", [[], ["--limit", "0.7"], ["--out-rate", "48000"]], ids=["plain", "limit", "out-rate"])
def test_eq_schedule_writes_the_same_wav(tmp_path, behind):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, R = 6, 2, 300                                  # an xfade shorter than a buffer
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (4, 1, (0.0, 1.0, 0.0))]
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    (tmp_path / "pan.txt").write_text("0 0 1.0 0.0 0.25 30.5\n")
    # (the first line at buffer 1: the schedule counts the identity as a predecessor at sample 0)
    (tmp_path / "eq.txt").write_text("# buffer section kind f0 Q gain\n1 0 highpass 30.0 0.707 0.0\n3 1 peak 1000.0 2.0 -9.0\n"
                                     "3 2 lowshelf 200.0 0.707 6.0\n5 0 highpass 80.0 1.0 0.0\n")
    wavs = []
    for flag in ([], ["--eq-schedule"]):
        out = tmp_path / ("scheduled.wav" if flag else "cut.wav")
        cmd = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--pan",
               str(tmp_path / "pan.txt"), "--eq", str(tmp_path / "eq.txt"), "--eq-xfade", str(R), "--time-chunks", "1", "--out", str(out)] + behind + flag
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        wavs.append(open(out, "rb").read())
    assert len(wavs[0]) > 44 + 2 * C * nb * 513 and any(wavs[0][44:])
    assert wavs[0] == wavs[1]
