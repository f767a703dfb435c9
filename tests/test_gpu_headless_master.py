"""pbso_headless --limit T [--lookahead L] [--gain G] [--pcm16]: the master bus behind what the tool would have written.  The
limited WAV against the float WAV of the same run without --limit (stepped as far as the limited run steps) sent through the
model, bit for bit; the 16-bit file; the refusal of a device group."""
import struct
import subprocess

import numpy as np
import pytest

from tests.master_model import Model, pcm16
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def test_headless_limit_is_the_unlimited_run_through_the_model(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, ramp, L, T = 7, 2, 300, 64, 0.7
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    pan = [(0, (1.0, 0.0, 0.25, 30.5)), (3, (0.5, 400.0, 0.75, 700.25))]
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    line = lambda b, gd: f"{b} 0 " + " ".join(repr(x) for x in gd) + "\n"
    (tmp_path / "pan.txt").write_text("".join(line(b, gd) for b, gd in pan))
    # the limited run steps one more buffer behind a cut at nb: the same segments for the unlimited run of nb + 1 buffers (a set
    # to the values in force, long after their ramp, changes nothing)
    (tmp_path / "pan_cut.txt").write_text("".join(line(b, gd) for b, gd in pan + [(nb, pan[-1][1])]))
    base = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--channels", str(C), "--ramp", str(ramp)]
    _run(base + ["--pan", str(tmp_path / "pan.txt"), "--buffers", str(nb), "--out", str(tmp_path / "plain.wav")])
    _run(base + ["--pan", str(tmp_path / "pan_cut.txt"), "--buffers", str(nb + 1), "--out", str(tmp_path / "long.wav")])
    ch, plain = _wav(tmp_path / "plain.wav")
    _, x = _wav(tmp_path / "long.wav")
    assert ch == C and plain.shape == (C, nb * B) and x.shape == (C, (nb + 1) * B)
    assert np.array_equal(plain, x[:, :nb * B])
    peak = float(np.abs(x).max())
    assert peak > 0
    G = float(np.float32(3 * T / peak))                              # the loudest sample lands at 3 T
    lim = ["--pan", str(tmp_path / "pan.txt"), "--buffers", str(nb), "--limit", repr(T), "--lookahead", str(L), "--gain", repr(G)]
    _run(base + lim + ["--out", str(tmp_path / "lim.wav")])
    ch, got = _wav(tmp_path / "lim.wav")
    assert ch == C and got.shape == plain.shape                      # the length of the run without --limit
    m = Model(C, T, L, 0, 0)
    m.set_gain(G)
    y = m.process(np.ascontiguousarray(x))
    want = np.ascontiguousarray(y[:, L:L + nb * B])
    assert (m.gains < 1).any() and np.abs(want).max() <= np.float32(T)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    # --pcm16: a format-1 file of 16 bits and C channels with lrintf(y * 32767.f)
    _run(base + lim + ["--pcm16", "--out", str(tmp_path / "lim16.wav")])
    raw = open(tmp_path / "lim16.wav", "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and raw[36:40] == b"data"
    fmt, chans, rate, _, align, bits = struct.unpack("<HHIIHH", raw[20:36])
    assert (fmt, chans, rate, align, bits) == (1, C, 44100, 2 * C, 16)
    assert struct.unpack("<I", raw[40:44])[0] == nb * B * C * 2 == len(raw) - 44
    assert np.array_equal(np.frombuffer(raw[44:], dtype="<i2").reshape(-1, C), pcm16(want))


def test_headless_limit_on_the_mono_mix_and_with_a_device_group(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, L, T = 3, 600, 0.5
    (tmp_path / "hits.txt").write_text("0 3 0.2 -0.5 1.0 point\n1 7 1.0 0.0 0.3 point\n")
    base = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--out", str(tmp_path / "o.wav")]
    r = subprocess.run(base + ["--buffers", str(nb), "--limit", "0.7", "--devices", "0"], capture_output=True, text=True)
    assert r.returncode != 0 and "device group" in r.stderr, r.stderr
    _run(base + ["--buffers", str(nb + 2)])                          # ceil(600 / 513) = 2 more buffers, one step
    _, x = _wav(tmp_path / "o.wav")
    G = float(np.float32(4 * T / float(np.abs(x).max())))
    _run(base + ["--buffers", str(nb), "--limit", repr(T), "--lookahead", str(L), "--hold", "100", "--gain", repr(G)])
    ch, got = _wav(tmp_path / "o.wav")
    assert ch == 1 and got.shape == (1, nb * B)
    m = Model(1, T, L, 100, 0)
    m.set_gain(G)
    want = np.ascontiguousarray(m.process(np.ascontiguousarray(x))[:, L:L + nb * B])
    assert (m.gains < 1).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
