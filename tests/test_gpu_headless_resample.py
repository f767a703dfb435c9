"""pbso_headless --out-rate R [--rs-taps T]: the resampler bus behind what the tool would have written.  The 48 kHz WAV against the
float WAV of the same run without --limit and --out-rate (stepped as far as the resampled run steps) sent through the models of
the master bus and the resampler, bit for bit, with the engine's own taps (resample_taps() of an engine enabled alike); the
header's rate and frame count; the 16-bit file."""
import struct
import subprocess

import numpy as np
import pytest
import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

from openpbso_amd import Engine, synth
from tests import resample_model as rm
from tests.master_model import Model as MasterModel
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def _wav_at(path, rate_want):
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and raw[36:40] == b"data"
    fmt, ch, rate, byte_rate, align, bits = struct.unpack("<HHIIHH", raw[20:36])
    assert (fmt, rate, bits, align, byte_rate) == (3, rate_want, 32, 4 * ch, 4 * ch * rate_want)
    assert struct.unpack("<I", raw[40:44])[0] == len(raw) - 44
    return ch, np.frombuffer(raw[44:], dtype=np.float32).reshape(-1, ch).T


def _taps(C, rate_out, T):
    eng = Engine()
    try:
        eng.add_object(synth.eigenvalues(64, 9000), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        eng.resample_enable(rate_out, C, T)
        return eng.resample_taps()
    finally:
        eng.close()


def test_headless_out_rate_is_the_plain_run_through_the_models(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, ramp, LA, ceiling, R, T = 7, 2, 300, 64, 0.7, 48000, 32
    L, M = rm.ratio(44100, R)
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    pan = [(0, (1.0, 0.0, 0.25, 30.5)), (3, (0.5, 400.0, 0.75, 700.25))]
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    line = lambda b, gd: f"{b} 0 " + " ".join(repr(x) for x in gd) + "\n"
    (tmp_path / "pan.txt").write_text("".join(line(b, gd) for b, gd in pan))
    # d = 64 + 5119 / 320 = 80 input samples: one more buffer behind a cut at nb; the same segments for the plain run of nb + 1
    # buffers (a set to the values in force, long after their ramp, changes nothing)
    drop = (2 * L * LA + L * T - 1 + M) // (2 * M)
    keep = rm.ceil_div(nb * B * L, M)
    assert (drop, keep) == (87, 3909) and rm.ceil_div((nb + 1) * B * L, M) >= drop + keep
    (tmp_path / "pan_cut.txt").write_text("".join(line(b, gd) for b, gd in pan + [(nb, pan[-1][1])]))
    base = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--channels", str(C), "--ramp", str(ramp)]
    _run(base + ["--pan", str(tmp_path / "pan_cut.txt"), "--buffers", str(nb + 1), "--out", str(tmp_path / "long.wav")])
    ch, x = _wav(tmp_path / "long.wav")
    assert ch == C and x.shape == (C, (nb + 1) * B)
    peak = float(np.abs(x).max())
    assert peak > 0
    G = float(np.float32(3 * ceiling / peak))                        # the loudest sample lands at 3 T
    flags = ["--pan", str(tmp_path / "pan.txt"), "--buffers", str(nb), "--limit", repr(ceiling), "--lookahead", str(LA), "--gain", repr(G),
             "--out-rate", str(R), "--rs-taps", str(T)]
    _run(base + flags + ["--out", str(tmp_path / "rs.wav")])
    ch, got = _wav_at(tmp_path / "rs.wav", R)
    assert ch == C and got.shape == (C, keep)                        # ceil(buffers * 513 * L / M) frames at R Hz
    m = MasterModel(C, ceiling, LA, 0, 0)
    m.set_gain(G)
    v = m.process(np.ascontiguousarray(x))
    assert (m.gains < 1).any()
    y = rm.Model(C, L, M, _taps(C, R, T)).process(v)
    want = np.ascontiguousarray(y[:, drop:drop + keep])
    assert np.abs(want).max() > 0.5 * ceiling
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    # --pcm16: a format-1 file of 16 bits and C channels at R Hz with the resampler's saturating conversion
    _run(base + flags + ["--pcm16", "--out", str(tmp_path / "rs16.wav")])
    raw = open(tmp_path / "rs16.wav", "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt " and raw[36:40] == b"data"
    fmt, chans, rate, _, align, bits = struct.unpack("<HHIIHH", raw[20:36])
    assert (fmt, chans, rate, align, bits) == (1, C, R, 2 * C, 16)
    assert struct.unpack("<I", raw[40:44])[0] == keep * C * 2 == len(raw) - 44
    assert np.array_equal(np.frombuffer(raw[44:], dtype="<i2").reshape(-1, C), rm.pcm16(want))


def test_headless_out_rate_on_the_mono_mix_without_a_limiter(tmp_path):
    """22050 Hz (1 / 2) from the mono object mix, T = 7: d = 6 / 2 = 3 input samples, floor(1.5 + 0.5) = 2 frames dropped"""
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, R, T = 3, 22050, 7
    (tmp_path / "hits.txt").write_text("0 3 0.2 -0.5 1.0 point\n1 7 1.0 0.0 0.3 point\n")
    base = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--out", str(tmp_path / "o.wav")]
    _run(base + ["--buffers", str(nb + 1)])                          # one more buffer, one step
    _, x = _wav(tmp_path / "o.wav")
    _run(base + ["--buffers", str(nb), "--out-rate", str(R), "--rs-taps", str(T)])
    ch, got = _wav_at(tmp_path / "o.wav", R)
    keep = rm.ceil_div(nb * B, 2)
    assert ch == 1 and got.shape == (1, keep)
    y = rm.Model(1, 1, 2, _taps(1, R, T)).process(np.ascontiguousarray(x))
    want = np.ascontiguousarray(y[:, 2:2 + keep])
    assert np.abs(want).max() > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
