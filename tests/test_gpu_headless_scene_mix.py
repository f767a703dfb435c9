"""pbso_headless --channels C --pan FILE: the tool steps the segments between the pan script's change points, mixes each one with
the scene mixer (one engine; with --devices through PBSO_GATHER_SCENE) and writes a C-channel interleaved float32 WAV.  Its
channels against the same scene, the same script and the same segments driven through the Python wrapper."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513


def _wav(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"RIFF" and raw[8:16] == b"WAVEfmt "
    fmt, ch, rate = struct.unpack("<HHI", raw[20:28])
    assert fmt == 3 and rate == 44100 and raw[36:40] == b"data"
    return ch, np.frombuffer(raw[44:], dtype=np.float32).reshape(-1, ch).T


def _python_scene_mix(d, hits, pan, nb_total, C, ramp, copies, shift):
    """the tool's calls through the wrapper: objects from the directory, hits of copy c shifted by c * shift buffers, unit
    transfer, the scene mixer stepped segment by segment"""
    eng = Engine(qnorm=capi.QNORM_OFF)
    try:
        for _ in range(copies):
            eng.add_object_from_files(str(d / "bowl_surf.modes"), str(d / "bowl_material.txt"), str(d / "bowl_ffat_maps"))
        eng.finalize()
        for c in range(copies):
            eng.set_use_transfer(c, False)
            for b, v, n in hits:
                n = np.asarray(n, dtype=np.float64)
                assert eng.enqueue_force(c, ForceMessage(vid=v, vn=n / math.sqrt(float(n @ n))), b + c * shift)
        eng.scene_mix_enable(C, math.ceil(max(x for _, _, gd in pan for x in gd[1::2])), ramp)
        gain, delay = np.zeros((C, copies), np.float32), np.zeros((C, copies), np.float32)
        cuts = sorted({0, nb_total} | {b for b, _, _ in pan if 0 < b < nb_total})
        out = np.zeros((C, nb_total * B), np.float32)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            lines = [(cp, gd) for b, cp, gd in pan if b == b0]
            for cp, gd in lines:
                gain[:, cp], delay[:, cp] = gd[0::2], gd[1::2]
            if lines:
                eng.scene_mix_set(gain, delay)
            eng.step(b1 - b0)
            eng.scene_mix()
            out[:, b0 * B:b1 * B] = eng.read_scene_mix()
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("devices", [None, "0"])
def test_headless_channels_and_pan_write_the_scene_mix(tmp_path, devices):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, ramp = 9, 2, 300
    copies = 1 if devices is None else 2
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    # <buffer> <copy> g_0 d_0 g_1 d_1: a source that moves from left to right and away, with a delay of more than one buffer
    pan = [(0, 0, (1.0, 0.0, 0.25, 30.5)), (3, 0, (0.5, 400.0, 0.75, 700.25)), (7, 0, (-0.3, 12.75, 1.0, 0.0))]
    if copies == 2:
        pan += [(0, 1, (0.2, 100.0, 0.9, 3.0)), (4, 1, (0.6, 1.5, 0.1, 520.0))]
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    (tmp_path / "pan.txt").write_text("# buffer copy g0 d0 g1 d1\n" + "".join(f"{b} {cp} " + " ".join(repr(x) for x in gd) + "\n"
                                                                             for b, cp, gd in pan))
    cmd = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--pan",
           str(tmp_path / "pan.txt"), "--ramp", str(ramp), "--out", str(tmp_path / "o.wav")]
    if devices is not None:
        cmd += ["--devices", devices, "--copies", str(copies)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    assert ch == C and wav.shape == (C, nb * B)
    want = _python_scene_mix(d, hits, [(b, cp, list(gd)) for b, cp, gd in pan], nb, C, ramp, copies, 1)
    want = (want.astype(np.float64) / 1e10).astype(np.float32)
    assert np.abs(want).max() > 0 and np.abs(want[0] - want[1]).max() > 0
    assert np.abs(wav - want).max() <= 1e-6 * np.abs(want).max(), np.abs(wav - want).max()


def test_headless_pan_needs_channels_and_a_valid_script(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    (tmp_path / "pan.txt").write_text("0 0 1.0 0.0\n")
    (tmp_path / "late.txt").write_text("0 0 1.0 0.0\n1 0 0.5 2.0\n")          # buffer 1 of a one-buffer run
    base = [EXE, "-d", str(d), "--buffers", "1", "--out", str(tmp_path / "o.wav")]
    for extra, msg in ((["--pan", str(tmp_path / "pan.txt")], "--channels"), (["--channels", "2", "--pan", str(tmp_path / "pan.txt")], "bad pan line"),
                       (["--channels", "9", "--pan", str(tmp_path / "pan.txt")], "--channels"),
                       (["--channels", "1", "--pan", str(tmp_path / "late.txt")], "outside buffers")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
