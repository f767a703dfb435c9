"""pbso_headless --track-hits FILE: hits whose force is a signal read from a file (raw float32 or a mono IEEE-float WAV), fed
through pbso_track_create / pbso_enqueue_track_force.  The WAV samples equal, sample for sample, the same scene fed through
Engine.create_track / Engine.enqueue_track_force in Python: mono beside a --hits script, and with --devices 0 --copies 3
--channels 2 --pan (the copies hear the script shifted, the segments between the pan script's change points mixed one by one)."""
import math
import struct
import subprocess

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513
N_VERTS = 12


def _write_wav(path, samples):
    data = np.asarray(samples, dtype="<f4").tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 3, 1, 44100, 44100 * 4, 4, 32)
    path.write_bytes(hdr + b"data" + struct.pack("<I", len(data)) + data)


def _tracks(tmp_path):
    rng = np.random.default_rng(31)
    a = rng.standard_normal(700).astype(np.float32)
    b = (0.5 * rng.standard_normal(1900)).astype(np.float32)
    a.astype("<f4").tofile(tmp_path / "mallet.f32")
    _write_wav(tmp_path / "bow.wav", b)
    return {"mallet.f32": a, "bow.wav": b}


# (buffer, start_sample, vertex, normal, file, gain, rate, first, n_samples, loop)
TRACK_HITS = [
    (1, 17, 3, (0.2, -0.5, 1.0), "mallet.f32", 1.0, 1.0, 0.0, 0, 0),
    (2, 0, 7, (1.0, 0.0, 0.3), "bow.wav", -0.75, 0.37, 2.5, 0, 0),
    (6, 512, 1, (0.0, 1.0, 0.0), "mallet.f32", 2.0, 2.5, 10.25, 1300, 1),
    (9, 256, 5, (0.3, 0.3, -1.0), "bow.wav", 0.5, 1.0, 100.0, 0, 0),
]
HITS = [(0, 4, (0.0, 0.0, 1.0)), (6, 9, (1.0, 1.0, 0.0)), (12, 2, (0.0, -1.0, 0.2))]


def _write_scripts(tmp_path):
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in HITS))
    lines = ["# buffer start_sample vertex nx ny nz file [gain [rate [first [n_samples [loop]]]]]"]
    for b, s, v, n, f, gain, rate, first, ns, loop in TRACK_HITS:
        lines.append(f"{b} {s} {v} {n[0]} {n[1]} {n[2]} {tmp_path / f} {gain!r} {rate!r} {first!r} {ns} {loop}")
    lines.append(f"11 5 6 0.0 0.0 1.0 {tmp_path / 'mallet.f32'}")                      # the defaults: gain 1, rate 1, first 0, to the track's end
    (tmp_path / "track_hits.txt").write_text("\n".join(lines) + "\n")


def _unit(n):
    n = np.asarray(n, dtype=np.float64)
    return n / math.sqrt(float(n @ n))


def _feed(eng, obj, ids, shift):
    """one copy's messages in the tool's order: by buffer, the --hits line first at equal buffers"""
    msgs = [(b, 0, ("hit", v, n)) for b, v, n in HITS]
    msgs += [(t[0], 1, ("track",) + t[1:]) for t in TRACK_HITS] + [(11, 1, ("track", 5, 6, (0.0, 0.0, 1.0), "mallet.f32", 1.0, 1.0, 0.0, 0, 0))]
    for b, _, m in sorted(msgs, key=lambda x: (x[0], x[1])):
        if m[0] == "hit":
            assert eng.enqueue_force(obj, ForceMessage(vid=m[1], vn=_unit(m[2])), b + shift)
        else:
            _, s, v, n, f, gain, rate, first, ns, loop = m
            assert eng.enqueue_track_force(obj, ForceMessage(vid=v, vn=_unit(n)), ids[f], first=first, rate=rate, gain=gain, n_samples=ns,
                                           start_sample=s, loop=bool(loop), not_before=b + shift)


def _engine(d, copies):
    eng = Engine(qnorm=capi.QNORM_OFF)
    for _ in range(copies):
        eng.add_object_from_files(str(d / "bowl_surf.modes"), str(d / "bowl_material.txt"), str(d / "bowl_ffat_maps"))
    eng.finalize()
    for c in range(copies):
        eng.set_use_transfer(c, False)
    return eng


def test_headless_track_hits_mono_equal_the_python_feed(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb = 16
    tracks = _tracks(tmp_path)
    _write_scripts(tmp_path)
    r = subprocess.run([EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--track-hits", str(tmp_path / "track_hits.txt"),
                        "--buffers", str(nb), "--out", str(tmp_path / "o.wav")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    assert ch == 1 and wav.shape == (1, nb * B)
    eng = _engine(d, 1)
    try:
        ids = {f: eng.create_track(s) for f, s in tracks.items()}
        _feed(eng, 0, ids, 0)
        eng.step(nb)
        want = (eng.audio()[0].astype(np.float64) / 1e10).astype(np.float32)
        stats = eng.track_stats()
    finally:
        eng.close()
    assert stats[0] == 2 and stats[2] == len(TRACK_HITS) + 1, stats          # every distinct file once, every line a message
    assert np.abs(want).max() > 0 and np.array_equal(wav[0], want)


def test_headless_track_hits_with_copies_channels_and_pan_equal_the_python_feed(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, ramp, copies, shift = 16, 2, 200, 3, 1
    tracks = _tracks(tmp_path)
    _write_scripts(tmp_path)
    pan = [(0, 0, (1.0, 0.0, 0.25, 30.5)), (0, 1, (0.2, 100.0, 0.9, 3.0)), (0, 2, (0.6, 1.5, 0.1, 52.0)), (6, 0, (0.5, 100.0, 0.75, 40.25)),
           (11, 2, (-0.3, 12.75, 1.0, 0.0))]
    (tmp_path / "pan.txt").write_text("".join(f"{b} {cp} " + " ".join(repr(x) for x in gd) + "\n" for b, cp, gd in pan))
    r = subprocess.run([EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--track-hits", str(tmp_path / "track_hits.txt"),
                        "--buffers", str(nb), "--devices", "0", "--copies", str(copies), "--channels", str(C), "--pan", str(tmp_path / "pan.txt"),
                        "--ramp", str(ramp), "--out", str(tmp_path / "o.wav")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    assert ch == C and wav.shape == (C, nb * B)
    eng = _engine(d, copies)
    try:
        ids = {f: eng.create_track(s) for f, s in tracks.items()}
        for c in range(copies):
            _feed(eng, c, ids, c * shift)
        eng.scene_mix_enable(C, math.ceil(max(x for _, _, gd in pan for x in gd[1::2])), ramp)
        gain, delay = np.zeros((C, copies), np.float32), np.zeros((C, copies), np.float32)
        cuts = sorted({0, nb} | {b for b, _, _ in pan if 0 < b < nb})
        out = np.zeros((C, nb * B), np.float32)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            lines = [(cp, gd) for b, cp, gd in pan if b == b0]
            for cp, gd in lines:
                gain[:, cp], delay[:, cp] = gd[0::2], gd[1::2]
            if lines:
                eng.scene_mix_set(gain, delay)
            eng.step(b1 - b0)
            eng.scene_mix()
            out[:, b0 * B:b1 * B] = eng.read_scene_mix()
    finally:
        eng.close()
    want = (out.astype(np.float64) / 1e10).astype(np.float32)
    assert np.abs(want).max() > 0 and np.abs(want[0] - want[1]).max() > 0
    assert np.array_equal(wav, want)


def test_headless_track_hits_bad_lines_are_reported(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    _tracks(tmp_path)
    (tmp_path / "stereo.wav").write_bytes((tmp_path / "bow.wav").read_bytes()[:22] + struct.pack("<H", 2) + (tmp_path / "bow.wav").read_bytes()[24:])
    (tmp_path / "odd.f32").write_bytes(b"\0" * 7)
    ok = str(tmp_path / "mallet.f32")
    for text, msg in ((f"0 0 3\n", "bad track-hit line"), (f"0 0 3 0 0 1\n", "track file"), (f"0 0 3 0 0 1 {tmp_path / 'none.f32'}\n", "cannot read track"),
                      (f"0 0 3 0 0 1 {tmp_path / 'stereo.wav'}\n", "mono IEEE float32"), (f"0 0 3 0 0 1 {tmp_path / 'odd.f32'}\n", "whole float32"),
                      (f"0 513 3 0 0 1 {ok}\n", "start_sample"), (f"0 0 3 0 0 1 {ok} 1.0 0.0\n", "rate"), (f"0 0 3 - {ok}\n", None)):
        (tmp_path / "t.txt").write_text(text)
        r = subprocess.run([EXE, "-d", str(d), "--track-hits", str(tmp_path / "t.txt"), "--buffers", "2", "--out", str(tmp_path / "o.wav")],
                           capture_output=True, text=True)
        if msg is None:
            assert r.returncode == 0, r.stderr                                   # `-`: the mesh's vertex normal
        else:
            assert r.returncode != 0 and msg in r.stderr, (text, r.stderr)
