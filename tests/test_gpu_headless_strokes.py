"""pbso_headless --strokes FILE: sustained contact from a file -- the dummy start message, a face entry per line, the stop
message -- fed one step ahead through pbso_enqueue_strokes.  The WAV samples equal, bit for bit, the same script fed through
Engine.enqueue_strokes in Python: mono (one step), and with --channels 2 --pan (the segments between the pan script's change
points, each fed its own entries)."""
import subprocess

import numpy as np
import pytest

from openpbso_amd import Engine, capi
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513
N_VERTS = 12


def _script(nb):
    """(buffer, flags, vids, coords, vn): dummy start at 1, a face entry per buffer with a gap and a burst, the stop message"""
    rng = np.random.default_rng(21)
    out = [(1, capi.STROKE_START | capi.STROKE_ZERO, (0, 0, 0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))]
    for b in [2, 3, 4, 4, 4, 8, 9, 10, 11]:
        bary = rng.random(3)
        bary /= bary.sum()
        vn = rng.standard_normal(3)
        out.append((b, 0, tuple(int(v) for v in rng.integers(0, N_VERTS, 3)), tuple(bary), tuple(vn / np.linalg.norm(vn))))
    out.append((nb - 3, capi.STROKE_END | capi.STROKE_ZERO, (0, 0, 0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
    return out


def _write(path, script):
    lines = ["# buffer v0 v1 v2 c0 c1 c2 nx ny nz [start|end]"]
    for b, fl, v, c, n in script:
        tail = " start" if fl & capi.STROKE_START else (" end" if fl & capi.STROKE_END else "")
        if fl & capi.STROKE_ZERO:
            lines.append(f"{b} -{tail}")
        else:
            lines.append(f"{b} {v[0]} {v[1]} {v[2]} " + " ".join(repr(float(x)) for x in c + n) + tail)
    path.write_text("\n".join(lines) + "\n")


def _feed(eng, script, b0, b1):
    part = [e for e in script if b0 <= e[0] < b1]
    if part:
        eng.enqueue_strokes([0] * len(part), [e[2] for e in part], [e[3] for e in part], [e[4] for e in part], [e[0] for e in part],
                            np.array([e[1] for e in part], dtype=np.uint8))


def _engine(d, arprm):
    eng = Engine(qnorm=capi.QNORM_OFF)
    eng.add_object_from_files(str(d / "bowl_surf.modes"), str(d / "bowl_material.txt"), str(d / "bowl_ffat_maps"))
    eng.finalize()
    eng.set_use_transfer(0, False)
    if arprm is not None:
        eng.enqueue_arprm(0, arprm[:2], arprm[2], arprm[3], 0)
    return eng


@pytest.mark.parametrize("arprm", [None, (0.6, 0.2, 0.003, 0.1)])
def test_headless_strokes_mono_equals_the_python_feed(tmp_path, arprm):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb = 16
    script = _script(nb)
    _write(tmp_path / "strokes.txt", script)
    cmd = [EXE, "-d", str(d), "--strokes", str(tmp_path / "strokes.txt"), "--buffers", str(nb), "--out", str(tmp_path / "o.wav")]
    if arprm is not None:
        cmd += ["--arprm", " ".join(repr(x) for x in arprm)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    assert ch == 1 and wav.shape == (1, nb * B)
    eng = _engine(d, arprm)
    try:
        _feed(eng, script, 0, nb)
        eng.step(nb)
        want = (eng.audio()[0].astype(np.float64) / 1e10).astype(np.float32)
        assert eng.stroke_stats()["direct"] == len(script)
    finally:
        eng.close()
    assert np.abs(want).max() > 0 and np.array_equal(wav[0], want)


def test_headless_strokes_with_channels_and_pan_equal_the_python_feed(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, ramp = 16, 2, 200
    script = _script(nb)
    _write(tmp_path / "strokes.txt", script)
    pan = [(0, (1.0, 0.0, 0.25, 30.5)), (6, (0.5, 100.0, 0.75, 40.25)), (11, (-0.3, 12.75, 1.0, 0.0))]
    (tmp_path / "pan.txt").write_text("".join(f"{b} 0 " + " ".join(repr(x) for x in gd) + "\n" for b, gd in pan))
    r = subprocess.run([EXE, "-d", str(d), "--strokes", str(tmp_path / "strokes.txt"), "--buffers", str(nb), "--channels", str(C), "--pan",
                        str(tmp_path / "pan.txt"), "--ramp", str(ramp), "--out", str(tmp_path / "o.wav")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    assert ch == C and wav.shape == (C, nb * B)
    eng = _engine(d, None)
    try:
        eng.scene_mix_enable(C, int(np.ceil(max(x for _, gd in pan for x in gd[1::2]))), ramp)
        cuts = sorted({0, nb} | {b for b, _ in pan if 0 < b < nb})
        out = np.zeros((C, nb * B), np.float32)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            for b, gd in pan:
                if b == b0:
                    eng.scene_mix_set(np.array(gd[0::2], np.float32).reshape(C, 1), np.array(gd[1::2], np.float32).reshape(C, 1))
            _feed(eng, script, b0, b1)
            eng.step(b1 - b0)
            eng.scene_mix()
            out[:, b0 * B:b1 * B] = eng.read_scene_mix()
    finally:
        eng.close()
    want = (out.astype(np.float64) / 1e10).astype(np.float32)
    assert np.abs(want).max() > 0 and np.abs(want[0] - want[1]).max() > 0
    assert np.array_equal(wav, want)


def test_headless_strokes_bad_lines_are_reported(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    for text, msg in (("0 1 2\n", "bad stroke line"), ("0 - stop\n", "start or end"), (f"0 0 1 {N_VERTS} 0.3 0.3 0.4 0 0 1\n", "vertex id out of range")):
        (tmp_path / "s.txt").write_text(text)
        r = subprocess.run([EXE, "-d", str(d), "--strokes", str(tmp_path / "s.txt"), "--buffers", "2", "--out", str(tmp_path / "o.wav")],
                           capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (text, r.stderr)
