"""pbso_headless --retune FILE: lines <buffer> <copy> <material file> [keep|zero]; the tool cuts the run at these buffers and gives the
copy its new material with pbso_set_material (with --devices: pbso_group_set_material).  Against the same run assembled in Python
with Engine.set_material, segment by segment, bit for bit: mono (keep and zero), through --channels 2 --pan, and through the
device group with two copies."""
import math
import subprocess

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513
HITS = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (4, 1, (0.0, 1.0, 0.0))]
GLASS = (2200.0, 1.5, 4e-8)              # rho, alpha, beta of glass.txt


def _setup(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    (tmp_path / "glass.txt").write_text("# rho E nu alpha beta\n2200 6.2e10 0.2 1.5 4e-8\n")
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in HITS))
    return d


def _python_run(d, nb, retunes, copies=1, shift=1, pan=None, C=0, ramp=0):
    """retunes: (buffer, copy, material, keep).  Returns the mono object mix [nb * B] (the tool's --raw; copies summed in f64 is NOT
    what the tool does, so copies > 1 is only used with pan), or with pan the scene mix [C][nb * B]."""
    eng = Engine(qnorm=capi.QNORM_OFF)
    try:
        for _ in range(copies):
            eng.add_object_from_files(str(d / "bowl_surf.modes"), str(d / "bowl_material.txt"), str(d / "bowl_ffat_maps"))
        eng.finalize()
        for c in range(copies):
            eng.set_use_transfer(c, False)
            for b, v, n in HITS:
                n = np.asarray(n, dtype=np.float64)
                assert eng.enqueue_force(c, ForceMessage(vid=v, vn=n / math.sqrt(float(n @ n))), b + c * shift)
        if pan:
            eng.scene_mix_enable(C, math.ceil(max(x for _, _, gd in pan for x in gd[1::2])), ramp)
            gain, delay = np.zeros((C, copies), np.float32), np.zeros((C, copies), np.float32)
        cuts = sorted({0, nb} | {b for b, *_ in retunes if 0 < b < nb} | {b for b, *_ in (pan or []) if 0 < b < nb})
        out = np.zeros((C or 1, nb * B), np.float32)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            for keep in (True, False):
                now = [(cp, m) for b, cp, m, k in retunes if b == b0 and k == keep]
                if now:
                    eng.set_material([cp for cp, _ in now], [m[0] for _, m in now], [m[1] for _, m in now], [m[2] for _, m in now],
                                     keep_state=keep)
            if pan:
                lines = [(cp, gd) for b, cp, gd in pan if b == b0]
                for cp, gd in lines:
                    gain[:, cp], delay[:, cp] = gd[0::2], gd[1::2]
                if lines:
                    eng.scene_mix_set(gain, delay)
            eng.step(b1 - b0)
            if pan:
                eng.scene_mix()
                out[:, b0 * B:b1 * B] = eng.read_scene_mix()
            else:
                out[0, b0 * B:b1 * B] = eng.audio()[0]
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("word", ["keep", "zero", ""])
def test_headless_retune_equals_the_run_assembled_with_set_material(tmp_path, word):
    d = _setup(tmp_path)
    nb = 6
    (tmp_path / "retune.txt").write_text(f"# buffer copy material [keep|zero]\n3 0 {tmp_path / 'glass.txt'} {word}\n")
    r = subprocess.run([EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--retune", str(tmp_path / "retune.txt"),
                        "--out", str(tmp_path / "o.wav"), "--raw", str(tmp_path / "o.raw")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(tmp_path / "o.raw", dtype=np.float32)
    want = _python_run(d, nb, [(3, 0, GLASS, word != "zero")])[0]
    plain = _python_run(d, nb, [])[0]
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(want[:3 * B], plain[:3 * B]) and not np.array_equal(want[3 * B:], plain[3 * B:])
    other = _python_run(d, nb, [(3, 0, GLASS, word == "zero")])[0]
    assert not np.array_equal(want, other)                  # keep and zero are different runs


def test_headless_retune_through_channels_and_pan(tmp_path):
    d = _setup(tmp_path)
    nb, C, ramp = 7, 2, 300
    pan = [(0, 0, (1.0, 0.0, 0.25, 30.5)), (2, 0, (0.5, 400.0, 0.75, 700.25)), (5, 0, (-0.3, 12.75, 1.0, 0.0))]
    (tmp_path / "pan.txt").write_text("".join(f"{b} {cp} " + " ".join(repr(x) for x in gd) + "\n" for b, cp, gd in pan))
    # the glass at buffer 3 (a cut of its own), the first material again at buffer 5 (a cut it shares with the pan script)
    (tmp_path / "retune.txt").write_text(f"3 0 {tmp_path / 'glass.txt'} keep\n5 0 {d / 'bowl_material.txt'} zero\n")
    r = subprocess.run([EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--pan",
                        str(tmp_path / "pan.txt"), "--ramp", str(ramp), "--retune", str(tmp_path / "retune.txt"), "--out", str(tmp_path / "o.wav")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    retunes = [(3, 0, GLASS, True), (5, 0, (2500.0, 6.0, 1e-7), False)]
    want = _python_run(d, nb, retunes, pan=[(b, cp, list(gd)) for b, cp, gd in pan], C=C, ramp=ramp)
    want = (want.astype(np.float64) / 1e10).astype(np.float32)
    assert ch == C and wav.shape == want.shape and np.array_equal(wav, want)
    plain = _python_run(d, nb, [], pan=[(b, cp, list(gd)) for b, cp, gd in pan], C=C, ramp=ramp)
    assert not np.array_equal(want, (plain.astype(np.float64) / 1e10).astype(np.float32))


def test_headless_retune_through_the_device_group(tmp_path):
    """--devices 0 --copies 2 --channels 2 --pan: the second copy alone gets the glass, through pbso_group_set_material"""
    d = _setup(tmp_path)
    nb, C, ramp = 6, 2, 200
    pan = [(0, 0, (1.0, 0.0, 0.25, 3.5)), (0, 1, (0.2, 10.0, 0.9, 3.0))]
    (tmp_path / "pan.txt").write_text("".join(f"{b} {cp} " + " ".join(repr(x) for x in gd) + "\n" for b, cp, gd in pan))
    (tmp_path / "retune.txt").write_text(f"3 1 {tmp_path / 'glass.txt'}\n")
    r = subprocess.run([EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--pan",
                        str(tmp_path / "pan.txt"), "--ramp", str(ramp), "--retune", str(tmp_path / "retune.txt"), "--devices", "0", "--copies", "2",
                        "--out", str(tmp_path / "o.wav")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    want = _python_run(d, nb, [(3, 1, GLASS, True)], copies=2, pan=[(b, cp, list(gd)) for b, cp, gd in pan], C=C, ramp=ramp)
    want = (want.astype(np.float64) / 1e10).astype(np.float32)
    assert ch == C and wav.shape == want.shape and np.array_equal(wav, want)
