"""pbso_headless --eq FILE [--eq-xfade N]: the EQ bus behind the mixer, in front of --limit.  The WAV against the float WAV of the
same run without --eq (cut at the same buffers) sent through the model of tests/eq_model.py, byte for byte; and with --limit behind
it, through the master bus's model as well."""
import subprocess

import numpy as np
import pytest
import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

from openpbso_amd import capi
from tests import eq_model as em
from tests.master_model import Model as MasterModel
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def _equalised(x, C, S, R, script, cuts):
    """x [C][n] through the model, stepped at `cuts` (buffers); script {buffer: [(section, kind, f0, Q, gain)]}, every channel alike"""
    model = em.Model(C, S, R)
    sos = em.identity(C, S)
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if lo in script:
            for section, kind, f0, q, gain in script[lo]:
                sos[:, section] = capi.eq_design(kind, 44100.0, f0, q, gain)
            model.set(sos)
        out.append(model.process(x[:, lo * B:hi * B]))
    return np.concatenate(out, axis=1)


def test_headless_eq_is_the_plain_run_through_the_model_and_sits_in_front_of_the_limiter(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, ramp, R, LA, ceiling = 7, 2, 300, 200, 64, 0.7
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    pan = [(0, (1.0, 0.0, 0.25, 30.5)), (3, (0.5, 400.0, 0.75, 700.25))]
    script = {0: [(0, "highpass", 30.0, 0.707, 0.0)], 2: [(1, "peak", 1000.0, 2.0, -9.0), (2, "lowshelf", 200.0, 0.707, 6.0)],
              5: [(0, "highpass", 80.0, 1.0, 0.0)]}
    S = 3
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    line = lambda b, gd: f"{b} 0 " + " ".join(repr(x) for x in gd) + "\n"
    (tmp_path / "pan.txt").write_text("".join(line(b, gd) for b, gd in pan))
    (tmp_path / "eq.txt").write_text("# buffer section kind f0 Q gain\n" + "".join(
        f"{b} {s} {k} {f0!r} {q!r} {g!r}\n" for b, rows in script.items() for s, k, f0, q, g in rows))
    # the plain runs are cut where the equalised ones are: a pan set to the values in force, long after their ramp, changes nothing
    cut_lines = pan + [(2, pan[0][1]), (5, pan[1][1])]
    (tmp_path / "pan_cut.txt").write_text("".join(line(b, gd) for b, gd in cut_lines))
    (tmp_path / "pan_cut_tail.txt").write_text("".join(line(b, gd) for b, gd in cut_lines + [(nb, pan[1][1])]))
    base = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--channels", str(C), "--ramp", str(ramp)]
    eq_flags = ["--pan", str(tmp_path / "pan.txt"), "--buffers", str(nb), "--eq", str(tmp_path / "eq.txt"), "--eq-xfade", str(R)]
    cuts = [0, 2, 3, 5, nb]

    _run(base + ["--pan", str(tmp_path / "pan_cut.txt"), "--buffers", str(nb), "--out", str(tmp_path / "plain.wav")])
    ch, x = _wav(tmp_path / "plain.wav")
    assert ch == C and x.shape == (C, nb * B) and np.abs(x).max() > 0
    _run(base + eq_flags + ["--out", str(tmp_path / "eq.wav")])
    ch, got = _wav(tmp_path / "eq.wav")
    want = _equalised(np.ascontiguousarray(x), C, S, R, script, cuts)
    assert ch == C and got.shape == want.shape
    assert np.abs(want - x).max() > 1e-3 * np.abs(x).max()                       # (the script does something)
    assert np.ascontiguousarray(got).tobytes() == want.tobytes(), np.abs(got - want).max()
    header = lambda p: open(p, "rb").read()[:44]
    assert header(tmp_path / "eq.wav") == header(tmp_path / "plain.wav")

    # in front of --limit: one more buffer for the look-ahead, the limiter's model behind the EQ's
    _run(base + ["--pan", str(tmp_path / "pan_cut_tail.txt"), "--buffers", str(nb + 1), "--out", str(tmp_path / "long.wav")])
    _, xl = _wav(tmp_path / "long.wav")
    v = _equalised(np.ascontiguousarray(xl), C, S, R, script, cuts + [nb + 1])
    G = float(np.float32(3 * ceiling / float(np.abs(v).max())))                   # the loudest equalised sample lands at 3 T
    _run(base + eq_flags + ["--limit", repr(ceiling), "--lookahead", str(LA), "--gain", repr(G), "--out", str(tmp_path / "lim.wav")])
    ch, got = _wav(tmp_path / "lim.wav")
    m = MasterModel(C, ceiling, LA, 0, 0)
    m.set_gain(G)
    y = np.concatenate([m.process(np.ascontiguousarray(v[:, lo * B:hi * B])) for lo, hi in zip(cuts, cuts[1:] + [nb + 1])], axis=1)
    assert (m.gains < 1).any()
    want = np.ascontiguousarray(y[:, LA:LA + nb * B])
    assert ch == C and got.shape == want.shape and np.abs(want).max() > 0.5 * ceiling
    assert np.ascontiguousarray(got).tobytes() == want.tobytes(), np.abs(got - want).max()
