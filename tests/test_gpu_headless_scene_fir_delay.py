"""pbso_headless --channels C --fir FILE --fir-delay FILE [--delay-ramp N]: the tool cuts the run at the change points of both
scripts, sets filters and delays at them, and writes the filter mix behind its delay stage as a C-channel float32 WAV.  Its
payload against the same scene, the same sets and the same segments driven through the Python wrapper, whose output is held to
the reference model bit for bit in the same run."""
import math
import subprocess

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi
from tests.scene_fir_delay_model import Model
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513


def _python_scene_fir_delay(d, hits, script, dscript, files, nb_total, C, K, xfade, ramp, copies, shift):
    """the tool's calls through the wrapper, segment by segment; every segment also compared with the model"""
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
        max_onset, max_delay = max(on for _, _, on, _ in script), math.ceil(max(dl for _, _, dl in dscript))
        eng.scene_fir_enable(C, K, max_onset, xfade)
        eng.scene_fir_delay_enable(max_delay, ramp)
        model = Model(C, copies, K, max_onset, xfade, max_delay, ramp)
        taps, onset, delay = np.zeros((C, copies, K), np.float32), np.zeros(copies, np.int32), np.zeros(copies, np.float32)
        cuts = sorted({0, nb_total} | {l[0] for l in script + dscript if 0 < l[0] < nb_total})
        out = np.zeros((C, nb_total * B), np.float32)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            lines = [l for l in script if l[0] == b0]
            for _, cp, on, name in lines:
                taps[:, cp], onset[cp] = files[name], on
            if lines:
                eng.scene_fir_set(taps, onset)
                model.set(taps, onset)
            dlines = [l for l in dscript if l[0] == b0]
            for _, cp, dl in dlines:
                delay[cp] = dl
            if dlines:
                eng.scene_fir_set_delay(delay)
                model.set_delay(delay)
            eng.step(b1 - b0)
            eng.scene_fir()
            got = eng.read_scene_fir()
            want = model.mix(eng.audio())
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (b0, np.abs(got - want).max())
            out[:, b0 * B:b1 * B] = got
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("devices", [None, "0"])
def test_headless_fir_delay_writes_the_delayed_filter_mix(tmp_path, devices):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, K, xfade, ramp = 9, 2, 40, 300, 700
    copies = 1 if devices is None else 2
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    rng = np.random.default_rng(13)
    files = {name: (rng.standard_normal((C, K)) * np.exp(-np.arange(K) / 9.0)).astype(np.float32) for name in ("near.f32", "far.f32")}
    for name, h in files.items():
        h.astype("<f4").tofile(tmp_path / name)
    script = [(0, 0, 30, "near.f32"), (3, 0, 700, "far.f32")]
    # <buffer> <copy> <delay>: at a filter change point, between two of them (a cut of its own), one buffer into a ramp of 700
    dscript = [(0, 0, 120.25), (3, 0, 640.5), (5, 0, 12.0), (6, 0, 333.125)]
    if copies == 2:
        script += [(0, 1, 100, "far.f32")]
        dscript += [(0, 1, 0.0), (5, 1, 512.75)]
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    (tmp_path / "fir.txt").write_text("".join(f"{b} {cp} {on} {tmp_path / name}\n" for b, cp, on, name in script))
    (tmp_path / "delay.txt").write_text("# buffer copy delay\n" + "".join(f"{b} {cp} {dl!r}\n" for b, cp, dl in dscript))
    cmd = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--fir",
           str(tmp_path / "fir.txt"), "--xfade", str(xfade), "--fir-delay", str(tmp_path / "delay.txt"), "--delay-ramp", str(ramp),
           "--out", str(tmp_path / "o.wav")]
    if devices is not None:
        cmd += ["--devices", devices, "--copies", str(copies)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    assert ch == C and wav.shape == (C, nb * B)
    want = _python_scene_fir_delay(d, hits, script, dscript, files, nb, C, K, xfade, ramp, copies, 1)
    want = (want.astype(np.float64) / 1e10).astype(np.float32)
    assert np.abs(want).max() > 0 and np.abs(want[0] - want[1]).max() > 0
    assert np.array_equal(wav.view(np.uint32), want.view(np.uint32)), np.abs(wav - want).max()


def test_headless_fir_delay_refusals(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    np.ones(2 * 8, dtype="<f4").tofile(tmp_path / "ok.f32")
    (tmp_path / "fir.txt").write_text(f"0 0 0 {tmp_path / 'ok.f32'}\n")
    (tmp_path / "delay.txt").write_text("0 0 3.5\n")
    (tmp_path / "bad.txt").write_text("0 0 far\n")
    (tmp_path / "neg.txt").write_text("0 0 -1.0\n")
    (tmp_path / "copy.txt").write_text("0 1 1.0\n")
    base = [EXE, "-d", str(d), "--buffers", "2", "--out", str(tmp_path / "o.wav"), "--channels", "2"]
    fir = ["--fir", str(tmp_path / "fir.txt")]
    for extra, msg in ((["--fir-delay", str(tmp_path / "delay.txt")], "needs --fir"),
                       (fir + ["--fir-delay", str(tmp_path / "bad.txt")], "bad fir-delay line"),
                       (fir + ["--fir-delay", str(tmp_path / "neg.txt")], "fir delay outside"),
                       (fir + ["--fir-delay", str(tmp_path / "copy.txt")], "copy that does not exist"),
                       (fir + ["--fir-delay", str(tmp_path / "delay.txt"), "--delay-ramp", "-3"], "--delay-ramp must be")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + fir + ["--fir-delay", str(tmp_path / "delay.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
