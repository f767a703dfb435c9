"""pbso_headless --channels C --fir FILE [--xfade N]: the tool steps the segments between the script's change points, filters each
one with the scene filter mix (one engine; with --devices through PBSO_GATHER_FIR) and writes a C-channel interleaved float32
WAV.  Its payload against the same scene, the same sets and the same segments driven through the Python wrapper, bit for bit."""
import math
import subprocess

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513


def _python_scene_fir(d, hits, script, files, nb_total, C, K, xfade, copies, shift):
    """the tool's calls through the wrapper: hits of copy c shifted by c * shift buffers, unit transfer, segment by segment"""
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
        eng.scene_fir_enable(C, K, max(on for _, _, on, _ in script), xfade)
        taps, onset = np.zeros((C, copies, K), np.float32), np.zeros(copies, np.int32)
        cuts = sorted({0, nb_total} | {b for b, _, _, _ in script if 0 < b < nb_total})
        out = np.zeros((C, nb_total * B), np.float32)
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            lines = [l for l in script if l[0] == b0]
            for _, cp, on, name in lines:
                taps[:, cp], onset[cp] = files[name], on
            if lines:
                eng.scene_fir_set(taps, onset)
            eng.step(b1 - b0)
            eng.scene_fir()
            out[:, b0 * B:b1 * B] = eng.read_scene_fir()
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("devices", [None, "0"])
def test_headless_channels_and_fir_write_the_filter_mix(tmp_path, devices):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, K, xfade = 9, 2, 40, 300
    copies = 1 if devices is None else 2
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    rng = np.random.default_rng(12)
    files = {name: (rng.standard_normal((C, K)) * np.exp(-np.arange(K) / 9.0)).astype(np.float32) for name in ("near.f32", "far.f32", "wall.f32")}
    for name, h in files.items():
        h.astype("<f4").tofile(tmp_path / name)
    # <buffer> <copy> <onset> <taps file>: two change points after the start, an onset of more than one buffer, a file used twice
    script = [(0, 0, 30, "near.f32"), (3, 0, 700, "far.f32"), (7, 0, 12, "near.f32")]
    if copies == 2:
        script += [(0, 1, 100, "wall.f32"), (3, 1, 5, "far.f32")]
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    (tmp_path / "fir.txt").write_text("# buffer copy onset taps\n" + "".join(f"{b} {cp} {on} {tmp_path / name}\n" for b, cp, on, name in script))
    cmd = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--fir",
           str(tmp_path / "fir.txt"), "--xfade", str(xfade), "--out", str(tmp_path / "o.wav")]
    if devices is not None:
        cmd += ["--devices", devices, "--copies", str(copies)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    assert ch == C and wav.shape == (C, nb * B)
    want = _python_scene_fir(d, hits, script, files, nb, C, K, xfade, copies, 1)
    want = (want.astype(np.float64) / 1e10).astype(np.float32)
    assert np.abs(want).max() > 0 and np.abs(want[0] - want[1]).max() > 0
    assert np.array_equal(wav.view(np.uint32), want.view(np.uint32)), np.abs(wav - want).max()


def test_headless_fir_refuses_pan_and_bad_files(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    np.ones(2 * 8, dtype="<f4").tofile(tmp_path / "ok.f32")
    np.ones(2 * 8 + 1, dtype="<f4").tofile(tmp_path / "odd.f32")          # not [2][K]
    np.ones(2 * 6, dtype="<f4").tofile(tmp_path / "short.f32")            # another K than the file before it
    (tmp_path / "pan.txt").write_text("0 0 1.0 0.0 1.0 0.0\n")
    (tmp_path / "fir.txt").write_text(f"0 0 0 {tmp_path / 'ok.f32'}\n")
    (tmp_path / "odd.txt").write_text(f"0 0 0 {tmp_path / 'odd.f32'}\n")
    (tmp_path / "two.txt").write_text(f"0 0 0 {tmp_path / 'ok.f32'}\n1 0 0 {tmp_path / 'short.f32'}\n")
    (tmp_path / "bad.txt").write_text("0 0 zero taps\n")
    base = [EXE, "-d", str(d), "--buffers", "2", "--out", str(tmp_path / "o.wav"), "--channels", "2"]
    for extra, msg in ((["--pan", str(tmp_path / "pan.txt"), "--fir", str(tmp_path / "fir.txt")], "exclude each other"),
                       (["--fir", str(tmp_path / "odd.txt")], "is not float32"),
                       (["--fir", str(tmp_path / "two.txt")], "taps per channel"),
                       (["--fir", str(tmp_path / "bad.txt")], "bad fir line")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + ["--fir", str(tmp_path / "fir.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
