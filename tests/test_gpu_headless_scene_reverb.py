"""pbso_headless --channels C --pan FILE --reverb FILE: the tool steps the segments between the pan script's change points, mixes
each one, sends the object mix through the scene reverb and writes dry + wet.  Its payload against the same scene, the same sets
and the same segments driven through the Python wrapper, bit for bit; and the refusals."""
import math
import subprocess

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi
from tests.test_gpu_headless_scene_mix import _wav
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu
B = 513


def _python_scene_reverb(d, hits, pan, nb_total, C, ramp, ir, xfade):
    """the tool's calls through the wrapper: scene_mix -> d_add, mix_objects -> the bus, scene_reverb, segment by segment"""
    import torch
    eng = Engine(qnorm=capi.QNORM_OFF)
    try:
        eng.add_object_from_files(str(d / "bowl_surf.modes"), str(d / "bowl_material.txt"), str(d / "bowl_ffat_maps"))
        eng.finalize()
        eng.set_use_transfer(0, False)
        for b, v, n in hits:
            n = np.asarray(n, dtype=np.float64)
            assert eng.enqueue_force(0, ForceMessage(vid=v, vn=n / math.sqrt(float(n @ n))), b)
        eng.scene_mix_enable(C, math.ceil(max(x for _, gd in pan for x in gd[1::2])), ramp)
        eng.scene_reverb_enable(1, C, ir.shape[1], xfade)
        eng.scene_reverb_set(ir.reshape(C, 1, -1))
        dry = torch.zeros(C * nb_total * B, dtype=torch.float32, device="cuda")
        bus = torch.zeros(nb_total * B, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        cuts = sorted({0, nb_total} | {b for b, _ in pan if 0 < b < nb_total})
        out = np.zeros((C, nb_total * B), np.float32)
        wet_differs = False
        for b0, b1 in zip(cuts[:-1], cuts[1:]):
            for b, gd in pan:
                if b == b0:
                    eng.scene_mix_set(np.asarray(gd[0::2], np.float32).reshape(C, 1), np.asarray(gd[1::2], np.float32).reshape(C, 1))
            eng.step(b1 - b0)
            eng.scene_mix(dry.data_ptr())
            eng.mix_objects(bus.data_ptr())
            eng.scene_reverb(bus.data_ptr(), dry.data_ptr())
            out[:, b0 * B:b1 * B] = eng.read_scene_reverb()
            wet_differs |= not np.array_equal(out[:, b0 * B:b1 * B], eng.read_scene_mix())
        assert wet_differs
        return out
    finally:
        eng.close()


def test_headless_reverb_writes_dry_plus_wet(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, ramp, K, xfade = 9, 2, 300, 2500, 100
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    pan = [(0, (1.0, 0.0, 0.25, 30.5)), (3, (0.5, 400.0, 0.75, 700.25)), (7, (-0.3, 12.75, 1.0, 0.0))]      # three segments
    rng = np.random.default_rng(21)
    ir = (rng.standard_normal((C, K)) * np.exp(-np.arange(K) / 500.0) * 0.05).astype(np.float32)           # > one buffer, two segments of taps
    ir.astype("<f4").tofile(tmp_path / "ir.f32")
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    (tmp_path / "pan.txt").write_text("".join(f"{b} 0 " + " ".join(repr(x) for x in gd) + "\n" for b, gd in pan))
    cmd = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--pan",
           str(tmp_path / "pan.txt"), "--ramp", str(ramp), "--reverb", str(tmp_path / "ir.f32"), "--reverb-xfade", str(xfade),
           "--out", str(tmp_path / "o.wav")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ch, wav = _wav(tmp_path / "o.wav")
    assert ch == C and wav.shape == (C, nb * B)
    want = _python_scene_reverb(d, hits, pan, nb, C, ramp, ir, xfade)
    want = (want.astype(np.float64) / 1e10).astype(np.float32)
    assert np.abs(want).max() > 0 and np.abs(want[0] - want[1]).max() > 0
    assert np.array_equal(wav.view(np.uint32), want.view(np.uint32)), np.abs(wav - want).max()


def test_headless_reverb_refusals(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    np.ones(2 * 8, dtype="<f4").tofile(tmp_path / "ok.f32")
    np.ones(2 * 8 + 1, dtype="<f4").tofile(tmp_path / "odd.f32")           # not [2][K]
    (tmp_path / "pan.txt").write_text("0 0 1.0 0.0 1.0 0.0\n")
    base = [EXE, "-d", str(d), "--buffers", "2", "--out", str(tmp_path / "o.wav")]
    mix = ["--channels", "2", "--pan", str(tmp_path / "pan.txt")]
    for extra, msg in ((["--reverb", str(tmp_path / "ok.f32")], "--reverb needs --channels"),
                       (mix + ["--reverb", str(tmp_path / "ok.f32"), "--devices", "0,1"], "device group"),
                       (mix + ["--reverb", str(tmp_path / "odd.f32")], "is not float32"),
                       (mix + ["--reverb", str(tmp_path / "none.f32")], "cannot read impulse response")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    r = subprocess.run(base + mix + ["--reverb", str(tmp_path / "ok.f32")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
