"""pbso_headless --fir-bank FILE --fir-taps K --fir-dirs SCRIPT: the filters of a script's lines come from a bank uploaded once,
a line names (index, weight) pairs into it.  The WAV is BYTE-IDENTICAL to the one --fir writes for per-line taps files that this
test builds from the same pairs with the C reference (tests/cpp/scene_fir_bank_ref.c), padded to the script's widest line as the
tool pads them -- cut at every line's buffer, and scheduled up front (--fir-schedule); for a single engine and a device group."""
import subprocess

import numpy as np
import pytest

from tests.scene_fir_bank_model import taps_from_bank
from tests.test_headless_cli import EXE, make_data_dir

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("devices", [None, "0"])
@pytest.mark.parametrize("schedule", [False, True])
def test_fir_dirs_writes_the_wav_of_fir_with_the_references_taps(tmp_path, devices, schedule):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    nb, C, K, F, xfade = 7, 2, 40, 6, 300
    copies = 1 if devices is None else 2
    hits = [(0, 3, (0.2, -0.5, 1.0)), (2, 7, (1.0, 0.0, 0.3)), (5, 1, (0.0, 1.0, 0.0))]
    rng = np.random.default_rng(17)
    bank = (rng.standard_normal((F, C, K)) * np.exp(-np.arange(K) / 9.0)).astype("<f4")
    bank.tofile(tmp_path / "bank.f32")
    # <buffer> <copy> <onset> then 1 .. 3 pairs: one filter as it is, a blend, a repeated index with a zero and a negative weight
    script = [(0, 0, 30, [(F - 1, 1.0)]), (3, 0, 700, [(0, 0.25), (2, 0.75)]), (5, 0, 5, [(4, -1.5), (4, 0.0), (1, 0.5)])]
    if copies == 2:
        script += [(0, 1, 100, [(3, 0.5), (5, 0.5)]), (5, 1, 0, [(0, 1.0)])]
    J = max(len(p) for *_, p in script)
    dirs, fir = [], []
    for k, (b, cp, on, pairs) in enumerate(script):
        dirs.append(f"{b} {cp} {on} " + " ".join(f"{i} {w!r}" for i, w in pairs) + "\n")
        padded = pairs + [(0, 0.0)] * (J - len(pairs))
        taps = taps_from_bank(bank, np.array([[i for i, _ in padded]], dtype=np.int32), np.array([[w for _, w in padded]], dtype=np.float32))
        taps[:, 0, :].astype("<f4").tofile(tmp_path / f"line{k}.f32")                 # [C][K]
        fir.append(f"{b} {cp} {on} {tmp_path / f'line{k}.f32'}\n")
    (tmp_path / "hits.txt").write_text("".join(f"{b} {v} {n[0]} {n[1]} {n[2]} point\n" for b, v, n in hits))
    (tmp_path / "dirs.txt").write_text("# buffer copy onset index weight ...\n" + "".join(dirs))
    (tmp_path / "fir.txt").write_text("".join(fir))
    wavs = []
    for how in ("dirs", "fir"):
        out = tmp_path / f"{how}.wav"
        cmd = [EXE, "-d", str(d), "--hits", str(tmp_path / "hits.txt"), "--buffers", str(nb), "--channels", str(C), "--xfade", str(xfade),
               "--time-chunks", "1", "--out", str(out)]
        cmd += (["--fir-bank", str(tmp_path / "bank.f32"), "--fir-taps", str(K), "--fir-dirs", str(tmp_path / "dirs.txt")] if how == "dirs"
                else ["--fir", str(tmp_path / "fir.txt")])
        if schedule:
            cmd += ["--fir-schedule"]
        if devices is not None:
            cmd += ["--devices", devices, "--copies", str(copies)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        wavs.append(open(out, "rb").read())
    assert len(wavs[0]) == 44 + 4 * C * nb * 513 and any(wavs[0][44:])
    assert wavs[0] == wavs[1]


def test_fir_dirs_is_refused_with_fir_or_pan_and_without_its_bank(tmp_path):
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    base = [EXE, "-d", str(d), "--buffers", "1", "--channels", "2", "--out", str(tmp_path / "o.wav")]
    for extra, word in ((["--fir-dirs", "x", "--fir-bank", "y", "--fir-taps", "4", "--fir", "z"], "--fir-dirs excludes --fir and --pan"),
                        (["--fir-dirs", "x", "--fir-bank", "y", "--fir-taps", "4", "--pan", "z"], "--fir-dirs excludes --fir and --pan"),
                        (["--fir-dirs", "x"], "go together")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr, r.stderr
    # every token of a pair is parsed whole: "0.5" where an index belongs is not index 0 with weight .5
    np.ones((2, 2, 4), dtype="<f4").tofile(tmp_path / "bank.f32")
    for text, word in (("0 0 0 0.5 1.0\n", "index is not an integer"), ("0 0 0 1 1.0x\n", "weight is not a number"),
                       ("0 0 0 1\n", "has no weight"), ("0 0 0 2 1.0\n", "outside the bank"), ("0 0 0\n", "needs 1 .. 8 pairs")):
        (tmp_path / "dirs.txt").write_text(text)
        r = subprocess.run(base + ["--fir-bank", str(tmp_path / "bank.f32"), "--fir-taps", "4", "--fir-dirs", str(tmp_path / "dirs.txt")],
                           capture_output=True, text=True)
        assert r.returncode != 0 and word in r.stderr, (text, r.stderr)
