"""The EQ bus's product boundary, without a GPU: the eight entry points in the header, in capi.EXPORTS and in the built library;
the unchanged ABI version; the stated arithmetic; the Python methods; the kernels' resource listing; the headless tool's refusals;
the block tables of csrc/eq_block.h (printed by the check program, which is built with the host compiler under ASan + UBSan and
run as a program of its own) against the model's, bit for bit; and pbso_eq_design against the same formulas in numpy scalars and
against the textbook magnitudes."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import eq_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_eq_enable", "pbso_eq_set", "pbso_eq", "pbso_read_eq", "pbso_eq_tables", "pbso_eq_reset", "pbso_eq_info",
                "pbso_eq_design")
RATE = 44100.0
# (kind, f0, Q, gain dB)
DESIGNS = [("highpass", 30.0, 0.707, 0.0), ("highpass", 20.0, 2.0, 0.0), ("highpass", 5.0, 8.0, 0.0), ("peak", 100.0, 4.0, 12.0),
           ("peak", 1000.0, 2.0, -9.0), ("highshelf", 8000.0, 0.707, 6.0), ("lowpass", 18000.0, 0.707, 0.0),
           ("lowshelf", 200.0, 0.707, -6.0), ("lowpass", 300.0, 1.5, 0.0), ("lowshelf", 120.0, 1.0, 9.0), ("highshelf", 3000.0, 1.0, -12.0)]


def _capi():
    from openpbso_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi


def _header():
    return open(os.path.join(ROOT, "include", "openpbso_amd.h")).read()


def _check_program():
    csrc = os.path.join(ROOT, "openpbso_amd", "csrc")
    b = subprocess.run(["make", "-C", csrc, "eq_block_check"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return os.path.join(ROOT, "openpbso_amd", "eq_block_check")


def _bits(lines):
    return np.array([int(x, 16) for x in lines], dtype=np.uint64).view(np.float64)


def test_entry_points_in_header_exports_and_library():
    capi = _capi()
    hdr = _header()
    declared = set(re.findall(r"\b(pbso_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.lib()
    for name in ENTRY_POINTS:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()
    assert int(re.search(r"#define\s+PBSO_EQ_BLOCK\s+(\d+)", hdr).group(1)) == capi.EQ_BLOCK == em.P
    for name, value in (("LOWPASS", 0), ("HIGHPASS", 1), ("PEAK", 2), ("LOWSHELF", 3), ("HIGHSHELF", 4)):
        assert re.search(rf"PBSO_EQ_{name} = {value}\b", hdr) and getattr(capi, "EQ_" + name) == value


def test_header_states_the_arithmetic():
    hdr = _header()
    for phrase in ("C channels, 1 .. 8; S sections per channel, 1 .. 8, in cascade", "five fp64 coefficients b0 b1 b2 a1 a2",
                   "Signal 0 of channel c is (double)u_c(t); signal s + 1 is the output of section s", "All signals are 0 for t < 0",
                   "P = PBSO_EQ_BLOCK is part of the definition", "T0 = t_set + g * P",
                   "o = b0 v + b1 x1 + b2 x2 - a1 y1 - a2 y2", "in this literal order of operations",
                   "x(T0-1), x(T0-2), y(T0-1), y(T0-2) respectively",
                   "y(T0+k): acc = 0.0; for j = k down to 0: acc = fma(h[j], x(T0+k-j), acc);",
                   "acc = fma(r[k], x(T0-1), acc); acc = fma(s[k], x(T0-2), acc);",
                   "acc = fma(q[k], y(T0-2), acc); acc = fma(p[k], y(T0-1), acc)",
                   "two fma per block and\n * section", "out_c(t) = (float)signal S", "Subnormals are kept", "rounded to f32 once at the end",
                   "install the identity cascade (b0 = 1, the rest 0, t_set = 0)", "the input bit for bit",
                   "through t_set + R - 2", "the direct-form-I state", "out = yf + w * (yt - yf)",
                   "w = (float)((double)(t - t_set + 1) / (double)R)", "three separately rounded f32 operations",
                   "A set with no step since the previous set\n * replaces it", "A set while a fade runs is PBSO_ERR_STATE",
                   "|a2| < 1 and |a1| < 1 + a2", "the stage stays as it was", "the last P + 2 fp64 samples",
                   "finishes that block from the same origin", "d_out == d_in is allowed", "A refused call changes nothing",
                   "A device group has none", "w0 = 2 pi f0 / rate, cs = cos(w0), sn = sin(w0), alpha = sn / (2 Q), A = pow(10, gain_db / 40)",
                   "b1 = 1 - cs, b0 = b2 = b1 / 2", "b1 = -(1 + cs), b0 = b2 = (1 + cs) / 2", "b0 = 1 + alpha A, b1 = -2 cs, b2 = 1 - alpha A",
                   "a0 = (A+1) + (A-1) cs + g, a1 = -2 ((A-1) + (A+1) cs), a2 = (A+1) + (A-1) cs - g",
                   "a0 = (A+1) - (A-1) cs + g, a1 = 2 ((A-1) - (A+1) cs), a2 = (A+1) - (A-1) cs - g"):
        assert phrase in hdr, phrase


def test_python_methods_exist():
    capi = _capi()
    from openpbso_amd.solver import Engine
    for m in ("eq_enable", "eq_set", "eq", "read_eq", "eq_tables", "eq_reset", "eq_info"):
        assert callable(getattr(Engine, m)), m
    assert callable(capi.eq_design) and set(capi.EQ_KINDS) == set(em.KINDS)


def test_kernels_use_no_scratch():
    _capi()
    path = os.path.join(ROOT, "openpbso_amd", "csrc", "kernels_eq.resources.txt")
    if not os.path.exists(path):                         # (a library from another build of the tree: make the listing)
        subprocess.run(["make", "-C", os.path.dirname(path), "kernels_eq.o"], check=True, capture_output=True)
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == 5
    for kernel in ("eq_input_kernel", "eq_forward_kernel", "eq_chain_kernel", "eq_finish_kernel", "eq_output_kernel"):
        assert sum(kernel in n for n in names) == 1, kernel
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    assert "warning" not in text


def test_headless_refuses_bad_eq_flags_before_it_needs_a_device(tmp_path):
    _capi()
    from tests.test_headless_cli import EXE, make_data_dir
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    (tmp_path / "pan.txt").write_text("0 0 1.0 0.0 0.5 10.0\n")
    good = tmp_path / "eq.txt"
    good.write_text("0 0 highpass 30 0.707 0\n1 1 peak 1000 2 -9\n")

    scripts = []

    def script(text):
        p = tmp_path / f"bad{len(scripts)}.txt"
        p.write_text(text)
        scripts.append(p)
        return str(p)

    base = [EXE, "-d", str(d), "--buffers", "2", "--out", str(tmp_path / "o.wav")]
    mixed = ["--channels", "2", "--pan", str(tmp_path / "pan.txt")]
    for extra, msg in ((["--eq", str(good)], "--eq needs --channels"),
                       (["--eq", str(good), "--channels", "2"], "--eq needs --channels"),
                       (["--eq-xfade", "100"] + mixed, "belongs to --eq"),
                       (mixed + ["--eq", str(good), "--devices", "0,1"], "device group"),
                       (mixed + ["--eq", str(good), "--devices", "0"], "device group"),
                       (mixed + ["--eq", str(good), "--raw", str(tmp_path / "o.f32")], "not with --eq"),
                       (mixed + ["--eq", str(good), "--eq-xfade", "-1"], "--eq-xfade must be"),
                       (mixed + ["--eq", str(good), "--eq-xfade", "1048577"], "--eq-xfade must be"),
                       (mixed + ["--eq", str(tmp_path / "none.txt")], "cannot read"),
                       (mixed + ["--eq", script("# nothing\n")], "no lines"),
                       (mixed + ["--eq", script("0 0 highpass 30\n")], "bad eq line"),
                       (mixed + ["--eq", script("0 0 notch 30 1 0\n")], "eq kind must be"),
                       (mixed + ["--eq", script("2 0 highpass 30 1 0\n")], "outside buffers"),
                       (mixed + ["--eq", script("-1 0 highpass 30 1 0\n")], "outside buffers"),
                       (mixed + ["--eq", script("0 8 highpass 30 1 0\n")], "section must be 0 .. 7"),
                       (mixed + ["--eq", script("0 0 highpass 22050 1 0\n")], "0 < f0 < rate / 2"),
                       (mixed + ["--eq", script("0 0 highpass 0 1 0\n")], "0 < f0 < rate / 2"),
                       (mixed + ["--eq", script("0 0 highpass 30 0 0\n")], "Q must be positive"),
                       (mixed + ["--eq", script("0 0 peak 30 1 nan\n")], "gain dB"),
                       (mixed + ["--eq", script("0 0 peak 30 1 121\n")], "gain dB"),
                       (mixed + ["--eq"], "missing value")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "o.wav").exists()


def test_the_check_program_passes_under_the_sanitizers():
    r = subprocess.run([_check_program()], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "eq_block_check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("design", DESIGNS + [("identity",)])
def test_the_tables_of_the_host_header_are_the_models(design):
    exe = _check_program()
    c = np.array([1.0, 0.0, 0.0, 0.0, 0.0]) if design == ("identity",) else em.design(design[0], RATE, *design[1:])
    r = subprocess.run([exe, "tables"] + [float(v).hex() for v in c], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split()
    assert int(lines[0]) == em.P and len(lines) == 1 + 5 * em.P
    got, want = _bits(lines[1:]).reshape(5, em.P), em.tables(c)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.abs(got - want).max()
    # an unstable section is refused by the same header
    r = subprocess.run([exe, "tables", "1", "0", "0", "-2", "1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "stable" in r.stderr


@pytest.mark.parametrize("design", DESIGNS)
def test_the_designs_are_the_formulas_and_the_textbook_responses(design):
    capi = _capi()
    kind, f0, q, gain = design
    got = np.array(capi.eq_design(kind, RATE, f0, q, gain))
    want = em.design(kind, RATE, f0, q, gain)
    ulp = np.spacing(np.abs(want))
    assert (np.abs(got - want) <= 4 * ulp).all(), (got, want, np.abs(got - want) / ulp)
    # the check program's design is the library's
    r = subprocess.run([_check_program(), "design", str(capi.EQ_KINDS[kind]), repr(RATE), repr(f0), repr(q), repr(gain)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert (np.abs(_bits(r.stdout.split()) - want) <= 4 * ulp).all()
    # magnitudes: at f0, at DC and at Nyquist
    A = 10.0 ** (gain / 40.0)
    at = lambda f: em.response(got, f, RATE)
    textbook = {"lowpass": (q, 1.0, 0.0), "highpass": (q, 0.0, 1.0), "peak": (A * A, 1.0, 1.0),
                "lowshelf": (None, A * A, 1.0), "highshelf": (None, 1.0, A * A)}[kind]
    for f, value in zip((f0, 0.0, 0.5 * RATE), textbook):
        if value is None:
            # a shelf at its corner, from the analog prototype at s = j: |A ((A - 1) + j sqrt(A) / Q)| / |(1 - A) + j sqrt(A) / Q| = A, half the gain in dB
            value = A
        assert abs(at(f) - value) < 1e-9, (kind, f, at(f), value)
    assert abs(got[4]) < 1 and abs(got[3]) < 1 + got[4]


def test_design_refusals():
    capi = _capi()
    lib = capi.lib()
    out = (C.c_double * 5)()
    assert lib.pbso_eq_design(0, 44100.0, 100.0, 1.0, 0.0, out) == 0
    for bad in ((5, 44100.0, 100.0, 1.0, 0.0), (-1, 44100.0, 100.0, 1.0, 0.0), (0, 0.0, 100.0, 1.0, 0.0), (0, 44100.0, 22050.0, 1.0, 0.0),
                (0, 44100.0, 0.0, 1.0, 0.0), (0, 44100.0, 100.0, 0.0, 0.0), (0, 44100.0, math.nan, 1.0, 0.0), (2, 44100.0, 100.0, 1.0, math.inf),
                (2, 44100.0, 100.0, 1.0, 121.0)):
        assert lib.pbso_eq_design(*bad, out) == capi.ERR_INVALID, bad
    assert lib.pbso_eq_design(0, 44100.0, 100.0, 1.0, 0.0, None) == capi.ERR_INVALID
    with pytest.raises(ValueError):
        capi.eq_design("peak", 44100.0, 30000.0, 1.0, 0.0)
