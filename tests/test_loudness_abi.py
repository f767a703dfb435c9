"""The loudness bus's product boundary, without a GPU: the nine entry points in the header, in capi.EXPORTS and in the built library;
the unchanged ABI version; the stated definition; the Python methods; the kernels' resource listing; the headless tool's refusals;
the check program of csrc/loudness_gate.h (built with the host compiler under ASan + UBSan and run as a program of its own);
pbso_loudness_design against the BS.1770-4 table at 48 kHz and, bit for bit, against the same formulas in numpy scalars; and the
true peak's taps against the model's."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import loudness_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_loudness_enable", "pbso_loudness", "pbso_read_loudness_blocks", "pbso_loudness_report", "pbso_loudness_taps",
                "pbso_loudness_reset", "pbso_loudness_info", "pbso_loudness_design", "pbso_loudness_report_from_blocks")
RATES = [44100, 48000, 22050, 96000, 32000, 88200, 192000]
BS1770 = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                   [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])


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
    b = subprocess.run(["make", "-C", csrc, "loudness_gate_check"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return os.path.join(ROOT, "openpbso_amd", "loudness_gate_check")


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
    assert C.sizeof(capi.LoudnessBlock) == 16 == np.dtype(capi.LOUDNESS_BLOCK).itemsize == lm.BLOCK.itemsize
    assert C.sizeof(capi.LoudnessSummary) == 80
    assert "} pbso_loudness_block;   /* 16 bytes */" in hdr and "} pbso_loudness_summary; /* 80 bytes */" in hdr


def test_header_states_the_definition():
    hdr = _header()
    for phrase in ("Loudness bus: programme loudness and true peak", "ITU-R BS.1770-4", "EBU Tech 3341",
                   "t counts processed samples from the enable or the last reset, 64-bit", "u_c(t) is input channel c, 0 for t < 0",
                   "Hs = rate / 10 samples (100 ms)", "a multiple of 10 with Hs >= 256", "Sub-block j covers t in [j Hs, (j + 1) Hs)",
                   "f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196",
                   "K = tan(pi f0 / rate), Vh = pow(10, G / 20), Vb = pow(Vh, 0.4996667741545416), a0 = 1 + K/Q + K K",
                   "b0 = (Vh + Vb K/Q + K K) / a0, b1 = 2 (K K - Vh) / a0, b2 = (Vh - Vb K/Q + K K) / a0",
                   "a1 = 2 (K K - 1) / a0, a2 = (1 - K/Q + K K) / a0", "f0 = 38.13547087602444, Q = 0.5003270373238773",
                   "b = 1, -2, 1 (not normalised, as the standard has it)", "signal 2 of the EQ bus's block form",
                   "P = PBSO_EQ_BLOCK", "t_set = 0, installed at enable and\n * never changed", "kept in fp64 and not rounded to f32",
                   "the EQ's P + 2 fp64 samples per signal", "k = t - j Hs and l = k mod 64", "acc_l = fma(z, z, acc_l)  in ascending k",
                   "for s = 32, 16, 8, 4, 2, 1 and every\n * l < s:  acc_l = acc_l + acc_{l+s};  E_c(j) = acc_0",
                   "The device keeps the 64 accumulators per channel across steps",
                   "O = 4 for a\n * rate below 80 000 Hz and 2 from there up", "T = 12 taps per phase",
                   "h[phi][k] = (float)g[k L + phi]) with L = O, M = 1, beta = 8.0, cutoff = 1.0",
                   "acc = 0.f; for k = 11 down to 0: acc = fmaf(h[phi][k], u_c(t - k), acc)",
                   "TP_c(j) is the maximum of fabsf(acc) over the sub-block's t and all phi, SP_c(j) the maximum of fabsf(u_c(t))",
                   "the last 11 input samples per channel and the running maxima of an open sub-block", "Subnormals are kept",
                   "A non-finite input\n * leaves later records unspecified", "device-resident log [max_blocks][C]",
                   "refused with PBSO_ERR_STATE before anything changes",
                   "ms_c = (((E_c(i-3) + E_c(i-2)) + E_c(i-1)) + E_c(i)) / (4 Hs)", "w_i is the sum over ascending c of G_c ms_c",
                   "l_i = -0.691 + 10 log10(w_i), -infinity for w_i = 0", "A = {i : l_i > -70}",
                   "Gamma = -0.691 + 10 log10(mean of w over A, ascending i) - 10",
                   "integrated = -0.691 + 10 log10(mean of w over {i in A : l_i > Gamma})", "Momentary is l of the last\n * gating block",
                   "the last 30 sub-blocks, summed left-associated in ascending order", "is -HUGE_VAL",
                   "finite\n * and >= 0, given at enable; NULL means all 1", "read only", "A refused call changes nothing",
                   "A device group has none"):
        assert phrase in hdr, phrase


def test_python_methods_exist():
    capi = _capi()
    from openpbso_amd.solver import Engine
    for m in ("loudness_enable", "loudness", "read_loudness_blocks", "loudness_report", "loudness_taps", "loudness_reset", "loudness_info"):
        assert callable(getattr(Engine, m)), m
    assert callable(capi.loudness_design) and callable(capi.loudness_report_from_blocks)


def test_kernels_use_no_scratch():
    _capi()
    path = os.path.join(ROOT, "openpbso_amd", "csrc", "kernels_loudness.resources.txt")
    if not os.path.exists(path):                         # (a library from another build of the tree: make the listing)
        subprocess.run(["make", "-C", os.path.dirname(path), "kernels_loudness.o"], check=True, capture_output=True)
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == 3               # the energy kernel, the peak kernel for O = 4 and for O = 2
    assert sum("loudness_energy_kernel" in n for n in names) == 1 and sum("loudness_peak_kernel" in n for n in names) == 2
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    assert "warning" not in text


def test_headless_refuses_bad_loudness_flags_before_it_needs_a_device(tmp_path):
    _capi()
    from tests.test_headless_cli import EXE, make_data_dir
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    (tmp_path / "pan.txt").write_text("0 0 1.0 0.0 0.5 10.0\n")
    base = [EXE, "-d", str(d), "--buffers", "2", "--out", str(tmp_path / "o.wav")]
    loud = ["--loudness", str(tmp_path / "l.txt")]
    mixed = ["--channels", "2", "--pan", str(tmp_path / "pan.txt")]
    for extra, msg in ((loud + ["--limit", "0.9"], "not with --limit"),
                       (mixed + loud + ["--limit", "0.9", "--gain", "2"], "not with --limit"),
                       (loud + ["--out-rate", "48000"], "not with --out-rate"),
                       (loud + ["--devices", "0,1"], "device group"),
                       (loud + ["--devices", "0"], "device group"),
                       (loud + ["--raw", str(tmp_path / "o.f32")], "not with --loudness"),
                       (["--loudness-target", "-16"], "belongs to --loudness"),
                       (loud + ["--loudness-target", "3"], "--loudness-target must be"),
                       (loud + ["--loudness-target", "nan"], "--loudness-target must be"),
                       (loud + ["--loudness-target", "-71"], "--loudness-target must be"),
                       (["--loudness"], "missing value")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "o.wav").exists() and not (tmp_path / "l.txt").exists()


def test_the_check_program_passes_under_the_sanitizers():
    r = subprocess.run([_check_program()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "loudness_gate_check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_design_at_48_kHz_is_the_standards_table():
    """BS.1770-4 prints the table to 14 places; 9e-16 was measured"""
    capi = _capi()
    got = np.array(capi.loudness_design(48000.0))
    assert got.shape == (2, 5) and np.abs(got - BS1770).max() < 1e-12, np.abs(got - BS1770).max()


@pytest.mark.parametrize("rate", RATES)
def test_the_design_is_the_formulas_bit_for_bit(rate):
    capi = _capi()
    got, want = np.array(capi.loudness_design(float(rate))), lm.design(rate)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got - want)
    # the check program's design is the library's
    r = subprocess.run([_check_program(), "design", str(rate)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    bits = np.array([int(x, 16) for x in r.stdout.split()], dtype=np.uint64)
    assert np.array_equal(bits, want.view(np.uint64).ravel())
    # stable, as the EQ bus demands of a section
    for b0, b1, b2, a1, a2 in got:
        assert abs(a2) < 1 and abs(a1) < 1 + a2


@pytest.mark.parametrize("rate", [44100, 22050, 48000, 96000])
def test_the_true_peak_taps_are_the_models(rate):
    r = subprocess.run([_check_program(), "taps", str(rate)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split()
    O = int(lines[0])
    assert O == lm.oversampling(rate) == (4 if rate < 80000 else 2) and len(lines) == 1 + 12 * O
    got = np.array([int(x, 16) for x in lines[1:]], dtype=np.uint32).reshape(O, 12)
    want = lm.taps(rate)
    assert np.array_equal(got, want.view(np.uint32)), (got.view(np.float32) - want)
    # every phase passes DC within half a percent, and the phases together are the Kaiser-windowed sinc of gain O
    assert np.abs(want.astype(np.float64).sum(axis=1) - 1.0).max() < 5e-3


def test_design_and_report_refusals():
    capi = _capi()
    lib = capi.lib()
    out = (C.c_double * 10)()
    assert lib.pbso_loudness_design(44100.0, out) == 0
    for bad in (0.0, -48000.0, 3000.0, math.nan, math.inf):
        assert lib.pbso_loudness_design(bad, out) == capi.ERR_INVALID, bad
    assert lib.pbso_loudness_design(44100.0, None) == capi.ERR_INVALID
    blocks = np.zeros((5, 2), dtype=np.dtype(capi.LOUDNESS_BLOCK))
    bp = blocks.ctypes.data_as(C.POINTER(capi.LoudnessBlock))
    s = capi.LoudnessSummary()
    assert lib.pbso_loudness_report_from_blocks(bp, 5, 2, None, 4410, C.byref(s)) == 0 and s.n_blocks == 5 and s.integrated == -math.inf
    w = (C.c_double * 2)(1.0, -1.0)
    for args in ((bp, 5, 2, None, 4410, None), (bp, 5, 0, None, 4410, C.byref(s)), (bp, 5, 9, None, 4410, C.byref(s)),
                 (bp, 5, 2, None, 0, C.byref(s)), (bp, -1, 2, None, 4410, C.byref(s)), (None, 5, 2, None, 4410, C.byref(s)),
                 (bp, 5, 2, w, 4410, C.byref(s))):
        assert lib.pbso_loudness_report_from_blocks(*args) == capi.ERR_INVALID
    assert capi.loudness_report_from_blocks(blocks[:0], 4410)["n_blocks"] == 0
