"""The master bus's product boundary, without a GPU: the nine entry points in the header, in capi.EXPORTS and in the built library;
the unchanged ABI version; the stated order of arithmetic; the meter record; the Python methods; the headless tool's refusals."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_master_enable", "pbso_master_set_gain", "pbso_master", "pbso_read_master", "pbso_read_master_pcm16",
                "pbso_read_master_meters", "pbso_master_window", "pbso_master_reset", "pbso_master_info")


def _capi():
    from openpbso_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi


def _header():
    return open(os.path.join(ROOT, "include", "openpbso_amd.h")).read()


def test_entry_points_in_header_exports_and_library():
    capi = _capi()
    hdr = _header()
    declared = set(re.findall(r"\b(pbso_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.lib()
    for name in ENTRY_POINTS:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def test_header_states_the_order_of_arithmetic():
    hdr = _header()
    for phrase in ("v_c(t)  = (float)p(t) * u_c(t)", "pk(t)   = max over c of fabsf(v_c(t))", "r(t)    = pk(t) > T ? T / pk(t) : 1.f",
                   "a(t)    = min over j = 0 .. L + H of r(t - j)",
                   "acc = 0.f; for k = L-1 down to 0: acc = fmaf(w[k], a(t - k), acc);   g = fminf(acc, r(t - L))",
                   "y_c(t)  = fminf(fmaxf(v_c(t - L) * g(t), -T), T)", "h_k = 1 - cos(2 pi (k+1) / (L+1))", "w[k] = (float)(h_k / sum)",
                   "Subnormals are kept", "last 2 L + H samples", "(int16_t)lrintf(y * 32767.f)", "A device group has none"):
        assert phrase in hdr, phrase


def test_the_meter_record_is_24_bytes_in_c_and_python():
    capi = _capi()
    assert C.sizeof(capi.MasterMeter) == 24 and np.dtype(capi.MasterMeter).itemsize == 24
    assert [(n, getattr(capi.MasterMeter, n).offset) for n, _ in capi.MasterMeter._fields_] == [
        ("in_peak", 0), ("out_peak", 4), ("min_gain", 8), ("n_limited", 12), ("sumsq", 16)]
    body = re.search(r"typedef struct pbso_master_meter \{(.*?)\} pbso_master_meter;", _header(), re.S).group(1)
    assert re.findall(r"^\s*(float|double|int32_t)\s+(\w+);", body, re.M) == [
        ("float", "in_peak"), ("float", "out_peak"), ("float", "min_gain"), ("int32_t", "n_limited"), ("double", "sumsq")]
    from tests.master_model import METER_DTYPE
    assert METER_DTYPE == np.dtype(capi.MasterMeter)


def test_python_methods_exist():
    from openpbso_amd.solver import Engine
    for m in ("master_enable", "master_set_gain", "master", "read_master", "read_master_pcm16", "read_master_meters", "master_window",
              "master_reset", "master_info"):
        assert callable(getattr(Engine, m)), m


def test_headless_refuses_bad_master_flags_before_it_needs_a_device(tmp_path):
    _capi()
    from tests.test_headless_cli import EXE, make_data_dir
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    base = [EXE, "-d", str(d), "--buffers", "2", "--out", str(tmp_path / "o.wav")]
    for extra, msg in ((["--pcm16"], "--pcm16 needs --limit"),
                       (["--lookahead", "64"], "belong to --limit"),
                       (["--gain", "2"], "belong to --limit"),
                       (["--limit", "0.7", "--devices", "0,1"], "device group"),
                       (["--limit", "0.7", "--devices", "0"], "device group"),
                       (["--limit", "0"], "ceiling in (0, 1]"),
                       (["--limit", "1.5"], "ceiling in (0, 1]"),
                       (["--limit", "nan"], "ceiling in (0, 1]"),
                       (["--limit", "0.7", "--lookahead", "0"], "--lookahead must be 1 .. 4096"),
                       (["--limit", "0.7", "--lookahead", "4097"], "--lookahead must be 1 .. 4096"),
                       (["--limit", "0.7", "--hold", "-1"], "--hold must be 0 .. 65536"),
                       (["--limit", "0.7", "--gain", "inf"], "--gain must be finite"),
                       (["--limit", "0.7", "--raw", str(tmp_path / "o.f32")], "not with --limit"),
                       (["--limit"], "missing value")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "o.wav").exists()
