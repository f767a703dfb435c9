"""The resampler bus's product boundary, without a GPU: the nine entry points in the header, in capi.EXPORTS and in the built
library; the unchanged ABI version; the stated arithmetic; the meter record; the Python methods; the kernels' resource listing; the
headless tool's refusals; and the prototype design of csrc/resample_clock.h (printed by the check program, which is built with the
host compiler and run as a program of its own) against the same formula in numpy."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from tests import resample_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_resample_enable", "pbso_resample", "pbso_resample_max_out", "pbso_read_resample", "pbso_read_resample_pcm16",
                "pbso_read_resample_meters", "pbso_resample_taps", "pbso_resample_reset", "pbso_resample_info")


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
        assert getattr(lib, name).argtypes, name
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def test_header_states_the_arithmetic():
    hdr = _header()
    for phrase in ("L = rate_out / gcd(rate_in, rate_out), M = rate_in / gcd(rate_in, rate_out)", "both must be <= 4096 and L * T <= 1 << 18",
                   "fc = cutoff * 0.5 / max(L, M)", "g[j] = L * 2 fc * sinc(2 fc x) * I0(beta * sqrt(1 - (2 x / (N - 1))^2)) / I0(beta)",
                   "sinc(a) = sin(pi a) / (pi a), 1 at a = 0", "the window is 1 for N = 1", "until a term is below 1e-17 of the sum",
                   "h[phi][k] = (float)g[k * L + phi]", "i = floor(m * M / L) with phase phi = (m * M) mod L",
                   "m from ceil(t * L / M) to ceil((t + n) * L / M) - 1", "it is 559, then 558",
                   "acc = 0.f; for k = T-1 down to 0: acc = fmaf(h[phi][k], u_c(i - k), acc);   y_c(m) = acc",
                   "nothing split over accumulators", "Subnormals are kept", "delayed by (N - 1) / (2 L)", "last T - 1 input samples",
                   "p0 = m_lo * M - t * L, which lies in [0, M)", "never multiplies an absolute index", "must not overlap d_in",
                   "A refused call changes nothing", "overshoot the limiter's ceiling", "a ceiling with headroom",
                   "(int16_t)lrintf(fminf(fmaxf(y, -1.f), 1.f) * 32767.f)", "A device group\n * has none"):
        assert phrase in hdr, phrase


def test_the_meter_record_is_8_bytes_in_c_and_python():
    capi = _capi()
    assert C.sizeof(capi.ResampleMeter) == 8 and np.dtype(capi.ResampleMeter).itemsize == 8
    assert [(n, getattr(capi.ResampleMeter, n).offset) for n, _ in capi.ResampleMeter._fields_] == [("out_peak", 0), ("n_over", 4)]
    body = re.search(r"typedef struct pbso_resample_meter \{(.*?)\} pbso_resample_meter;", _header(), re.S).group(1)
    assert re.findall(r"^\s*(float|double|int32_t)\s+(\w+);", body, re.M) == [("float", "out_peak"), ("int32_t", "n_over")]
    assert rm.METER_DTYPE == np.dtype(capi.ResampleMeter)


def test_python_methods_exist():
    from openpbso_amd.solver import Engine
    for m in ("resample_enable", "resample", "resample_max_out", "read_resample", "read_resample_pcm16", "read_resample_meters",
              "resample_taps", "resample_reset", "resample_info"):
        assert callable(getattr(Engine, m)), m


def test_kernels_use_no_scratch():
    _capi()
    path = os.path.join(ROOT, "openpbso_amd", "csrc", "kernels_resample.resources.txt")
    if not os.path.exists(path):                         # (a library from another build of the tree: make the listing)
        subprocess.run(["make", "-C", os.path.dirname(path), "kernels_resample.o"], check=True, capture_output=True)
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) >= 4 and sum("resample_kernel" in n for n in names) == 2
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    assert "warning" not in text


def test_headless_refuses_bad_resampler_flags_before_it_needs_a_device(tmp_path):
    _capi()
    from tests.test_headless_cli import EXE, make_data_dir
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    base = [EXE, "-d", str(d), "--buffers", "2", "--out", str(tmp_path / "o.wav")]
    for extra, msg in ((["--rs-taps", "32"], "belong to --out-rate"),
                       (["--rs-beta", "9"], "belong to --out-rate"),
                       (["--rs-cutoff", "0.9"], "belong to --out-rate"),
                       (["--out-rate", "44101"], "must be <= 4096"),                     # L = 44101
                       (["--out-rate", "7"], "must be <= 4096"),                         # M = 44100
                       (["--out-rate", "0"], "must be positive"),
                       (["--out-rate", "48000", "--rs-taps", "0"], "taps must be 1 .. 256"),
                       (["--out-rate", "48000", "--rs-taps", "257"], "taps must be 1 .. 256"),
                       (["--out-rate", "48000", "--rs-beta", "21"], "0 <= beta <= 20"),
                       (["--out-rate", "48000", "--rs-cutoff", "0"], "0 < cutoff <= 1"),
                       (["--out-rate", "48000", "--rs-cutoff", "nan"], "0 < cutoff <= 1"),
                       (["--out-rate", "48000", "--devices", "0,1"], "device group"),
                       (["--out-rate", "48000", "--devices", "0"], "device group"),
                       (["--out-rate", "48000", "--raw", str(tmp_path / "o.f32")], "not with --out-rate"),
                       (["--out-rate", "48000", "--pcm16"], "--pcm16 needs --limit"),
                       (["--out-rate"], "missing value")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "o.wav").exists()


def _stopband_peak_db(g, L, M):
    """the peak of |G(f)| / L from 1.1 x Nyquist (of the lower rate) on, in dB; f in cycles per sample of the rate L x rate_in"""
    n_fft = 1 << 18
    mag = np.abs(np.fft.rfft(np.asarray(g, dtype=np.float64), n_fft)) / L
    f = np.arange(mag.size) / n_fft
    return 20.0 * np.log10(mag[f >= 1.1 * 0.5 / max(L, M)].max())


def test_the_design_of_the_clock_header_is_the_formula():
    """160 / 147 at T = 32, beta 9, cutoff 0.9: every tap within one f32 ulp or 1e-12 of numpy's (hosts' sin differ in the last fp64
    bit), and the stopband of the f32 table no more than 1 dB above that of the fp64 design (-92 dB; the rounding of 5120 taps to
    f32 lies near -120 dB, so 1 dB is generous and still catches a wrong window or cutoff)"""
    csrc = os.path.join(ROOT, "openpbso_amd", "csrc")
    b = subprocess.run(["make", "-C", csrc, "resample_clock_check"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([os.path.join(ROOT, "openpbso_amd", "resample_clock_check"), "design", "44100", "48000", "32", "9", "0.9"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split()
    L, M, T = (int(x) for x in lines[:3])
    assert (L, M, T) == (160, 147, 32) and len(lines) == 3 + L * T
    h = np.array([int(x, 16) for x in lines[3:]], dtype=np.uint32).view(np.float32).reshape(L, T)
    g64 = rm.prototype(L, M, T, 9.0, 0.9)
    want = rm.design(L, M, T, 9.0, 0.9, dtype=np.float64)
    assert np.array_equal(want, g64.reshape(T, L).T)
    err = np.abs(h.astype(np.float64) - want)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert ((err <= ulp) | (err <= 1e-12)).all(), (err / ulp).max()
    g32 = h.T.reshape(-1)                                # g[k L + phi] = h[phi][k]
    sb64, sb32 = _stopband_peak_db(g64, L, M), _stopband_peak_db(g32, L, M)
    print(f"stopband peak: fp64 design {sb64:.2f} dB, f32 table {sb32:.2f} dB")
    assert sb64 < -85.0 and sb32 <= sb64 + 1.0, (sb64, sb32)
    # the passband: unity at DC, through every phase
    assert abs(np.abs(np.fft.rfft(g32.astype(np.float64), 1 << 18))[0] / L - 1.0) < 1e-4
