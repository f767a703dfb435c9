"""The reference of the loudness bus's tests (tests/loudness_model.py around tests/cpp/loudness_ref.c) anchored independently, without
a GPU: its energies against the plain serial fp64 recurrence and numpy.sum; its report against pbso_loudness_report_from_blocks; the
known answers of EBU Tech 3341 (cases 1, 3, 4, 5 on synthesised stereo 1 kHz sines at full length, each within the document's
+-0.1 LU), the 997 Hz full-scale sine of BS.1770, and the true peak of 0.5-amplitude sines within Tech 3341's +0.2 / -0.4 dB."""
import math
import os

import numpy as np
import pytest

from tests import loudness_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _capi():
    from openpbso_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi


def sine(rate, seconds, freq, dbfs, phase_deg=0.0):
    n = int(round(rate * seconds))
    t = np.arange(n, dtype=np.float64)
    return (10.0 ** (dbfs / 20.0) * np.sin(2.0 * np.pi * freq * t / rate + np.deg2rad(phase_deg))).astype(np.float32)


def stereo_programme(rate, parts):
    """parts: (seconds, dBFS) of a 1 kHz sine, the same on both channels, phase-continuous"""
    n = [int(round(rate * s)) for s, _ in parts]
    t = np.arange(sum(n), dtype=np.float64)
    amp = np.concatenate([np.full(k, 10.0 ** (db / 20.0)) for k, (_, db) in zip(n, parts)])
    x = (amp * np.sin(2.0 * np.pi * 1000.0 * t / rate)).astype(np.float32)
    return np.stack([x, x])


def measure(rate, x, true_peak=False, step=None):
    m = lm.Model(rate, x.shape[0], true_peak=true_peak)
    step = x.shape[1] if step is None else step
    for at in range(0, x.shape[1], step):
        m.process(x[:, at:at + step])
    return m


def test_the_design_is_the_standards_table_at_48_kHz():
    want = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585],
                     [1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621]])
    assert np.abs(lm.design(48000) - want).max() < 1e-12


@pytest.mark.parametrize("rate", [44100, 48000, 22050, 96000])
def test_energies_against_the_serial_recurrence(rate):
    """signals whose rms is within 20 dB of peak: the block form is within 1e-9 of peak of the serial recurrence (the header's
    bound), which is about 4e-8 dB in a sub-block's energy; 1e-6 LU holds that with a 25x margin"""
    rng = np.random.default_rng(rate)
    n = 12 * lm.hop(rate) + 77
    noise = rng.standard_normal(n) * 0.2
    tone = 0.7 * np.sin(2 * np.pi * 63.0 * np.arange(n) / rate) + 0.1 * rng.standard_normal(n)
    x = np.stack([noise, tone]).astype(np.float32)
    for v in x:
        assert 20 * math.log10(np.sqrt(np.mean(v.astype(np.float64) ** 2)) / np.abs(v).max()) > -20.0
    m = measure(rate, x, step=513 * 7)
    hs = lm.hop(rate)
    assert m.records.shape == (12, 2)
    sos = lm.design(rate)
    for c in range(2):
        z = lm.serial(sos, x[c].astype(np.float64))
        for j in range(12):
            want = np.sum(z[j * hs:(j + 1) * hs] ** 2)
            got = m.records["energy"][j, c]
            assert abs(10 * math.log10(got / want)) < 1e-6, (rate, c, j, got, want)


def test_the_cut_into_steps_does_not_matter_to_the_model():
    rng = np.random.default_rng(3)
    rate = 22050
    x = (rng.standard_normal((3, 5 * 2205 + 100)) * 0.3).astype(np.float32)
    a, b, c = measure(rate, x, True), measure(rate, x, True, step=513), measure(rate, x, True, step=2205)
    assert a.records.shape == (5, 3)
    assert a.records.tobytes() == b.records.tobytes() == c.records.tobytes()
    assert (a.records["true_peak"] >= a.records["sample_peak"] * 0.5).all() and (a.records["sample_peak"] > 0).all()


@pytest.mark.parametrize("weight", [None, [1.0, 1.0, 1.41], [0.0, 1.0, 0.5]])
def test_the_models_report_is_the_librarys(weight):
    capi = _capi()
    rng = np.random.default_rng(8)
    rate, hs = 44100, 4410
    # 6 s in three levels, the quiet one below the relative gate, with silence at the end: every gate takes part
    level = np.repeat([0.3, 0.001, 0.1, 0.0], [20, 15, 20, 5])
    x = (rng.standard_normal((3, level.size * hs)) * np.repeat(level, hs)).astype(np.float32)
    m = lm.Model(rate, 3, weight=weight, true_peak=True)
    m.process(x)
    want = m.report()
    got = capi.loudness_report_from_blocks(m.records, hs, weight)
    assert got["n_blocks"] == want["n_blocks"] == 60 and got["n_gated"] == want["n_gated"] and 0 < got["n_gated"] < 57
    for k in ("integrated", "momentary", "short_term", "max_momentary", "max_short_term", "relative_threshold"):
        assert math.isfinite(want[k]) and abs(got[k] - want[k]) < 1e-9, (k, got[k], want[k])
    assert want["momentary"] < -70.0 < want["relative_threshold"]      # only the filters' tails in the four sub-blocks at the end
    assert got["true_peak"] == want["true_peak"] and got["sample_peak"] == want["sample_peak"] == float(np.abs(x[:, :55 * hs]).max())
    # too few blocks
    short = capi.loudness_report_from_blocks(m.records[:3], hs, weight)
    assert short["integrated"] == short["momentary"] == short["short_term"] == short["relative_threshold"] == -math.inf and short["n_gated"] == 0
    assert capi.loudness_report_from_blocks(m.records[:29], hs, weight)["short_term"] == -math.inf
    assert math.isfinite(capi.loudness_report_from_blocks(m.records[:30], hs, weight)["short_term"])


# EBU Tech 3341, table 1: (case, the programme, the target); stereo 1 kHz sines
EBU = [(1, [(20.0, -23.0)], -23.0),
       (3, [(10.0, -36.0), (60.0, -23.0), (10.0, -36.0)], -23.0),
       (4, [(10.0, -72.0), (10.0, -36.0), (60.0, -23.0), (10.0, -36.0), (10.0, -72.0)], -23.0),
       (5, [(20.0, -26.0), (20.1, -20.0), (20.0, -26.0)], -23.0)]
# the numpy values of this design, 44100 and 48000 Hz
EXPECTED = {1: (-22.9905, -22.9933), 3: (-23.0111, -23.0139), 4: (-23.0111, -23.0139), 5: (-22.9759, -22.9787)}


@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("case", EBU, ids=[f"case{c[0]}" for c in EBU])
def test_ebu_tech_3341_known_answers(case, rate):
    number, parts, target = case
    m = measure(rate, stereo_programme(rate, parts), step=rate * 10)
    got = m.report()["integrated"]
    print(f"case {number} at {rate} Hz: integrated {got:.4f} LUFS (expected {EXPECTED[number][rate == 48000]})")
    assert abs(got - target) <= 0.1, (number, rate, got)


@pytest.mark.parametrize("rate", [44100, 48000])
def test_a_full_scale_997_Hz_sine_is_minus_3_01(rate):
    m = measure(rate, sine(rate, 5.0, 997.0, 0.0)[None])
    got = m.report()["integrated"]
    print(f"997 Hz 0 dBFS mono at {rate} Hz: {got:.4f} LUFS")
    assert abs(got + 3.01) <= 0.1, got


@pytest.mark.parametrize("divisor,phase", [(4, 0.0), (4, 45.0), (6, 30.0), (8, 22.5)])
def test_true_peak_of_half_scale_sines(divisor, phase):
    rate = 44100
    m = measure(rate, sine(rate, 1.0, rate / divisor, 20 * math.log10(0.5), phase)[None], true_peak=True)
    r = m.report()
    dbtp = 20 * math.log10(r["true_peak"])
    print(f"fs/{divisor} at {phase} degrees: {dbtp:.3f} dBTP, sample peak {20 * math.log10(r['sample_peak']):.3f} dBFS")
    assert -6.02 - 0.4 <= dbtp <= -6.02 + 0.2, dbtp
