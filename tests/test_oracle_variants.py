"""The oracle compiled for another buffer length / sample rate (oracle_py.lib(frames=, rate=)) anchored before anything is
compared with it (no GPU): the 513 / 44100 variant is the default library bit for bit, a variant's impulse response is the closed
form at its own h, its Gaussian is as wide as its rate says, and what it computes does not depend on the buffer length."""
import math

import numpy as np
import pytest

from openpbso_amd import synth
from oracle import oracle_py as orc
from tests.scenarios import ObjSpec, _oracle_one, force_ev, run_oracle

VARIANTS = [(270, 48000), (864, 96000)]


def _scripted_scene():
    """one object with FFAT maps: all three force types, two messages stamped for one buffer, a sustained stroke with a parameter
    change, a clearAllForces hole and a listener move"""
    n = 37
    lam = synth.eigenvalues(n, 11)
    rng = np.random.default_rng(5)
    d = [rng.standard_normal(n) * 1e-3 for _ in range(8)]
    o = ObjSpec(lam, maps=synth.ffat_maps(lam, 12, dim=4))
    evs = [force_ev(0, 0, data=d[0]),
           force_ev(1, 0, data=d[1], force_type=1, width=3000.0),
           force_ev(1, 0, data=d[2]),
           dict(t=2, obj=0, kind="listener", pos=np.array([0.4, -0.7, 0.9])),
           force_ev(3, 0, data=d[3], force_type=2),
           force_ev(5, 0, clear=True),
           force_ev(6, 0, data=d[4], force_type=2, start=True),
           dict(t=7, obj=0, kind="arprm", a=[0.6, 0.1], sigma=2e-3, mu=0.2),
           force_ev(8, 0, data=d[5], force_type=2),
           force_ev(9, 0, force_type=2, end=True),
           force_ev(10, 0, data=d[6], force_type=1, width=60.0)]
    return o, evs, 12


def test_default_pair_built_as_a_variant_is_the_default_library_bit_for_bit():
    d, v = orc.lib(), orc.lib(frames=513, rate=44100)
    assert d is not v and (d.B, d.rate) == (v.B, v.rate) == (513, 44100) and d.h == v.h == 1.0 / 44100
    o, evs, nb = _scripted_scene()
    a = _oracle_one(0, o, evs, nb, d)
    b = _oracle_one(0, o, evs, nb, v)
    assert not a[1].all() and a[1].any()                      # the hole is there, and so is sound
    assert np.abs(a[0]).max() > 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2].keys() == b[2].keys() and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3])) and np.array_equal(a[4], b[4])
    # and run_oracle's default call still is the default library
    w = run_oracle([o], evs, nb)
    assert np.array_equal(w["audio"][0], a[0])


def _one_mode(freq, rate):
    """(c1, c2, c3, eps, theta) of one mode from alpha, beta, lambda, rho and h = 1 / rate, in Python floats
    (modal_integrator.h:63-99)"""
    h = 1.0 / rate
    lam = synth.RHO * (2 * math.pi * freq) ** 2
    omega0 = math.sqrt(lam / synth.RHO)
    xi = 0.5 * (synth.ALPHA / omega0 + synth.BETA * omega0)
    a, b = 2.0 * xi * omega0, omega0 ** 2
    eps = math.exp(-a / 2 * h)
    theta = h * math.sqrt(b - a * a / 4.0)
    gamma = math.asin(a / (2.0 * math.sqrt(b)))
    c3 = 2.0 * (eps * math.cos(theta + gamma) - eps ** 2 * math.cos(2.0 * theta + gamma))
    c3 = c3 / (3.0 * math.sqrt(b) * math.sqrt(b - a * a / 4.0)) * 1e9
    return lam, c3, eps, theta


@pytest.mark.parametrize("frames,rate", VARIANTS)
def test_variant_impulse_response_is_the_closed_form_at_its_rate(frames, rate):
    """q_k = c3 eps^k sin((k + 1) theta) / sin(theta) with eps and theta from h = 1 / rate; three buffers of one 6 kHz mode"""
    l = orc.lib(frames=frames, rate=rate)
    assert (l.B, l.rate, l.h) == (frames, rate, 1.0 / rate)
    lam, c3, eps, theta = _one_mode(6000.0, rate)
    s = orc.Solver(np.array([lam]), synth.RHO, synth.ALPHA, synth.BETA, l=l)
    s.set_use_transfer(False)
    assert s.enqueue_force(np.array([1.0]), orc.make_force(orc.POINT, l=l))
    got = np.concatenate([s.step()[0] for _ in range(3)])
    assert got.size == 3 * frames
    k = np.arange(3 * frames, dtype=np.float64)
    want = 1e7 * (c3 * eps ** k * np.sin((k + 1.0) * theta) / math.sin(theta))     # (unit transfer: 1e7)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{frames} / {rate}: max |oracle - closed form| / peak = {err:.3e}")
    assert err <= 1e-12
    # the same mode at the default rate is another signal: the variant really uses its own h
    d = orc.Solver(np.array([lam]), synth.RHO, synth.ALPHA, synth.BETA)
    d.set_use_transfer(False)
    d.enqueue_force(np.array([1.0]), orc.make_force(orc.POINT))
    assert np.abs(d.step()[0][:27] - got[:27]).max() > 1e-3 * np.abs(want).max()


@pytest.mark.parametrize("frames,rate", VARIANTS + [(27, 44100), (513, 22050)])
@pytest.mark.parametrize("width_us", [5.0, 60.0, 400.0, 2500.0, 9000.0])
def test_variant_gaussian_width_in_samples(frames, rate, width_us):
    l = orc.lib(frames=frames, rate=rate)
    f = orc.make_force(orc.GAUSSIAN, width_us, l)
    ws = max(1, int(width_us * 1e-6 * rate))
    assert ws == max(1, int(width_us / 1000000. * rate))      # (the widths used here round the same either way)
    assert f.width_samples == ws and f.center == int(4.5 * ws)
    # and the profile it adds: frames samples per call, alive for 10 widths
    total = np.zeros(0)
    buf = np.zeros(frames)
    calls = 0
    while orc.force_add(f, buf):
        total = np.concatenate([total, buf])
        buf = np.zeros(frames)
        calls += 1
    assert calls == -(-10 * ws // frames)
    i = np.arange(total.size)
    assert np.allclose(total, np.exp(-0.5 * ((i - int(4.5 * ws)) / ws) ** 2), rtol=1e-15, atol=0)


@pytest.mark.parametrize("rate", [44100, 48000, 96000])
def test_variant_output_does_not_depend_on_the_buffer_length(rate):
    """one point force at sample 0 of buffer 0, five modes and unit transfer: 27, 270 and 864 frames per step give one fp64 stream"""
    lam = synth.eigenvalues(5, 21, f_hi=9000.0)
    S = np.random.default_rng(2).standard_normal(5) * 1e-3
    total = 2 * 864
    streams = []
    for frames in (27, 270, 864):
        l = orc.lib(frames=frames, rate=rate)
        s = orc.Solver(lam, synth.RHO, synth.ALPHA, synth.BETA, l=l)
        s.set_use_transfer(False)
        assert s.enqueue_force(S, orc.make_force(orc.POINT, l=l))
        n = -(-total // frames)
        streams.append(np.concatenate([s.step()[0] for _ in range(n)])[:total])
    assert np.abs(streams[0]).max() > 0
    assert np.array_equal(streams[0], streams[1]) and np.array_equal(streams[0], streams[2])
