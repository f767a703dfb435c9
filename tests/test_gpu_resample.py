"""The resampler bus (include/openpbso_amd.h "resampler bus"; kernels_resample.hip) on the device.  Every output is compared BIT FOR
BIT with the reference of the stated arithmetic (tests/cpp/resample_ref.c through tests/resample_model.py, anchored by
tests/test_resample_model.py); the taps are the engine's own, read back with resample_taps(), so nothing here depends on a sin.
The engine behind it is one object of 64 modes: the stage does not care what made its input."""
import ctypes as C

import numpy as np
import pytest
import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from tests import resample_model as rm
from tests.resample_model import Model, ceil_div, pcm16

pytestmark = pytest.mark.gpu
PATTERN = np.float32(-7.5)


def make_engine(n_obj=1, n_modes=64, nb_total=4, seed=1, **kw):
    eng = Engine(**kw)
    for i in range(n_obj):
        eng.add_object(synth.eigenvalues(n_modes, 9000 + 131 * seed + i), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    rng = np.random.default_rng(seed)
    for i in range(n_obj):
        eng.set_use_transfer(i, False)
        for t in [0] + sorted(int(x) for x in rng.integers(1, max(nb_total, 2), 2)):
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(n_modes) * 1e-3), t)
    return eng


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    return t


def signal(rng, rows, n, scale=1.0):
    return (rng.standard_normal((rows, n)) * scale).astype(np.float32)


def same_bits(got, want, label):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (label, bad.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def same_meters(got, want, label):
    same_bits(np.ascontiguousarray(got["out_peak"]), np.ascontiguousarray(want["out_peak"]), (label, "out_peak"))
    assert np.array_equal(got["n_over"], want["n_over"]), (label, got["n_over"], want["n_over"])


def run(eng, model, x, cuts, label):
    """x [C][n] through the engine and the model in steps of cuts[i] buffers; every step's output, count and meters compared"""
    outs, at, B = [], 0, eng.B
    for k, nb in enumerate(cuts):
        part = x[:, at * B:(at + nb) * B]
        dx = device(part)
        eng.step(nb)
        want_n = model.n_out(nb * B)
        n_out = eng.resample(dx.data_ptr())
        assert n_out == want_n <= eng.resample_max_out(nb) == ceil_div(nb * B * model.L, model.M), (label, k, n_out, want_n)
        got = eng.read_resample()
        same_bits(got, model.process(part), (label, k))
        same_meters(eng.read_resample_meters(), model.meters, (label, k))
        i = eng.resample_info()
        assert (i["t"], i["m"], i["n_out"]) == (model.t, model.m, n_out), (label, k, i)
        outs.append(got)
        at += nb
    return np.concatenate(outs, axis=1)


def enable(eng, Cn, rate_out, T, **kw):
    """enable and a model with the engine's own taps"""
    eng.resample_enable(rate_out, Cn, T, **kw)
    i = eng.resample_info()
    L, M = rm.ratio(eng.sample_rate, rate_out)
    assert (i["L"], i["M"], i["T"], i["delay_num"], i["t"], i["m"], i["calls"]) == (L, M, T, L * T - 1, 0, 0, 0)
    h = eng.resample_taps()
    assert h.shape == (L, T)
    return Model(Cn, L, M, h)


# (rate_in, rate_out): 160 / 147, 320 / 147, 1 / 2, 147 / 160 (an engine at 48000), 1 / 1
RATES = [(44100, 48000), (44100, 96000), (44100, 22050), (48000, 44100), (44100, 44100)]


@pytest.mark.parametrize("Cn", [1, 3, 8])
@pytest.mark.parametrize("rates", RATES)
def test_ratios_channels_and_taps(rates, Cn):
    """every T on one engine (a new enable replaces the stage): a step of one buffer, then one of two"""
    rate_in, rate_out = rates
    rng = np.random.default_rng(rate_out + Cn)
    eng = make_engine(sample_rate=0 if rate_in == 44100 else rate_in)
    try:
        assert eng.sample_rate == rate_in
        for T in (1, 2, 7, 32, 256):
            model = enable(eng, Cn, rate_out, T)
            y = run(eng, model, signal(rng, Cn, 3 * eng.B), [1, 2], (rates, Cn, T))
            assert y.shape == (Cn, ceil_div(3 * eng.B * model.L, model.M)) and np.abs(y).max() > 0
    finally:
        eng.close()


def test_the_largest_table():
    """L = 4096 (45045 -> 45056 Hz), T = 64: 1 << 18 taps, 1 MB; one more tap per phase is refused and leaves the stage as it was"""
    rng = np.random.default_rng(5)
    eng = make_engine(sample_rate=45045)
    try:
        model = enable(eng, 2, 45056, 64)
        assert (model.L, model.M) == (4096, 4095)
        x = signal(rng, 2, 3 * eng.B)
        run(eng, model, x[:, :eng.B], [1], "L = 4096, first")
        before = eng.resample_info()
        with pytest.raises(PbsoError) as ei:
            eng.resample_enable(45056, 2, 65)
        assert ei.value.status == capi.ERR_INVALID and eng.resample_info() == before
        run(eng, model, x[:, eng.B:], [2], "L = 4096, behind the refusal")
    finally:
        eng.close()


@pytest.mark.parametrize("rates", [(44100, 48000), (44100, 22050)])
def test_the_cut_into_steps_does_not_matter(rates):
    rng = np.random.default_rng(6)
    outs = []
    x = signal(rng, 2, 7 * 513)
    for cuts in ([1, 1, 3, 2], [7]):
        eng = make_engine()
        try:
            model = enable(eng, 2, rates[1], 32)
            outs.append(run(eng, model, x, cuts, (rates, cuts)))
        finally:
            eng.close()
    same_bits(outs[0], outs[1], "1 + 1 + 3 + 2 against 7")


@pytest.mark.parametrize("T", [64, 256])
def test_a_history_longer_than_the_steps(T):
    """an engine of 27 frames: T - 1 samples of history against steps of 27 and 54"""
    rng = np.random.default_rng(T)
    x = signal(rng, 3, 12 * 27)
    outs = []
    for cuts in ([1] * 12, [12], [2, 1, 2, 7]):
        eng = make_engine(frames_per_buffer=27)
        try:
            assert eng.B == 27
            outs.append(run(eng, enable(eng, 3, 48000, T), x, cuts, (T, cuts)))
        finally:
            eng.close()
    same_bits(outs[1], outs[0], "12 against 12 x 1")
    same_bits(outs[2], outs[0], "2 + 1 + 2 + 7 against 12 x 1")


def test_a_ratio_whose_window_does_not_fit_in_lds():
    """M / L = 4095 (45045 -> 11 Hz): 256 outputs span a million input samples, which the kernel reads from memory; most calls
    of one buffer have no output at all"""
    rng = np.random.default_rng(11)
    eng = make_engine(sample_rate=45045)
    try:
        model = enable(eng, 2, 11, 8)
        assert (model.L, model.M) == (1, 4095)
        x = signal(rng, 2, 20 * eng.B)
        y = run(eng, model, x, [1, 1, 2, 16], "1 / 4095")
        assert y.shape == (2, ceil_div(20 * eng.B, 4095)) and y.shape[1] == 3
    finally:
        eng.close()


def test_a_stride_beyond_n_out_read_twice_pcm16_and_meters():
    rng = np.random.default_rng(8)
    Cn, nb = 3, 2
    eng = make_engine()
    try:
        model = enable(eng, Cn, 48000, 32)
        n = nb * eng.B
        x = signal(rng, Cn, 3 * n, 0.2)
        x[:, n:2 * n] *= 8.0                                         # the second step overshoots full scale
        x[0, 2 * n:] = 1e-41                                         # the third: subnormals on channel 0, silence on 1, -0.f on 2
        x[1, 2 * n:] = 0.0
        x[2, 2 * n:] = -0.0
        stride = eng.resample_max_out(nb) + 37
        out = torch.full((Cn, stride), float(PATTERN), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        dx = device(x[:, :n])
        eng.step(nb)
        k = eng.resample(dx.data_ptr(), out.data_ptr(), stride)
        eng.sync()
        want = model.process(x[:, :n])
        got = out.cpu().numpy()
        same_bits(got[:, :k], want, "caller's buffer")
        assert (got[:, k:] == PATTERN).all()                         # the words behind n_out are untouched
        same_bits(eng.read_resample(), want, "read from the caller's buffer")
        assert np.array_equal(eng.read_resample_pcm16(), pcm16(want))
        same_meters(eng.read_resample_meters(), model.meters, "meters")
        assert (model.meters["n_over"] == 0).all() and np.array_equal(dx.cpu().numpy(), x[:, :n])    # (d_in is read only)
        # engine-owned, read twice; saturation
        dx = device(x[:, n:2 * n])
        eng.step(nb)
        k = eng.resample(dx.data_ptr())
        want = model.process(x[:, n:2 * n])
        same_bits(eng.read_resample(), want, "engine-owned")
        same_bits(eng.read_resample(), want, "read twice")
        p = eng.read_resample_pcm16()
        assert p.shape == (k, Cn) and np.array_equal(p, pcm16(want)) and p.max() == 32767 and p.min() == -32767
        m = eng.read_resample_meters()
        same_meters(m, model.meters, "meters of the loud step")
        assert (m["n_over"] > 0).all() and (m["out_peak"] > 1).all()
        assert np.array_equal(m["n_over"], (np.abs(want) > 1).sum(axis=1)) and np.array_equal(m["out_peak"], np.abs(want).max(axis=1))
        # subnormals are kept (behind the history of the loud step has left the taps)
        dx = device(x[:, 2 * n:])
        eng.step(nb)
        eng.resample(dx.data_ptr())
        want = model.process(x[:, 2 * n:])
        got = eng.read_resample()
        same_bits(got, want, "subnormals")
        tail = got[0, 40:]
        assert (tail != 0).any() and (np.abs(tail) < np.finfo(np.float32).tiny).all()
        same_meters(eng.read_resample_meters(), model.meters, "meters of the quiet step")
        assert np.array_equal(eng.read_resample_pcm16(), pcm16(want))
    finally:
        eng.close()


def test_refusals_leave_the_state_as_it_was_and_the_reset():
    rng = np.random.default_rng(9)
    eng = Engine()
    try:
        eng.add_object(synth.eigenvalues(32, 40), synth.RHO, synth.ALPHA, synth.BETA)
        with pytest.raises(PbsoError) as ei:
            eng.resample_enable(48000, 2)                            # before finalize
        assert ei.value.status == capi.ERR_STATE
        eng.finalize()
        lib, fp = capi.lib(), C.POINTER(C.c_float)
        nb = 2
        n = nb * eng.B
        x = signal(rng, 2, n)
        dx = device(x)
        for call in (lambda: eng.resample(dx.data_ptr()), eng.resample_reset, eng.resample_info, lambda: eng.resample_max_out(1)):
            with pytest.raises(PbsoError) as ei:
                call()                                               # not enabled
            assert ei.value.status == capi.ERR_STATE
        for bad in ((48000, 0), (48000, 9), (48000, 2, 0), (48000, 2, 257), (0, 2), (-48000, 2), (44101, 2), (48000, 2, 32, -1.0),
                    (48000, 2, 32, 20.5), (48000, 2, 32, float("nan")), (48000, 2, 32, 9.0, 0.0), (48000, 2, 32, 9.0, 1.5),
                    (48000, 2, 32, 9.0, float("inf")), (44100 * 4096, 2, 65)):
            with pytest.raises(PbsoError) as ei:
                eng.resample_enable(*bad)
            assert ei.value.status == capi.ERR_INVALID, bad
        model = enable(eng, 2, 48000, 32)
        stride = eng.resample_max_out(nb)
        out = torch.zeros((2, stride), dtype=torch.float32, device="cuda")
        both = torch.zeros(2 * n + 2 * stride, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def refused(call, status):
            before = eng.resample_info()
            with pytest.raises(PbsoError) as ei:
                call()
            assert ei.value.status == status and eng.resample_info() == before

        refused(lambda: eng.resample(dx.data_ptr()), capi.ERR_STATE)                                  # no step since enable
        host = np.empty(2 * stride, dtype=np.float32)
        assert lib.pbso_read_resample(eng._h, host.ctypes.data_as(fp), host.size) == capi.ERR_STATE   # nothing processed yet
        eng.step(nb)
        before = eng.resample_info()
        assert lib.pbso_resample(eng._h, None, None, 0, None) == capi.ERR_INVALID and eng.resample_info() == before   # NULL d_in
        refused(lambda: eng.resample(dx.data_ptr(), out.data_ptr(), stride - 1), capi.ERR_INVALID)    # a stride that is too small
        refused(lambda: eng.resample(dx.data_ptr(), out.data_ptr(), 0), capi.ERR_INVALID)
        refused(lambda: eng.resample(dx.data_ptr(), out.data_ptr(), (1 << 40) + 1), capi.ERR_INVALID)   # ... or absurd
        refused(lambda: eng.resample(both.data_ptr(), both.data_ptr(), stride), capi.ERR_INVALID)     # d_out == d_in
        refused(lambda: eng.resample(both.data_ptr(), both.data_ptr() + 4 * (2 * n - 1), stride), capi.ERR_INVALID)   # the last word of d_in
        refused(lambda: eng.resample(both.data_ptr() + 4 * (2 * stride - 1), both.data_ptr(), stride), capi.ERR_INVALID)
        k = eng.resample(dx.data_ptr(), out.data_ptr(), stride)      # (the refusals did not use the step up)
        eng.sync()
        want = model.process(x)
        same_bits(out.cpu().numpy()[:, :k], want, "first step")
        big = np.empty(2 * k + 1, dtype=np.float32)
        assert lib.pbso_read_resample(eng._h, big.ctypes.data_as(fp), big.size) == capi.ERR_INVALID
        assert lib.pbso_resample_taps(eng._h, big.ctypes.data_as(fp), 160 * 32 - 1) == capi.ERR_INVALID
        rec = (capi.ResampleMeter * 3)()
        assert lib.pbso_read_resample_meters(eng._h, rec, 3) == capi.ERR_INVALID
        refused(lambda: eng.resample(dx.data_ptr()), capi.ERR_STATE)                                  # the same step twice
        same_bits(eng.read_resample(), want, "the refusal left the last output readable")
        eng.step(nb)
        eng.step(nb)
        refused(lambda: eng.resample(dx.data_ptr()), capi.ERR_STATE)                                  # a step was skipped
        # the reset in the middle: the history gone, t = m = p0 = 0
        eng.resample_reset()
        model.reset()
        i = eng.resample_info()
        assert (i["t"], i["m"]) == (0, 0)
        refused(lambda: eng.resample(dx.data_ptr()), capi.ERR_STATE)                                  # armed for the NEXT step
        eng.step(nb)
        assert eng.resample(dx.data_ptr()) == k
        want2 = model.process(x)
        same_bits(eng.read_resample(), want2, "after the reset")
        same_bits(want2, want, "the reset is a fresh start")
        host_buf = eng.host_buffer(nb)                               # a step to host memory: the input is the caller's buffer
        eng.step_to_host(nb, host_buf)
        eng.host_wait()
        eng.resample(dx.data_ptr())
        same_bits(eng.read_resample(), model.process(x), "after a host step")
    finally:
        eng.close()


def test_chain_of_scene_mix_master_and_resample_on_real_audio():
    """4 objects -> scene_mix (C = 2) -> master -> resample at 160 / 147, bit for bit against the three models in a row"""
    from tests.master_model import Model as MasterModel
    from tests.scene_mix_model import Model as MixModel
    n_obj, nb, Cn, T = 4, 2, 2, 0.5
    rng = np.random.default_rng(10)
    eng = make_engine(n_obj, 64, 3 * nb, 6)
    try:
        g, d = rng.uniform(-1, 1, (Cn, n_obj)), rng.uniform(0, 100, (Cn, n_obj))
        eng.scene_mix_enable(Cn, 100, 0)
        eng.scene_mix_set(g, d)
        mix = MixModel(Cn, n_obj, 100, 0)
        mix.set(g, d)
        n = nb * eng.B
        bus = torch.zeros((Cn, n), dtype=torch.float32, device="cuda")
        lim = torch.zeros((Cn, n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        master = rs = None
        for k in range(3):
            eng.step(nb)
            rows = eng.audio()
            eng.scene_mix(bus.data_ptr())
            u = mix.mix(rows)
            same_bits(eng.read_scene_mix(), u, ("mix", k))
            if master is None:
                # enabled behind the first step: armed for the next one; that step's peak would land at 50 T
                gain = float(np.float32(50 * T / float(np.abs(u).max())))
                eng.master_enable(Cn, T, 64, 32, 0)
                eng.master_set_gain(gain)
                master = MasterModel(Cn, T, 64, 32, 0, eng.master_window())
                master.set_gain(gain)
                rs = enable(eng, Cn, 48000, 32)
                continue
            eng.master(bus.data_ptr(), lim.data_ptr())
            v = master.process(u)
            same_bits(eng.read_master(), v, ("master", k))
            n_out = eng.resample(lim.data_ptr())
            want = rs.process(v)
            got = eng.read_resample()
            assert n_out == want.shape[1]
            same_bits(got, want, ("resample", k))
            same_meters(eng.read_resample_meters(), rs.meters, ("chain", k))
            assert np.abs(got).max() > 0.25                          # (limited audio, not silence; it may overshoot T between samples)
            same_bits(eng.read_master(), v, "the bus is read only")
    finally:
        eng.close()
