"""The master bus (include/openpbso_amd.h "master bus"; kernels_master.hip) on the device: the ramped gain, the look-ahead limiter,
the meters and the 16-bit PCM.  Every output is compared BIT FOR BIT with the reference of the stated order of arithmetic
(tests/cpp/master_ref.c through tests/master_model.py, anchored by tests/test_master_model.py) unless noted.  The engine behind it
is one object of 64 modes unless a test is about the engine: the stage does not care what made its input."""
import ctypes as C

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from tests.master_model import Model, pcm16, window

pytestmark = pytest.mark.gpu
B = 513


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
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    return t


def signal(rng, rows, nb, scale=1.0):
    return (rng.standard_normal((rows, nb * B)) * scale).astype(np.float32)


def same_bits(got, want, label):
    assert got.shape == want.shape, label
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (label, bad.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def same_meters(got, want, label):
    for f in ("in_peak", "out_peak", "min_gain"):
        same_bits(np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f]), (label, f))
    assert np.array_equal(got["n_limited"], want["n_limited"]), label
    # any order of 513 non-negative fp64 terms is within 512 * 2^-53 of exact: two orders differ by at most 1.2e-13 relative
    assert (np.abs(got["sumsq"] - want["sumsq"]) <= 1e-12 * want["sumsq"]).all(), label


def run(eng, model, x, cuts, label, meters=True):
    """x [C][n] through the engine and the model in steps of cuts[i] buffers; every step's output and meters compared"""
    outs, at = [], 0
    for k, nb in enumerate(cuts):
        part = x[:, at * B:(at + nb) * B]
        dx = device(part)
        eng.step(nb)
        eng.master(dx.data_ptr())
        got = eng.read_master()
        same_bits(got, model.process(part), (label, k))
        if meters:
            same_meters(eng.read_master_meters(), model.meters, (label, k))
        outs.append(got)
        at += nb
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("L", [1, 64, 65])
def test_unlimited_input_comes_out_delayed_bit_for_bit(L):
    """T = 1 and |u| < 1: the output is the input L samples late, -0.f and subnormals included"""
    rng = np.random.default_rng(L)
    x = rng.uniform(-0.999, 0.999, (2, 3 * B)).astype(np.float32)
    x[0, 5], x[1, 700], x[0, 9], x[1, 10] = -0.0, -0.0, 1e-41, -3e-39
    eng = make_engine()
    try:
        eng.master_enable(2, 1.0, L, 0, 0)
        y = run(eng, Model(2, 1.0, L, 0, 0), x, [1, 2], L)
        want = np.concatenate([np.zeros((2, L), dtype=np.float32), x[:, :-L]], axis=1)
        same_bits(y, want, "delayed input")
        assert np.signbit(y[0, 5 + L]) and y[0, 9 + L] == np.float32(1e-41)
        m = eng.read_master_meters()
        assert (m["n_limited"] == 0).all() and (m["min_gain"] == 1).all()
    finally:
        eng.close()


@pytest.mark.parametrize("Cn", [1, 2, 3, 8])
@pytest.mark.parametrize("L,H", [(1, 0), (63, 0), (64, 37), (200, 0)])
def test_dense_limiting(Cn, L, H):
    rng = np.random.default_rng(100 * Cn + L)
    eng = make_engine()
    try:
        eng.master_enable(Cn, 0.7, L, H, 0)
        y = run(eng, Model(Cn, 0.7, L, H, 0), signal(rng, Cn, 3), [3], (Cn, L, H))
        assert np.abs(y).max() <= np.float32(0.7)
        assert eng.read_master_meters()["n_limited"].min() > 0
    finally:
        eng.close()


def test_a_history_longer_than_the_steps():
    """L = 1100, H = 700: 2 L + H = 2900 samples of history against steps of 513; three cuts of the same 12 buffers"""
    L, H = 1100, 700
    rng = np.random.default_rng(3)
    x = signal(rng, 2, 12)
    outs = []
    for cuts in ([1] * 12, [12], [5, 7]):
        eng = make_engine()
        try:
            eng.master_enable(2, 0.7, L, H, 0)
            outs.append(run(eng, Model(2, 0.7, L, H, 0), x, cuts, cuts))
        finally:
            eng.close()
    same_bits(outs[1], outs[0], "12 against 12 x 1")
    same_bits(outs[2], outs[0], "5 + 7 against 12 x 1")


def test_the_longest_look_ahead():
    rng = np.random.default_rng(4)
    eng = make_engine()
    try:
        eng.master_enable(2, 0.5, 4096, 0, 0)
        y = run(eng, Model(2, 0.5, 4096, 0, 0), signal(rng, 2, 16), [1, 3, 1, 2, 9], "L = 4096")
        assert 0.49 < np.abs(y).max() <= np.float32(0.5)
    finally:
        eng.close()


def test_the_longest_hold():
    """H = 65536: every doubling level in LDS and six more over the whole array, the history 128 times the step"""
    rng = np.random.default_rng(5)
    x = signal(rng, 2, 3, 0.2)
    x[0, [100, 600, 1400]] = (2.0, -3.0, 1.5)
    eng = make_engine()
    try:
        eng.master_enable(2, 0.9, 2, 65536, 0)
        run(eng, Model(2, 0.9, 2, 65536, 0), x, [1, 1, 1], "H = 65536")
        assert eng.read_master_meters()["n_limited"].min() == B      # held since sample 100
    finally:
        eng.close()


def test_a_hold_beyond_the_lds_levels_on_the_wide_gain_launch():
    """L + H + 1 = 5301: ten doubling levels in LDS, two more over the whole array; 33 buffers = 16929 samples: strips of 1024"""
    rng = np.random.default_rng(6)
    x = signal(rng, 1, 34, 0.2)
    x[0, [100, 9000, 16000]] = (2.0, -3.0, 1.5)
    eng = make_engine()
    try:
        eng.master_enable(1, 0.9, 300, 5000, 0)
        run(eng, Model(1, 0.9, 300, 5000, 0), x, [33, 1], "H = 5000")
    finally:
        eng.close()


@pytest.mark.parametrize("Cn,L,H,nb", [(2, 64, 0, 33), (8, 200, 37, 32), (3, 4096, 0, 40)])
def test_long_steps_on_the_wide_gain_launch(Cn, L, H, nb):
    rng = np.random.default_rng(nb)
    eng = make_engine()
    try:
        eng.master_enable(Cn, 0.7, L, H, 0)
        run(eng, Model(Cn, 0.7, L, H, 0), signal(rng, Cn, nb + 1), [nb, 1], (Cn, L, H, nb))
    finally:
        eng.close()


@pytest.mark.parametrize("L", [64, 600])
def test_sparse_peaks_across_lane_buffer_and_step_borders(L):
    rng = np.random.default_rng(L)
    nb = 2
    n = 2 * nb * B
    x = signal(rng, 2, 2 * nb, 0.05)
    for i, s in enumerate((0, 63, 64, 512, 513, n - 1)):
        x[i % 2, s] = (-1) ** i * (2.0 + i)
    eng = make_engine()
    try:
        eng.master_enable(2, 0.8, L, 0, 0)
        y = run(eng, Model(2, 0.8, L, 0, 0), x, [nb, nb], L)
        assert 0.79 < np.abs(y).max() <= np.float32(0.8)
    finally:
        eng.close()


def gain_script(set_gain, process):
    """R = 700: a set, a second set inside its ramp, the ramp's end, and steps between.  process(k) runs step k (one buffer each)"""
    process(0)
    set_gain(0.25)
    process(1)                                           # 513 < 700: still ramping
    set_gain(3.0)
    process(2)
    process(3)                                           # the ramp ends at t_set + 699 inside this step
    process(4)


def test_gain_script():
    rng = np.random.default_rng(7)
    x = signal(rng, 2, 5, 0.4)
    eng = make_engine(nb_total=6)
    model = Model(2, 0.7, 64, 0, 700)
    try:
        eng.master_enable(2, 0.7, 64, 0, 700)
        assert eng.master_info() == {"t": 0, "ramp_end": 0, "calls": 0, "sets": 0}

        def sets(g):
            eng.master_set_gain(g)
            model.set_gain(g)

        def process(k):
            run(eng, model, x[:, k * B:(k + 1) * B], [1], ("gain script", k))
            assert eng.master_info()["ramp_end"] == model.ramp_end() and eng.master_info()["t"] == model.t

        gain_script(sets, process)
        assert eng.master_info() == {"t": 5 * B, "ramp_end": 5 * B, "calls": 5, "sets": 2}
    finally:
        eng.close()
    # R = 0: at once
    eng = make_engine()
    model = Model(2, 0.7, 64, 0, 0)
    try:
        eng.master_enable(2, 0.7, 64, 0, 0)
        eng.master_set_gain(0.5)
        eng.master_set_gain(-2.0)                        # replaces the one before: no step in between
        model.set_gain(0.5)
        model.set_gain(-2.0)
        run(eng, model, x[:, :2 * B], [1, 1], "R = 0")
    finally:
        eng.close()


def test_in_place_read_twice_pcm16_and_window():
    rng = np.random.default_rng(8)
    L, Cn = 65, 3
    x = signal(rng, Cn, 4)
    eng = make_engine()
    model = Model(Cn, 0.7, L, 5, 0)
    try:
        eng.master_enable(Cn, 0.7, L, 5, 0)
        w = eng.master_window()
        ref = window(L)
        assert w.shape == (L,) and (np.abs(w.view(np.int32) - ref.view(np.int32)) <= 1).all()
        model = Model(Cn, 0.7, L, 5, 0, w)
        dx = device(x[:, :2 * B])
        eng.step(2)
        eng.master(dx.data_ptr(), dx.data_ptr())         # d_out == d_in
        eng.sync()
        want = model.process(x[:, :2 * B])
        same_bits(dx.cpu().numpy(), want, "in place")
        same_bits(eng.read_master(), want, "read after in place")
        assert np.array_equal(eng.read_master_pcm16(), pcm16(want))
        dx = device(x[:, 2 * B:])
        eng.step(2)
        eng.master(dx.data_ptr())                        # engine-owned
        want = model.process(x[:, 2 * B:])
        same_bits(eng.read_master(), want, "engine-owned")
        same_bits(eng.read_master(), want, "read twice")
        p = eng.read_master_pcm16()
        assert p.shape == (2 * B, Cn) and np.array_equal(p, pcm16(want)) and np.abs(p).max() == 22937   # lrintf(0.7f * 32767.f)
        same_meters(eng.read_master_meters(), model.meters, "meters")
        assert np.array_equal(dx.cpu().numpy(), x[:, 2 * B:])        # (d_in is read only)
    finally:
        eng.close()


def test_master_error_paths_and_reset():
    rng = np.random.default_rng(9)
    eng = Engine()
    try:
        eng.add_object(synth.eigenvalues(32, 40), synth.RHO, synth.ALPHA, synth.BETA)
        with pytest.raises(PbsoError) as ei:
            eng.master_enable(2, 0.7, 64, 0, 0)                      # before finalize
        assert ei.value.status == capi.ERR_STATE
        eng.finalize()
        for bad in ((0, 0.7, 64, 0, 0), (9, 0.7, 64, 0, 0), (2, 0.0, 64, 0, 0), (2, 1.5, 64, 0, 0), (2, float("nan"), 64, 0, 0),
                    (2, float("inf"), 64, 0, 0), (2, -0.5, 64, 0, 0), (2, 0.7, 0, 0, 0), (2, 0.7, 4097, 0, 0), (2, 0.7, 64, -1, 0),
                    (2, 0.7, 64, 65537, 0), (2, 0.7, 64, 0, -1), (2, 0.7, 64, 0, (1 << 20) + 1)):
            with pytest.raises(PbsoError) as ei:
                eng.master_enable(*bad)
            assert ei.value.status == capi.ERR_INVALID, bad
        lib, fp = capi.lib(), C.POINTER(C.c_float)
        x = signal(rng, 2, 2)
        dx = device(x)
        for call in (lambda: eng.master(dx.data_ptr()), eng.master_reset, eng.master_info, lambda: eng.master_set_gain(1.0)):
            with pytest.raises(PbsoError) as ei:
                call()                                               # not enabled
            assert ei.value.status == capi.ERR_STATE
        eng.master_enable(2, 0.7, 64, 0, 100)
        for g in (float("nan"), float("inf")):
            with pytest.raises(PbsoError) as ei:
                eng.master_set_gain(g)
            assert ei.value.status == capi.ERR_INVALID
        assert eng.master_info()["sets"] == 0
        with pytest.raises(PbsoError) as ei:
            eng.master(dx.data_ptr())                                # no step since enable
        assert ei.value.status == capi.ERR_STATE
        out = np.empty(2 * 2 * B, dtype=np.float32)
        assert lib.pbso_read_master(eng._h, out.ctypes.data_as(fp), out.size) == capi.ERR_STATE   # nothing processed yet
        eng.step(2)
        assert lib.pbso_master(eng._h, None, None) == capi.ERR_INVALID                            # NULL d_in
        model = Model(2, 0.7, 64, 0, 100)
        eng.master_set_gain(2.0)
        model.set_gain(2.0)
        eng.master(dx.data_ptr())                                    # (the refusal did not use the step up)
        same_bits(eng.read_master(), model.process(x), "first step")
        big = np.empty(2 * 2 * B + 1, dtype=np.float32)
        assert lib.pbso_read_master(eng._h, big.ctypes.data_as(fp), big.size) == capi.ERR_INVALID
        assert lib.pbso_master_window(eng._h, big.ctypes.data_as(fp), 63) == capi.ERR_INVALID
        with pytest.raises(PbsoError) as ei:
            eng.master(dx.data_ptr())                                # the same step twice
        assert ei.value.status == capi.ERR_STATE
        eng.step(2)
        eng.step(2)
        with pytest.raises(PbsoError) as ei:
            eng.master(dx.data_ptr())                                # a step was skipped
        assert ei.value.status == capi.ERR_STATE
        # the reset: the history gone, t back at 0, the gain stays at 2 with its ramp finished
        eng.master_reset()
        model.reset()
        assert eng.master_info()["t"] == 0 and eng.master_info()["ramp_end"] == 0
        eng.step(2)
        eng.master(dx.data_ptr())
        want = model.process(x)
        same_bits(eng.read_master(), want, "after the reset")
        fresh = Model(2, 0.7, 64, 0, 0)
        fresh.set_gain(2.0)
        same_bits(want, fresh.process(x), "the reset is a fresh start at the gain last set")
        host = eng.host_buffer(2)                                    # a step to host memory: the input is the caller's buffer
        eng.step_to_host(2, host)
        eng.host_wait()
        eng.master(dx.data_ptr())
        same_bits(eng.read_master(), model.process(x), "after a host step")
    finally:
        eng.close()


def test_chain_of_scene_mix_reverb_and_master_on_real_audio():
    """4 objects -> scene_mix (C = 2) -> scene_reverb with d_add -> master: the model is fed read_scene_reverb()"""
    import torch
    n_obj, nb, Cn, K, T = 4, 2, 2, 900, 0.5
    rng = np.random.default_rng(10)
    eng = make_engine(n_obj, 64, 3 * nb, 6)
    try:
        eng.scene_mix_enable(Cn, 100, 0)
        eng.scene_mix_set(rng.uniform(-1, 1, (Cn, n_obj)), rng.uniform(0, 100, (Cn, n_obj)))
        eng.scene_reverb_enable(Cn, Cn, K, 0)
        eng.scene_reverb_set((rng.standard_normal((Cn, Cn, K)) * np.exp(-np.arange(K) / 200.0) * 0.05).astype(np.float32))
        n = nb * B
        dry = torch.zeros((Cn, n), dtype=torch.float32, device="cuda")
        bus = torch.zeros((Cn, n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        model = None
        for k in range(3):
            eng.step(nb)
            eng.scene_mix(dry.data_ptr())
            eng.scene_reverb(dry.data_ptr(), dry.data_ptr(), bus.data_ptr())
            u = eng.read_scene_reverb()
            peak = float(np.abs(u).max())
            assert peak > 0
            if model is None:
                # enabled behind the first step: armed for the next one; that step's peak would land at 50 T
                gain = float(np.float32(50 * T / peak))
                eng.master_enable(Cn, T, 64, 32, 0)
                eng.master_set_gain(gain)
                model = Model(Cn, T, 64, 32, 0)
                model.set_gain(gain)
                continue
            eng.master(bus.data_ptr())
            got = eng.read_master()
            same_bits(got, model.process(u), ("chain", k))
            same_meters(eng.read_master_meters(), model.meters, ("chain", k))
            assert 0 < np.abs(got).max() <= np.float32(T)
            same_bits(eng.read_scene_reverb(), u, "the bus is read only")
    finally:
        eng.close()
