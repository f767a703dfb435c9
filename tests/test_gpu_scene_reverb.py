"""The scene reverb (include/openpbso_amd.h "scene reverb"; kernels_reverb.hip) on the device: n_in bus signals through K taps per
(output channel, input), the history kept across steps.  Every output is compared BIT FOR BIT with the reference of the stated
order of arithmetic (tests/cpp/scene_reverb_ref.c through tests/scene_reverb_model.py, anchored by tests/test_scene_reverb_model.py).
The engine behind it is one object of 64 modes unless a test is about the engine: the reverb does not care what made its input."""
import ctypes as C

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from tests.scene_reverb_model import FadeRunning, Model

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


def taps_of(rng, n_out, n_in, K):
    """decaying noise: an impulse response's shape, every tap a full f32 mantissa"""
    return (rng.standard_normal((n_out, n_in, K)) * np.exp(-np.arange(K) / max(K / 4.0, 1.0))).astype(np.float32)


def device(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    return t


def signal(rng, rows, nb, scale=1.0):
    return (rng.standard_normal((rows, nb * B)) * scale).astype(np.float32)


def same_bits(got, want, label):
    assert got.shape == want.shape, label
    assert np.abs(want).max() > 0, label
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (label, bad.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def step_and_process(eng, model, x, label, add=None, samples=None):
    """one step of x.shape[1] / 513 buffers, x [n_in][n] (host) through the engine and the model"""
    eng.step(x.shape[1] // B)
    dx, da = device(x), None if add is None else device(add)
    eng.scene_reverb(dx.data_ptr(), None if da is None else da.data_ptr())
    got = eng.read_scene_reverb()
    want = model.process(x, add, samples)
    same_bits(got if samples is None else np.ascontiguousarray(got[:, samples]), want, label)
    return got


def test_unit_response_is_the_input_and_adds_onto_a_dry_mix():
    """n_in = n_out = 1, K = 1, tap 1: out == in; with d_add: out == add + in; with d_add == d_out: the same, in place"""
    rng = np.random.default_rng(1)
    eng = make_engine()
    try:
        eng.scene_reverb_enable(1, 1, 1, 0)
        eng.scene_reverb_set(np.ones((1, 1, 1)))
        x, add = signal(rng, 1, 2), signal(rng, 1, 2)
        dx, da = device(x), device(add)
        eng.step(2)
        eng.scene_reverb(dx.data_ptr())
        same_bits(eng.read_scene_reverb(), x, "out == in")
        eng.step(2)
        eng.scene_reverb(dx.data_ptr(), da.data_ptr())
        same_bits(eng.read_scene_reverb(), add + x, "out == add + in")
        assert np.array_equal(da.cpu().numpy(), add)                 # (d_add is read only)
        eng.step(2)
        eng.scene_reverb(dx.data_ptr(), da.data_ptr(), da.data_ptr())
        eng.sync()
        same_bits(da.cpu().numpy(), add + x, "in place")
        same_bits(eng.read_scene_reverb(), add + x, "read after in place")
    finally:
        eng.close()


def test_one_hot_taps_shift_the_input_exactly():
    """K = 4101 > n = 513: tap k alone, at both sides of the two segment borders and at both ends, over four one-buffer steps: the
    history spans several steps"""
    K, ks = 4101, (0, 1, 2047, 2048, 2049, 4100)
    rng = np.random.default_rng(2)
    x = signal(rng, 1, 4 * 3)
    eng = make_engine()
    try:
        eng.scene_reverb_enable(1, len(ks), K, 0)
        h = np.zeros((len(ks), 1, K), dtype=np.float32)
        for c, k in enumerate(ks):
            h[c, 0, k] = 1.0
        eng.scene_reverb_set(h)
        outs = []
        for s in range(12):
            dx = device(x[:, s * B:(s + 1) * B])
            eng.step(1)
            eng.scene_reverb(dx.data_ptr())
            outs.append(eng.read_scene_reverb())
        y = np.concatenate(outs, axis=1)
        for c, k in enumerate(ks):
            want = np.concatenate([np.zeros(k, dtype=np.float32), x[0, :x.shape[1] - k]])
            assert np.abs(want[4 * B:]).max() > 0 and np.array_equal(y[c], want), (k, np.abs(y[c] - want).max())
    finally:
        eng.close()


def test_script_with_fades_a_replaced_and_a_refused_set():
    """n_in = n_out = 2, K = 4101, R = 700, steps of 1, 3, 1 and 2 buffers behind a step of silence: the first set without a fade,
    a set replaced before its step, a fade wholly inside a step, a set refused while the next fade runs, the info at every step"""
    n_in, n_out, K, R = 2, 2, 4101, 700
    rng = np.random.default_rng(3)
    eng = make_engine()
    model = Model(n_in, n_out, K, R)
    new = lambda: taps_of(rng, n_out, n_in, K)
    try:
        eng.scene_reverb_enable(n_in, n_out, K, R)
        x, add = signal(rng, n_in, 1), signal(rng, n_out, 1)
        eng.step(1)
        dx, da = device(x), device(add)
        eng.scene_reverb(dx.data_ptr())                              # nothing set yet: silence (and the history starts)
        assert not eng.read_scene_reverb().any()
        model.process(x)
        eng.step(1)
        eng.scene_reverb(dx.data_ptr(), da.data_ptr())               # ... or add alone
        assert np.array_equal(eng.read_scene_reverb(), add)
        model.process(x, add)
        assert eng.scene_reverb_info() == {"t": 2 * B, "fade_end": 2 * B, "calls": 2, "sets": 0}
        eng.scene_reverb_set(new())
        h = new()
        eng.scene_reverb_set(h)                                      # replaces the one before: no step in between
        model.set(h)
        step_and_process(eng, model, signal(rng, n_in, 1), "step 0")         # the first set: no fade
        assert eng.scene_reverb_info() == {"t": 3 * B, "fade_end": 3 * B, "calls": 3, "sets": 2}
        h = new()
        eng.scene_reverb_set(h)
        model.set(h)
        step_and_process(eng, model, signal(rng, n_in, 3), "step 1", add=signal(rng, n_out, 3))   # fade and steady state in one step
        info = eng.scene_reverb_info()
        assert info["t"] == info["fade_end"] == 6 * B == model.fade_end()
        h = new()
        eng.scene_reverb_set(h)
        model.set(h)
        step_and_process(eng, model, signal(rng, n_in, 1), "step 2")         # wholly inside the fade
        info = eng.scene_reverb_info()
        assert info["t"] == 7 * B and info["fade_end"] == 6 * B + R - 1 == model.fade_end()
        with pytest.raises(PbsoError) as ei:
            eng.scene_reverb_set(new())                              # the fade is still running
        assert ei.value.status == capi.ERR_STATE
        with pytest.raises(FadeRunning):
            model.set(new())
        assert eng.scene_reverb_info()["sets"] == 4
        step_and_process(eng, model, signal(rng, n_in, 2), "step 3")         # the fade ends inside this step
        assert eng.scene_reverb_info() == {"t": 9 * B, "fade_end": 9 * B, "calls": 6, "sets": 4}
    finally:
        eng.close()


def _cut_run(cuts, x, add, sets, n_in, n_out, K, R):
    eng = make_engine()
    try:
        eng.scene_reverb_enable(n_in, n_out, K, R)
        outs, done = [], 0
        for nb in cuts:
            if done in sets:
                eng.scene_reverb_set(sets[done])
            dx, da = device(x[:, done * B:(done + nb) * B]), device(add[:, done * B:(done + nb) * B])
            eng.step(nb)
            eng.scene_reverb(dx.data_ptr(), da.data_ptr())
            outs.append(eng.read_scene_reverb())
            done += nb
        return np.concatenate(outs, axis=1)
    finally:
        eng.close()


def test_the_cut_into_steps_and_the_run_do_not_change_a_bit():
    """behind a first step of one buffer, six buffers as one step, as 1 + 2 + 3 and one at a time; the sets at samples 0 and 513 in
    every run (the fade of the second one crosses the cuts); and one of the cuts run twice.  The first run is also the reference's."""
    n_in, n_out, K, R = 2, 3, 2500, 1300
    rng = np.random.default_rng(4)
    x, add = signal(rng, n_in, 7), signal(rng, n_out, 7)
    sets = {0: taps_of(rng, n_out, n_in, K), 1: taps_of(rng, n_out, n_in, K)}
    base = _cut_run([1, 6], x, add, sets, n_in, n_out, K, R)
    model = Model(n_in, n_out, K, R)
    model.set(sets[0])
    want = [model.process(x[:, :B], add[:, :B])]
    model.set(sets[1])
    want.append(model.process(x[:, B:], add[:, B:]))
    same_bits(base, np.concatenate(want, axis=1), "one step")
    for cuts in ([1, 1, 2, 3], [1] * 7, [1] * 7):
        same_bits(_cut_run(cuts, x, add, sets, n_in, n_out, K, R), base, cuts)


@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (3, 8)])
@pytest.mark.parametrize("K", [1, 5, 2047, 2048, 2049, 6144])
def test_tap_counts_around_the_padding_and_the_segment(K, shape):
    """two steps of one and two buffers with a fade, all samples: K at, below and above the segment and the instruction's four
    window positions"""
    n_in, n_out = shape
    R = 300
    rng = np.random.default_rng(K + n_out)
    eng = make_engine()
    model = Model(n_in, n_out, K, R)
    try:
        eng.scene_reverb_enable(n_in, n_out, K, R)
        for k, nb in enumerate((1, 2)):
            h = taps_of(rng, n_out, n_in, K)
            eng.scene_reverb_set(h)
            model.set(h)
            step_and_process(eng, model, signal(rng, n_in, nb), (K, shape, k))
    finally:
        eng.close()


def test_the_most_taps_there_are():
    """K = 1 << 17, one input, one output: one step of 300 buffers (1500 seeded samples of it, its ends among them), then two of one
    buffer whose history is that long step (every sample)"""
    K = 1 << 17
    rng = np.random.default_rng(6)
    eng = make_engine()
    model = Model(1, 1, K, 0)
    try:
        eng.scene_reverb_enable(1, 1, K, 0)
        h = taps_of(rng, 1, 1, K)
        eng.scene_reverb_set(h)
        model.set(h)
        n = 300 * B
        samples = np.unique(np.concatenate([np.arange(8), n - 1 - np.arange(8), rng.choice(n, 1500, replace=False)]))
        step_and_process(eng, model, signal(rng, 1, 300), "long", samples=samples)
        for k in range(2):
            step_and_process(eng, model, signal(rng, 1, 1), ("short", k))
    finally:
        eng.close()


def test_widest_matrix():
    """n_in = n_out = 8, K = 2049 (a second segment of one tap per pair): 16 partial rows per channel in (i, j) order"""
    rng = np.random.default_rng(7)
    eng = make_engine()
    model = Model(8, 8, 2049, 0)
    try:
        eng.scene_reverb_enable(8, 8, 2049, 0)
        h = taps_of(rng, 8, 8, 2049)
        eng.scene_reverb_set(h)
        model.set(h)
        for nb in (1, 2):
            step_and_process(eng, model, signal(rng, 8, nb), nb, add=signal(rng, 8, nb))
    finally:
        eng.close()


@pytest.mark.parametrize("n_in,n_out,K,nb", [(3, 8, 4101, 230), (2, 3, 16389, 232), (2, 4, 16389, 233)])
def test_long_steps_on_the_launch_of_many_tiles_per_wave(n_in, n_out, K, nb):
    """steps long enough for the launch of four waves x several tiles (the short tests above all run one tile per workgroup), with
    a ragged last strip, a fade that ends inside a strip, and d_add: seeded samples, the fade's end and both ends of the step"""
    R = 70000
    rng = np.random.default_rng(K + n_out)
    eng = make_engine()
    model = Model(n_in, n_out, K, R)
    n = nb * B
    samples = np.unique(np.concatenate([np.arange(40), n - 1 - np.arange(40), R - 1 + np.arange(-3, 3), rng.choice(n, 500, replace=False)]))
    try:
        eng.scene_reverb_enable(n_in, n_out, K, R)
        for k in range(2):
            h = taps_of(rng, n_out, n_in, K)
            eng.scene_reverb_set(h)
            model.set(h)
            step_and_process(eng, model, signal(rng, n_in, nb), (n_in, n_out, K, k), add=signal(rng, n_out, nb), samples=samples)
    finally:
        eng.close()


def test_subnormal_inputs_come_through():
    """inputs of scale 1e-41 through taps of magnitude <= 1: every product and sum is a subnormal f32, which the reference's fmaf
    keeps -- so must the kernel"""
    rng = np.random.default_rng(8)
    n_in, n_out, K = 2, 2, 2100
    eng = make_engine()
    model = Model(n_in, n_out, K, 0)
    try:
        eng.scene_reverb_enable(n_in, n_out, K, 0)
        h = np.clip(taps_of(rng, n_out, n_in, K), -1, 1)
        eng.scene_reverb_set(h)
        model.set(h)
        x = signal(rng, n_in, 2, 1e-41)
        assert 0 < np.abs(x).max() < np.finfo(np.float32).tiny
        got = step_and_process(eng, model, x, "subnormal")
        assert 0 < np.abs(got).max() < np.finfo(np.float32).tiny
    finally:
        eng.close()


def test_object_mix_through_the_unit_response_is_the_object_mix():
    """33 objects with real hits: mix_objects -> scene_reverb on the engine's stream, K = 1, tap 1"""
    import torch
    nb = 2
    eng = make_engine(33, 64, 2 * nb, 5)
    try:
        eng.scene_reverb_enable(1, 1, 1, 0)
        eng.scene_reverb_set(np.ones((1, 1, 1)))
        mono = torch.zeros(nb * B, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(2):
            eng.step(nb)
            eng.mix_objects(mono.data_ptr())
            eng.scene_reverb(mono.data_ptr())
            got = eng.read_scene_reverb()
            want = mono.cpu().numpy()
            assert np.abs(want).max() > 0 and np.array_equal(got[0], want), k
    finally:
        eng.close()


def test_scene_mix_channels_as_bus_and_dry_mix():
    """a scene mix of C + 1 channels: the last one is the send bus, the first C are d_add; the result is the model's, fed with
    read_scene_mix()"""
    import torch
    n_obj, nb, Cd, K, R = 9, 2, 2, 3000, 400
    rng = np.random.default_rng(9)
    eng = make_engine(n_obj, 64, 3 * nb, 6)
    model = Model(1, Cd, K, R)
    try:
        eng.scene_mix_enable(Cd + 1, 100, 0)
        eng.scene_mix_set(rng.uniform(-1, 1, (Cd + 1, n_obj)), rng.uniform(0, 100, (Cd + 1, n_obj)))
        eng.scene_reverb_enable(1, Cd, K, R)
        n = nb * B
        buf = torch.zeros((Cd + 1, n), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(3):
            h = taps_of(rng, Cd, 1, K) * 0.05
            eng.scene_reverb_set(h)
            model.set(h)
            eng.step(nb)
            eng.scene_mix(buf.data_ptr())
            eng.scene_reverb(buf.data_ptr() + Cd * n * 4, buf.data_ptr())
            got, mix = eng.read_scene_reverb(), eng.read_scene_mix()
            assert np.abs(mix[Cd]).max() > 0
            same_bits(got, model.process(mix[Cd:], mix[:Cd]), k)
    finally:
        eng.close()


def test_reverb_leaves_the_engine_and_both_mixers_alone():
    n_obj, nb = 40, 2
    rng = np.random.default_rng(10)
    h, d = (rng.standard_normal((2, n_obj, 20)) * 0.1).astype(np.float32), rng.integers(0, 301, n_obj)
    g, dl = rng.uniform(-1, 1, (2, n_obj)), rng.uniform(0, 300, (2, n_obj))
    outs = {}
    for reverb in (False, True):
        eng = make_engine(n_obj, 64, 2 * nb, 31)
        try:
            eng.scene_fir_enable(2, 20, 300, 100)
            eng.scene_fir_set(h, d)
            eng.scene_mix_enable(2, 300, 100)
            eng.scene_mix_set(g, dl)
            if reverb:
                eng.scene_reverb_enable(1, 2, 700, 0)
                eng.scene_reverb_set(taps_of(rng, 2, 1, 700))
                dx = device(signal(rng, 1, nb))
            got = []
            for k in range(2):
                eng.step(nb)
                eng.scene_mix()
                eng.scene_fir()
                if reverb:
                    eng.scene_reverb(dx.data_ptr())
                    assert np.abs(eng.read_scene_reverb()).max() > 0
                got.append([eng.audio(), eng.read_scene_fir(), eng.read_scene_mix(), eng.state(7)[0], eng.qnorm(3, nb - 1)])
            outs[reverb] = got
        finally:
            eng.close()
    for k in range(2):
        for i, (a, b) in enumerate(zip(outs[False][k], outs[True][k])):
            assert (i > 2 or np.abs(a).max() > 0) and np.array_equal(a, b), (k, i)


def test_headline_size():
    """n = 860 buffers, one bus, stereo, K = 65536, behind a one-buffer step: 1500 seeded samples inside a fade and after it"""
    n_in, n_out, K, R, nb = 1, 2, 65536, 200000, 860
    rng = np.random.default_rng(11)
    eng = make_engine()
    model = Model(n_in, n_out, K, R)
    n = nb * B
    try:
        eng.scene_reverb_enable(n_in, n_out, K, R)
        h = taps_of(rng, n_out, n_in, K)
        eng.scene_reverb_set(h)
        model.set(h)
        step_and_process(eng, model, signal(rng, n_in, 1), "first")
        h = taps_of(rng, n_out, n_in, K)
        eng.scene_reverb_set(h)
        model.set(h)
        samples = np.unique(np.concatenate([rng.choice(R - 1, 700, replace=False), R - 1 + np.arange(-3, 3),
                                            R + rng.choice(n - R, 800, replace=False)]))
        step_and_process(eng, model, signal(rng, n_in, nb), "headline", samples=samples)
        assert eng.scene_reverb_info()["fade_end"] == eng.scene_reverb_info()["t"] == B + n
    finally:
        eng.close()


def test_reverb_error_paths():
    rng = np.random.default_rng(12)
    K = 4
    eng = Engine()
    try:
        eng.add_object(synth.eigenvalues(32, 40), synth.RHO, synth.ALPHA, synth.BETA)
        with pytest.raises(PbsoError) as ei:
            eng.scene_reverb_enable(1, 2, K, 0)                      # before finalize
        assert ei.value.status == capi.ERR_STATE
        eng.finalize()
        for bad in ((0, 2, K, 0), (9, 2, K, 0), (1, 0, K, 0), (1, 9, K, 0), (1, 2, 0, 0), (1, 2, (1 << 17) + 1, 0), (1, 2, K, -1),
                    (1, 2, K, (1 << 20) + 1)):
            with pytest.raises(PbsoError) as ei:
                eng.scene_reverb_enable(*bad)
            assert ei.value.status == capi.ERR_INVALID, bad
        lib, fp = capi.lib(), C.POINTER(C.c_float)
        ones = np.ones((2, 1, K), dtype=np.float32)
        dx = device(signal(rng, 1, 2))
        assert lib.pbso_scene_reverb_set(eng._h, ones.ctypes.data_as(fp)) == capi.ERR_STATE          # set before enable
        for call in (lambda: eng.scene_reverb(dx.data_ptr()), eng.scene_reverb_reset, eng.scene_reverb_info):
            with pytest.raises(PbsoError) as ei:
                call()                                               # not enabled
            assert ei.value.status == capi.ERR_STATE
        eng.scene_reverb_enable(1, 2, K, 4)
        assert lib.pbso_scene_reverb_set(eng._h, None) == capi.ERR_INVALID                          # NULL taps
        nan, inf = ones.copy(), ones.copy()
        nan[1, 0, 3], inf[0, 0, 0] = np.nan, np.inf
        for hh in (nan, inf):
            with pytest.raises(PbsoError) as ei:
                eng.scene_reverb_set(hh)
            assert ei.value.status == capi.ERR_INVALID
        assert eng.scene_reverb_info()["sets"] == 0
        eng.scene_reverb_set(ones)
        with pytest.raises(PbsoError) as ei:
            eng.scene_reverb(dx.data_ptr())                          # no step since enable
        assert ei.value.status == capi.ERR_STATE
        eng.step(2)
        assert lib.pbso_scene_reverb(eng._h, None, None, None) == capi.ERR_INVALID                   # NULL d_in
        with pytest.raises(PbsoError) as ei:
            eng.scene_reverb(dx.data_ptr(), None, dx.data_ptr())     # d_out overlaps d_in
        assert ei.value.status == capi.ERR_INVALID
        eng.scene_reverb(dx.data_ptr())                              # (neither refusal used the step up)
        first = eng.read_scene_reverb()
        assert first.shape == (2, 2 * B) and np.abs(first).max() > 0
        out = np.empty(2 * 2 * B + 1, dtype=np.float32)
        assert lib.pbso_read_scene_reverb(eng._h, out.ctypes.data_as(fp), out.size) == capi.ERR_INVALID
        with pytest.raises(PbsoError) as ei:
            eng.scene_reverb(dx.data_ptr())                          # the same step twice
        assert ei.value.status == capi.ERR_STATE
        eng.step(2)
        eng.step(2)
        with pytest.raises(PbsoError) as ei:
            eng.scene_reverb(dx.data_ptr())                          # a step was skipped
        assert ei.value.status == capi.ERR_STATE
        eng.scene_reverb_reset()
        eng.step(2)
        eng.scene_reverb(dx.data_ptr())                              # works again: silence, the taps went with the reset
        assert not eng.read_scene_reverb().any() and eng.scene_reverb_info()["t"] == 2 * B
        host = eng.host_buffer(2)                                    # a step to host memory: the input is the caller's buffer
        eng.scene_reverb_set(ones)
        eng.step_to_host(2, host)
        eng.host_wait()
        eng.scene_reverb(dx.data_ptr())
        model = Model(1, 2, K, 4)
        model.process(dx.cpu().numpy())
        model.set(ones)
        same_bits(eng.read_scene_reverb(), model.process(dx.cpu().numpy()), "after a host step")
    finally:
        eng.close()
