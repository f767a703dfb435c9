"""The scene filter mix (include/openpbso_amd.h "scene filter mix"; kernels_fir.hip) on the device: C channels, a K-tap FIR per
(channel, object) behind an onset per object.  Every output is compared BIT FOR BIT with the reference of the stated order of
arithmetic (tests/cpp/scene_fir_ref.c through tests/scene_fir_model.py, anchored by tests/test_scene_fir_model.py), fed the rows
Engine.audio() returned."""
import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from tests.scene_fir_model import FadeRunning, Model

B = 513


def make_engine(n_obj, n_modes, nb_total, seed, hits_per_obj=3, **kw):
    """n_obj objects with explicit-data impulses at buffer 0 and spread over nb_total buffers, unit transfer"""
    eng = Engine(**kw)
    for i in range(n_obj):
        eng.add_object(synth.eigenvalues(n_modes, 9000 + 131 * seed + i), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    rng = np.random.default_rng(seed)
    for i in range(n_obj):
        eng.set_use_transfer(i, False)
        for t in [0] + sorted(int(x) for x in rng.integers(1, max(nb_total, 2), hits_per_obj - 1)):
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(n_modes) * 1e-3), t)
    return eng


def taps_of(rng, C, n_obj, K):
    """decaying noise: an impulse response's shape, every tap a full f32 mantissa"""
    return (rng.standard_normal((C, n_obj, K)) * np.exp(-np.arange(K) / max(K / 4.0, 1.0))).astype(np.float32)


def same_bits(got, want, label):
    assert got.shape == want.shape, label
    assert np.abs(want).max() > 0, label
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (label, bad.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def step_and_mix(eng, model, nb, label, samples=None):
    eng.step(nb)
    eng.scene_fir()
    rows, got = eng.audio(), eng.read_scene_fir()
    want = model.mix(rows, samples)
    same_bits(got if samples is None else np.ascontiguousarray(got[:, samples]), want, label)
    return rows, got


@pytest.mark.gpu
@pytest.mark.parametrize("n_obj", [1, 33, 1024])
def test_unit_tap_equals_the_object_mix_bit_for_bit(n_obj):
    """C = 1, K = 1, tap 1, onset 0: fmaf(1, x, acc) = acc + x in the order of pbso_mix_objects"""
    import torch
    nb = 3
    eng = make_engine(n_obj, 64, 2 * nb, n_obj)
    try:
        eng.scene_fir_enable(1, 1, 0, 0)
        eng.scene_fir_set(np.ones((1, n_obj, 1)))
        mono = torch.zeros(nb * B, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(2):
            eng.step(nb)
            eng.scene_fir()
            eng.mix_objects(mono.data_ptr())
            eng.sync()
            got, want = eng.read_scene_fir(), mono.cpu().numpy()
            same_bits(got[0], want, (n_obj, k))
    finally:
        eng.close()


@pytest.mark.gpu
def test_one_hot_taps_shift_the_row_exactly():
    """one object, tap k_c = 1 per channel, an onset: channel c is the row shifted by D + k_c, over steps of 2, 1 and 2 buffers --
    the middle step is shorter than the shift, its data is in the history of two steps back"""
    K, D, ks = 64, 600, (5, 63)
    eng = make_engine(1, 64, 5, 1)
    try:
        eng.scene_fir_enable(2, K, 700, 0)
        h = np.zeros((2, 1, K), dtype=np.float32)
        for c, k in enumerate(ks):
            h[c, 0, k] = 1.0
        eng.scene_fir_set(h, [D])
        rows, outs = [], []
        for nb in (2, 1, 2):
            eng.step(nb)
            eng.scene_fir()
            rows.append(eng.audio())
            outs.append(eng.read_scene_fir())
        x, y = np.concatenate(rows, axis=1)[0], np.concatenate(outs, axis=1)
        assert np.abs(x).max() > 0
        for c, k in enumerate(ks):
            want = np.concatenate([np.zeros(D + k, dtype=np.float32), x[:x.size - D - k]])
            assert np.array_equal(y[c], want), (c, np.abs(y[c] - want).max())
    finally:
        eng.close()


@pytest.mark.gpu
def test_script_over_five_steps_with_fades_and_a_refused_set():
    """C = 3, 40 objects (a ragged second group), K = 37, onsets up to 1400, R = 700, steps of 2, 1, 1, 3, 2 buffers: silence before
    the first set; a fade that starts at a step boundary and crosses the next one; a set refused while it runs, with the info
    saying when it ends; a set accepted at the first step after that; a set of taps alone"""
    n_obj, C, K, max_onset, R = 40, 3, 37, 1400, 700
    steps = [2, 1, 1, 3, 2]
    eng = make_engine(n_obj, 96, sum(steps) + 1, 11)
    model = Model(C, n_obj, K, max_onset, R)
    rng = np.random.default_rng(5)
    new = lambda hi: (taps_of(rng, C, n_obj, K), rng.integers(0, hi + 1, n_obj).astype(np.int32))
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        eng.step(1)
        eng.scene_fir()                                  # nothing set yet: silence (and the history starts)
        assert not eng.read_scene_fir().any()
        model.mix(eng.audio())
        h, d = new(max_onset)
        d[:3] = [0, max_onset, 513]
        eng.scene_fir_set(h, d)
        model.set(h, d)
        step_and_mix(eng, model, steps[0], "step 0")     # the first set: no fade
        assert eng.scene_fir_info() == {"t": 3 * B, "fade_end": 3 * B, "mixes": 2, "sets": 1}
        h, d = new(max_onset)
        eng.scene_fir_set(h, d)
        model.set(h, d)
        step_and_mix(eng, model, steps[1], "step 1")     # wholly inside the fade
        info = eng.scene_fir_info()
        assert info["t"] == 4 * B and info["fade_end"] == 3 * B + R - 1 == model.fade_end()
        with pytest.raises(PbsoError) as ei:
            eng.scene_fir_set(*new(50))                  # the fade is still running
        assert ei.value.status == capi.ERR_STATE
        with pytest.raises(FadeRunning):
            model.set(*new(50))
        assert eng.scene_fir_info()["sets"] == 2
        step_and_mix(eng, model, steps[2], "step 2")     # the fade ends inside this step
        info = eng.scene_fir_info()
        assert info["t"] == info["fade_end"] == 5 * B
        h, d = new(50)
        eng.scene_fir_set(h, d)                          # accepted at the first step after the fade
        model.set(h, d)
        step_and_mix(eng, model, steps[3], "step 3")     # fade and steady state in one step
        h = taps_of(rng, C, n_obj, K)
        eng.scene_fir_set(h)                             # taps alone: the onsets stay
        model.set(h)
        step_and_mix(eng, model, steps[4], "step 4")
        assert eng.scene_fir_info()["sets"] == 4 and eng.scene_fir_info()["mixes"] == 6
    finally:
        eng.close()


def _cut_run(cuts, n_obj, seed, C=2, K=48, max_onset=900, R=1500):
    """the same scene stepped in `cuts`; the set calls fall at samples 0 and 2 * 513 in every run"""
    eng = make_engine(n_obj, 64, sum(cuts), seed, time_chunks=1)      # time_chunks = 1: the rows themselves do not depend on the cut
    rng = np.random.default_rng(seed)
    sets = {0: (taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj)),
            2: (taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj))}
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        mixes, rows, done = [], [], 0
        for nb in cuts:
            if done in sets:
                eng.scene_fir_set(*sets[done])
            eng.step(nb)
            eng.scene_fir()
            mixes.append(eng.read_scene_fir())
            rows.append(eng.audio())
            done += nb
        return np.concatenate(mixes, axis=1), np.concatenate(rows, axis=1), sets
    finally:
        eng.close()


@pytest.mark.gpu
def test_the_cut_into_steps_and_the_run_do_not_change_a_bit():
    """the same ten buffers as two steps, one buffer at a time and in uneven steps, the sets at the same absolute samples; and one
    of the cuts run twice.  The first run is also the reference's."""
    n_obj = 37
    base_mix, base_rows, sets = _cut_run([2, 8], n_obj, 3)
    model = Model(2, n_obj, 48, 900, 1500)
    model.set(*sets[0])
    want = [model.mix(base_rows[:, :2 * B])]
    model.set(*sets[2])
    want.append(model.mix(base_rows[:, 2 * B:]))
    same_bits(base_mix, np.concatenate(want, axis=1), "one step")
    for cuts in ([1] * 10, [2, 1, 4, 3], [2, 1, 4, 3]):
        mix, rows, _ = _cut_run(cuts, n_obj, 3)
        assert np.array_equal(rows, base_rows), cuts                 # (the precondition: the same rows)
        same_bits(mix, base_mix, cuts)


@pytest.mark.gpu
def test_headline_size():
    """1024 objects x 512 modes, stereo, K = 128, two steps of 8 buffers with a set and a fade between them: 2048 seeded samples per
    step and channel and the first and last 256 of each step"""
    n_obj, M, nb, C, K, max_onset, R = 1024, 512, 8, 2, 128, 2048, 1500
    eng = make_engine(n_obj, M, 2 * nb, 17, hits_per_obj=2)
    model = Model(C, n_obj, K, max_onset, R)
    rng = np.random.default_rng(17)
    n = nb * B
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        for k in range(2):
            h, d = taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj)
            eng.scene_fir_set(h, d)
            model.set(h, d)
            samples = np.unique(np.concatenate([np.arange(256), np.arange(n - 256, n), rng.choice(n, 2048, replace=False),
                                                R - 1 + np.arange(-2, 3)]))
            step_and_mix(eng, model, nb, f"step {k}", samples)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 4, 5, 127, 128, 1024])
def test_tap_counts_around_the_padding_and_at_the_limit(K):
    """33 objects (a second group of one), two steps with a fade: K at, below and above a multiple of the instruction's four window
    positions, and the most taps there are"""
    n_obj, C, max_onset, R = 33, 2, 300, 200
    eng = make_engine(n_obj, 64, 3, K)
    model = Model(C, n_obj, K, max_onset, R)
    rng = np.random.default_rng(K)
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        for k, nb in enumerate((2, 1)):
            h, d = taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj)
            eng.scene_fir_set(h, d)
            model.set(h, d)
            samples = None if K < 1024 else np.unique(np.concatenate([np.arange(300), nb * B - 1 - np.arange(40)]))
            step_and_mix(eng, model, nb, (K, k), samples)
    finally:
        eng.close()


@pytest.mark.gpu
def test_subnormal_samples_come_through():
    """a quiet scene (the audio is linear in the force: scaled to a peak near 1e-34) through taps near 1e-6: every product and every
    sum is a subnormal f32, which the reference's fmaf keeps -- so must the kernel"""
    n_obj, C, K = 5, 1, 8

    def run(scale, taps):
        eng = Engine()
        try:
            for i in range(n_obj):
                eng.add_object(synth.eigenvalues(64, 77 + i), synth.RHO, synth.ALPHA, synth.BETA)
            eng.finalize()
            rng = np.random.default_rng(7)
            for i in range(n_obj):
                eng.set_use_transfer(i, False)
                assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(64) * scale), 0)
            eng.scene_fir_enable(C, K, 0, 0)
            eng.scene_fir_set(taps)
            eng.step(1)
            eng.scene_fir()
            return eng.audio(), eng.read_scene_fir()
        finally:
            eng.close()

    h = (taps_of(np.random.default_rng(1), C, n_obj, K) * 1e-6).astype(np.float32)
    loud, _ = run(1.0, h)
    rows, got = run(1e-34 / float(np.abs(loud).max()), h)
    assert 1e-36 < np.abs(rows).max() < 1e-32
    model = Model(C, n_obj, K, 0, 0)
    model.set(h)
    same_bits(got, model.mix(rows), "subnormal")
    assert 0 < np.abs(got).max() < np.finfo(np.float32).tiny


@pytest.mark.gpu
def test_filter_mix_leaves_the_engines_output_alone():
    """with the mixer enabled and mixing every step, the audio, state and qnorm rows are those of an engine without it"""
    n_obj, nb = 70, 3
    plain = make_engine(n_obj, 128, 3 * nb, 23)
    mixed = make_engine(n_obj, 128, 3 * nb, 23)
    rng = np.random.default_rng(2)
    try:
        mixed.scene_fir_enable(2, 33, 700, 300)
        for k in range(3):
            mixed.scene_fir_set(taps_of(rng, 2, n_obj, 33), rng.integers(0, 701, n_obj))
            plain.step(nb)
            mixed.step(nb)
            mixed.scene_fir()
            a, b = plain.audio(), mixed.audio()
            assert np.abs(a).max() > 0 and np.array_equal(a, b), k
            for o in (0, 33, n_obj - 1):
                for u, v in zip(plain.state(o), mixed.state(o)):
                    assert np.array_equal(u, v), (k, o)
                assert np.array_equal(plain.qnorm(o, nb - 1), mixed.qnorm(o, nb - 1)), (k, o)
            assert np.abs(mixed.read_scene_fir()).max() > 0
    finally:
        plain.close()
        mixed.close()


@pytest.mark.gpu
def test_both_mixers_on_one_engine_equal_each_alone():
    n_obj, nb = 40, 2
    rng = np.random.default_rng(8)
    h, d = taps_of(rng, 2, n_obj, 20), rng.integers(0, 301, n_obj)
    g, dl = rng.uniform(-1, 1, (2, n_obj)), rng.uniform(0, 300, (2, n_obj))
    outs = {}
    for which in ("fir", "mix", "both"):
        eng = make_engine(n_obj, 64, 2 * nb, 31)
        try:
            if which != "mix":
                eng.scene_fir_enable(2, 20, 300, 100)
                eng.scene_fir_set(h, d)
            if which != "fir":
                eng.scene_mix_enable(2, 300, 100)
                eng.scene_mix_set(g, dl)
            got = []
            for k in range(2):
                eng.step(nb)
                if which != "fir":
                    eng.scene_mix()
                if which != "mix":
                    eng.scene_fir()
                got.append([eng.read_scene_fir() if which != "mix" else None, eng.read_scene_mix() if which != "fir" else None])
            outs[which] = got
        finally:
            eng.close()
    for k in range(2):
        same_bits(outs["both"][k][0], outs["fir"][k][0], ("fir", k))
        same_bits(outs["both"][k][1], outs["mix"][k][1], ("mix", k))


@pytest.mark.gpu
def test_filter_mix_error_paths():
    n_obj, K = 3, 4
    eng = Engine()
    try:
        for i in range(n_obj):
            eng.add_object(synth.eigenvalues(32, 40 + i), synth.RHO, synth.ALPHA, synth.BETA)
        with pytest.raises(PbsoError) as ei:
            eng.scene_fir_enable(2, K, 10, 0)                # before finalize
        assert ei.value.status == capi.ERR_STATE
        eng.finalize()
        for i in range(n_obj):
            eng.set_use_transfer(i, False)
            eng.enqueue_force(i, ForceMessage(data=np.ones(32) * 1e-3), 0)
        for bad in ((0, K, 10, 0), (9, K, 10, 0), (2, 0, 10, 0), (2, 1025, 10, 0), (2, K, -1, 0), (2, K, (1 << 20) + 1, 0),
                    (2, K, 10, -1), (2, K, 10, (1 << 20) + 1)):
            with pytest.raises(PbsoError) as ei:
                eng.scene_fir_enable(*bad)
            assert ei.value.status == capi.ERR_INVALID, bad
        for call in (eng.scene_fir, eng.scene_fir_reset, eng.scene_fir_info):
            with pytest.raises(PbsoError) as ei:
                call()                                       # not enabled
            assert ei.value.status == capi.ERR_STATE
        eng.scene_fir_enable(2, K, 10, 4)
        h, d = np.ones((2, n_obj, K), dtype=np.float32), np.full(n_obj, 3)
        nan, inf = h.copy(), h.copy()
        nan[1, 2, 3], inf[0, 0, 0] = np.nan, np.inf
        for hh, dd in ((nan, d), (inf, None), (h, d + 8), (h, -d)):
            with pytest.raises(PbsoError) as ei:
                eng.scene_fir_set(hh, dd)                    # a NaN / infinite tap; an onset above max_onset, negative
            assert ei.value.status == capi.ERR_INVALID
        assert eng.scene_fir_info()["sets"] == 0
        eng.scene_fir_set(h, d)
        with pytest.raises(PbsoError) as ei:
            eng.scene_fir()                                  # no step since enable
        assert ei.value.status == capi.ERR_STATE
        eng.step(1)
        eng.scene_fir()
        first = eng.read_scene_fir()
        assert first.shape == (2, B) and np.abs(first).max() > 0
        out = np.empty(2 * B + 1, dtype=np.float32)
        import ctypes as C
        assert capi.lib().pbso_read_scene_fir(eng._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size) == capi.ERR_INVALID
        with pytest.raises(PbsoError) as ei:
            eng.scene_fir()                                  # the same step twice
        assert ei.value.status == capi.ERR_STATE
        eng.step(1)
        eng.step(1)
        with pytest.raises(PbsoError) as ei:
            eng.scene_fir()                                  # a step was not mixed
        assert ei.value.status == capi.ERR_STATE
        eng.scene_fir_reset()
        eng.step(2)
        eng.scene_fir()                                      # works again: silence, the filters went with the reset
        assert eng.read_scene_fir().shape == (2, 2 * B) and not eng.read_scene_fir().any()
        assert eng.scene_fir_info()["t"] == 2 * B
        host = eng.host_buffer(1)                            # rows of a step to host memory are not on the device
        eng.step_to_host(1, host)
        eng.host_wait()
        with pytest.raises(PbsoError) as ei:
            eng.scene_fir()
        assert ei.value.status == capi.ERR_STATE
        eng.scene_fir_reset()
        eng.scene_fir_set(h, d)
        eng.enqueue_force(0, ForceMessage(data=np.ones(32) * 1e-3), 0)
        eng.step(1)
        eng.scene_fir()
        assert np.isfinite(eng.read_scene_fir()).all()
    finally:
        eng.close()
