"""The delay stage of the scene filter mix (include/openpbso_amd.h "scene filter mix"; kernels_fir.hip) on the device: a
ramped fractional delay per object in front of the K-tap filters.  Every comparison is BIT FOR BIT: with the undelayed mix where
the two must agree, with the reference (tests/cpp/scene_fir_delay_ref.c and tests/cpp/scene_fir_ref.c through
tests/scene_fir_delay_model.py, anchored by tests/test_scene_fir_delay_model.py) fed the rows Engine.audio() returned, and with
the scene mix, an independent implementation of the same read."""
import numpy as np
import pytest

from openpbso_amd import capi
from openpbso_amd.solver import PbsoError
from tests.scene_fir_delay_model import Model
from tests.test_gpu_scene_fir import make_engine, same_bits, taps_of

pytestmark = pytest.mark.gpu

B = 513


def step_and_mix(eng, model, nb, label, samples=None):
    eng.step(nb)
    eng.scene_fir()
    rows, got = eng.audio(), eng.read_scene_fir()
    want = model.mix(rows, samples)
    same_bits(got if samples is None else np.ascontiguousarray(got[:, samples]), want, label)
    return got


def refused(status, call, *args):
    with pytest.raises(PbsoError) as ei:
        call(*args)
    assert ei.value.status == status, (call, args)


@pytest.mark.parametrize("zeros", [False, True])
def test_delay_zero_changes_nothing(zeros):
    """40 objects, C = 2, K = 37, onsets up to 700, steps of 2, 1, 2 buffers: the delay stage enabled and never set, or set to
    zeros, gives the bits of the mix without it"""
    n_obj, C, K, max_onset, R = 40, 2, 37, 700, 300
    engs = [make_engine(n_obj, 64, 6, 41) for _ in range(2)]
    rng = np.random.default_rng(41)
    try:
        for e in engs:
            e.scene_fir_enable(C, K, max_onset, R)
        engs[1].scene_fir_delay_enable(1000, 441)
        for k, nb in enumerate((2, 1, 2)):
            if k != 1:
                h, d = taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj)
                for e in engs:
                    e.scene_fir_set(h, d)
            if zeros and k < 2:
                engs[1].scene_fir_set_delay(np.zeros(n_obj))
            outs = []
            for e in engs:
                e.step(nb)
                e.scene_fir()
                outs.append(e.read_scene_fir())
            same_bits(outs[1], outs[0], k)
    finally:
        for e in engs:
            e.close()


def test_an_integer_delay_is_an_onset():
    """33 objects, K = 64, one-buffer steps: onsets D + d without the stage against onsets D behind integer delays d.  The window
    of the filters and the delay both reach into histories two steps back (max_onset + K - 1 and max_delay + 1 exceed 513)"""
    n_obj, C, K = 33, 2, 64
    rng = np.random.default_rng(42)
    D, d = rng.integers(0, 601, n_obj), rng.integers(0, 701, n_obj)
    D[:2], d[:2] = [600, 0], [700, 0]
    h = taps_of(rng, C, n_obj, K)
    engs = [make_engine(n_obj, 64, 5, 42) for _ in range(2)]
    try:
        engs[0].scene_fir_enable(C, K, 1300, 0)
        engs[0].scene_fir_set(h, D + d)
        engs[1].scene_fir_enable(C, K, 600, 0)
        engs[1].scene_fir_delay_enable(700, 250)
        engs[1].scene_fir_set(h, D)
        engs[1].scene_fir_set_delay(d)                   # the first set: no ramp
        for k in range(5):
            outs = []
            for e in engs:
                e.step(1)
                e.scene_fir()
                outs.append(e.read_scene_fir())
            same_bits(outs[1], outs[0], k)
    finally:
        for e in engs:
            e.close()


# the script of the tests below: C = 3, 40 objects, K = 37, strips of 512 samples (one wave per workgroup at these sizes)
N_OBJ, C3, K3, MAX_ONSET, XFADE, MAX_DELAY, RD = 40, 3, 37, 1400, 700, 1200, 600
STEPS = [2, 1, 1, 3, 2]


def _script(rng):
    """per step: (filter set or None, delay set or None)"""
    taps = lambda hi: (taps_of(rng, C3, N_OBJ, K3), rng.integers(0, hi + 1, N_OBJ).astype(np.int32))
    delays = lambda: rng.uniform(0, MAX_DELAY, N_OBJ).astype(np.float32)
    d0 = delays()
    d0[:4] = [0.0, MAX_DELAY, 513.0, 0.5]
    h0, on0 = taps(MAX_ONSET)
    on0[:3] = [0, MAX_ONSET, 513]
    return [((h0, on0), d0),                              # first sets: no fade, no ramp
            (taps(MAX_ONSET), delays()),                 # a delay set in the step of a filter set: a cross-fade over a moving z;
                                                         # the ramp (600) crosses the step boundary (513)
            (None, delays()),                            # a delay set during the running ramp
            (taps(50), None),                            # that ramp ends inside this step
            (None, delays())]


def _run_script(cuts_of, check_model):
    """the script with step k cut into cuts_of[k] (the sets stay at the starts of the steps); returns the concatenated output"""
    eng = make_engine(N_OBJ, 96, sum(STEPS) + 1, 43, time_chunks=1)   # time_chunks = 1: the rows do not depend on the cut
    model = Model(C3, N_OBJ, K3, MAX_ONSET, XFADE, MAX_DELAY, RD) if check_model else None
    script = _script(np.random.default_rng(43))
    outs = []
    try:
        eng.scene_fir_enable(C3, K3, MAX_ONSET, XFADE)
        eng.scene_fir_delay_enable(MAX_DELAY, RD)
        assert eng.scene_fir_delay_info() == {"max_delay": MAX_DELAY, "ramp_samples": RD, "ramp_end": 0, "sets": 0}
        for k, (fs, ds) in enumerate(script):
            if fs is not None:
                eng.scene_fir_set(*fs)
                if model:
                    model.set(*fs)
            if ds is not None:
                eng.scene_fir_set_delay(ds)
                if model:
                    model.set_delay(ds)
            for nb in cuts_of[k]:
                if model:
                    outs.append(step_and_mix(eng, model, nb, ("step", k)))
                    assert eng.scene_fir_delay_info() == model.info(), k
                else:
                    eng.step(nb)
                    eng.scene_fir()
                    outs.append(eng.read_scene_fir())
        return np.concatenate(outs, axis=1)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def script_whole():
    return _run_script([[nb] for nb in STEPS], True)


def test_script_against_the_reference(script_whole):
    """fractional delays; a ramp across a step boundary; a set during a running ramp; a delay set in the step of a filter set;
    the info after every step (all inside _run_script) -- and the model says the ramps ended where the script puts them"""
    assert script_whole.shape == (C3, sum(STEPS) * B) and np.abs(script_whole).max() > 0


@pytest.mark.parametrize("end_at", [511, 512, 513, 1023, 1024, 1025])
def test_ramp_ends_on_either_side_of_a_strip_border(end_at):
    """the ramp of the second delay set is over from sample end_at of its step on (strips of 512): the strip that holds the end
    stages per sample, the next one takes the steady path, and both must give the reference's bits"""
    n_obj, C, K, max_onset, max_delay = 40, 3, 37, 300, 1200
    Rd = end_at + 1                                      # over once t - t_set + 1 >= Rd
    eng = make_engine(n_obj, 96, 5, 44)
    model = Model(C, n_obj, K, max_onset, 0, max_delay, Rd)
    rng = np.random.default_rng(end_at)
    try:
        eng.scene_fir_enable(C, K, max_onset, 0)
        eng.scene_fir_delay_enable(max_delay, Rd)
        h, on = taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj)
        on[:2] = [0, K - 1]                              # (windows that begin exactly at, and K - 1 before, their strip)
        eng.scene_fir_set(h, on)
        model.set(h, on)
        for k, nb in enumerate((1, 3, 1)):
            d = rng.uniform(0, max_delay, n_obj)
            eng.scene_fir_set_delay(d)
            model.set_delay(d)
            step_and_mix(eng, model, nb, (end_at, k))
            assert eng.scene_fir_delay_info() == model.info()
        assert model.info()["sets"] == 3
    finally:
        eng.close()


def test_refusals_and_error_codes():
    n_obj = 5
    eng = make_engine(n_obj, 64, 3, 45)
    try:
        for call, args in ((eng.scene_fir_delay_enable, (10, 0)), (eng.scene_fir_set_delay, (np.zeros(n_obj),)), (eng.scene_fir_delay_info, ())):
            refused(capi.ERR_STATE, call, *args)         # the filter mix is not enabled
        eng.scene_fir_enable(2, 4, 10, 0)
        refused(capi.ERR_STATE, eng.scene_fir_set_delay, np.zeros(n_obj))     # the delay stage is not enabled
        refused(capi.ERR_STATE, eng.scene_fir_delay_info)
        for bad in ((-1, 0), ((1 << 20) + 1, 0), (10, -1), (10, (1 << 20) + 1)):
            refused(capi.ERR_INVALID, eng.scene_fir_delay_enable, *bad)
        eng.scene_fir_delay_enable(1 << 20, 1 << 20)     # the largest of both; replaced by the next enable
        eng.scene_fir_delay_enable(10, 4)
        assert capi.lib().pbso_scene_fir_set_delay(eng._h, None) == capi.ERR_INVALID
        assert capi.lib().pbso_scene_fir_delay_info(eng._h, None) == capi.ERR_INVALID
        ok = np.full(n_obj, 3.25, dtype=np.float32)
        for i, v in ((1, np.nan), (0, np.inf), (4, -0.5), (2, 10.5)):
            bad = ok.copy()
            bad[i] = v
            refused(capi.ERR_INVALID, eng.scene_fir_set_delay, bad)
        assert eng.scene_fir_delay_info()["sets"] == 0
        eng.scene_fir_set_delay(ok)
        eng.scene_fir_set_delay(np.full(n_obj, 10.0))    # at max_delay; replaces the set before it
        assert eng.scene_fir_delay_info()["sets"] == 2
        eng.scene_fir_set(np.ones((2, n_obj, 4)))
        eng.step(1)
        eng.scene_fir()
        refused(capi.ERR_STATE, eng.scene_fir_delay_enable, 10, 4)            # after a mix, without a reset
        eng.scene_fir_set(np.ones((2, n_obj, 4)))        # xfade 0: no fade runs
        eng.scene_fir_set_delay(ok)
        eng.step(1)
        eng.scene_fir()
        assert eng.scene_fir_delay_info() == {"max_delay": 10, "ramp_samples": 4, "ramp_end": 2 * B, "sets": 3}
    finally:
        eng.close()


def test_a_delay_set_is_accepted_while_a_fade_runs():
    n_obj, C, K = 7, 2, 8
    eng = make_engine(n_obj, 64, 4, 46)
    model = Model(C, n_obj, K, 20, 2000, 64, 100)
    rng = np.random.default_rng(46)
    try:
        eng.scene_fir_enable(C, K, 20, 2000)
        eng.scene_fir_delay_enable(64, 100)
        for k in range(3):
            if k < 2:
                h, on = taps_of(rng, C, n_obj, K), rng.integers(0, 21, n_obj)
                eng.scene_fir_set(h, on)
                model.set(h, on)
            else:
                refused(capi.ERR_STATE, eng.scene_fir_set, h, on)            # the fade of 2000 samples is still running ...
            d = rng.uniform(0, 64, n_obj)
            eng.scene_fir_set_delay(d)                   # ... which a delay set does not mind
            model.set_delay(d)
            step_and_mix(eng, model, 1, k)
    finally:
        eng.close()


def test_cuts_between_two_sets_do_not_change_a_bit(script_whole):
    """the same sets at the same step starts, the steps between them cut further: 3 -> 1 + 2, 2 -> 1 + 1"""
    cut = _run_script([[1, 1], [1], [1], [1, 2], [1, 1]], False)
    same_bits(cut, script_whole, "cut")


@pytest.mark.parametrize("n_obj", [1, 33])
def test_unit_tap_equals_the_scene_mix(n_obj):
    """C = 1, K = 1, tap 1, onset 0, fractional delays newly set every step, R_d = 513: fmaf(1, z, acc) = acc + 1 * z with the
    same read and the same grouping as pbso_scene_mix at unit gain -- an independent implementation of the read and its ramp"""
    max_delay, R = 900, 513
    eng = make_engine(n_obj, 64, 6, 47 + n_obj)
    rng = np.random.default_rng(n_obj)
    try:
        eng.scene_fir_enable(1, 1, 0, 0)
        eng.scene_fir_delay_enable(max_delay, R)
        eng.scene_mix_enable(1, max_delay, R)
        eng.scene_fir_set(np.ones((1, n_obj, 1)))
        for k, nb in enumerate((2, 1, 1, 2)):
            d = rng.uniform(0, max_delay, n_obj).astype(np.float32)
            if k == 2:
                d[:] = np.floor(d)                       # whole samples too
            eng.scene_fir_set_delay(d)
            eng.scene_mix_set(np.ones((1, n_obj)), d[None, :])
            eng.step(nb)
            eng.scene_fir()
            eng.scene_mix()
            same_bits(eng.read_scene_fir(), eng.read_scene_mix(), (n_obj, k))
    finally:
        eng.close()


def test_four_wave_launch_shape():
    """1024 objects x 64 modes, 64 buffers in one step (32 groups x 17 strips of 2048: over 512 workgroups, four waves each),
    C = 2, K = 16, delays ramping through the step: a few thousand samples, among them the step's first and last 20 and 20 on
    either side of several strip borders"""
    n_obj, nb, C, K, max_onset, max_delay, Rd = 1024, 64, 2, 16, 100, 300, 20000
    eng = make_engine(n_obj, 64, nb + 1, 48, hits_per_obj=2)
    model = Model(C, n_obj, K, max_onset, 0, max_delay, Rd)
    rng = np.random.default_rng(48)
    try:
        eng.scene_fir_enable(C, K, max_onset, 0)
        eng.scene_fir_delay_enable(max_delay, Rd)
        h, on = taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj)
        eng.scene_fir_set(h, on)
        model.set(h, on)
        for k, nbk in enumerate((1, nb)):                # the first set has no ramp: the long step ramps from it
            d = rng.uniform(0, max_delay, n_obj)
            eng.scene_fir_set_delay(d)
            model.set_delay(d)
            nk = nbk * B
            borders = [2048 * s for s in (1, 2, 9, 10, 16) if 2048 * s + 20 < nk]      # (Rd - 1 = 19999 lies in strip 9)
            samples = np.unique(np.concatenate([np.arange(20), np.arange(nk - 20, nk), rng.choice(nk, min(nk, 2048), replace=False)] +
                                               [b + np.arange(-20, 21) for b in borders] +
                                               ([Rd - 1 + np.arange(-3, 4)] if Rd + 3 < nk else [])))
            step_and_mix(eng, model, nbk, k, samples)
    finally:
        eng.close()


def test_reset_and_re_enable():
    n_obj, C, K, max_onset, max_delay, Rd = 9, 2, 12, 600, 700, 700
    eng = make_engine(n_obj, 64, 6, 49, hits_per_obj=6)
    model = Model(C, n_obj, K, max_onset, 0, max_delay, Rd)
    rng = np.random.default_rng(49)
    try:
        eng.scene_fir_enable(C, K, max_onset, 0)
        eng.scene_fir_delay_enable(max_delay, Rd)
        h, on = taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj)
        for k in range(2):
            eng.scene_fir_set(h, on)
            model.set(h, on)
            d = rng.uniform(0, max_delay, n_obj)
            eng.scene_fir_set_delay(d)
            model.set_delay(d)
            step_and_mix(eng, model, 1, k)
        assert eng.scene_fir_delay_info()["ramp_end"] == B + Rd - 1           # a ramp is running
        eng.scene_fir_reset()
        model.reset()
        assert eng.scene_fir_delay_info() == model.info() == {"max_delay": max_delay, "ramp_samples": Rd, "ramp_end": 0, "sets": 2}
        eng.scene_fir_delay_enable(max_delay, Rd)        # t == 0 again: allowed, and drops the delays
        model = Model(C, n_obj, K, max_onset, 0, max_delay, Rd)
        eng.scene_fir_set_delay(d)
        model.set_delay(d)
        eng.scene_fir_reset()                            # keeps the delays last set: the pending ones
        model.reset()
        eng.scene_fir_set(h, on)                         # (the filters went with the reset)
        model.set(h, on)
        # no delay set: the delays kept by the reset, steady from sample 0, over cleared histories
        step_and_mix(eng, model, 2, "after the reset")
        d2 = rng.uniform(0, max_delay, n_obj)
        eng.scene_fir_set_delay(d2)                      # the first set after the reset: no ramp
        model.set_delay(d2)
        step_and_mix(eng, model, 1, "first set after the reset")
        assert eng.scene_fir_delay_info()["ramp_end"] == 3 * B == model.info()["ramp_end"]
        refused(capi.ERR_STATE, eng.scene_fir_delay_enable, max_delay, Rd)    # after a mix, without a reset
        eng.scene_fir_enable(C, K, max_onset, 0)         # again: drops the delay stage with everything else
        refused(capi.ERR_STATE, eng.scene_fir_set_delay, d2)
        refused(capi.ERR_STATE, eng.scene_fir_delay_info)
    finally:
        eng.close()
