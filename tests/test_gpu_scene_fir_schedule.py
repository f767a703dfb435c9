"""The scene filter mix's schedule (include/openpbso_amd.h "scene filter mix", SCHEDULE; kernels_fir.hip) on the device:
filter sets and delay sets that take effect at any sample of a step.  Every comparison is BIT FOR BIT, and never with the
scheduled engine itself: the reference is the existing models (tests/scene_fir_model.py, tests/scene_fir_delay_model.py through
tests/scene_fir_sched_ref.py) fed the rows Engine.audio() returned, cut at every t_set with a plain set before each piece; or a
second engine driven with plain sets between cut steps.  Objects of 1 .. 8 modes, runs of 3 .. 12 buffers."""
import numpy as np
import pytest

from openpbso_amd import capi
from openpbso_amd.solver import PbsoError
from tests.scene_fir_sched_ref import Piecewise
from tests.test_gpu_scene_fir import make_engine, same_bits, taps_of

pytestmark = pytest.mark.gpu

B = 513


def filter_times(R, n1, total):
    """change points for steps of n1 and total - n1 samples, thinned to the spacing rule t - t_prev + 1 >= R: the step's first
    sample, two exactly R - 1 apart (inside one 512-sample strip for R <= 7), segments of 511, 512 and 513 samples, the step's
    last sample, the next step's first (pending across the boundary; a fade of R = 600 runs across it), and later ones"""
    g = max(R - 1, 1)
    a = 200 + g
    cands = [0, g, 200, a, a + 511, a + 511 + 512, a + 511 + 512 + 513, n1 - 1, n1, n1 + g, n1 + 700, total - 1]
    out = []
    for t in sorted(set(cands)):
        if t < total and (not out or R < 2 or t - out[-1] + 1 >= R):
            out.append(t)
    return out


def delay_times(n1, total):
    """the first set behind the step's start (zeros until then), several inside one window, a ramp (300) cut short by the next
    set, one whose ramp crosses the step boundary, one on the next step's first sample"""
    return [t for t in (5, 100, 130, 131, 700, n1 - 40, n1, n1 + 250, total - 1) if t < total]


def sets_for(rng, C, n_obj, K, max_onset, times):
    taps = np.stack([taps_of(rng, C, n_obj, K) for _ in times])
    onsets = rng.integers(0, max_onset + 1, (len(times), n_obj)).astype(np.int32)
    onsets[0, :min(n_obj, 3)] = [0, max_onset, max_onset // 2][:min(n_obj, 3)]
    return taps, onsets


def step_and_mix(eng, ref, nb, label, frames=B):
    eng.step(nb)
    eng.scene_fir()
    rows, got = eng.audio(), eng.read_scene_fir()
    assert rows.shape[1] == nb * frames
    same_bits(got, ref.mix(rows), label)
    return got


def sched_info(eng):
    return tuple(eng.scene_fir_schedule_info().values())


# ---- 1. against the model ------------------------------------------------------------------------------------------------------

# every N in {1, 33, 70}, C in {1, 2, 3, 8}, K in {1, 17, 128}, R in {0, 2, 7, 600}, with and without the delay stage
CASES = [(1, 1, 1, 0, False), (1, 2, 17, 7, True), (33, 1, 128, 2, True), (33, 2, 17, 600, False), (33, 3, 1, 7, False),
         (33, 8, 17, 0, True), (70, 2, 128, 600, True), (70, 3, 17, 2, False), (70, 8, 128, 7, False), (70, 1, 1, 600, True)]


@pytest.mark.parametrize("n_obj,C,K,R,delay", CASES)
def test_schedule_against_the_model(n_obj, C, K, R, delay):
    """steps of 3 and 3 buffers, everything scheduled before the first; onsets differ between sets; a second batch with
    onset == NULL is scheduled between the steps"""
    max_onset, max_delay, Rd = 300, 400, 300
    n1, total = 3 * B, 6 * B
    rng = np.random.default_rng(1000 * n_obj + 100 * C + K + R)
    ft = filter_times(R, n1, total)
    beyond = [t for t in ft if t >= n1]                               # the first of them is scheduled with the first step's
    first, later = [t for t in ft if t < n1] + beyond[:1], beyond[1:]
    assert len(first) >= 3 and later
    eng = make_engine(n_obj, 1 + (n_obj + C + K) % 8, 6, n_obj + C + K)
    ref = Piecewise(C, n_obj, K, max_onset, R, max_delay if delay else None, Rd)
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        taps, onsets = sets_for(rng, C, n_obj, K, max_onset, first)
        eng.scene_fir_schedule(first, taps, onsets)
        ref.schedule(first, taps, onsets)
        n_delay = 0
        if delay:
            eng.scene_fir_delay_enable(max_delay, Rd)
            dt = delay_times(n1, total)
            dl = rng.uniform(0, max_delay, (len(dt), n_obj)).astype(np.float32)
            dl[1, :min(n_obj, 3)] = [0.0, max_delay, 100.0][:min(n_obj, 3)]
            eng.scene_fir_delay_schedule(dt, dl)
            ref.delay_schedule(dt, dl)
            n_delay = len(dt)
        assert sched_info(eng)[:3] == (0, len(first), n_delay)
        step_and_mix(eng, ref, 3, "first step")
        # the set at the next step's first sample stayed pending, as did the later delay sets
        info = sched_info(eng)
        assert info[:2] == (n1, 1) and info[2] == (sum(t >= n1 for t in delay_times(n1, total)) if delay else 0)
        taps2 = np.stack([taps_of(rng, C, n_obj, K) for _ in later])
        eng.scene_fir_schedule(later, taps2)                          # onset == NULL: the onsets of the set before
        ref.schedule(later, taps2)
        step_and_mix(eng, ref, 3, "second step")
        assert sched_info(eng)[:3] == (total, 0, 0)
        assert eng.scene_fir_info()["sets"] == len(ft)
    finally:
        eng.close()


# ---- 2. every launch shape ---------------------------------------------------------------------------------------------------

def test_four_wave_strips():
    """the launcher's rule is launch_scene_fir's without the fade's factor: four waves (strips of 2048) once ceil(n / 2048) *
    groups >= 512, one wave (strips of 512) below -- every other test here.  1024 one-mode objects x 64 buffers: 17 * 32 = 544.
    Segments shorter than, equal to and longer than a strip; delay sets inside and between windows."""
    n_obj, C, K, R, max_onset, max_delay, Rd, nb = 1024, 2, 5, 40, 60, 90, 300, 64
    rng = np.random.default_rng(64)
    times = [0, 100, 100 + 2048, 100 + 2048 + 2047, 9000, 9000 + 2049, 20000, nb * B - 1]
    dt = [7, 3000, 3100, 3101, 12000, 30000]
    eng = make_engine(n_obj, 1, nb, 64, hits_per_obj=2)
    ref = Piecewise(C, n_obj, K, max_onset, R, max_delay, Rd)
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        eng.scene_fir_delay_enable(max_delay, Rd)
        taps, onsets = sets_for(rng, C, n_obj, K, max_onset, times)
        dl = rng.uniform(0, max_delay, (len(dt), n_obj)).astype(np.float32)
        eng.scene_fir_schedule(times, taps, onsets)
        eng.scene_fir_delay_schedule(dt, dl)
        ref.schedule(times, taps, onsets)
        ref.delay_schedule(dt, dl)
        step_and_mix(eng, ref, nb, "four waves")
    finally:
        eng.close()


# ---- 3. the cut does not matter ------------------------------------------------------------------------------------------------

N3, C3, K3, R3, ON3, MD3, RD3, NB3 = 40, 3, 37, 150, 700, 600, 400, 6


def _cut_run(cuts, up_front):
    rng = np.random.default_rng(3)
    ft = filter_times(R3, 2 * B, NB3 * B)
    dt = delay_times(2 * B, NB3 * B)
    taps, onsets = sets_for(rng, C3, N3, K3, ON3, ft)
    dl = rng.uniform(0, MD3, (len(dt), N3)).astype(np.float32)
    eng = make_engine(N3, 8, NB3, 3, time_chunks=1)                   # time_chunks = 1: the rows do not depend on the cut
    outs = []
    try:
        eng.scene_fir_enable(C3, K3, ON3, R3)
        eng.scene_fir_delay_enable(MD3, RD3)
        if up_front:
            eng.scene_fir_schedule(ft, taps, onsets)
            eng.scene_fir_delay_schedule(dt, dl)
        t = 0
        for nb in cuts:
            if not up_front:                                         # what lies inside the next step, just before it
                for k, ts in enumerate(ft):
                    if t <= ts < t + nb * B:
                        eng.scene_fir_set_at(ts, taps[k], onsets[k])
                ks = [k for k, ts in enumerate(dt) if t <= ts < t + nb * B]
                eng.scene_fir_delay_schedule([dt[k] for k in ks], dl[ks])
            eng.step(nb)
            eng.scene_fir()
            outs.append((eng.audio(), eng.read_scene_fir()))
            t += nb * B
        return np.concatenate([r for r, _ in outs], axis=1), np.concatenate([y for _, y in outs], axis=1)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def one_step():
    rows, out = _cut_run([NB3], True)
    rows.setflags(write=False)
    out.setflags(write=False)
    return rows, out


@pytest.mark.parametrize("cuts,up_front", [([1] * NB3, True), ([3, 3], True), ([1] * NB3, False), ([3, 3], False)])
def test_the_cut_into_steps_does_not_matter(one_step, cuts, up_front):
    rows, out = _cut_run(cuts, up_front)
    assert np.array_equal(rows, one_step[0])                          # (the precondition: the same rows)
    same_bits(out, one_step[1], (cuts, up_front))


def test_the_one_step_run_equals_the_model(one_step):
    rng = np.random.default_rng(3)
    ft = filter_times(R3, 2 * B, NB3 * B)
    dt = delay_times(2 * B, NB3 * B)
    taps, onsets = sets_for(rng, C3, N3, K3, ON3, ft)
    dl = rng.uniform(0, MD3, (len(dt), N3)).astype(np.float32)
    ref = Piecewise(C3, N3, K3, ON3, R3, MD3, RD3)
    ref.schedule(ft, taps, onsets)
    ref.delay_schedule(dt, dl)
    same_bits(one_step[1], ref.mix(one_step[0]), "one step")


# ---- 4. equivalences with plain sets ---------------------------------------------------------------------------------------------

def _state(eng):
    """what the next set starts from, as far as the host tells: the clock, the running fade's and ramps' ends"""
    return eng.scene_fir_info()["t"], eng.scene_fir_info()["fade_end"], eng.scene_fir_delay_info()["ramp_end"]


def _plain_and_scheduled(n_obj=33, seed=4):
    return make_engine(n_obj, 4, 8, seed, time_chunks=1), make_engine(n_obj, 4, 8, seed, time_chunks=1)


def test_sets_on_buffer_boundaries_equal_plain_sets_between_one_buffer_steps():
    n_obj, C, K, R, max_onset, max_delay, Rd, nb = 33, 2, 17, 300, 200, 300, 700, 5
    rng = np.random.default_rng(4)
    taps, onsets = sets_for(rng, C, n_obj, K, max_onset, range(nb))
    dl = rng.uniform(0, max_delay, (nb, n_obj)).astype(np.float32)
    plain, sched = _plain_and_scheduled()
    try:
        for e in (plain, sched):
            e.scene_fir_enable(C, K, max_onset, R)
            e.scene_fir_delay_enable(max_delay, Rd)
        sched.scene_fir_schedule([b * B for b in range(nb)], taps, onsets)
        sched.scene_fir_delay_schedule([b * B for b in range(nb)], dl)
        sched.step(nb)
        sched.scene_fir()
        outs, rows = [], []
        for b in range(nb):
            plain.scene_fir_set(taps[b], onsets[b])
            plain.scene_fir_set_delay(dl[b])
            plain.step(1)
            plain.scene_fir()
            outs.append(plain.read_scene_fir())
            rows.append(plain.audio())
        assert np.array_equal(sched.audio(), np.concatenate(rows, axis=1))
        same_bits(sched.read_scene_fir(), np.concatenate(outs, axis=1), "boundaries")
        assert _state(sched) == _state(plain)
    finally:
        plain.close()
        sched.close()


def test_set_at_the_next_sample_and_a_plain_set_after_a_drained_schedule():
    """set_at at the next mixed sample with nothing pending is a plain set; after a schedule drained mid-fade the plain filter set
    is refused until the fade is over, as ever, and the plain delay set continues mid-ramp: both engines go on alike"""
    n_obj, C, K, R, max_onset, max_delay, Rd = 33, 2, 17, 700, 100, 300, 900
    rng = np.random.default_rng(5)
    taps, onsets = sets_for(rng, C, n_obj, K, max_onset, range(4))
    dl = rng.uniform(0, max_delay, (4, n_obj)).astype(np.float32)
    plain, sched = _plain_and_scheduled(seed=5)
    try:
        for e in (plain, sched):
            e.scene_fir_enable(C, K, max_onset, R)
            e.scene_fir_delay_enable(max_delay, Rd)
        outs = [[], []]

        def both(nb):
            for i, e in enumerate((plain, sched)):
                e.step(nb)
                e.scene_fir()
                outs[i].append(e.read_scene_fir())

        plain.scene_fir_set(taps[0], onsets[0])
        plain.scene_fir_set_delay(dl[0])
        sched.scene_fir_set_at(0, taps[0], onsets[0])
        sched.scene_fir_set_delay_at(0, dl[0])
        both(1)
        # the second pair of sets: plain between two steps, scheduled inside the longer step at the same sample
        sched.scene_fir_set_at(2 * B, taps[1], onsets[1])
        sched.scene_fir_set_delay_at(2 * B, dl[1])
        with pytest.raises(PbsoError) as ei:
            sched.scene_fir_set(taps[2])                              # a scheduled set of its kind is pending
        assert ei.value.status == capi.ERR_STATE
        with pytest.raises(PbsoError) as ei:
            sched.scene_fir_set_delay(dl[2])
        assert ei.value.status == capi.ERR_STATE
        plain.step(1)
        plain.scene_fir()
        outs[0].append(plain.read_scene_fir())
        plain.scene_fir_set(taps[1], onsets[1])
        plain.scene_fir_set_delay(dl[1])
        plain.step(1)
        plain.scene_fir()
        outs[0].append(plain.read_scene_fir())
        sched.step(2)
        sched.scene_fir()
        outs[1].append(sched.read_scene_fir())
        # t = 3 B: the fade (700) and the ramp (900) of the sets at 2 B are both running
        assert _state(sched) == _state(plain) == (3 * B, 2 * B + R - 1, 2 * B + Rd - 1)
        for e in (plain, sched):
            with pytest.raises(PbsoError) as ei:                      # mid-fade: refused on both
                e.scene_fir_set(taps[2])
            assert ei.value.status == capi.ERR_STATE
            e.scene_fir_set_delay(dl[2])                              # mid-ramp: from the current value
        both(1)
        assert _state(sched) == _state(plain)
        for e in (plain, sched):
            e.scene_fir_set(taps[2])                                  # onset None: what the schedule left
            e.scene_fir_set_delay(dl[3])
        both(2)
        same_bits(np.concatenate(outs[1], axis=1), np.concatenate(outs[0], axis=1), "plain and scheduled")
    finally:
        plain.close()
        sched.close()


# ---- 5. refusals, and the mixer that never uses the schedule -------------------------------------------------------------------

def _refused(status, call, *args):
    with pytest.raises(PbsoError) as ei:
        call(*args)
    assert ei.value.status == status, (call, args)


def test_refused_calls_change_nothing():
    n_obj, C, K, R, max_onset, max_delay, Rd = 5, 2, 3, 10, 50, 60, 20
    rng = np.random.default_rng(6)
    a, twin = make_engine(n_obj, 4, 8, 6), make_engine(n_obj, 4, 8, 6)
    h = taps_of(rng, C, n_obj, K)
    h3 = np.stack([h, 2 * h, 3 * h])
    on = np.full(n_obj, 7, dtype=np.int32)
    dl = np.full(n_obj, 2.5, dtype=np.float32)
    try:
        for e in (a, twin):
            e.scene_fir_enable(C, K, max_onset, R)
        _refused(capi.ERR_STATE, a.scene_fir_set_delay_at, 0, dl)    # a delay schedule without the stage
        _refused(capi.ERR_STATE, a.scene_fir_delay_schedule, [0, 5], np.stack([dl, dl]))
        for e in (a, twin):
            e.scene_fir_delay_enable(max_delay, Rd)
            e.scene_fir_set_at(0, h, on)
            e.scene_fir_set_delay_at(3, dl)
        assert sched_info(a) == (0, 1, 1, R - 1)
        bad = h3.copy()
        bad[2, 1, 2, 1] = np.nan
        for args in (([20, 40, 30], h3), ([20, 30, 30], h3),          # descending, equal
                     ([R - 2, 40, 60], h3),                           # inside the fade of the pending set at 0
                     ([20, 20 + R - 2, 60], h3),                      # ... of its own predecessor
                     ([20, 40, 60], bad),
                     ([20, 40, 60], h3, np.stack([on, on, on + max_onset]))):
            _refused(capi.ERR_INVALID, a.scene_fir_schedule, *args)
        _refused(capi.ERR_INVALID, a.scene_fir_set_at, -1, h)
        _refused(capi.ERR_INVALID, a.scene_fir_delay_schedule, [4, 4], np.stack([dl, dl]))
        _refused(capi.ERR_INVALID, a.scene_fir_delay_schedule, [4, 5], np.stack([dl, dl + max_delay]))
        _refused(capi.ERR_INVALID, a.scene_fir_set_delay_at, 3, dl)  # not behind the pending one
        assert sched_info(a) == (0, 1, 1, R - 1) == sched_info(twin)
        a.scene_fir_schedule([], np.zeros((0, C, n_obj, K)))         # n_sets == 0 is accepted
        for e in (a, twin):
            e.scene_fir_schedule([R - 1, 2 * R - 2], h3[1:])         # exactly R - 1 apart: accepted
            e.step(2)
            e.scene_fir()
        same_bits(a.read_scene_fir(), twin.read_scene_fir(), "after the refusals")
        assert sched_info(a) == (2 * B, 0, 0, 2 * B) == sched_info(twin)
        _refused(capi.ERR_INVALID, a.scene_fir_set_at, 2 * B - 1, h)  # before the clock
        # clear_schedule drops both kinds; the reset drops them too
        a.scene_fir_set_at(3 * B, h)
        a.scene_fir_set_delay_at(3 * B, dl)
        assert sched_info(a)[1:3] == (1, 1)
        a.scene_fir_clear_schedule()
        assert sched_info(a) == sched_info(twin)
        a.scene_fir_set_at(3 * B, h)
        a.scene_fir_reset()
        twin.scene_fir_reset()
        assert sched_info(a) == (0, 0, 0, 0) == sched_info(twin)
        for e in (a, twin):
            e.scene_fir_set(h, on)
            e.step(1)
            e.scene_fir()
        same_bits(a.read_scene_fir(), twin.read_scene_fir(), "after the reset")
    finally:
        a.close()
        twin.close()


def test_more_than_4096_filter_sets_in_a_step_are_refused_and_nothing_changes():
    """one object, one tap: 4097 sets at consecutive samples of a 9-buffer step"""
    eng = make_engine(1, 2, 9, 7)
    ref = Piecewise(1, 1, 1, 0, 0)
    try:
        eng.scene_fir_enable(1, 1, 0, 0)
        times = np.arange(4097)
        taps = np.linspace(0.5, 1.5, 4097, dtype=np.float32).reshape(4097, 1, 1, 1)
        eng.scene_fir_schedule(times, taps)
        eng.step(9)
        _refused(capi.ERR_INVALID, eng.scene_fir)
        assert sched_info(eng) == (0, 4097, 0, 4097) and eng.scene_fir_info()["mixes"] == 0
        eng.scene_fir_clear_schedule()
        eng.scene_fir_schedule(times[:4096], taps[:4096])            # the cap itself is accepted: the same step, now mixed
        ref.schedule(times[:4096], taps[:4096])
        eng.scene_fir()
        same_bits(eng.read_scene_fir(), ref.mix(eng.audio()), "4096 sets")
        assert sched_info(eng) == (9 * B, 0, 0, 9 * B)
    finally:
        eng.close()


def test_an_unscheduled_mixer_is_what_it_was():
    """plain sets only, with the schedule's calls made and withdrawn around them (an empty schedule, a set scheduled and cleared,
    sets scheduled beyond every step that is mixed): bit for bit the twin that never called them"""
    n_obj, C, K, R, max_onset, max_delay, Rd = 40, 2, 37, 300, 400, 500, 441
    rng = np.random.default_rng(8)
    a, twin = make_engine(n_obj, 6, 6, 8), make_engine(n_obj, 6, 6, 8)
    try:
        for e in (a, twin):
            e.scene_fir_enable(C, K, max_onset, R)
            e.scene_fir_delay_enable(max_delay, Rd)
        for k, nb in enumerate((2, 1, 2)):
            h, on = taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj).astype(np.int32)
            dl = rng.uniform(0, max_delay, n_obj).astype(np.float32)
            a.scene_fir_clear_schedule()
            a.scene_fir_schedule([], np.zeros((0, C, n_obj, K)))
            a.scene_fir_set_at(10 ** 9, h, on)
            a.scene_fir_set_delay_at(10 ** 9, dl)
            a.scene_fir_clear_schedule()
            for e in (a, twin):
                if k != 1:
                    e.scene_fir_set(h, on)
                e.scene_fir_set_delay(dl)
            a.scene_fir_set_delay_at(10 ** 9 + k, dl)                 # pending beyond the step: the step is launched as ever
            for e in (a, twin):
                e.step(nb)
                e.scene_fir()
            same_bits(a.read_scene_fir(), twin.read_scene_fir(), k)
        assert a.scene_fir_info()["fade_end"] == twin.scene_fir_info()["fade_end"]
    finally:
        a.close()
        twin.close()


# ---- 6. other buffer lengths -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [27, 864])
def test_other_buffer_lengths(frames):
    """27 frames with a filter set and a delay set every buffer, at its samples 5 and 11: a 512-sample window spans nineteen
    blocks of delay records; 864 frames with sets on and off the strip grid.  Steps of 5, 1 and 6 buffers (27) or 2, 1 and 1"""
    n_obj, C, K, max_onset, max_delay = 37, 3, 17, 30, 60
    R, Rd = (20, 40) if frames == 27 else (300, 700)
    steps = (5, 1, 6) if frames == 27 else (2, 1, 1)
    total = sum(steps) * frames
    if frames == 27:
        ft, dt = [27 * k + 5 for k in range(12)], [27 * k + 11 for k in range(12)]
    else:
        ft, dt = [0, 511, 1023, 1728, 2240, 3455], [3, 500, 512, 513, 1728, 2000, 3000]
    rng = np.random.default_rng(frames)
    eng = make_engine(n_obj, 4, sum(steps), 11, form=capi.FORM_VELOCITY, frames_per_buffer=frames)
    ref = Piecewise(C, n_obj, K, max_onset, R, max_delay, Rd)
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        eng.scene_fir_delay_enable(max_delay, Rd)
        taps, onsets = sets_for(rng, C, n_obj, K, max_onset, ft)
        dl = rng.uniform(0, max_delay, (len(dt), n_obj)).astype(np.float32)
        eng.scene_fir_schedule(ft, taps, onsets)
        eng.scene_fir_delay_schedule(dt, dl)
        ref.schedule(ft, taps, onsets)
        ref.delay_schedule(dt, dl)
        for k, nb in enumerate(steps):
            step_and_mix(eng, ref, nb, (frames, k), frames)
        assert sched_info(eng)[:3] == (total, 0, 0)
    finally:
        eng.close()
