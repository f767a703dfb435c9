"""The scene mix's schedule (include/openpbso_amd.h "The scene mix's SCHEDULE"; scene_schedule_expand_kernel and the schedule-aware
stage 1 of kernels_mix.hip) on the device, every output compared BIT FOR BIT: with the reference model
(tests/scene_mix_sched_model.py, anchored by tests/test_scene_mix_sched_model.py on the scene mix's own reference), between
different cuts of the same samples into steps, with today's pbso_scene_mix_set between cut steps, and -- for every refused call --
with a twin engine that never saw the call.  Objects of 64 modes, at most 70 of them, at most 12 buffers."""
import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from tests.scene_mix_sched_model import SchedModel

pytestmark = pytest.mark.gpu
B = 513


def make_engine(n_obj, nb_total, seed, n_modes=64, **kw):
    eng = Engine(**kw)
    for i in range(n_obj):
        eng.add_object(synth.eigenvalues(n_modes, 8000 + 131 * seed + i), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    rng = np.random.default_rng(seed)
    for i in range(n_obj):
        eng.set_use_transfer(i, False)
        for t in [0] + sorted(int(x) for x in rng.integers(1, max(nb_total, 2), 2)):
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(n_modes) * 1e-3), t)
    return eng


def same_bits(got, want, label):
    assert got.shape == want.shape, label
    assert np.abs(want).max() > 0, label
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (label, bad.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def signed(rng, lo, hi, shape):
    return (rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def set_at_both(eng, model, t, gain, delay=None):
    eng.scene_mix_set_at(t, gain, delay)
    model.set_at(t, gain, delay)


def step_and_mix(eng, model, nb, label, frames=B):
    """one step of nb buffers through the engine's mixer and, with the same rows, through the model -> (the mix, the rows)"""
    eng.step(nb)
    eng.scene_mix()
    rows = eng.audio()
    got = eng.read_scene_mix()
    assert got.shape == (model.C, nb * frames) and np.abs(rows).max(axis=1).min() > 0, label
    same_bits(got, model.mix(rows), label)
    return got, rows


def info(eng):
    v = eng.scene_mix_info()
    return v["t"], v["pending"], v["mixes"], v["sets"]


# ---- 1. against the reference model ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_obj", [1, 37, 70])
@pytest.mark.parametrize("C", [1, 2, 3, 5, 8])
def test_schedule_against_the_model(C, n_obj):
    """batches of 8, 4, 2 and 1 objects; one object, a ragged second group, three groups.  Steps of 3, 2, 1 and 2 buffers, every
    set given before the first step: at the step's local samples 0, 1, 63, 64 and 65 (a tile of three blocks, a set at a tile's
    first sample), 513 + 17 and 2 * 513 + 17, 700 and 703 (two sets inside one tile, the first of gains only and during the delay
    ramp that began at 530), at the step's last sample; one that waits for the second step, and one of gains only exactly at
    the third step's first sample.  The last step has no set inside it: the plain kernels, from what the schedule left."""
    max_delay, R = 1400, 700
    rng = np.random.default_rng(1000 + 10 * C + n_obj)
    eng = make_engine(n_obj, 8, C)
    model = SchedModel(C, n_obj, max_delay, R)
    try:
        eng.scene_mix_enable(C, max_delay, R)
        times = [(0, True), (1, True), (63, False), (64, True), (65, True), (B + 17, True), (700, False), (703, True),
                 (2 * B + 17, True), (3 * B - 1, True), (3 * B + 100, True), (5 * B, False)]
        for t, with_delay in times:
            d = rng.uniform(0, max_delay, (C, n_obj)).astype(np.float32) if with_delay else None
            if t == 0:
                d[0, 0], d[C - 1, n_obj - 1] = 513.25, max_delay
            set_at_both(eng, model, t, signed(rng, 0.1, 1.5, (C, n_obj)), d)
        assert info(eng) == (0, 12, 0, 12)
        step_and_mix(eng, model, 3, "ten sets inside the step")
        assert info(eng) == (3 * B, 2, 1, 12)
        step_and_mix(eng, model, 2, "the set that waited")
        assert info(eng) == (5 * B, 1, 2, 12)
        step_and_mix(eng, model, 1, "a set at the step's first sample")
        assert info(eng) == (6 * B, 0, 3, 12)
        step_and_mix(eng, model, 2, "no set inside the step")
    finally:
        eng.close()


# ---- 2. the cut does not matter ----------------------------------------------------------------------------------------------

SCHED_T = [0, 300, B, 1000, 1003, 4 * B + 17, 5 * B - 1, 5 * B, 7 * B + 64, 11 * B + 512]


def _cut_run(cuts, up_front):
    """12 buffers of 37 objects at C = 2 stepped in `cuts`, the schedule SCHED_T given up front or step by step (before each step
    the sets that fall into it, and the one after them) -> (mix, rows, what the model says for these rows)"""
    n_obj, C, max_delay, R = 37, 2, 900, 700
    rng = np.random.default_rng(31)
    g = signed(rng, 0.1, 1.5, (len(SCHED_T), C, n_obj))
    d = rng.uniform(0, max_delay, (len(SCHED_T), C, n_obj)).astype(np.float32)
    eng = make_engine(n_obj, 12, 5, time_chunks=1)        # time_chunks = 1: the rows themselves do not depend on the cut
    model = SchedModel(C, n_obj, max_delay, R)
    try:
        eng.scene_mix_enable(C, max_delay, R)
        model.schedule(SCHED_T, g, d)
        given = 0
        if up_front:
            eng.scene_mix_schedule(SCHED_T, g, d)
            given = len(SCHED_T)
        mixes, rows, a = [], [], 0
        for nb in cuts:
            upto = given
            while upto < len(SCHED_T) and SCHED_T[upto] < (a + nb) * B:
                upto += 1
            upto = min(upto + 1, len(SCHED_T))                       # (and one that stays pending beyond this step)
            if upto > given:
                eng.scene_mix_schedule(SCHED_T[given:upto], g[given:upto], d[given:upto])
                given = upto
            eng.step(nb)
            eng.scene_mix()
            mixes.append(eng.read_scene_mix())
            rows.append(eng.audio())
            a += nb
        assert info(eng) == (12 * B, 0, len(cuts), len(SCHED_T))
        rows = np.concatenate(rows, axis=1)
        return np.concatenate(mixes, axis=1), rows, model.mix(rows)
    finally:
        eng.close()


@pytest.mark.parametrize("up_front", [True, False])
def test_the_cut_into_steps_does_not_matter(up_front):
    base_mix, base_rows, want = _cut_run([12], up_front)
    same_bits(base_mix, want, "one step against the model")
    for cuts in ([1] * 12, [4] * 3, [5, 7]):
        mix, rows, _ = _cut_run(cuts, up_front)
        assert np.array_equal(rows, base_rows), cuts                 # (the precondition: the same rows)
        same_bits(mix, base_mix, cuts)


# ---- 3. equals today's API ---------------------------------------------------------------------------------------------------

def test_sets_on_buffer_boundaries_equal_plain_sets_between_one_buffer_steps():
    n_obj, C, max_delay, R = 37, 3, 1200, 700
    at = [0, 3, 4, 9]
    rng = np.random.default_rng(41)
    g = signed(rng, 0.1, 1.5, (len(at), C, n_obj))
    d = rng.uniform(0, max_delay, (len(at), C, n_obj)).astype(np.float32)
    one = make_engine(n_obj, 12, 6, time_chunks=1)
    cut = make_engine(n_obj, 12, 6, time_chunks=1)
    try:
        one.scene_mix_enable(C, max_delay, R)
        cut.scene_mix_enable(C, max_delay, R)
        one.scene_mix_schedule([b * B for b in at], g, d)
        one.step(12)
        one.scene_mix()
        mixes, rows = [], []
        for b in range(12):
            if b in at:
                cut.scene_mix_set(g[at.index(b)], d[at.index(b)])
            cut.step(1)
            cut.scene_mix()
            mixes.append(cut.read_scene_mix())
            rows.append(cut.audio())
        assert np.array_equal(one.audio(), np.concatenate(rows, axis=1))
        same_bits(one.read_scene_mix(), np.concatenate(mixes, axis=1), "schedule in one step against plain sets")
        assert info(one) == (12 * B, 0, 1, 4) and info(cut) == (12 * B, 0, 12, 4)
    finally:
        one.close()
        cut.close()


def test_set_at_the_next_sample_with_nothing_pending_equals_a_plain_set():
    """before steps of 2, 1 and 3 buffers, the first set after the enable included (no ramp), one of gains only"""
    n_obj, C, max_delay, R = 9, 2, 300, 400
    rng = np.random.default_rng(43)
    plain = make_engine(n_obj, 6, 7)
    sched = make_engine(n_obj, 6, 7)
    try:
        plain.scene_mix_enable(C, max_delay, R)
        sched.scene_mix_enable(C, max_delay, R)
        for k, nb in enumerate((2, 1, 3)):
            g = signed(rng, 0.1, 1.5, (C, n_obj))
            d = None if k == 1 else rng.uniform(0, max_delay, (C, n_obj)).astype(np.float32)
            plain.scene_mix_set(g, d)
            t = info(sched)[0]
            assert t == info(plain)[0]
            sched.scene_mix_set_at(t, g, d)
            assert info(sched)[1] == 1
            for e in (plain, sched):
                e.step(nb)
                e.scene_mix()
            assert np.array_equal(plain.audio(), sched.audio())
            same_bits(sched.read_scene_mix(), plain.read_scene_mix(), k)
            assert info(sched) == info(plain)
    finally:
        plain.close()
        sched.close()


# ---- 4. a plain set after a drained schedule ---------------------------------------------------------------------------------

def test_a_plain_set_after_a_drained_schedule_continues_mid_ramp():
    """R = 900: the plain set before the second step lands 313 samples into the ramp of the set scheduled at 513 + 200; then a
    reset keeps the targets last in force, and a schedule after it begins without a ramp"""
    n_obj, C, max_delay, R = 37, 2, 600, 900
    rng = np.random.default_rng(47)
    eng = make_engine(n_obj, 6, 8)
    model = SchedModel(C, n_obj, max_delay, R)
    new = lambda: (signed(rng, 0.1, 1.5, (C, n_obj)), rng.uniform(0, max_delay, (C, n_obj)).astype(np.float32))
    try:
        eng.scene_mix_enable(C, max_delay, R)
        set_at_both(eng, model, 0, *new())
        set_at_both(eng, model, B + 200, *new())
        step_and_mix(eng, model, 2, "the schedule")
        g, d = new()
        eng.scene_mix_set(g, d)
        model.set(g, d)
        step_and_mix(eng, model, 1, "the plain set, from mid-ramp")
        set_at_both(eng, model, 3 * B + 5, *new())
        step_and_mix(eng, model, 1, "a scheduled set during the plain set's ramp")
        set_at_both(eng, model, 4 * B + 100, *new())                 # ... in force from sample 100 of the next step on
        step_and_mix(eng, model, 1, "one more, which the reset has to keep")
        set_at_both(eng, model, 6 * B, *new())                       # never in force: dropped by the reset
        eng.scene_mix_reset()
        model.reset()
        assert info(eng)[:2] == (0, 0)
        step_and_mix(eng, model, 1, "after the reset: the targets last in force")
        set_at_both(eng, model, B + 7, *new())
        step_and_mix(eng, model, 1, "the first set after the reset: no ramp, inside the step")
    finally:
        eng.close()


# ---- 5. refusals, each against an untouched twin ------------------------------------------------------------------------------

def _refused(status, call, *args):
    with pytest.raises(PbsoError) as ei:
        call(*args)
    assert ei.value.status == status, (call.__name__, args[:1], ei.value)


def test_refused_calls_change_nothing():
    n_obj, C, max_delay, R = 9, 2, 100, 50
    rng = np.random.default_rng(53)
    a, twin = make_engine(n_obj, 8, 9), make_engine(n_obj, 8, 9)
    g = signed(rng, 0.1, 1.5, (3, C, n_obj))
    d = rng.uniform(0, max_delay, (3, C, n_obj)).astype(np.float32)
    nan_g, big_d = g.copy(), d.copy()
    nan_g[1, 1, 4] = np.nan
    big_d[1, 0, 2] = max_delay + 0.5

    def both_step(label):
        for e in (a, twin):
            e.step(1)
            e.scene_mix()
        assert np.array_equal(a.audio(), twin.audio())
        same_bits(a.read_scene_mix(), twin.read_scene_mix(), label)

    try:
        for call, args in ((a.scene_mix_set_at, (0, g[0], d[0])), (a.scene_mix_schedule, ([0, 5], g[:2], d[:2])),
                           (a.scene_mix_clear_schedule, ()), (a.scene_mix_info, ())):
            _refused(capi.ERR_STATE, call, *args)                    # before the enable
        a.scene_mix_enable(C, max_delay, R)
        twin.scene_mix_enable(C, max_delay, R)
        assert info(a) == (0, 0, 0, 0)
        for e in (a, twin):
            e.scene_mix_schedule([10, B + 87], g[:2], d[:2])
        assert info(a) == (0, 2, 0, 2)
        _refused(capi.ERR_INVALID, a.scene_mix_set_at, B + 87, g[2], d[2])                    # equal to the last pending one
        _refused(capi.ERR_INVALID, a.scene_mix_set_at, B + 86, g[2], d[2])                    # before it
        _refused(capi.ERR_INVALID, a.scene_mix_schedule, [700, 700], g[:2], d[:2])            # equal inside one call
        _refused(capi.ERR_INVALID, a.scene_mix_schedule, [700, 650], g[:2], d[:2])            # descending inside one call
        _refused(capi.ERR_INVALID, a.scene_mix_set_at, 800, nan_g[1], d[1])                   # a gain that is not finite
        _refused(capi.ERR_INVALID, a.scene_mix_set_at, 800, g[1], big_d[1])                   # a delay above max_delay
        _refused(capi.ERR_INVALID, a.scene_mix_schedule, [800, 900, 1000], nan_g, d)          # one bad set in the middle
        _refused(capi.ERR_INVALID, a.scene_mix_schedule, [800, 900, 1000], g, big_d)
        _refused(capi.ERR_STATE, a.scene_mix_set, g[2], d[2])                                 # a plain set while sets are pending
        assert info(a) == (0, 2, 0, 2) == info(twin)
        both_step("after refused calls")
        assert info(a) == (B, 1, 1, 2)
        _refused(capi.ERR_INVALID, a.scene_mix_set_at, B - 1, g[2], d[2])                     # in the past
        _refused(capi.ERR_STATE, a.scene_mix_set, g[2], d[2])
        both_step("the set that stayed pending")
        assert info(a) == (2 * B, 0, 2, 2) == info(twin)
        _refused(capi.ERR_INVALID, a.scene_mix_set_at, 2 * B - 1, g[2], d[2])                 # in the past, nothing pending
        # clear_schedule drops the pending sets: the twin never had them
        a.scene_mix_schedule([2 * B + 30, 2 * B + 60], g[1:], d[1:])
        assert info(a) == (2 * B, 2, 2, 4)
        a.scene_mix_clear_schedule()
        assert info(a) == (2 * B, 0, 2, 4)
        both_step("after clear_schedule")
        for e in (a, twin):                                          # (and a plain set is accepted again)
            e.scene_mix_set(g[2], d[2])
        both_step("a plain set after clear_schedule")
        # the reset drops them too, and keeps the targets last in force
        a.scene_mix_set_at(4 * B + 20, g[0], d[0])
        a.scene_mix_reset()
        twin.scene_mix_reset()
        assert info(a) == (0, 0, 4, 6) and info(twin) == (0, 0, 4, 3)
        both_step("after the reset")
        # ... and so does a new enable
        a.scene_mix_set_at(B + 20, g[0], d[0])
        for e in (a, twin):
            e.scene_mix_enable(C, max_delay, R)
        assert info(a) == (0, 0, 0, 0)
        for e in (a, twin):
            e.scene_mix_set_at(40, g[1], d[1])
        both_step("after a new enable")
        assert info(a) == (B, 0, 1, 1) == info(twin)
    finally:
        a.close()
        twin.close()


# ---- 6. other buffer lengths -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("frames", [27, 864])
def test_other_buffer_lengths(frames):
    """27 frames with a set every buffer, at its sample 5: every 64-sample tile spans three blocks of records; 864 frames with sets
    on and off the tile grid.  Steps of 5, 1 and 6 buffers (27) or 2, 1 and 1 (864).  The 27-frame run is 324 samples long: its
    delays stay below 80 samples (three buffers back), so that every step hears its objects."""
    n_obj, C, max_delay, R = 37, 3, 1400, 100 if frames == 27 else 700
    steps = (5, 1, 6) if frames == 27 else (2, 1, 1)
    times = [27 * k + 5 for k in range(12)] if frames == 27 else [0, 63, 128, 863, 864, 1000, 2 * 864 + 320, 3 * 864 + 863]
    rng = np.random.default_rng(frames)
    eng = make_engine(n_obj, sum(steps), 11, form=capi.FORM_VELOCITY, frames_per_buffer=frames)
    model = SchedModel(C, n_obj, max_delay, R)
    try:
        eng.scene_mix_enable(C, max_delay, R)
        g = signed(rng, 0.1, 1.5, (len(times), C, n_obj))
        d = rng.uniform(0, 80 if frames == 27 else max_delay, (len(times), C, n_obj)).astype(np.float32)
        eng.scene_mix_schedule(times, g, d)
        model.schedule(times, g, d)
        for k, nb in enumerate(steps):
            step_and_mix(eng, model, nb, (frames, k), frames)
        assert info(eng) == (sum(steps) * frames, 0, len(steps), len(times))
    finally:
        eng.close()


# ---- 7. a device group -------------------------------------------------------------------------------------------------------

def test_loopback_group_schedule_in_one_step_equals_cut_steps_with_plain_sets():
    from openpbso_amd.group import Group
    from tests.test_gpu_group_scene_mix import _feed, _scene
    modes = [64] * 5
    at = [0, 2, 3]
    C, max_delay, R, nb_total = 2, 800, 600, 6
    lams, shapes, hits, vns = _scene(modes, nb_total, 61)
    rng = np.random.default_rng(61)
    g = signed(rng, 0.1, 1.0, (len(at), C, len(modes)))
    d = rng.uniform(0, max_delay, (len(at), C, len(modes))).astype(np.float32)
    with Group([0, 0], transport=capi.GROUP_LOOPBACK, time_chunks=1) as one, Group([0, 0], transport=capi.GROUP_LOOPBACK, time_chunks=1) as cut:
        for grp in (one, cut):
            _feed(None, grp, modes, lams, shapes, hits, vns)
            grp.scene_mix_enable(C, max_delay, R)
        one.scene_mix_set_at(0, g[0], d[0])
        one.scene_mix_schedule([b * B for b in at[1:]], g[1:], d[1:])
        assert tuple(one.scene_mix_info().values()) == (0, 3, 0, 3)
        one.step(nb_total)
        one.gather(capi.GATHER_ALL)
        rows_one = one.result(0)
        one.gather(capi.GATHER_SCENE)
        assert tuple(one.scene_mix_info().values()) == (nb_total * B, 0, 1, 3)
        mixes, rows = [[], []], []
        edges = at + [nb_total]
        for k in range(len(at)):
            cut.scene_mix_set(g[k], d[k])
            cut.step(edges[k + 1] - edges[k])
            cut.gather(capi.GATHER_ALL)
            rows.append(cut.result(0))
            cut.gather(capi.GATHER_SCENE)
            for r in range(2):
                mixes[r].append(cut.result(r))
        assert np.array_equal(rows_one, np.concatenate(rows, axis=1))         # (the precondition: the same rows)
        for r in range(2):
            got = one.result(r)
            assert got.shape == (C, nb_total * B)
            same_bits(got, np.concatenate(mixes[r], axis=1), r)
        one.scene_mix_set_at(nb_total * B + 9, g[0], d[0])
        one.scene_mix_clear_schedule()
        assert tuple(one.scene_mix_info().values()) == (nb_total * B, 0, 1, 4)
        with pytest.raises(PbsoError) as ei:
            one.scene_mix_set_at(nb_total * B - 1, g[0], d[0])       # in the past: refused for the whole group
        assert ei.value.status == capi.ERR_INVALID
