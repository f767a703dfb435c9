"""The scene filter mix's bank (include/openpbso_amd.h "scene filter mix", BANK; kernels_fir_bank.hip) on the device: filters that
stay there, and sets given as J (index, weight) pairs per object.  Every comparison is BIT FOR BIT, and never with the engine under
test alone: the reference is the existing models (through tests/scene_fir_sched_ref.py) fed the taps that
tests/cpp/scene_fir_bank_ref.c builds from the same pairs, or a second engine given those taps through the taps calls.  Objects of
1 .. 8 modes, runs of 3 .. 6 buffers."""
import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from tests.scene_fir_bank_model import taps_from_bank
from tests.scene_fir_sched_ref import Piecewise
from tests.test_gpu_scene_fir import make_engine, same_bits, taps_of
from tests.test_gpu_scene_fir_schedule import delay_times, filter_times, sched_info, step_and_mix

pytestmark = pytest.mark.gpu

B = 513
FLT_MAX = float(np.finfo(np.float32).max)


def bank_of(rng, F, C, K):
    """[F][C][K]: decaying noise, every tap a full f32 mantissa"""
    return np.ascontiguousarray(taps_of(rng, C, F, K).transpose(1, 0, 2))


def pairs_for(rng, n_sets, n_obj, J, F):
    """index, weight [n_sets][n_obj][J]: indices 0 and F - 1, an index repeated within an object, weights 0, negative and 1.f"""
    index = rng.integers(0, F, (n_sets, n_obj, J)).astype(np.int32)
    weight = rng.standard_normal((n_sets, n_obj, J)).astype(np.float32)
    index[0, 0, :] = F - 1                                            # (repeated for J > 1)
    index[-1, -1, 0] = 0
    weight[0, 0, 0] = 1.0
    weight[0, -1, -1] = -0.75
    weight[-1, 0, -1] = 0.0
    if n_sets > 1:
        index[1, 0, :] = 0
        weight[1, 0, :] = 1.0
    return index, weight


def taps_for(bank, index, weight):
    """[n_sets][C][N][K]: the taps each of the sets stands for, by the C reference"""
    return np.stack([taps_from_bank(bank, index[k], weight[k]) for k in range(index.shape[0])])


def onsets_for(rng, n_sets, n_obj, max_onset):
    on = rng.integers(0, max_onset + 1, (n_sets, n_obj)).astype(np.int32)
    on[0, :min(n_obj, 3)] = [0, max_onset, max_onset // 2][:min(n_obj, 3)]
    return on


def _refused(status, call, *args):
    with pytest.raises(PbsoError) as ei:
        call(*args)
    assert ei.value.status == status, (call, args)


# ---- 1. against the model ------------------------------------------------------------------------------------------------------

# every N in {1, 33, 70}, C in {1, 2, 8}, K in {1, 2, 17, 128, 1024}, J in {1, 3, 8}, F in {1, 37}, R in {0, 7, 600}, with and
# without the delay stage
CASES = [(1, 1, 1, 1, 1, 0, False), (1, 2, 17, 3, 37, 7, True), (1, 8, 128, 8, 37, 600, False), (33, 1, 1024, 3, 37, 0, False),
         (33, 2, 2, 3, 1, 7, False), (33, 8, 17, 1, 37, 0, True), (33, 1, 128, 8, 37, 600, True), (70, 2, 128, 3, 37, 600, False),
         (70, 8, 17, 8, 1, 7, True), (70, 1, 2, 1, 37, 600, True)]


@pytest.mark.parametrize("n_obj,C,K,J,F,R,delay", CASES)
def test_bank_schedule_against_the_model(n_obj, C, K, J, F, R, delay):
    """steps of 3 and 3 buffers; onsets differ between sets; a second batch with onset == NULL is scheduled between the steps"""
    max_onset, max_delay, Rd = 300, 400, 300
    n1, total = 3 * B, 6 * B
    rng = np.random.default_rng(1000 * n_obj + 100 * C + K + R + J)
    ft = filter_times(R, n1, total)
    beyond = [t for t in ft if t >= n1]                               # the first of them is scheduled with the first step's
    first, later = [t for t in ft if t < n1] + beyond[:1], beyond[1:]
    assert len(first) >= 3 and later
    bank = bank_of(rng, F, C, K)
    eng = make_engine(n_obj, 1 + (n_obj + C + K) % 8, 6, n_obj + C + K)
    ref = Piecewise(C, n_obj, K, max_onset, R, max_delay if delay else None, Rd)
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        eng.scene_fir_bank_create(bank)
        assert eng.scene_fir_bank_info() == {"n_filters": F, "max_j": 8, "sets": 0, "bytes": 4 * F * C * K}
        index, weight = pairs_for(rng, len(first), n_obj, J, F)
        onsets = onsets_for(rng, len(first), n_obj, max_onset)
        eng.scene_fir_bank_schedule(first, index, weight, onsets)
        ref.schedule(first, taps_for(bank, index, weight), onsets)
        n_delay = 0
        if delay:
            eng.scene_fir_delay_enable(max_delay, Rd)
            dt = delay_times(n1, total)
            dl = rng.uniform(0, max_delay, (len(dt), n_obj)).astype(np.float32)
            eng.scene_fir_delay_schedule(dt, dl)
            ref.delay_schedule(dt, dl)
            n_delay = len(dt)
        assert sched_info(eng)[:3] == (0, len(first), n_delay)
        step_and_mix(eng, ref, 3, "first step")
        assert sched_info(eng)[:2] == (n1, 1)                         # the set at the next step's first sample stayed pending
        index2, weight2 = pairs_for(rng, len(later), n_obj, J, F)
        eng.scene_fir_bank_schedule(later, index2, weight2)           # onset == NULL: the onsets of the set before
        ref.schedule(later, taps_for(bank, index2, weight2))
        step_and_mix(eng, ref, 3, "second step")
        assert sched_info(eng)[:3] == (total, 0, 0)
        assert eng.scene_fir_info()["sets"] == len(ft) == eng.scene_fir_bank_info()["sets"]
    finally:
        eng.close()


# ---- 2. the twin engine given the same sets as taps -----------------------------------------------------------------------------

def test_bank_and_taps_sets_alternate_inside_one_step_and_equal_the_taps_twin():
    """sets of both forms, of different J, at the schedule test's times inside two steps; the twin gets all of them as taps"""
    n_obj, C, K, F, R, max_onset, max_delay, Rd = 33, 2, 17, 37, 7, 200, 300, 700
    n1, total = 3 * B, 5 * B
    rng = np.random.default_rng(21)
    ft = filter_times(R, n1, total)
    bank = bank_of(rng, F, C, K)
    onsets = onsets_for(rng, len(ft), n_obj, max_onset)
    a, twin = (make_engine(n_obj, 4, 5, 21, time_chunks=1) for _ in range(2))
    ref = Piecewise(C, n_obj, K, max_onset, R, max_delay, Rd)
    try:
        for e in (a, twin):
            e.scene_fir_enable(C, K, max_onset, R)
            e.scene_fir_delay_enable(max_delay, Rd)
        a.scene_fir_bank_create(bank)
        dt = delay_times(n1, total)
        dl = rng.uniform(0, max_delay, (len(dt), n_obj)).astype(np.float32)
        taps = []
        for k, t in enumerate(ft):                                    # bank, taps, taps, bank (J differs), ...
            if k % 4 in (0, 3):
                index, weight = pairs_for(rng, 1, n_obj, (3, 8, 1)[k % 3], F)
                a.scene_fir_set_bank_at(t, index[0], weight[0], onsets[k])
                taps.append(taps_from_bank(bank, index[0], weight[0]))
            else:
                taps.append(taps_of(rng, C, n_obj, K))
                a.scene_fir_set_at(t, taps[-1], onsets[k])
        taps = np.stack(taps)
        twin.scene_fir_schedule(ft, taps, onsets)
        ref.schedule(ft, taps, onsets)
        for e in (a, twin):
            e.scene_fir_delay_schedule(dt, dl)
        ref.delay_schedule(dt, dl)
        assert sched_info(a) == sched_info(twin)
        for nb in (3, 2):
            got = step_and_mix(a, ref, nb, ("bank", nb))
            twin.step(nb)
            twin.scene_fir()
            same_bits(got, twin.read_scene_fir(), ("twin", nb))
        assert sched_info(a) == sched_info(twin) and a.scene_fir_info() == twin.scene_fir_info()
    finally:
        a.close()
        twin.close()


def test_bank_sets_on_buffer_boundaries_equal_plain_taps_sets_and_a_plain_set_bank_between_steps():
    """a 4-buffer step with a set on every buffer boundary (bank, taps, bank, taps) against plain taps sets between one-buffer steps;
    then plain set_bank calls between one-buffer steps on the one, plain taps sets on the other -- the last with onset None"""
    n_obj, C, K, F, J, R, max_onset = 33, 2, 17, 37, 3, 300, 200
    rng = np.random.default_rng(22)
    bank = bank_of(rng, F, C, K)
    index, weight = pairs_for(rng, 6, n_obj, J, F)
    taps = taps_for(bank, index, weight)
    for k in (1, 3):
        taps[k] = taps_of(rng, C, n_obj, K)
    onsets = onsets_for(rng, 6, n_obj, max_onset)
    a, plain = (make_engine(n_obj, 4, 6, 22, time_chunks=1) for _ in range(2))
    try:
        for e in (a, plain):
            e.scene_fir_enable(C, K, max_onset, R)
        a.scene_fir_bank_create(bank)
        for k in range(4):
            if k in (1, 3):
                a.scene_fir_set_at(k * B, taps[k], onsets[k])
            else:
                a.scene_fir_set_bank_at(k * B, index[k], weight[k], onsets[k])
        a.step(4)
        a.scene_fir()
        outs_a, outs_p, rows_p = [a.read_scene_fir()], [], []
        rows_a = [a.audio()]
        for k in range(4):
            plain.scene_fir_set(taps[k], onsets[k])
            plain.step(1)
            plain.scene_fir()
            outs_p.append(plain.read_scene_fir())
            rows_p.append(plain.audio())
        for k in (4, 5):
            a.scene_fir_set_bank(index[k], weight[k], onsets[k] if k == 4 else None)
            plain.scene_fir_set(taps[k], onsets[k] if k == 4 else None)
            for e, outs, rows in ((a, outs_a, rows_a), (plain, outs_p, rows_p)):
                e.step(1)
                e.scene_fir()
                outs.append(e.read_scene_fir())
                rows.append(e.audio())
        assert np.array_equal(np.concatenate(rows_a, axis=1), np.concatenate(rows_p, axis=1))   # (the precondition: the same rows)
        same_bits(np.concatenate(outs_a, axis=1), np.concatenate(outs_p, axis=1), "boundaries and plain sets")
        ia, ip = a.scene_fir_info(), plain.scene_fir_info()
        assert (ia["t"], ia["fade_end"], ia["sets"]) == (ip["t"], ip["fade_end"], ip["sets"]) and (ia["mixes"], ip["mixes"]) == (3, 6)
        assert a.scene_fir_bank_info()["sets"] == 4
    finally:
        a.close()
        plain.close()


# ---- 3. the cut does not matter ------------------------------------------------------------------------------------------------

def _cut_run(cuts):
    n_obj, C, K, F, J, R, max_onset, max_delay, Rd, nb_total = 40, 3, 37, 37, 3, 150, 700, 600, 400, 6
    rng = np.random.default_rng(3)
    ft = filter_times(R, 2 * B, nb_total * B)
    dt = delay_times(2 * B, nb_total * B)
    bank = bank_of(rng, F, C, K)
    index, weight = pairs_for(rng, len(ft), n_obj, J, F)
    onsets = onsets_for(rng, len(ft), n_obj, max_onset)
    dl = rng.uniform(0, max_delay, (len(dt), n_obj)).astype(np.float32)
    eng = make_engine(n_obj, 8, nb_total, 3, time_chunks=1)           # time_chunks = 1: the rows do not depend on the cut
    outs = []
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        eng.scene_fir_delay_enable(max_delay, Rd)
        eng.scene_fir_bank_create(bank)
        eng.scene_fir_bank_schedule(ft, index, weight, onsets)
        eng.scene_fir_delay_schedule(dt, dl)
        for nb in cuts:
            eng.step(nb)
            eng.scene_fir()
            outs.append((eng.audio(), eng.read_scene_fir()))
        return np.concatenate([r for r, _ in outs], axis=1), np.concatenate([y for _, y in outs], axis=1)
    finally:
        eng.close()


def test_the_cut_into_steps_does_not_matter():
    rows, out = _cut_run([6])
    rows2, out2 = _cut_run([1, 2, 3])
    assert np.array_equal(rows, rows2)                                # (the precondition: the same rows)
    same_bits(out2, out, "1 + 2 + 3 against 6")


# ---- 4. the bank's lifetime -------------------------------------------------------------------------------------------------------

def test_lifetime_of_the_bank():
    n_obj, C, K, F, J, R, max_onset = 9, 2, 17, 5, 2, 40, 30
    rng = np.random.default_rng(4)
    bank1, bank2 = bank_of(rng, F, C, K), bank_of(rng, F + 2, C, K)
    index, weight = pairs_for(rng, 3, n_obj, J, F)
    onsets = onsets_for(rng, 3, n_obj, max_onset)
    eng = make_engine(n_obj, 4, 8, 4)
    ref = Piecewise(C, n_obj, K, max_onset, R)
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        _refused(capi.ERR_STATE, eng.scene_fir_set_bank, index[0], weight[0])          # no bank yet
        eng.scene_fir_bank_create(bank1)
        eng.scene_fir_set_bank(index[0], weight[0], onsets[0])
        ref.schedule([0], taps_for(bank1, index[:1], weight[:1]), onsets[:1])
        step_and_mix(eng, ref, 1, "first set")
        # a replace while bank sets are pending is refused, scheduled or waiting for the next mix; taps sets do not hold it up
        eng.scene_fir_set_bank_at(5 * B, index[1], weight[1])
        _refused(capi.ERR_STATE, eng.scene_fir_bank_create, bank2)
        eng.scene_fir_clear_schedule()
        eng.scene_fir_set_bank(index[1], weight[1])
        _refused(capi.ERR_STATE, eng.scene_fir_bank_create, bank2)
        eng.scene_fir_set(taps_for(bank1, index[1:2], weight[1:2])[0])                 # replaces the waiting bank set
        eng.scene_fir_bank_create(bank2)
        assert eng.scene_fir_bank_info()["n_filters"] == F + 2
        # the replaced bank does not change the set in force, nor the taps set that waited
        ref.schedule([B], taps_for(bank1, index[1:2], weight[1:2]))
        step_and_mix(eng, ref, 1, "after the replace")
        step_and_mix(eng, ref, 1, "the set in force, a step later")
        eng.scene_fir_set_bank(index[2], weight[2], onsets[2])                         # ... and the next set reads the new bank
        ref.schedule([3 * B], taps_for(bank2, index[2:], weight[2:]), onsets[2:])
        step_and_mix(eng, ref, 1, "the new bank")
        # the reset keeps the bank
        eng.scene_fir_reset()
        ref = Piecewise(C, n_obj, K, max_onset, R)
        assert eng.scene_fir_bank_info()["n_filters"] == F + 2
        eng.scene_fir_set_bank_at(7, index[0], weight[0], onsets[1])
        ref.schedule([7], taps_for(bank2, index[:1], weight[:1]), onsets[1:2])
        step_and_mix(eng, ref, 1, "after the reset")
        # a new enable drops it
        eng.scene_fir_enable(C, K, max_onset, R)
        assert eng.scene_fir_bank_info() == {"n_filters": 0, "max_j": 8, "sets": 0, "bytes": 0}
        _refused(capi.ERR_STATE, eng.scene_fir_set_bank, index[0], weight[0])
        _refused(capi.ERR_STATE, eng.scene_fir_bank_schedule, [0], index[:1], weight[:1])
    finally:
        eng.close()


# ---- 5. refused calls change nothing --------------------------------------------------------------------------------------------

def test_refused_calls_change_nothing():
    n_obj, C, K, F, J, R, max_onset = 5, 2, 3, 4, 2, 10, 50
    rng = np.random.default_rng(5)
    bank = bank_of(rng, F, C, K)
    A = float(np.abs(bank).max())
    h = taps_of(rng, C, n_obj, K)
    on = np.full(n_obj, 7, dtype=np.int32)
    index, weight = pairs_for(rng, 3, n_obj, J, F)
    a, twin = make_engine(n_obj, 4, 8, 5), make_engine(n_obj, 4, 8, 5)
    ref = Piecewise(C, n_obj, K, max_onset, R)
    try:
        for e in (a, twin):
            e.scene_fir_enable(C, K, max_onset, R)
        _refused(capi.ERR_STATE, a.scene_fir_set_bank_at, 0, index[0], weight[0])      # no bank
        _refused(capi.ERR_STATE, a.scene_fir_bank_schedule, [0, 20, 40], index, weight)
        for e in (a, twin):
            e.scene_fir_bank_create(bank)
            e.scene_fir_set_at(0, h, on)                                               # a taps set is the predecessor
        ref.schedule([0], h[None], on[None])
        state = (sched_info(a), a.scene_fir_info(), a.scene_fir_bank_info())
        assert state[0] == (0, 1, 0, R - 1) and state[2]["sets"] == 0
        times = [20, 40, 60]
        for bad_index in (F, -1):
            bad = index.copy()
            bad[2, 3, 1] = bad_index
            _refused(capi.ERR_INVALID, a.scene_fir_bank_schedule, times, bad, weight)
        for bad_weight in (np.nan, np.inf):
            bad = weight.copy()
            bad[2, 4, 0] = bad_weight
            _refused(capi.ERR_INVALID, a.scene_fir_bank_schedule, times, index, bad)
        big = weight.copy()                                                            # sum |w| A = 1.2 FLT_MAX, every w finite
        big[1, 2, :] = [0.6 * FLT_MAX / A, -0.6 * FLT_MAX / A]
        assert np.isfinite(big).all()
        _refused(capi.ERR_INVALID, a.scene_fir_bank_schedule, times, index, big)
        for bad_j in (0, 9):
            _refused(capi.ERR_INVALID, a.scene_fir_bank_schedule, times, np.zeros((3, n_obj, bad_j), dtype=np.int32),
                     np.zeros((3, n_obj, bad_j), dtype=np.float32))
            _refused(capi.ERR_INVALID, a.scene_fir_set_bank_at, 20, np.zeros((n_obj, bad_j), dtype=np.int32),
                     np.zeros((n_obj, bad_j), dtype=np.float32))
        _refused(capi.ERR_INVALID, a.scene_fir_set_bank_at, R - 2, index[0], weight[0])       # inside the fade of the taps set at 0
        _refused(capi.ERR_INVALID, a.scene_fir_bank_schedule, [20, 20 + R - 2, 60], index, weight)   # ... of its own predecessor
        _refused(capi.ERR_INVALID, a.scene_fir_bank_schedule, [20, 60, 40], index, weight)
        _refused(capi.ERR_INVALID, a.scene_fir_bank_schedule, times, index, weight, np.stack([on, on, on + max_onset]))
        _refused(capi.ERR_STATE, a.scene_fir_set_bank, index[0], weight[0])                   # a scheduled set is pending
        assert (sched_info(a), a.scene_fir_info(), a.scene_fir_bank_info()) == state
        assert state == (sched_info(twin), twin.scene_fir_info(), twin.scene_fir_bank_info())
        for e in (a, twin):
            e.scene_fir_bank_schedule([R - 1, 2 * R - 2, 600], index, weight)                  # exactly R - 1 apart: accepted
        ref.schedule([R - 1, 2 * R - 2, 600], taps_for(bank, index, weight))
        got = step_and_mix(a, ref, 2, "after the refusals")
        twin.step(2)
        twin.scene_fir()
        same_bits(got, twin.read_scene_fir(), "the twin that was never refused")
        assert sched_info(a) == (2 * B, 0, 0, 2 * B) == sched_info(twin)
        assert a.scene_fir_info()["sets"] == 4 and a.scene_fir_bank_info()["sets"] == 3
    finally:
        a.close()
        twin.close()


def test_a_set_just_inside_the_overflow_bound_mixes_finite():
    """one bank tap of 2^100, weights whose sum of magnitudes times it is FLT_MAX less a few ulps: accepted, taps next to FLT_MAX,
    and the mix has the model's bits without an inf or a NaN"""
    n_obj, C, K, F = 3, 1, 3, 2
    bank = np.zeros((F, C, K), dtype=np.float32)
    bank[0, 0, 0], bank[1, 0, :] = 2.0 ** 100, [0.5, -0.25, 0.125]
    w = np.float32(FLT_MAX / 2.0 ** 100 / 2 * (1 - 2.0 ** -20))
    index = np.array([[0, 0], [1, 1], [1, 0]], dtype=np.int32)
    weight = np.array([[w, w], [1.0, 0.5], [1.0, 0.0]], dtype=np.float32)
    assert 2.0 * float(w) * 2.0 ** 100 <= FLT_MAX < 2.0 * float(np.nextafter(w, np.float32(np.inf))) * 2.0 ** 100 * (1 + 2.0 ** -19)
    taps = taps_from_bank(bank, index, weight)
    assert np.isfinite(taps).all() and taps[0, 0, 0] > 0.99 * FLT_MAX

    def engine(scale):
        eng = Engine()
        rng = np.random.default_rng(6)
        for i in range(n_obj):
            eng.add_object(synth.eigenvalues(2, 660 + i), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        for i in range(n_obj):
            eng.set_use_transfer(i, False)
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(2) * scale), 0)
        return eng

    loud = engine(1.0)                                                # the audio is linear in the force: scaled to a peak near 0.01
    try:
        loud.step(3)
        peak = float(np.abs(loud.audio()).max())
    finally:
        loud.close()
    eng = engine(0.01 / peak)
    ref = Piecewise(C, n_obj, K, 0, 0)
    try:
        eng.scene_fir_enable(C, K, 0, 0)
        eng.scene_fir_bank_create(bank)
        over = weight.copy()
        over[0] = np.nextafter(w, np.float32(np.inf)) * np.float32(1 + 2.0 ** -19)
        _refused(capi.ERR_INVALID, eng.scene_fir_set_bank, index, over)
        eng.scene_fir_set_bank(index, weight)
        ref.schedule([0], taps[None])
        got = step_and_mix(eng, ref, 3, "inside the bound")
        assert np.isfinite(got).all() and np.abs(got).max() > 1e30
    finally:
        eng.close()


def test_subnormal_bank_taps_come_through_the_chain():
    """bank taps among the f32 subnormals under weights of 2^100 and 2^90: the taps the set stands for are ordinary numbers only if
    the kernel's fmaf reads its subnormal operands as they are (flushed, they would be zeros and the object silent)"""
    n_obj, C, K, F = 2, 1, 3, 2
    bank = np.zeros((F, C, K), dtype=np.float32)
    bank[0, 0, :] = [1e-42, -3e-40, 7e-45]
    bank[1, 0, :] = [2e-41, 1e-39, -4e-43]
    assert (np.abs(bank) < np.finfo(np.float32).tiny).all() and (bank != 0).all()
    index = np.array([[0, 1], [1, 1]], dtype=np.int32)
    weight = np.array([[2.0 ** 100, -2.0 ** 90], [2.0 ** 100, 2.0 ** 100]], dtype=np.float32)
    taps = taps_from_bank(bank, index, weight)
    assert (np.abs(taps) > 1e-16).all()
    eng = make_engine(n_obj, 4, 2, 9)
    ref = Piecewise(C, n_obj, K, 0, 0)
    try:
        eng.scene_fir_enable(C, K, 0, 0)
        eng.scene_fir_bank_create(bank)
        eng.scene_fir_set_bank(index, weight)
        ref.schedule([0], taps[None])
        step_and_mix(eng, ref, 2, "subnormal bank taps")
    finally:
        eng.close()


# ---- 6. an engine that never creates a bank is what it was ----------------------------------------------------------------------

@pytest.mark.parametrize("delay", [False, True])
def test_an_engine_without_a_bank_is_what_it_was(delay):
    """plain taps sets between steps, then scheduled ones inside a step: the bits of the existing model"""
    n_obj, C, K, R, max_onset, max_delay, Rd = 40, 2, 37, 300, 400, 500, 441
    rng = np.random.default_rng(8)
    eng = make_engine(n_obj, 6, 5, 8)
    ref = Piecewise(C, n_obj, K, max_onset, R, max_delay if delay else None, Rd)
    try:
        eng.scene_fir_enable(C, K, max_onset, R)
        if delay:
            eng.scene_fir_delay_enable(max_delay, Rd)
        assert eng.scene_fir_bank_info()["n_filters"] == 0
        for k, nb in enumerate((1, 1)):
            h, on = taps_of(rng, C, n_obj, K), rng.integers(0, max_onset + 1, n_obj).astype(np.int32)
            eng.scene_fir_set(h, on)
            ref.schedule([k * B], h[None], on[None])
            if delay:
                dl = rng.uniform(0, max_delay, n_obj).astype(np.float32)
                eng.scene_fir_set_delay(dl)
                ref.delay_schedule([k * B], dl[None])
            step_and_mix(eng, ref, nb, ("plain", k))
        ft = [2 * B + t for t in filter_times(R, 2 * B, 3 * B)]
        taps = np.stack([taps_of(rng, C, n_obj, K) for _ in ft])
        onsets = onsets_for(rng, len(ft), n_obj, max_onset)
        eng.scene_fir_schedule(ft, taps, onsets)
        ref.schedule(ft, taps, onsets)
        if delay:
            dt = [2 * B + t for t in delay_times(2 * B, 3 * B)]
            dl = rng.uniform(0, max_delay, (len(dt), n_obj)).astype(np.float32)
            eng.scene_fir_delay_schedule(dt, dl)
            ref.delay_schedule(dt, dl)
        step_and_mix(eng, ref, 3, "scheduled")
        assert sched_info(eng)[:3] == (5 * B, 0, 0) and eng.scene_fir_bank_info()["sets"] == 0
    finally:
        eng.close()
