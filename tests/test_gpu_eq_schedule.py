"""The EQ bus's schedule on the device (include/openpbso_amd.h "The EQ bus's SCHEDULE"; kernels_eq_schedule.hip).  Every output is
compared BIT FOR BIT with tests/eq_model.Model stepped in pieces cut at every t_set with set() before each piece (the definition of
a scheduled set); the model builds its tables with the C reference, and the engine's eq_tables() behind every step must equal the
reference's tables of the last set taken, bit for bit.  The plans are those of tests/eq_schedule_plan.py, whose reach
tests/test_eq_schedule_plan.py proves without a GPU.  Steps are whole buffers, so "cut exactly at the t_sets" is run on the plans
whose sets lie on buffer edges (the aligned plans below); the model is cut at every t_set in every test."""
import ctypes as C

import numpy as np
import pytest
import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

from openpbso_amd import capi
from openpbso_amd.solver import PbsoError
from tests import eq_model as em
from tests import eq_phase_plan as pp
from tests import eq_schedule_plan as sp
from tests.test_gpu_eq import device, make_engine, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(frames):
        if frames not in made:
            made[frames] = make_engine(frames_per_buffer=frames) if frames != 513 else make_engine()
        return made[frames]

    yield get
    for e in made.values():
        e.close()


_MODEL = {}


def model_output(pl):
    """the model's output of a plan, computed once and shared"""
    if pl["name"] not in _MODEL:
        _MODEL[pl["name"]] = sp.run_model(pl)
        _MODEL[pl["name"]].setflags(write=False)
    return _MODEL[pl["name"]]


def expected_fade_end(ts_taken, R, t):
    if not ts_taken or R < 2 or t - ts_taken[-1] + 1 >= R:
        return t
    return ts_taken[-1] + R - 1


def run_plan(eng, pl, cuts=None, mode="own", one_by_one=False):
    """the plan on eng (enabled anew), every set scheduled up front, in steps of cuts buffers -> out [C][n].  mode: "own" the
    engine's buffer, "in place" d_out == d_in, "caller" a d_out of the caller's.  The clocks are checked behind every step."""
    assert eng.B == pl["frames"]
    cuts = pl["cuts"] if cuts is None else cuts
    Cn, S, R = pl["C"], pl["S"], pl["R"]
    eng.eq_enable(Cn, S, R)
    ts = sorted(pl["sets"])
    sos = np.array([sp.coefficients(pl, t) for t in ts])
    if one_by_one:
        for t, c in zip(ts, sos):
            eng.eq_set_at(t, c)
    else:
        eng.eq_schedule(ts, sos)
    i = eng.eq_schedule_info()
    assert (i["t"], i["pending"], i["sets_in_step"]) == (0, len(ts), 0) and eng.eq_info()["sets"] == len(ts)
    assert i["next_t_min"] == max(ts[-1] + 1, ts[-1] + R - 1)
    x = sp.signal(pl)
    outs, at, label = [], 0, (pl["name"], len(cuts), mode)
    for k, nb in enumerate(cuts):
        n = nb * eng.B
        part = x[:, at:at + n]
        dx = device(part)
        eng.step(nb)
        if mode == "in place":
            eng.eq(dx.data_ptr(), dx.data_ptr())
            eng.sync()
            got = dx.cpu().numpy()
            same_bits(eng.read_eq(), got, (label, k, "read from the caller's buffer"))
        elif mode == "caller":
            dy = torch.zeros_like(dx)
            eng.eq(dx.data_ptr(), dy.data_ptr())
            eng.sync()
            got = dy.cpu().numpy()
            same_bits(eng.read_eq(), got, (label, k, "read_eq returns the caller's buffer"))
            assert np.array_equal(dx.cpu().numpy(), part), (label, k, "d_in is read only")
        else:
            eng.eq(dx.data_ptr())
            got = eng.read_eq()
            assert np.array_equal(dx.cpu().numpy(), part), (label, k, "d_in is read only")
        taken = [t for t in ts if t < at + n]
        inside = [t for t in taken if t >= at]
        i, j = eng.eq_info(), eng.eq_schedule_info()
        assert (i["t"], i["fade_end"], i["calls"]) == (at + n, expected_fade_end(taken, R, at + n), k + 1), (label, k, i)
        assert (j["t"], j["pending"], j["sets_in_step"]) == (at + n, len(ts) - len(taken), len(inside)), (label, k, j)
        if inside:
            assert np.array_equal(eng.eq_tables(), em.tables(sp.coefficients(pl, taken[-1]))), (label, k, "the tables of the last set taken")
        outs.append(got)
        at += n
    assert at == x.shape[1]
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("name", [p["name"] for p in sp.PLANS])
def test_plan(engines, name):
    """the plan in its own steps against the model; then the same samples in one step and in one buffer per step: the same bits"""
    pl = sp.BY_NAME[name]
    eng = engines(pl["frames"])
    want = model_output(pl)
    y = run_plan(eng, pl)
    same_bits(y, want, (name, "against the model"))
    for label, cuts in sp.other_cuts(pl).items():
        same_bits(run_plan(eng, pl, cuts=cuts, one_by_one=label == "one step"), want, (name, label))


ALIGNED = [sp.plan("aligned R=64", 27, 2, 2, 64, [3, 3, 4, 10, 5], [81, 162, 270, 540]),
           sp.plan("aligned R=0", 27, 2, 2, 0, [1, 1, 1, 2], [27, 54, 81]),
           sp.plan("aligned R=200 513", 513, 2, 2, 200, [1, 1, 2], [513, 1026])]


@pytest.mark.parametrize("pl", ALIGNED, ids=[p["name"] for p in ALIGNED])
def test_cuts_exactly_at_the_sets_and_a_set_at_a_steps_first_sample_is_eq_set(engines, pl):
    """every set on the first sample of a step: scheduled, it equals eq_set before that step -- the same bits, the same eq_tables --,
    and both equal the same samples in one step"""
    eng = engines(pl["frames"])
    assert sp.step_edges(pl)[1:-1] == sorted(pl["sets"])
    want = model_output(pl)
    scheduled = run_plan(eng, pl)
    same_bits(scheduled, want, (pl["name"], "scheduled at the cuts"))
    tables_scheduled = eng.eq_tables()
    same_bits(run_plan(eng, pl, cuts=[sum(pl["cuts"])]), want, (pl["name"], "one step"))
    same_bits(run_plan(eng, pl, cuts=[1] * sum(pl["cuts"]), mode="in place"), want, (pl["name"], "one buffer per step, in place"))
    # the plain sets
    eng.eq_enable(pl["C"], pl["S"], pl["R"])
    x, at, outs = sp.signal(pl), 0, []
    for nb in pl["cuts"]:
        if at in pl["sets"]:
            eng.eq_set(sp.coefficients(pl, at))
        eng.step(nb)
        eng.eq(device(x[:, at:at + nb * eng.B]).data_ptr())
        outs.append(eng.read_eq())
        assert eng.eq_schedule_info()["sets_in_step"] == (1 if at in pl["sets"] else 0)
        at += nb * eng.B
    same_bits(np.concatenate(outs, axis=1), scheduled, (pl["name"], "eq_set before each step"))
    assert np.array_equal(eng.eq_tables(), tables_scheduled)


def test_in_place_and_a_callers_output(engines):
    for name in ("spacing R=64", "short-steps R=200", "group-edge R=3"):
        pl = sp.BY_NAME[name]
        eng = engines(pl["frames"])
        for mode in ("in place", "caller"):
            same_bits(run_plan(eng, pl, mode=mode), model_output(pl), (name, mode))


@pytest.mark.parametrize("Cn,S,R", [(8, 8, 67), (1, 1, 3)])
def test_channels_and_sections(engines, Cn, S, R):
    pl = sp.plan(f"C{Cn} S{S}", 27, Cn, S, R, [3, 20, 1, 6], [R + 10, 200, 200 + R - 1, 400, 470, 3 * 27 + 20 * 27 - 1, 700])
    eng = engines(27)
    want = model_output(pl)
    same_bits(run_plan(eng, pl), want, pl["name"])
    same_bits(run_plan(eng, pl, cuts=[30]), want, (pl["name"], "one step"))


def test_pending_sets_beyond_the_step_leave_the_plain_path(engines):
    """a set waits beyond the steps processed: they are the plain path's, with a plain set's fade running through them"""
    eng = engines(27)
    rng = np.random.default_rng(5)
    Cn, S, R, B = 2, 2, 40, 27
    x = (rng.standard_normal((Cn, 6 * B))).astype(np.float32)
    a, b = pp.coefficients(Cn, S, 2), pp.coefficients(Cn, S, 5)
    eng.eq_enable(Cn, S, R)
    model = em.Model(Cn, S, R)
    eng.eq_set(a)
    model.set(a)
    eng.eq_set_at(5 * B + 3, b)                           # behind the plain set, which counts as pending at sample 0
    with pytest.raises(PbsoError) as ei:
        eng.eq_set(a)                                     # plain sets wait while scheduled ones are pending
    assert ei.value.status == capi.ERR_STATE
    for k in range(5):
        eng.step(1)
        eng.eq(device(x[:, k * B:(k + 1) * B]).data_ptr())
        same_bits(eng.read_eq(), model.process(x[:, k * B:(k + 1) * B]), ("plain path", k))
        j = eng.eq_schedule_info()
        assert (j["pending"], j["sets_in_step"]) == (1, 1 if k == 0 else 0) and eng.eq_info()["fade_end"] == model.fade_end()
    eng.step(1)
    eng.eq(device(x[:, 5 * B:]).data_ptr())
    got = eng.read_eq()
    head = model.process(x[:, 5 * B:5 * B + 3])
    model.set(b)
    same_bits(got, np.concatenate([head, model.process(x[:, 5 * B + 3:])], axis=1), "the scheduled set behind plain steps")
    assert eng.eq_schedule_info()["pending"] == 0 and eng.eq_info()["fade_end"] == model.fade_end() == 5 * B + 3 + R - 1


def test_4096_sets_in_one_step_and_one_more(engines):
    eng = engines(27)
    B, nb, t0 = 27, 160, 100
    ts = [t0 + j for j in range(4096)]
    # a new cascade every sample is a time-varying filter: a gentle band that moves keeps it bounded, so that finite bits are compared
    bands = [np.array([[em.design("peak", 44100.0, 800.0 + 40.0 * k, 1.0, 2.0)]]) for k in range(10)]
    pl = dict(name="4096 sets", frames=27, C=1, S=1, R=0, cuts=[nb], sets={t: j % 10 for j, t in enumerate(ts)}, coef=lambda k: bands[k])
    want = model_output(pl)
    assert np.isfinite(want).all() and np.abs(want).max() < 100.0
    same_bits(run_plan(eng, pl), want, "4096 sets one sample apart in one step")
    # one more: refused, nothing changes; after the clear the step passes under the set in force
    x = sp.signal(dict(pl, name="4097 sets", cuts=[nb + 1]))
    eng.eq_enable(1, 1, 0)
    first = pp.coefficients(1, 1, 3)
    eng.eq_set(first)
    eng.step(1)
    eng.eq(device(x[:, :B]).data_ptr())
    model = em.Model(1, 1, 0)
    model.set(first)
    same_bits(eng.read_eq(), model.process(x[:, :B]), "the set in force")
    eng.eq_schedule([B + j for j in range(4097)], np.array([pp.coefficients(1, 1, j % 10) for j in range(4097)]))
    dx = device(x[:, B:B + nb * B])
    eng.step(nb)
    before, sched, tab = eng.eq_info(), eng.eq_schedule_info(), eng.eq_tables()
    assert sched["pending"] == 4097
    with pytest.raises(PbsoError) as ei:
        eng.eq(dx.data_ptr())
    assert ei.value.status == capi.ERR_INVALID
    assert eng.eq_info() == before and eng.eq_schedule_info() == sched and np.array_equal(eng.eq_tables(), tab)
    eng.eq_clear_schedule()
    assert eng.eq_schedule_info()["pending"] == 0
    eng.eq(dx.data_ptr())
    same_bits(eng.read_eq(), model.process(x[:, B:B + nb * B]), "behind the clear: the set in force")


def test_refusals_change_nothing(engines):
    eng = engines(27)
    lib, dp, tp = capi.lib(), C.POINTER(C.c_double), C.POINTER(C.c_int64)
    Cn, S, R, B = 2, 2, 50, 27
    a, b = pp.coefficients(Cn, S, 1), pp.coefficients(Cn, S, 6)
    # before the enable: a fresh engine
    fresh = make_engine(frames_per_buffer=27)
    try:
        one = np.zeros(Cn * S * 5)
        t1 = np.array([10], dtype=np.int64)
        info = (C.c_int64 * 4)()
        assert lib.pbso_eq_set_at(fresh._h, 10, one.ctypes.data_as(dp)) == capi.ERR_STATE
        assert lib.pbso_eq_schedule(fresh._h, 1, t1.ctypes.data_as(tp), one.ctypes.data_as(dp)) == capi.ERR_STATE
        assert lib.pbso_eq_schedule(fresh._h, 0, None, None) == capi.ERR_STATE
        assert lib.pbso_eq_clear_schedule(fresh._h) == capi.ERR_STATE == lib.pbso_eq_schedule_info(fresh._h, info)
        for call in (lambda: fresh.eq_set_at(10, a), lambda: fresh.eq_schedule([10], [a]), fresh.eq_clear_schedule, fresh.eq_schedule_info):
            with pytest.raises(PbsoError) as ei:
                call()
            assert ei.value.status == capi.ERR_STATE
    finally:
        fresh.close()
    eng.eq_enable(Cn, S, R)

    def refused(call, status=capi.ERR_INVALID):
        before, sched, tab = eng.eq_info(), eng.eq_schedule_info(), eng.eq_tables()
        with pytest.raises(PbsoError) as ei:
            call()
        assert ei.value.status == status
        assert eng.eq_info() == before and eng.eq_schedule_info() == sched and np.array_equal(eng.eq_tables(), tab)

    assert eng.eq_schedule_info()["next_t_min"] == R - 1    # the identity is a predecessor at 0
    refused(lambda: eng.eq_set_at(R - 2, a))
    eng.eq_schedule([], np.zeros((0, Cn, S, 5)))          # n_sets == 0
    assert eng.eq_info()["sets"] == 0
    x = sp.signal(dict(name="refusals", C=Cn, cuts=[10], frames=B))
    eng.step(2)
    eng.eq(device(x[:, :2 * B]).data_ptr())
    same_bits(eng.read_eq(), x[:, :2 * B], "the identity")
    refused(lambda: eng.eq_set_at(2 * B - 1, a))          # below the next processed sample
    eng.eq_set_at(2 * B + 5, a)
    assert eng.eq_schedule_info()["next_t_min"] == 2 * B + 5 + R - 1
    refused(lambda: eng.eq_set_at(2 * B + 5, b))          # not ascending
    refused(lambda: eng.eq_set_at(2 * B + 4, b))
    refused(lambda: eng.eq_set_at(2 * B + 5 + R - 2, b))  # inside the predecessor's fade
    refused(lambda: eng.eq_schedule([200, 260, 259], [b, a, b]))         # the last one not ascending: none is taken
    refused(lambda: eng.eq_schedule([200, 248], [b, a]))                 # 248 - 200 + 1 < 50
    for k, v in ((4, 1.0), (3, 2.5), (0, float("nan")), (1, float("inf"))):
        bad = b.copy()
        bad[1, 0, k] = v
        refused(lambda: eng.eq_schedule([200, 260, 320], [b, bad, a]))  # a bad section in the middle
    refused(lambda: eng.eq_schedule([200], [b[:1]]))
    assert lib.pbso_eq_set_at(eng._h, 200, None) == capi.ERR_INVALID and lib.pbso_eq_schedule(eng._h, -1, None, None) == capi.ERR_INVALID
    assert lib.pbso_eq_schedule_info(eng._h, None) == capi.ERR_INVALID
    refused(lambda: eng.eq_set(b), capi.ERR_STATE)        # a plain set while scheduled sets are pending
    eng.eq_schedule([200, 249], [b, a])                   # exactly R - 1 apart
    assert (eng.eq_schedule_info()["pending"], eng.eq_info()["sets"]) == (3, 3)
    # the schedule drains; a plain set is then refused mid-fade and accepted once the fade is over
    model = em.Model(Cn, S, R)
    pieces = [model.process(x[:, :2 * B])]
    for lo, hi, c in ((2 * B, 2 * B + 5, None), (2 * B + 5, 200, a), (200, 249, b), (249, 270, a)):
        if c is not None:
            model.set(c)
        pieces.append(model.process(x[:, lo:hi]))
    eng.step(8)
    eng.eq(device(x[:, 2 * B:10 * B]).data_ptr())
    same_bits(eng.read_eq(), np.concatenate(pieces[1:], axis=1), "the drained schedule")
    i = eng.eq_info()
    assert (i["t"], i["fade_end"]) == (270, 249 + R - 1) and eng.eq_schedule_info() == dict(t=270, pending=0, next_t_min=249 + R - 1, sets_in_step=3)
    refused(lambda: eng.eq_set(b), capi.ERR_STATE)        # mid-fade, as if the last scheduled set had been a plain one
    more = sp.signal(dict(name="refusals more", C=Cn, cuts=[3], frames=B))
    eng.step(2)
    eng.eq(device(more[:, :2 * B]).data_ptr())
    same_bits(eng.read_eq(), model.process(more[:, :2 * B]), "the fade goes on, and ends, in a plain step")
    assert eng.eq_info()["fade_end"] == eng.eq_info()["t"] == 324 and eng.eq_schedule_info()["sets_in_step"] == 0
    eng.eq_set(b)
    model.set(b)
    eng.step(1)
    eng.eq(device(more[:, 2 * B:]).data_ptr())
    same_bits(eng.read_eq(), model.process(more[:, 2 * B:]), "a plain set behind the drained schedule")
    # the reset drops what is pending
    eng.eq_set_at(1000, a)
    assert eng.eq_schedule_info()["pending"] == 1
    eng.eq_reset()
    assert eng.eq_schedule_info() == dict(t=0, pending=0, next_t_min=R - 1, sets_in_step=0)
    eng.step(1)
    eng.eq(device(more[:, :B]).data_ptr())
    same_bits(eng.read_eq(), more[:, :B], "the identity behind the reset")
    # ... and so does a new enable
    eng.eq_set_at(1000, a)
    eng.eq_enable(Cn, S, R)
    assert eng.eq_schedule_info()["pending"] == 0
