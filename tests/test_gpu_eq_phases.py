"""The EQ bus on the device at every block phase, step length and fade length: the plans of tests/eq_phase_plan.py (anchored without
a GPU by tests/test_eq_phase_plan.py, which proves what they reach) through test_gpu_eq.py's run(): the engine against the model BIT
FOR BIT, step by step, the model fed the engine's own tables, eq_info()'s t and fade_end checked behind every step.  No tolerance
anywhere in this file.  The engine behind the bus is one object of 64 modes; the longest step is 306 buffers of 27 frames."""
import numpy as np
import pytest
import torch                      # before the engine's library (as in test_gpu_eq.py)

from tests import eq_model as em
from tests import eq_phase_plan as pp
from tests.eq_model import Model
from tests.test_gpu_eq import BANK, coefficients, device, enable, make_engine, run, same_bits

pytestmark = pytest.mark.gpu


def sets_of(pl):
    return {k: coefficients(pl["C"], pl["S"], shift) for k, shift in pl["sets"].items()}


def run_plan(eng, pl, in_place=False, cuts=None):
    """the plan on eng (enabled anew: t = 0, silence, the identity) against the model step by step -> the output [C][n].  cuts: the
    same samples in other steps (plans whose only set comes before step 0)"""
    assert eng.B == pl["frames"]
    cuts = pl["cuts"] if cuts is None else cuts
    model = enable(eng, pl["C"], pl["S"], pl["R"])
    x = pp.signal(pl)
    y = run(eng, model, x, cuts, (pl["name"], tuple(cuts) if len(cuts) < 8 else len(cuts), in_place), sets=sets_of(pl), in_place=in_place)
    i = eng.eq_info()
    assert (i["calls"], i["sets"], i["t"]) == (len(cuts), len(pl["sets"]), x.shape[1]), (pl["name"], i)      # every step was processed
    assert y.shape == x.shape
    return y


def engine_for(pl):
    return make_engine(frames_per_buffer=pl["frames"]) if pl["frames"] != 513 else make_engine()


def test_the_plans_use_the_bank_of_test_gpu_eq():
    assert pp.BANK == BANK and pp.RATE == 44100.0 and pp.P == em.P == 64
    for shift in (0, 4):
        assert np.array_equal(pp.coefficients(3, 3, shift), coefficients(3, 3, shift))


@pytest.mark.parametrize("name", ["sweep-1", "sweep-3", "sweep-9", "sweep-513", "sweep-1 C8 S8", "sweep-1 C3 S3"])
def test_sweep(name):
    """66 steps of one length: every k0, and at 27 frames every end phase; the 27-frame sweeps of two channels once more in ONE step
    on a fresh engine: the same bits"""
    pl = pp.BY_NAME[name]
    eng = engine_for(pl)
    try:
        y = run_plan(eng, pl)
    finally:
        eng.close()
    same_bits(y, pp.run_model(pl), (name, "the model with its own tables"))
    if name in ("sweep-1", "sweep-3", "sweep-9"):
        eng = engine_for(pl)
        try:
            one = run_plan(eng, pl, cuts=[pp.total_buffers(pl)])
        finally:
            eng.close()
        same_bits(one, y, (name, "one cut against the sweep"))


@pytest.mark.parametrize("name", [p["name"] for p in pp.PLANS if p["name"].startswith("batches")])
def test_batches(name):
    """one long step: the serial chain's batches of 64 blocks exactly full, one short of it and one over, once and twice; a long
    step that ends on sample P - 2 of a block and one that ends just before it; then two short steps that read what it left"""
    pl = pp.BY_NAME[name]
    eng = engine_for(pl)
    try:
        y = run_plan(eng, pl)
    finally:
        eng.close()
    same_bits(y, pp.run_model(pl), (name, "the model with its own tables"))


@pytest.mark.parametrize("group", ["m=7 ", "m=26 ", "m=45 ", "m=64 ", "long"])
def test_fades(group):
    """From at k0 = 61, 62, 63 and 0 for 1, 2, 3 samples, about a step and about a block; fades that end around a step edge; From
    in one long step to the tail store and to the edges of the workgroup grid.  One engine, enabled anew for every plan"""
    plans = [p for p in pp.PLANS if p["name"].startswith("fades ") and group in p["name"] and ("long" in p["name"]) == (group == "long")]
    assert len(plans) == (3 if group == "long" else 9)
    eng = engine_for(plans[0])
    try:
        for pl in plans:
            same_bits(run_plan(eng, pl), pp.run_model(pl), (pl["name"], "the model with its own tables"))
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["fade-long", "fade-sets R=0", "fade-sets R=1", "fade-sets R=2", "fade-sets R=28", "big"])
def test_fade_long_sets_behind_a_fade_and_the_largest_buffers(name):
    pl = pp.BY_NAME[name]
    eng = engine_for(pl)
    try:
        y = run_plan(eng, pl)
    finally:
        eng.close()
    same_bits(y, pp.run_model(pl), (name, "the model with its own tables"))
    if pl["R"] < 2:
        assert not any(s["frm"] for s in pp.steps(pl))


def test_in_place_without_and_during_a_fade():
    """d_out == d_in over sweep-1 (every phase) with no fade, and over sweep-1 with R = 200 and two sets: sixteen steps inside a fade"""
    for name in ("sweep-1", "sweep-1 fades"):
        pl = pp.BY_NAME[name]
        assert name == "sweep-1" or sum(1 for s in pp.steps(pl) if s["frm"]) == 16
        eng = engine_for(pl)
        try:
            y = run_plan(eng, pl, in_place=True)
            same_bits(run_plan(eng, pl), y, (name, "the engine-owned output against d_out == d_in"))
        finally:
            eng.close()
        same_bits(y, pp.run_model(pl), (name, "the model with its own tables"))


def test_an_output_buffer_of_the_caller():
    """d_out neither NULL nor d_in, through fade-long (two fades, From's rows growing): the output is the model's, d_in is
    unchanged, read_eq() returns the same bits"""
    pl = pp.BY_NAME["fade-long"]
    eng = engine_for(pl)
    try:
        model = enable(eng, pl["C"], pl["S"], pl["R"])
        x, sets, at, B = pp.signal(pl), sets_of(pl), 0, eng.B
        for k, nb in enumerate(pl["cuts"]):
            part = np.ascontiguousarray(x[:, at * B:(at + nb) * B])
            dx, dy = device(part), device(np.full_like(part, np.nan))
            if k in sets:
                eng.eq_set(sets[k])
            eng.step(nb)
            eng.eq(dx.data_ptr(), dy.data_ptr())
            eng.sync()
            got = dy.cpu().numpy()
            if k in sets:
                model.set(tables_=eng.eq_tables())
            same_bits(got, model.process(part), ("caller's d_out", k))
            same_bits(dx.cpu().numpy(), part, ("d_in is read only", k))
            same_bits(eng.read_eq(), got, ("read_eq from the caller's buffer", k))
            if k in sets:
                assert np.array_equal(eng.eq_tables(), em.tables(sets[k]))
            i = eng.eq_info()
            assert (i["t"], i["fade_end"], i["calls"]) == (model.t, model.fade_end(), k + 1), (k, i)
            at += nb
    finally:
        eng.close()


def test_reset_in_the_middle_of_a_fade_and_with_a_set_pending():
    """behind either reset the next steps are a fresh model's: the identity passes the bits through (silent histories, t = 0), the
    pending set is gone, and the next set is the first one of a fresh stage"""
    Cn, S, R, B = 2, 2, 200, 27
    rng = np.random.default_rng(2027)
    x = rng.standard_normal((Cn, 40 * B)).astype(np.float32)
    a, b, c = coefficients(Cn, S), coefficients(Cn, S, 4), coefficients(Cn, S, 7)
    eng = make_engine(frames_per_buffer=B)
    try:
        model = enable(eng, Cn, S, R)
        run(eng, model, x[:, :3 * B], [1, 1, 1], "before the reset", sets={0: a})
        i = eng.eq_info()
        assert i["t"] == 3 * B < i["fade_end"] == R - 1                    # in the middle of the fade
        eng.eq_reset()
        i = eng.eq_info()
        assert (i["t"], i["fade_end"]) == (0, 0) and np.array_equal(eng.eq_tables(), em.tables(em.identity(Cn, S)))
        fresh = Model(Cn, S, R)
        part = x[:, 3 * B:18 * B]
        y = run(eng, fresh, part, [1, 1, 3, 9, 1], "behind the reset in a fade", sets={1: b})
        same_bits(y[:, :B], part[:, :B], "the identity behind the reset")
        twin = Model(Cn, S, R)
        twin.process(part[:, :B])
        twin.set(b)
        same_bits(y[:, B:], twin.process(part[:, B:]), "the set behind the reset is a fresh stage's first")
        i = eng.eq_info()
        assert i["t"] == 15 * B == i["fade_end"] and i["calls"] == 8
        # a set pending: the reset drops it
        eng.eq_set(c)
        eng.eq_reset()
        i = eng.eq_info()
        assert (i["t"], i["fade_end"]) == (0, 0) and np.array_equal(eng.eq_tables(), em.tables(em.identity(Cn, S)))
        fresh = Model(Cn, S, R)
        part = x[:, 18 * B:24 * B]
        y = run(eng, fresh, part, [1, 1, 3, 1], "behind the reset with a set pending", sets={1: a})
        same_bits(y[:, :B], part[:, :B], "the identity behind the reset: the pending set is gone")
        twin = Model(Cn, S, R)
        twin.process(part[:, :B])
        twin.set(a)
        same_bits(y[:, B:], twin.process(part[:, B:]), "the set behind the reset is a fresh stage's first")
        assert eng.eq_info()["calls"] == 12
    finally:
        eng.close()
