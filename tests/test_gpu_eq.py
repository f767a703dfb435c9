"""The EQ bus (include/openpbso_amd.h "EQ bus"; kernels_eq.hip) on the device.  Every output is compared BIT FOR BIT with the
reference of the stated arithmetic (tests/cpp/eq_ref.c through tests/eq_model.py, anchored by tests/test_eq_model.py); the model is
fed the engine's own tables, read back with eq_tables() once a set has taken effect.  The engine behind it is one object of 64
modes: the stage does not care what made its input."""
import ctypes as C

import numpy as np
import pytest
import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

from openpbso_amd import Engine, capi, synth
from openpbso_amd.solver import PbsoError
from tests import eq_model as em
from tests.eq_model import Model

pytestmark = pytest.mark.gpu
RATE = 44100.0
# ten sections across the band, the low ones among them: what test_eq_model.py measures, and three more kinds
BANK = [("highpass", 30.0, 0.707, 0.0), ("peak", 100.0, 4.0, 12.0), ("highshelf", 8000.0, 0.707, 6.0), ("highpass", 5.0, 8.0, 0.0),
        ("peak", 1000.0, 2.0, -9.0), ("lowpass", 18000.0, 0.707, 0.0), ("lowshelf", 200.0, 0.707, -6.0), ("highpass", 20.0, 2.0, 0.0),
        ("peak", 3000.0, 1.0, 3.0), ("lowpass", 9000.0, 1.2, 0.0)]


def make_engine(n_modes=64, **kw):
    eng = Engine(**kw)
    eng.add_object(synth.eigenvalues(n_modes, 9131), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    eng.set_use_transfer(0, False)
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


def coefficients(Cn, S, shift=0):
    """[C][S][5]: every channel its own sections of BANK"""
    return np.array([[capi.eq_design(*BANK[(shift + 3 * c + s) % len(BANK)][:1], RATE, *BANK[(shift + 3 * c + s) % len(BANK)][1:])
                      for s in range(S)] for c in range(Cn)])


def run(eng, model, x, cuts, label, sets=None, in_place=False):
    """x [C][n] through the engine and the model in steps of cuts[i] buffers; sets {step index: sos} are given before that step.
    The model takes a set's tables from the engine once the step has made them the ones in force."""
    outs, at, B = [], 0, eng.B
    for k, nb in enumerate(cuts):
        part = x[:, at * B:(at + nb) * B]
        dx = device(part)
        if sets and k in sets:
            eng.eq_set(sets[k])
        eng.step(nb)
        if in_place:
            eng.eq(dx.data_ptr(), dx.data_ptr())
            eng.sync()
            got = dx.cpu().numpy()
            same_bits(eng.read_eq(), got, (label, k, "read from the caller's buffer"))
        else:
            eng.eq(dx.data_ptr())
            got = eng.read_eq()
            assert np.array_equal(dx.cpu().numpy(), part), (label, k, "d_in is read only")
        if sets and k in sets:
            tab = eng.eq_tables()
            assert np.array_equal(tab, em.tables(sets[k])), (label, k, "the engine's tables are the reference's")
            model.set(tables_=tab)
        same_bits(got, model.process(part), (label, k))
        i = eng.eq_info()
        assert (i["t"], i["fade_end"]) == (model.t, model.fade_end()), (label, k, i)
        outs.append(got)
        at += nb
    return np.concatenate(outs, axis=1)


def enable(eng, Cn, S, R=0):
    eng.eq_enable(Cn, S, R)
    i = eng.eq_info()
    assert (i["t"], i["fade_end"], i["calls"]) == (0, 0, 0)
    assert np.array_equal(eng.eq_tables(), em.tables(em.identity(Cn, S)))
    return Model(Cn, S, R)


@pytest.mark.parametrize("S", [1, 2, 8])
@pytest.mark.parametrize("Cn", [1, 3, 8])
def test_channels_and_sections(Cn, S):
    """a step of one buffer, then one of two (513 mod P = 1: every step begins inside a block)"""
    rng = np.random.default_rng(10 * Cn + S)
    eng = make_engine()
    try:
        model = enable(eng, Cn, S)
        y = run(eng, model, signal(rng, Cn, 3 * eng.B), [1, 2], (Cn, S), sets={0: coefficients(Cn, S)})
        assert np.isfinite(y).all() and np.abs(y).max() > 0
    finally:
        eng.close()


def test_the_cut_into_steps_does_not_matter_and_in_place_is_the_same():
    rng = np.random.default_rng(6)
    Cn, S = 2, 4
    x = signal(rng, Cn, 4 * 513)
    sos = coefficients(Cn, S)
    outs = []
    for cuts, in_place in (([1, 1, 1, 1], False), ([3, 1], False), ([4], False), ([1, 2, 1], True)):
        eng = make_engine()
        try:
            outs.append(run(eng, enable(eng, Cn, S), x, cuts, (cuts, in_place), sets={0: sos}, in_place=in_place))
        finally:
            eng.close()
    same_bits(outs[1], outs[0], "[3, 1] against [1, 1, 1, 1]")
    same_bits(outs[2], outs[0], "[4] against [1, 1, 1, 1]")
    same_bits(outs[3], outs[0], "d_out == d_in against the engine-owned output")


@pytest.mark.parametrize("R", [0, 100, 513, 700, 1])
def test_a_set_between_steps(R):
    """identity, then a set before the second step and another before the fourth: R = 700 fades across a step edge, R = 513 ends
    one sample before it, R = 1 reaches w = 1 at once"""
    rng = np.random.default_rng(R)
    Cn, S = 3, 2
    eng = make_engine()
    try:
        model = enable(eng, Cn, S, R)
        x = signal(rng, Cn, 6 * eng.B)
        y = run(eng, model, x, [1, 1, 1, 2, 1], R, sets={1: coefficients(Cn, S), 3: coefficients(Cn, S, 5)})
        same_bits(y[:, :eng.B], x[:, :eng.B], "the identity before the first set")
        assert eng.eq_info()["sets"] == 2 and eng.eq_info()["calls"] == 5
    finally:
        eng.close()


def test_refusals_change_nothing_and_the_reset():
    rng = np.random.default_rng(9)
    Cn, S, R = 2, 2, 700
    eng = Engine()
    try:
        eng.add_object(synth.eigenvalues(32, 40), synth.RHO, synth.ALPHA, synth.BETA)
        with pytest.raises(PbsoError) as ei:
            eng.eq_enable(Cn, S)                                         # before finalize
        assert ei.value.status == capi.ERR_STATE
        eng.finalize()
        lib, fp, dp = capi.lib(), C.POINTER(C.c_float), C.POINTER(C.c_double)
        x = signal(rng, Cn, 8 * eng.B)
        B = eng.B
        dx = device(x[:, :B])
        for call in (lambda: eng.eq(dx.data_ptr()), eng.eq_reset, eng.eq_info):
            with pytest.raises(PbsoError) as ei:
                call()                                                   # not enabled
            assert ei.value.status == capi.ERR_STATE
        one = np.zeros(5)
        assert lib.pbso_eq_set(eng._h, one.ctypes.data_as(dp)) == capi.ERR_STATE == lib.pbso_eq_tables(eng._h, one.ctypes.data_as(dp), 5)
        for bad in ((0, 1), (9, 1), (1, 0), (1, 9), (1, 1, -1), (1, 1, (1 << 20) + 1)):
            with pytest.raises(PbsoError) as ei:
                eng.eq_enable(*bad)
            assert ei.value.status == capi.ERR_INVALID, bad
        model = enable(eng, Cn, S, R)

        def refused(call, status):
            before, tab = eng.eq_info(), eng.eq_tables()
            with pytest.raises(PbsoError) as ei:
                call()
            assert ei.value.status == status and eng.eq_info() == before and np.array_equal(eng.eq_tables(), tab)

        refused(lambda: eng.eq(dx.data_ptr()), capi.ERR_STATE)                                      # no step since enable
        host = np.empty(Cn * B, dtype=np.float32)
        assert lib.pbso_read_eq(eng._h, host.ctypes.data_as(fp), host.size) == capi.ERR_STATE       # nothing processed yet
        a, b = coefficients(Cn, S), coefficients(Cn, S, 4)
        # a set during a fade is refused: the running fade goes on as the model's
        run(eng, model, x[:, :B], [1], "first", sets={0: a})
        assert eng.eq_info()["fade_end"] == R - 1 > eng.eq_info()["t"]
        refused(lambda: eng.eq_set(b), capi.ERR_STATE)
        run(eng, model, x[:, B:2 * B], [1], "behind the refused set")
        assert eng.eq_info()["fade_end"] == eng.eq_info()["t"] == 2 * B
        # an unstable, a NaN and a wrong-size set
        for k, v in ((4, 1.0), (4, -1.0), (3, 2.5), (0, float("nan")), (3, float("inf"))):
            bad = b.copy()
            bad[1, 1, k] = v
            refused(lambda: eng.eq_set(bad), capi.ERR_INVALID)
        refused(lambda: eng.eq_set(b[:1]), capi.ERR_INVALID)
        refused(lambda: eng.eq_set(np.zeros((Cn, S, 6))), capi.ERR_INVALID)
        assert lib.pbso_eq_set(eng._h, None) == capi.ERR_INVALID
        big = np.empty(Cn * S * 5 * em.P + 1)
        assert lib.pbso_eq_tables(eng._h, big.ctypes.data_as(dp), big.size) == capi.ERR_INVALID
        run(eng, model, x[:, 2 * B:3 * B], [1], "behind the refused sets")
        # a set replaced before any step took it up
        eng.eq_set(a)
        y3 = run(eng, model, x[:, 3 * B:4 * B], [1], "a replaced set", sets={0: b})
        assert eng.eq_info()["sets"] == 3
        # the same step twice, a skipped step, a NULL input, an overlap that is not d_in itself
        dx = device(x[:, 4 * B:5 * B])
        refused(lambda: eng.eq(dx.data_ptr()), capi.ERR_STATE)
        same_bits(eng.read_eq(), y3, "the refusal left the last output readable")
        eng.step(1)
        before = eng.eq_info()
        assert lib.pbso_eq(eng._h, None, None) == capi.ERR_INVALID and eng.eq_info() == before
        refused(lambda: eng.eq(dx.data_ptr(), dx.data_ptr() + 4), capi.ERR_INVALID)
        eng.eq(dx.data_ptr())                                                                         # (the refusals did not use the step up)
        same_bits(eng.read_eq(), model.process(x[:, 4 * B:5 * B]), "behind the refusals")
        eng.step(1)
        eng.step(1)
        refused(lambda: eng.eq(dx.data_ptr()), capi.ERR_STATE)                                      # a step was skipped
        # the reset: the identity again, the histories silent, t = 0, armed for the NEXT step
        eng.eq_reset()
        model.reset()
        i = eng.eq_info()
        assert (i["t"], i["fade_end"]) == (0, 0) and np.array_equal(eng.eq_tables(), em.tables(em.identity(Cn, S)))
        refused(lambda: eng.eq(dx.data_ptr()), capi.ERR_STATE)
        y = run(eng, model, x[:, 5 * B:7 * B], [1, 1], "after the reset", sets={1: a})
        same_bits(y[:, :B], x[:, 5 * B:6 * B], "the identity behind the reset")
        fresh = Model(Cn, S, R)
        fresh.process(x[:, 5 * B:6 * B])
        fresh.set(a)
        same_bits(y[:, B:], fresh.process(x[:, 6 * B:7 * B]), "the reset is a fresh start")
    finally:
        eng.close()


def test_identity_passes_the_bits_through():
    rng = np.random.default_rng(12)
    eng = make_engine()
    try:
        model = enable(eng, 8, 8, 64)
        x = signal(rng, 8, 3 * eng.B)
        x[0, :4] = [1e-41, -1e-41, 3.0e38, -3.0e38]                     # subnormals are kept
        y = run(eng, model, x, [1, 2], "identity")
        same_bits(y, x, "identity")
    finally:
        eng.close()


def test_a_step_shorter_than_a_block():
    """an engine of 27 frames: steps of 27 and 81 samples against P + 2 samples of history"""
    rng = np.random.default_rng(27)
    Cn, S = 2, 3
    x = signal(rng, Cn, 12 * 27)
    sos = coefficients(Cn, S)
    outs = []
    for cuts in ([1] * 12, [3] * 4, [1, 3, 1, 1, 3, 3]):
        eng = make_engine(frames_per_buffer=27)
        try:
            assert eng.B == 27
            outs.append(run(eng, enable(eng, Cn, S, 40), x, cuts, cuts, sets={0: sos, 2: coefficients(Cn, S, 2)} if len(cuts) == 12 else {0: sos}))
        finally:
            eng.close()
    same_bits(outs[2], outs[1], "[1, 3, 1, 1, 3, 3] against [3, 3, 3, 3]")
    assert outs[0].shape == outs[1].shape


def test_a_step_of_130_buffers():
    """66 690 samples: the serial chain crosses 1 042 blocks, seventeen batches of the chain kernel's wave"""
    rng = np.random.default_rng(130)
    Cn, S = 2, 2
    eng = make_engine()
    try:
        model = enable(eng, Cn, S, 100)
        x = signal(rng, Cn, 131 * eng.B)
        run(eng, model, x, [1, 130], "130 buffers", sets={0: coefficients(Cn, S), 1: coefficients(Cn, S, 3)})
    finally:
        eng.close()
