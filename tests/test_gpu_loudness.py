"""The loudness bus (include/openpbso_amd.h "Loudness bus"; kernels_loudness.hip) on the device.  Every record is compared BIT FOR
BIT with the reference of the stated arithmetic (tests/cpp/loudness_ref.c through tests/loudness_model.py, anchored by
tests/test_loudness_model.py): the energy as uint64, the two peaks as uint32.  The engine behind it is one object of 64 modes: the
stage does not care what made its input, which is the test's own device tensor."""
import ctypes as C
import math

import numpy as np
import pytest
import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

from openpbso_amd import Engine, capi, synth
from openpbso_amd.solver import PbsoError
from tests import loudness_model as lm

pytestmark = pytest.mark.gpu


def make_engine(rate=44100, n_modes=64):
    kw = {} if rate == 44100 else dict(sample_rate=rate)
    eng = Engine(**kw)
    eng.add_object(synth.eigenvalues(n_modes, 9131, **(dict(f_hi=9000.0) if rate < 40000 else {})), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    eng.set_use_transfer(0, False)
    return eng


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    return t


def signal(rng, rows, n, scale=0.3):
    """noise under a slow swell, so that sub-blocks and channels differ in level, with a few loud samples for the peaks"""
    x = rng.standard_normal((rows, n)) * scale * (0.6 + 0.4 * np.sin(np.arange(n) / 3000.0 + np.arange(rows)[:, None]))
    x[:, rng.integers(0, n, 8)] *= 3.0
    return x.astype(np.float32)


def same_records(got, want, label):
    assert got.shape == want.shape, (label, got.shape, want.shape)
    for field, bits in (("energy", np.uint64), ("true_peak", np.uint32), ("sample_peak", np.uint32)):
        g, w = np.ascontiguousarray(got[field]).view(bits), np.ascontiguousarray(want[field]).view(bits)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (label, field, len(bad), bad[:4].tolist(), got[field][tuple(bad[0])], want[field][tuple(bad[0])])


def enable(eng, Cn, weight=None, max_blocks=1000, true_peak=True):
    eng.loudness_enable(Cn, weight, max_blocks, true_peak)
    assert eng.loudness_info() == {"t": 0, "blocks": 0, "calls": 0, "max_blocks": max_blocks}
    h = eng.loudness_taps()
    assert h.dtype == np.float32 and np.array_equal(h.view(np.uint32), lm.taps(eng.sample_rate).view(np.uint32)), "the taps are the model's"
    return lm.Model(eng.sample_rate, Cn, weight, true_peak, taps_=h)


def run(eng, model, x, cuts, label):
    """x [C][n] through the engine and the model in steps of cuts[i] buffers; the records each step appends are compared"""
    at, B = 0, eng.B
    for k, nb in enumerate(cuts):
        part = x[:, at * B:(at + nb) * B]
        dx = device(part)
        before = eng.loudness_info()["blocks"]
        eng.step(nb)
        eng.loudness(dx.data_ptr())
        want = model.process(part)
        i = eng.loudness_info()
        assert (i["t"], i["blocks"]) == (model.t, model.records.shape[0]) and i["blocks"] - before == want.shape[0], (label, k, i)
        same_records(eng.read_loudness_blocks(before), want, (label, k))
        assert np.array_equal(dx.cpu().numpy(), part), (label, k, "d_in is read only")
        at += nb
    same_records(eng.read_loudness_blocks(), model.records, (label, "the whole log"))
    return eng.read_loudness_blocks()


@pytest.mark.parametrize("true_peak", [True, False])
@pytest.mark.parametrize("Cn", [1, 3, 8])
def test_channels_and_true_peak(Cn, true_peak):
    """one-buffer steps (513 < Hs = 4410: a sub-block is built over nine steps of carries), then a step of 18 buffers with two
    sub-block ends inside it, then three more buffers"""
    rng = np.random.default_rng(10 * Cn + true_peak)
    eng = make_engine()
    try:
        model = enable(eng, Cn, true_peak=true_peak)
        rec = run(eng, model, signal(rng, Cn, 31 * eng.B), [1] * 10 + [18, 3], (Cn, true_peak))
        assert rec.shape == (3, Cn) and (rec["energy"] > 0).all()
        if true_peak:
            assert (rec["sample_peak"] > 0).all() and (rec["true_peak"] > 0).all()
        else:
            assert (rec["sample_peak"] == 0).all() and (rec["true_peak"] == 0).all()
        r = eng.loudness_report()
        assert r["n_blocks"] == 3 and r["integrated"] == r["momentary"] == -math.inf       # fewer than four sub-blocks
    finally:
        eng.close()


@pytest.mark.parametrize("rate", [22050, 96000])
def test_other_rates(rate):
    """22050 Hz: Hs = 2205 = 34 * 64 + 29, a tail of 29 samples behind the last full row of the 64 accumulators; 96000 Hz: O = 2"""
    rng = np.random.default_rng(rate)
    eng = make_engine(rate)
    try:
        model = enable(eng, 2)
        assert model.O == (2 if rate == 96000 else 4) and model.hs == rate // 10
        rec = run(eng, model, signal(rng, 2, 64 * eng.B), [1, 1, 1, 18, 1, 2, 40], rate)
        assert rec.shape[0] == 64 * eng.B // model.hs >= 3
    finally:
        eng.close()


def test_a_step_that_ends_exactly_on_a_sub_block_end():
    """1 + 489 buffers end at sample 251 370 = lcm(513, 4410), the end of sub-block 56; the first step left a carry behind, which the
    one-buffer step behind the boundary must not pick up: it starts from zeroed accumulators and maxima"""
    rng = np.random.default_rng(490)
    eng = make_engine()
    try:
        model = enable(eng, 2)
        assert 490 * eng.B == 57 * model.hs
        rec = run(eng, model, signal(rng, 2, 499 * eng.B), [1, 489, 1, 8], "lcm")
        assert rec.shape[0] == 58
        i = eng.loudness_info()
        assert i == {"t": 499 * eng.B, "blocks": 58, "calls": 4, "max_blocks": 1000}
        # and a single step of 490 buffers, from the enable
        model = enable(eng, 2)
        run(eng, model, signal(rng, 2, 491 * eng.B), [490, 1], "490")
        assert eng.loudness_info()["blocks"] == 57
    finally:
        eng.close()


def test_the_cut_into_steps_does_not_matter():
    rng = np.random.default_rng(20)
    Cn = 3
    x = signal(rng, Cn, 20 * 513)
    logs = []
    for cuts in ([1] * 20, [20], [7, 1, 12]):
        eng = make_engine()
        try:
            logs.append(run(eng, enable(eng, Cn, [1.0, 0.5, 1.41]), x, cuts, cuts))
        finally:
            eng.close()
    same_records(logs[1], logs[0], "[20] against [1] * 20")
    same_records(logs[2], logs[0], "[7, 1, 12] against [1] * 20")
    assert logs[0].shape == (2, Cn)


def test_subnormal_and_large_inputs_are_kept():
    rng = np.random.default_rng(5)
    eng = make_engine()
    try:
        model = enable(eng, 2)
        x = signal(rng, 2, 18 * eng.B)
        x[0, :4410] = 1e-41                                   # a sub-block of subnormals: their peaks are subnormal, their energy underflows
        x[1, 100:104] = [3.0e18, -3.0e18, 1e-41, -1e-41]
        rec = run(eng, model, x, [18], "subnormals")
        assert 0 < rec["sample_peak"][0, 0] < 1.2e-38 and rec["sample_peak"][0, 1] == np.float32(3.0e18)
    finally:
        eng.close()


def test_refusals_change_nothing_the_full_log_and_the_reset():
    rng = np.random.default_rng(9)
    Cn = 2
    eng = Engine()
    try:
        eng.add_object(synth.eigenvalues(32, 40), synth.RHO, synth.ALPHA, synth.BETA)
        with pytest.raises(PbsoError) as ei:
            eng.loudness_enable(Cn)                                      # before finalize
        assert ei.value.status == capi.ERR_STATE
        eng.finalize()
        lib = capi.lib()
        B = eng.B
        x = signal(rng, Cn, 60 * B)
        dx = device(x[:, :B])
        for call in (lambda: eng.loudness(dx.data_ptr()), eng.loudness_reset, eng.loudness_info, eng.loudness_report,
                     lambda: eng.read_loudness_blocks(0, 0)):
            with pytest.raises(PbsoError) as ei:
                call()                                                   # not enabled
            assert ei.value.status == capi.ERR_STATE
        one = np.zeros(48, dtype=np.float32)
        assert lib.pbso_loudness_taps(eng._h, one.ctypes.data_as(C.POINTER(C.c_float)), 48) == capi.ERR_STATE
        for bad in ((0,), (9,), (2, None, 0), (2, None, (1 << 22) + 1), (2, [1.0, -1.0]), (2, [1.0, float("nan")]), (2, [float("inf"), 1.0])):
            with pytest.raises(PbsoError) as ei:
                eng.loudness_enable(*bad)
            assert ei.value.status == capi.ERR_INVALID, bad
        with pytest.raises(PbsoError) as ei:
            eng.loudness_enable(2, [1.0])                                # weight of the wrong size
        assert ei.value.status == capi.ERR_INVALID
        model = enable(eng, Cn, max_blocks=3)

        def refused(call, status):
            before, log = eng.loudness_info(), eng.read_loudness_blocks()
            with pytest.raises(PbsoError) as ei:
                call()
            assert ei.value.status == status and eng.loudness_info() == before
            same_records(eng.read_loudness_blocks(), log, "the log behind a refusal")

        refused(lambda: eng.loudness(dx.data_ptr()), capi.ERR_STATE)                               # no step since enable
        run(eng, model, x[:, :18 * B], [18], "two records")
        dx = device(x[:, 18 * B:19 * B])
        refused(lambda: eng.loudness(dx.data_ptr()), capi.ERR_STATE)                               # the same step twice
        eng.step(1)
        before = eng.loudness_info()
        assert lib.pbso_loudness(eng._h, None) == capi.ERR_INVALID and eng.loudness_info() == before
        eng.loudness(dx.data_ptr())                                                                  # (the refusals did not use the step up)
        same_records(eng.read_loudness_blocks(2), model.process(x[:, 18 * B:19 * B]), "behind the refusals")
        # read-backs out of range; taps of the wrong size
        for first, n in ((-1, 1), (0, 3), (3, 0), (2, 1), (0, -1)):
            refused(lambda: eng.read_loudness_blocks(first, n), capi.ERR_INVALID)
        assert eng.read_loudness_blocks(2, 0).shape == (0, Cn)
        assert lib.pbso_loudness_taps(eng._h, one.ctypes.data_as(C.POINTER(C.c_float)), 47) == capi.ERR_INVALID
        assert lib.pbso_loudness_taps(eng._h, None, 48) == capi.ERR_INVALID
        assert lib.pbso_loudness_report(eng._h, None) == capi.ERR_INVALID and lib.pbso_loudness_info(eng._h, None) == capi.ERR_INVALID
        # the log full: 19 buffers are in, records 0 and 1 logged; 18 more would end sub-blocks 2 and 3, and max_blocks is 3
        d18 = device(x[:, 19 * B:37 * B])
        eng.step(18)
        refused(lambda: eng.loudness(d18.data_ptr()), capi.ERR_STATE)
        eng.step(1)
        refused(lambda: eng.loudness(dx.data_ptr()), capi.ERR_STATE)                               # a step was skipped
        # the reset: the log empty, every state silent, t = 0, armed for the NEXT step; what follows equals a fresh start
        eng.loudness_reset()
        model.reset()
        assert eng.loudness_info() == {"t": 0, "blocks": 0, "calls": 2, "max_blocks": 3}
        refused(lambda: eng.loudness(dx.data_ptr()), capi.ERR_STATE)
        rec = run(eng, model, x[:, 37 * B:60 * B], [1, 4, 13, 5], "after the reset")
        fresh = lm.Model(44100, Cn, taps_=eng.loudness_taps())
        fresh.process(x[:, 37 * B:60 * B])
        same_records(rec, fresh.records, "the reset is a fresh start")
        assert rec.shape[0] == 2
    finally:
        eng.close()


def test_a_rate_without_a_hop_is_refused():
    eng = make_engine(45045)
    try:
        with pytest.raises(PbsoError) as ei:
            eng.loudness_enable(2)
        assert ei.value.status == capi.ERR_INVALID
    finally:
        eng.close()


def test_ebu_tech_3341_case_5_on_the_device():
    """20 s at -26 dBFS, 20.1 s at -20, 20 s at -26, a stereo 1 kHz sine at 44100 Hz: 601 sub-blocks; integrated -23 +-0.1 LU.  The
    last step is filled up to whole buffers with silence, which ends no further sub-block."""
    from tests.test_loudness_model import stereo_programme
    eng = make_engine()
    try:
        B, hs = eng.B, 4410
        x = stereo_programme(44100, [(20.0, -26.0), (20.1, -20.0), (20.0, -26.0)])
        assert x.shape[1] == 601 * hs
        nb = -(-x.shape[1] // B)
        x = np.concatenate([x, np.zeros((2, nb * B - x.shape[1]), dtype=np.float32)], axis=1)
        eng.loudness_enable(2, None, 700, True)
        dx = device(x)
        at = 0
        while at < nb:
            k = min(500, nb - at)
            part = dx[:, at * B:(at + k) * B].contiguous()
            torch.cuda.synchronize()
            eng.step(k)
            eng.loudness(part.data_ptr())
            eng.sync()
            at += k
        r = eng.loudness_report()
        print(f"case 5 on the device: integrated {r['integrated']:.4f} LUFS, true peak {20 * math.log10(r['true_peak']):.3f} dBTP")
        assert r["n_blocks"] == 601 and abs(r["integrated"] + 23.0) <= 0.1, r
        assert abs(20 * math.log10(r["sample_peak"]) + 20.0) < 0.01 and -20.4 <= 20 * math.log10(r["true_peak"]) <= -19.8
        blocks = eng.read_loudness_blocks()
        host = capi.loudness_report_from_blocks(blocks, hs)
        assert host == r
    finally:
        eng.close()
