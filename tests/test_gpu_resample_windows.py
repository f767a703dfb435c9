"""The resampler bus on the device where tests/test_gpu_resample.py does not reach: both sides of the window limit of
kernels_resample.hip (256 outputs read floor(255 M / L) + 1 + T samples; up to RS_MAX_WINDOW = 12288 of them are staged in LDS, more
are read from memory), the memory path with full workgroups, every phase and both tap loops, a history longer than the step on that
path, every p0 of a ratio, the edges of the two tap loops, and buffers of 27 and 864 frames.  Everything goes through that file's
run() and enable(): every output, count, meter and resample_info() BIT FOR BIT against tests/resample_model.py (anchored at these
ratios and tap counts by tests/test_resample_model.py), the taps the engine's own.  No tolerance anywhere in this file.

The ratios, all about 1 / 48 so that T alone decides the path:
  A  45600 -> 960 Hz,  L = 2,  M = 95:    window 12113 + T; two phases; a full workgroup stages 12113 + T samples when p0 is odd
  B  44869 -> 935 Hz,  L = 85, M = 4079:  window 12238 + T; M mod L = 84, so neighbouring threads step through all 85 phases.
     255 M is a multiple of L here, so a full workgroup stages 12237 + T samples whatever p0 is: one below the window
  C  44341 -> 924 Hz,  L = 84, M = 4031:  window 12237 + T; M mod L = 83; as B, but a full workgroup does stage the whole window"""
import os
import re

import numpy as np
import pytest
import torch                      # before the engine's library (as in test_gpu_resample.py)

from tests import resample_model as rm
from tests import test_gpu_resample as base
from tests.resample_model import pcm16

pytestmark = pytest.mark.gpu
TPB, LIMIT = 256, 12288           # RS_TPB and RS_MAX_WINDOW of kernels_resample.hip
A, B, C = (45600, 960), (44869, 935), (44341, 924)
FACTORS = {A: (2, 95), B: (85, 4079), C: (84, 4031)}
STEPS = [1, 3, 1, 3, 3]           # of tests/test_gpu_buffer_shapes_buses.py


def engine(rates, frames=0):
    eng = base.make_engine(sample_rate=0 if rates[0] == 44100 else rates[0], frames_per_buffer=frames)
    assert (eng.sample_rate, eng.B) == (rates[0], frames or 513)
    return eng


def enable(eng, Cn, rates, T):
    model = base.enable(eng, Cn, rates[1], T)
    if rates in FACTORS:
        assert (model.L, model.M) == FACTORS[rates]
    return model


def window(model):
    """what launch_resample compares with the limit"""
    return (TPB - 1) * model.M // model.L + 1 + model.T


def staged_counts(p0, n_out, L, M, T):
    """the kernel's own cnt of every workgroup of a call: E[r0 .. r_last + T - 1]"""
    cnt = []
    for j0 in range(0, n_out, TPB):
        jl = min(j0 + TPB - 1, n_out - 1)
        cnt.append((p0 + jl * M) // L - (p0 + j0 * M) // L + T)
    return cnt


def walk(eng, model, x, cuts, label):
    """base.run() cut by cut -> the output and, per call, (p0, n_out) as the engine's resample_info() and the model have them"""
    outs, calls, at, Bf = [], [], 0, eng.B
    for k, nb in enumerate(cuts):
        i = eng.resample_info()
        p0 = i["m"] * model.M - i["t"] * model.L
        assert p0 == model.p0 and 0 <= p0 < model.M, (label, k, i, model.p0)
        calls.append((p0, model.n_out(nb * Bf)))
        outs.append(base.run(eng, model, x[:, at * Bf:(at + nb) * Bf], [nb], (label, k)))
        assert outs[-1].shape[1] == calls[-1][1] == eng.resample_info()["n_out"]
        at += nb
    assert at * Bf == x.shape[1] and eng.resample_info()["calls"] == len(cuts)
    return np.concatenate(outs, axis=1), calls


def test_the_constants_are_the_kernels():
    src = open(os.path.join(os.path.dirname(base.__file__), "..", "openpbso_amd", "csrc", "kernels_resample.hip")).read()
    assert int(re.search(r"RS_TPB = (\d+);", src).group(1)) == TPB
    assert int(re.search(r"RS_MAX_WINDOW = (\d+);", src).group(1)) == LIMIT
    for rates, (L, M) in FACTORS.items():
        assert rm.ratio(*rates) == (L, M)
    assert [(TPB - 1) * M // L + 1 for L, M in FACTORS.values()] == [12113, 12238, 12237]
    assert [(TPB - 1) * M % L != 0 for L, M in FACTORS.values()] == [True, False, True] and 4079 % 85 == 84 and 4031 % 84 == 83


# (ratio, T, the window, the most samples a workgroup stages in the run; None: the memory path)
#   A 172 staged, float4     A 175 staged, the window exactly the limit     A 176 memory, float4      A 177 memory, scalar
#   B 50  staged, the window exactly the limit, scalar                      B 51  memory, scalar      B 52  memory, float4
#   C 51  staged, the window exactly the limit and all of it staged, scalar                           C 52  memory, float4
LIMIT_CASES = [(A, 172, 12285, 12285), (A, 175, LIMIT, LIMIT), (A, 176, 12289, None), (A, 177, 12290, None),
               (B, 50, LIMIT, LIMIT - 1), (B, 51, 12289, None), (B, 52, 12290, None),
               (C, 51, LIMIT, LIMIT), (C, 52, 12289, None)]
# 24 buffers of 513: one full workgroup and a few outputs; one buffer, which moves p0 and leaves a history; 36: a full group and a
# ragged one; 50: two full groups and a ragged third (the only step here of more than 512 outputs), and for A a full group at odd p0
LIMIT_CUTS = [24, 1, 36, 50]


@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("rates,T,win,most", LIMIT_CASES, ids=[f"{'ABC'[(A, B, C).index(c[0])]}-{c[1]}" for c in LIMIT_CASES])
def test_both_sides_of_the_window_limit(rates, T, win, most, Cn):
    rng = np.random.default_rng(1000 * T + Cn)
    eng = engine(rates)
    try:
        model = enable(eng, Cn, rates, T)
        L, M = model.L, model.M
        assert window(model) == win
        y, calls = walk(eng, model, base.signal(rng, Cn, sum(LIMIT_CUTS) * eng.B), LIMIT_CUTS, (rates, T, Cn))
        assert np.abs(y).max(axis=1).min() > 0
        assert [n >= TPB for _, n in calls] == [True, False, True, True]
        if most is not None:
            assert win <= LIMIT
            cnt = [c for p0, n in calls for c in staged_counts(p0, n, L, M, T)]
            # a full group stages floor((p + 255 M) / L) - floor(p / L) + T: the window, or one less where p or 255 M is a multiple of L
            assert max(cnt) == most == (win if (TPB - 1) * M % L else win - 1) and min(cnt) < win // 2, cnt
        else:
            assert win > LIMIT
            p0, n = max(calls, key=lambda c: c[1])
            assert n > 2 * TPB
            phases = {(p0 + j * M) % L for j in range(n)}
            assert len(phases) == L and phases == set(range(L))          # (A: both; B: all 85; C: all 84)
            # its first output reads at local sample p0 div L < T - 1: its late taps the history, tap 0 the input (the per-tap switch)
            assert p0 // L < T - 1
    finally:
        eng.close()


@pytest.mark.parametrize("rates,T", [(A, 176), (A, 177), (B, 51), (C, 52)], ids=["A-176", "A-177", "B-51", "C-52"])
def test_a_history_longer_than_the_steps_on_the_memory_path(rates, T):
    """27 frames: T - 1 samples of history against steps of 27, each with no output or one, which reads history and input; the same
    1080 samples in one step and in four"""
    rng = np.random.default_rng(T)
    Cn = 2
    x = base.signal(rng, Cn, 40 * 27)
    outs = []
    for cuts in ([1] * 40, [40], [3, 1, 20, 16]):
        eng = engine(rates, 27)
        try:
            model = enable(eng, Cn, rates, T)
            assert window(model) > LIMIT and T - 1 > eng.B
            y, calls = walk(eng, model, x, cuts, (rates, T, cuts))
            outs.append(y)
            if len(cuts) == 40:
                assert {n for _, n in calls} == {0, 1} and len({p0 for p0, _ in calls}) == 40
        finally:
            eng.close()
    assert outs[0].shape == (Cn, rm.ceil_div(40 * 27 * model.L, model.M)) and np.abs(outs[0]).max() > 0
    base.same_bits(outs[1], outs[0], "40 against 40 x 1")
    base.same_bits(outs[2], outs[0], "3 + 1 + 20 + 16 against 40 x 1")


@pytest.mark.parametrize("T", [4, 7])
@pytest.mark.parametrize("rates,factors,counts", [((44100, 50400), (8, 7), {30, 31}), ((44100, 6300), (1, 7), {3, 4})],
                         ids=["8/7", "1/7"])
def test_every_p0_of_a_ratio(rates, factors, counts, T):
    """27 frames, 15 steps of one buffer: 27 L mod 7 = 6, so p0 walks 0, 1, .., 6 and round again; then the same in one step"""
    rng = np.random.default_rng(T + factors[0])
    Cn = 2
    x = base.signal(rng, Cn, 15 * 27)
    outs = []
    for cuts in ([1] * 15, [15]):
        eng = engine(rates, 27)
        try:
            model = enable(eng, Cn, rates, T)
            assert (model.L, model.M) == factors
            y, calls = walk(eng, model, x, cuts, (rates, T, cuts))
            outs.append(y)
            if len(cuts) == 15:
                assert [p0 for p0, _ in calls] == [k % 7 for k in range(15)]
                assert {p0 for p0, _ in calls} == set(range(7)) and {n for _, n in calls} == counts
        finally:
            eng.close()
    assert outs[0].shape == (Cn, rm.ceil_div(15 * 27 * factors[0], 7)) and np.abs(outs[0]).max() > 0
    base.same_bits(outs[1], outs[0], "15 against 15 x 1")


@pytest.mark.parametrize("rates", [(44100, 48000), (44100, 22050)])
def test_tap_count_edges(rates):
    """the scalar loop at 3, 5 and 255, the float4 loop at its first (4), at 12 and at its last but one (252); every T on one engine,
    a step of one buffer, then one of two"""
    rng = np.random.default_rng(rates[1])
    eng = engine(rates)
    try:
        for T in (3, 4, 5, 12, 252, 255):
            model = enable(eng, 2, rates, T)
            assert window(model) <= LIMIT
            y = base.run(eng, model, base.signal(rng, 2, 3 * eng.B), [1, 2], (rates, T))
            assert y.shape == (2, rm.ceil_div(3 * eng.B * model.L, model.M)) and np.abs(y).max() > 0
    finally:
        eng.close()


@pytest.mark.parametrize("frames", [27, 864])
@pytest.mark.parametrize("rates,T", [((44100, 96000), 32), ((44100, 22050), 7), (A, 176)], ids=["320/147", "1/2", "A-176"])
def test_buffers_of_27_and_864_frames(rates, T, frames):
    """C = 3 in steps of 1 and 3 buffers; A, on the memory path, at 864 frames with a step of 16 more: a full workgroup and a
    ragged one.  The 16-bit PCM of the last step"""
    rng = np.random.default_rng(frames + T)
    Cn = 3
    cuts = STEPS + [16] if rates == A and frames == 864 else STEPS
    eng = engine(rates, frames)
    try:
        model = enable(eng, Cn, rates, T)
        assert (window(model) > LIMIT) == (rates == A)
        y, calls = walk(eng, model, base.signal(rng, Cn, sum(cuts) * frames, 0.5), cuts, (rates, T, frames))
        assert y.shape == (Cn, rm.ceil_div(sum(cuts) * frames * model.L, model.M)) and np.abs(y).max() > 0
        if len(cuts) > len(STEPS):
            assert calls[-1][1] > TPB
        n_last = calls[-1][1]
        assert n_last > 0
        p = eng.read_resample_pcm16()
        assert p.shape == (n_last, Cn) and np.array_equal(p, pcm16(y[:, y.shape[1] - n_last:])) and np.abs(p).max() > 0
    finally:
        eng.close()
