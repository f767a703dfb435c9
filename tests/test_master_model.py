"""The reference of the master bus (tests/cpp/master_ref.c through tests/master_model.py) held to independent answers, without a
GPU: a literal Python transcription of the header's lines with an exact rational fmaf on tiny shapes, the hard ceiling, the exact
pass-through of unlimited stretches, independence of how the samples are cut into steps, the gain ramp and the window.  The C file
takes the sliding minimum twice, in linear time and by the header's double loop; the transcription anchors the loop, and the two
are held bit-equal at windows around every power of two up to 4097."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import master_window_plan as wp
from tests.master_model import B, Model, evaluate, pcm16, window


def f32(x):
    return float(np.float32(x))


def round_f32(v):
    """the rational v rounded once to f32 (nearest, ties to even, subnormals included); an exact zero is +0"""
    if v == 0:
        return 0.0
    e = abs(v.numerator).bit_length() - v.denominator.bit_length()   # 2^(e-1) <= |v| < 2^(e+1)
    if Fraction(2) ** e > abs(v):
        e -= 1
    ulp = max(e, -126) - 23
    return math.ldexp(round(v / Fraction(2) ** ulp), ulp)            # (round() of a Fraction rounds halves to even)


def fmaf(a, b, c):
    """a * b + c rounded ONCE: the sum is taken exactly, as a rational.  The accumulators here start at +0.f and never become -0"""
    return round_f32(Fraction(a) * Fraction(b) + Fraction(c))


def brute(u, p, L, H, T, w):
    """the header's lines, literally, in Python: u [C][n] from t = 0, p [n] the f32 gain per sample"""
    Cn, n = u.shape
    T = f32(T)

    def v(c, t):
        return f32(float(p[t]) * float(u[c, t])) if t >= 0 else 0.0

    rs = {}

    def r(t):
        if t < 0:
            return 1.0
        if t not in rs:
            pk = max(abs(v(c, t)) for c in range(Cn))
            rs[t] = round_f32(Fraction(T) / Fraction(pk)) if pk > T else 1.0
        return rs[t]

    def a(t):
        return min(r(t - j) for j in range(L + H + 1))

    y = np.zeros((Cn, n), dtype=np.float32)
    for t in range(n):
        acc = 0.0
        for k in range(L - 1, -1, -1):
            acc = fmaf(float(w[k]), a(t - k), acc)
        g = min(acc, r(t - L))
        for c in range(Cn):
            y[c, t] = min(max(f32(v(c, t - L) * g), -T), T)
    return y


def test_python_fmaf_rounds_once():
    a = f32(1 + 2.0 ** -23)
    assert fmaf(a, a, -1.0) == f32(2.0 ** -22 + 2.0 ** -46)          # the product's low bits survive: no intermediate rounding
    assert fmaf(3.0, 5.0, 7.0) == 22.0


@pytest.mark.parametrize("L", [1, 3, 5])
@pytest.mark.parametrize("H", [0, 2])
def test_model_equals_the_literal_transcription(L, H):
    rng = np.random.default_rng(10 * L + H)
    u = rng.standard_normal((2, 40)).astype(np.float32)
    for literal in (True, False):                                    # the header's double loop, and the linear-time minimum
        m = Model(2, 0.7, L, H, 7, literal=literal)
        m.set_gain(1.5)                                              # a ramp over the first 7 samples
        p = m._p(np.arange(40)).astype(np.float32)
        assert p[0] != p[3] and p[6] == p[39] == np.float32(1.5)
        got = np.concatenate([m.process(u[:, :13]), m.process(u[:, 13:])], axis=1)
        want = brute(u, p, L, H, 0.7, m.w)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), literal
    assert (want != np.concatenate([np.zeros((2, L), dtype=np.float32), p * u], axis=1)[:, :40]).any()   # (something was limited)


@pytest.mark.parametrize("W", [2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 4097])
def test_the_linear_time_minimum_equals_the_literal_loop_bit_for_bit(W):
    """y, g and the count of master_ref against master_ref_literal: L = 1 with H = W - 2 and H = 0 with L = W - 1, on dense noise
    and on the staircase of tests/master_window_plan.py (n = W + 3 x 513 at least; a staircase that needs more keeps its length)"""
    n = W + 3 * B
    for L, H in ((1, W - 2), (W - 1, 0)):
        case = dict(W=W, L=L, H=H, C=2, seed=W)
        stairs, _ = wp.staircase(case)
        if stairs.shape[1] < n:
            pad = np.random.default_rng(W).standard_normal((2, n - stairs.shape[1])) * wp.NOISE
            stairs = np.concatenate([stairs, pad.astype(np.float32)], axis=1)
        for name, u in (("dense", wp.dense(case, n)), ("staircase", stairs)):
            v = np.concatenate([np.zeros((2, 2 * L + H), dtype=np.float32), u], axis=1)
            y, g, cnt = evaluate(v, L, H, 0.7, window(L))
            yl, gl, cntl = evaluate(v, L, H, 0.7, window(L), literal=True)
            assert np.array_equal(y.view(np.uint32), yl.view(np.uint32)), (name, L, H)
            assert np.array_equal(g.view(np.uint32), gl.view(np.uint32)) and cnt == cntl, (name, L, H)
            assert (g < 1).any() and np.unique(g).size > 4


@pytest.mark.parametrize("L", [1, 64])
def test_the_ceiling_holds_exactly(L):
    rng = np.random.default_rng(L)
    u = rng.standard_normal((2, 3 * B)).astype(np.float32)
    T = np.float32(0.7)
    m = Model(2, 0.7, L, 0, 0)
    y = m.process(u)
    assert np.abs(y).max() <= T
    if L == 1:
        # w = [1], a(t) = min(r(t), r(t - 1)): where sample t - 1 alone sets it, y is v * fl(T / |v|) before the clamp
        assert m.w[0] == 1
        vd = np.concatenate([np.zeros((2, 1), dtype=np.float32), u[:, :-1]], axis=1)
        raw = vd * m.gains[None, :]
        assert (np.abs(raw) > T).any() and not np.array_equal(raw, y)     # the clamp changed at least one sample


def test_unlimited_stretches_pass_bit_for_bit_although_the_chain_exceeds_one():
    rng = np.random.default_rng(2)
    L, H, n = 128, 64, 6 * B
    u = (rng.standard_normal((2, n)) * 0.05).astype(np.float32)
    assert np.abs(u).max() < 0.7
    u[0, 700], u[1, 2000] = 2.0, -3.0
    m = Model(2, 0.7, L, H, 0)
    y = m.process(u)
    assert m.n_acc_above_one > 0                                     # the f32 taps sum to more than 1 ...
    assert m.gains.max() == 1                                        # ... and the fminf takes it back
    clear = np.ones(n, dtype=bool)                                   # g(t) reads r(t - (L - 1) - (L + H)) .. r(t): a peak at s
    for s in (700, 2000):                                            # touches the outputs s .. s + 2 L + H - 1
        clear[s:s + 2 * L + H] = False
    delayed = np.concatenate([np.zeros((2, L), dtype=np.float32), u[:, :-L]], axis=1)
    assert np.array_equal(y[:, clear].view(np.uint32), delayed[:, clear].view(np.uint32))
    assert (m.gains[~clear] < 1).any() and np.abs(y).max() <= np.float32(0.7)


def test_any_cut_of_six_buffers_gives_the_same_bits():
    rng = np.random.default_rng(3)
    u = rng.standard_normal((2, 6 * B)).astype(np.float32)
    outs, meters = [], []
    for cuts in ([6], [1, 5], [3, 3], [1] * 6):
        m = Model(2, 0.7, 300, 500, 900)                             # 2 L + H = 1100 > 513
        m.set_gain(0.5)
        parts, mm, at = [], [], 0
        for nb in cuts:
            parts.append(m.process(u[:, at * B:(at + nb) * B]))
            mm.append(m.meters)
            at += nb
        outs.append(np.concatenate(parts, axis=1))
        meters.append(np.concatenate(mm, axis=0))
    for o, mt in zip(outs[1:], meters[1:]):
        assert np.array_equal(o.view(np.uint32), outs[0].view(np.uint32))
        assert mt.tobytes() == meters[0].tobytes()
    assert meters[0].shape == (6, 2) and meters[0].dtype.itemsize == 24


def test_gain_sets_ramp_from_the_value_in_force():
    rng = np.random.default_rng(4)
    u = (rng.standard_normal((1, 5 * B)) * 0.05).astype(np.float32)   # nothing limited: y = delayed p * u
    R, L = 700, 1
    m = Model(1, 1.0, L, 0, R)
    ys = [m.process(u[:, :B])]
    assert m.ramp_end() == m.t
    m.set_gain(0.25)
    ys.append(m.process(u[:, B:2 * B]))
    assert m.ramp_end() == B + R - 1 > m.t
    mid = float(m._p(m.t - 1))
    assert 0.25 < mid < 1.0
    m.set_gain(3.0)                                                  # inside the ramp: from the value at t_set - 1
    assert m.frm == mid and m.t_set == 2 * B
    ys.append(m.process(u[:, 2 * B:]))
    assert m.ramp_end() == m.t
    y = np.concatenate(ys, axis=1)[0]
    t = np.arange(5 * B)
    k1, k2 = t - B + 1, t - 2 * B + 1
    p = np.where(t < B, 1.0, np.where(t < 2 * B, 1.0 + (0.25 - 1.0) / R * k1, np.where(k2 >= R, 3.0, mid + (3.0 - mid) / R * k2)))
    want = p.astype(np.float32) * u[0]
    assert np.array_equal(y[L:], want[:-L])
    # R = 0: at once, at the first sample of the next step
    m = Model(1, 1.0, 1, 0, 0)
    m.process(u[:, :B])
    m.set_gain(-2.0)
    assert np.array_equal(m.process(u[:, B:2 * B])[0, 1:], (np.float32(-2.0) * u[0, B:2 * B])[:-1])
    # the reset keeps the gain, finishes the ramp and forgets the history
    m.reset()
    assert m.t == 0 and m.ramp_end() == 0
    y = m.process(u[:, :B])
    assert y[0, 0] == 0 and np.array_equal(y[0, 1:], (np.float32(-2.0) * u[0, :B])[:-1])


@pytest.mark.parametrize("L", [1, 2, 64, 128, 4096])
def test_window(L):
    w = window(L)
    assert w.dtype == np.float32 and w.shape == (L,) and (w > 0).all()
    assert np.array_equal(w, w[::-1])
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= L * 2.0 ** -24
    if L == 1:
        assert w[0] == 1


def test_where_the_chain_over_the_taps_ends_below_one_unlimited_stretches_pass_just_below_one():
    """the header's remark: L = 12 is the first look-ahead whose f32 chain over the taps ends below 1.f"""
    ends = {L: float(np.cumsum(window(L)[::-1], dtype=np.float32)[-1]) for L in range(1, 13)}
    assert [L for L, e in ends.items() if e < 1] == [12]
    u = (np.random.default_rng(12).standard_normal((1, B)) * 0.1).astype(np.float32)
    m = Model(1, 1.0, 12, 0, 0)
    y = m.process(u)
    assert m.gains.max() == np.float32(ends[12]) and 1 - ends[12] <= 2.3e-6
    assert np.array_equal(y[0, 12:], u[0, :-12] * np.float32(ends[12]))


def test_pcm16_rounds_to_nearest_even_after_one_f32_product():
    y = np.array([[0.0, 1.0, -1.0, 0.7, 0.5 / 32767, 1.5 / 32767, -0.0]], dtype=np.float32)
    p = pcm16(y)
    assert p.shape == (7, 1) and p.dtype == np.int16
    assert p[:4, 0].tolist() == [0, 32767, -32767, 22937] and p[6, 0] == 0
    # the two ties: the f32 products are exactly 0.5 and 1.5, and ties go to the even neighbour
    assert (y[0, 4:6] * np.float32(32767.0)).tolist() == [0.5, 1.5] and p[4:6, 0].tolist() == [0, 2]
    assert evaluate(np.zeros((1, 2 + 4), dtype=np.float32), 1, 0, 1.0, np.ones(1, dtype=np.float32))[0].shape == (1, 4)
