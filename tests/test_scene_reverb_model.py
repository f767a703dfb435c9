"""The reference of the scene reverb (tests/cpp/scene_reverb_ref.c through tests/scene_reverb_model.py) held to independent
answers, without a GPU: a brute-force double loop in pure Python on tiny shapes, float64 convolution within the provable rounding
bound of the chains, and independence of how the samples are cut into steps."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests.scene_reverb_model import SEGMENT, FadeRunning, Model, evaluate


def f32(x):
    return float(np.float32(x))


def fmaf(a, b, c):
    """a * b + c rounded ONCE to f32 (nearest, ties to even, subnormals included): the sum is taken exactly, as a rational.  An
    exact zero is +0: the accumulators here start at +0.f and never become -0"""
    v = Fraction(a) * Fraction(b) + Fraction(c)
    if v == 0:
        return 0.0
    e = abs(v.numerator).bit_length() - v.denominator.bit_length()   # 2^(e-1) <= |v| < 2^(e+1)
    if Fraction(2) ** e > abs(v):
        e -= 1
    ulp = max(e, -126) - 23
    return math.ldexp(round(v / Fraction(2) ** ulp), ulp)            # (round() of a Fraction rounds halves to even)


def brute(u, base, r, t_set, R, r_from, ts, add=None):
    """the header's four lines, literally, in Python"""
    n_out, n_in, K = r.shape
    L = u.shape[1]

    def at(i, t):
        return float(u[i, t - base]) if 0 <= t - base < L else 0.0

    def Y(rr, c, t):
        y = 0.0
        for i in range(n_in):
            for j in range((K + SEGMENT - 1) // SEGMENT):
                acc = 0.0
                for k in range(min(K, (j + 1) * SEGMENT) - 1, j * SEGMENT - 1, -1):
                    acc = fmaf(float(rr[c, i, k]), at(i, t - k), acc)
                y = f32(y + acc)
        return y

    out = np.zeros((n_out, len(ts)), dtype=np.float32)
    for c in range(n_out):
        for n, t in enumerate(ts):
            y = Y(r, c, t)
            if r_from is not None and t - t_set + 1 < R:
                yf = Y(r_from, c, t)
                w = f32((t - t_set + 1) / R)
                y = f32(yf + f32(w * f32(y - yf)))
            if add is not None:
                y = f32(float(add[c, n]) + y)
            out[c, n] = y
    return out


def test_python_fmaf_rounds_once():
    assert fmaf(1.0, 1.0, 0.0) == 1.0
    a = f32(1 + 2.0 ** -23)
    assert fmaf(a, a, -1.0) == f32(2.0 ** -22 + 2.0 ** -46)          # the product's low bits survive: no intermediate rounding
    assert fmaf(f32(1e-30), f32(1e-10), 0.0) == f32(f32(1e-30) * np.float64(f32(1e-10)))   # a subnormal result
    assert fmaf(3.0, 5.0, 7.0) == 22.0


@pytest.mark.parametrize("n_in,n_out,K,R", [(1, 1, 1, 0), (2, 2, 5, 7), (1, 2, 6, 4)])
def test_reference_equals_the_brute_force_double_loop(n_in, n_out, K, R):
    rng = np.random.default_rng(K)
    u = rng.standard_normal((n_in, 40)).astype(np.float32)
    r = [rng.standard_normal((n_out, n_in, K)).astype(np.float32) for _ in range(2)]
    add = rng.standard_normal((n_out, 12)).astype(np.float32)
    ts = np.arange(18, 30)                                           # from t_set on: inside the fade and behind it
    for frm, a in ((None, None), (r[1], None), (r[1], add)):
        got = evaluate(u, 0, r[0], frm, 18, R, ts, a)
        want = brute(u, 0, r[0], 18, R, frm, ts, a)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (frm is None, a is None)


def test_reference_crosses_a_segment_border_as_the_double_loop_does():
    """K = SEGMENT + 3: two chains per input, added in (i, j) order -- at three output samples (the loop is pure Python)"""
    rng = np.random.default_rng(9)
    K = SEGMENT + 3
    u = rng.standard_normal((2, K + 4)).astype(np.float32)
    r = rng.standard_normal((1, 2, K)).astype(np.float32)
    ts = np.array([5, K - 1, K + 3])
    got = evaluate(u, 0, r, None, 0, 0, ts)
    assert np.array_equal(got.view(np.uint32), brute(u, 0, r, 0, 0, None, ts).view(np.uint32))


def _conv64(r, u, L):
    """(r * u)[0 .. L) in float64 through the FFT (np.convolve for short r)"""
    if r.size <= 64:
        return np.convolve(u, r)[:L]
    n = 1 << int(np.ceil(np.log2(L + r.size)))
    return np.fft.irfft(np.fft.rfft(r, n) * np.fft.rfft(u, n), n)[:L]


@pytest.mark.parametrize("n_in,n_out,K", [(1, 2, 65536), (2, 2, 4101), (1, 1, 131072), (3, 8, 2049)])
def test_random_data_within_the_chain_bound_of_fp64(n_in, n_out, K):
    """a chain of at most S fmaf is within S u sum|r u| of its exact value to first order, every one of the n_in J adds behind it
    rounds once more: (S + n_in J) 2^-24 1.001 sum_i |r_ci| * |u_i| per sample"""
    rng = np.random.default_rng(K + n_in)
    L = K + 3000
    u = rng.standard_normal((n_in, L)).astype(np.float32)
    r = (rng.standard_normal((n_out, n_in, K)) * np.exp(-np.arange(K) / (K / 6.0))).astype(np.float32)
    ts = np.sort(rng.choice(np.arange(K // 2, L), 1500, replace=False))
    got = evaluate(u, 0, r, None, 0, 0, ts).astype(np.float64)
    J = (K + SEGMENT - 1) // SEGMENT
    worst = 0.0
    for c in range(n_out):
        want, mag = np.zeros(L), np.zeros(L)
        for i in range(n_in):
            a, b = r[c, i].astype(np.float64), u[i].astype(np.float64)
            want += _conv64(a, b, L)
            mag += _conv64(np.abs(a), np.abs(b), L)
        bound = (SEGMENT + n_in * J) * 2.0 ** -24 * 1.001 * mag[ts]
        err = np.abs(got[c] - want[ts])
        assert (err <= bound).all(), (c, (err / bound).max())
        worst = max(worst, err.max())
    assert worst > 0                                                 # (f32 after all)


def test_three_cuts_of_the_same_samples_give_the_same_bits():
    rng = np.random.default_rng(5)
    n_in, n_out, K, R = 2, 2, 2100, 300
    x = rng.standard_normal((n_in, 1539)).astype(np.float32)
    add = rng.standard_normal((n_out, 1539)).astype(np.float32)
    r = [rng.standard_normal((n_out, n_in, K)).astype(np.float32) for _ in range(2)]
    outs = []
    for cuts in ([0, 513, 1539], [0, 513, 1026, 1539], [0, 200, 513, 514, 1300, 1539]):
        m = Model(n_in, n_out, K, R)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a == 0:
                m.set(r[0])
            if a == 513:
                m.set(r[1])
            parts.append(m.process(x[:, a:b], add[:, a:b]))
        outs.append(np.concatenate(parts, axis=1))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    # and the whole is what one evaluation of all samples gives: set 0 from t = 0, set 1 from t = 513 through a fade of R
    whole = np.concatenate([evaluate(x, 0, r[0], None, 0, R, np.arange(513), add[:, :513]),
                            evaluate(x, 0, r[1], r[0], 513, R, np.arange(513, 1539), add[:, 513:])], axis=1)
    assert np.array_equal(outs[0].view(np.uint32), whole.view(np.uint32))


def test_silence_before_the_first_set_a_replaced_set_and_a_refused_one():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((1, 1500)).astype(np.float32)
    add = rng.standard_normal((2, 500)).astype(np.float32)
    r = [rng.standard_normal((2, 1, 9)).astype(np.float32) for _ in range(3)]
    m = Model(1, 2, 9, 700)
    assert not m.process(x[:, :100]).any()                           # nothing set: silence ...
    assert np.array_equal(m.process(x[:, 100:600], add), add)        # ... or add alone
    m.set(r[0])
    m.set(r[1])                                                      # replaces the one before: no step in between
    got = m.process(x[:, 600:700])
    assert m.fade_end() == m.t == 700                                # the first set: no fade
    assert np.array_equal(got, evaluate(x, 0, r[1], None, 600, 700, np.arange(600, 700)))
    m.set(r[2])
    m.process(x[:, 700:900])
    assert m.fade_end() == 700 + 699
    with pytest.raises(FadeRunning):
        m.set(r[0])
    m.process(x[:, 900:1500])
    m.set(r[0])
