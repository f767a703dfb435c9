"""The reference of the scene filter mix (tests/cpp/scene_fir_ref.c through tests/scene_fir_model.py) held to independent
answers, without a GPU: exact integer convolution, exact rational arithmetic through a fade, an fp64 evaluation within the
provable rounding bound of the chain, and independence of how the samples are cut into steps."""
from fractions import Fraction

import numpy as np
import pytest

from tests.scene_fir_model import FadeRunning, Model, evaluate

N, K, C = 70, 37, 2                                      # 70 objects: a ragged third group of 32


def _int_case(seed):
    """integer-valued rows and taps: every partial sum is below 70 * 37 * 3 * 2 < 2^24, so every fmaf is exact"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (N, 1500)).astype(np.float32)
    h = [rng.integers(-2, 3, (C, N, K)).astype(np.float32) for _ in range(2)]
    d = [rng.integers(0, 91, N).astype(np.int32) for _ in range(2)]
    return x, h, d


def _exact(x, h, d):
    """y[c][t] = sum_o (h_co * x_o)(t - D_o) in int64"""
    n = x.shape[1]
    y = np.zeros((h.shape[0], n), dtype=np.int64)
    for c in range(h.shape[0]):
        for o in range(x.shape[0]):
            full = np.convolve(x[o].astype(np.int64), h[c, o].astype(np.int64))[:n]
            y[c, d[o]:] += full[:n - d[o]]
    return y


def test_integer_data_equals_exact_convolution():
    x, h, d = _int_case(1)
    m = Model(C, N, K, 90, 0)
    m.set(h[0], d[0])
    got = np.concatenate([m.mix(x[:, a:b]) for a, b in ((0, 513), (513, 700), (700, 1500))], axis=1)
    want = _exact(x, h[0], d[0])
    assert np.abs(want).max() > 100 and np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


def test_integer_data_through_a_fade_equals_rational_arithmetic():
    """R = 64: w = k / 64 is a dyadic fraction, the blend of two integers is exact in f32"""
    x, h, d = _int_case(2)
    R, cut = 64, 513
    m = Model(C, N, K, 90, R)
    m.set(h[0], d[0])
    first = m.mix(x[:, :cut])
    m.set(h[1], d[1])
    assert m.fade_end() == cut                           # (nothing runs before the mix that starts it)
    second = m.mix(x[:, cut:])
    y0, y1 = _exact(x, h[0], d[0]), _exact(x, h[1], d[1])
    assert np.array_equal(first, y0[:, :cut].astype(np.float32))
    for c in range(C):
        for j in range(x.shape[1] - cut):
            k = j + 1
            want = Fraction(int(y1[c, cut + j])) if k >= R else \
                Fraction(int(y0[c, cut + j])) + Fraction(k, R) * (int(y1[c, cut + j]) - int(y0[c, cut + j]))
            assert Fraction(float(second[c, j])) == want, (c, j)
    assert m.fade_end() == m.t                           # over: the step was longer than the fade


def test_set_during_a_fade_is_refused_and_replaced_sets_count_once():
    x, h, d = _int_case(3)
    m = Model(C, N, K, 90, 700)
    m.set(h[0], d[0])
    m.set(h[0], d[1])                                    # replaces the one before: no mix in between
    m.mix(x[:, :513])
    m.set(h[1])                                          # onsets unchanged
    m.mix(x[:, 513:1026])
    assert m.fade_end() == 513 + 699
    with pytest.raises(FadeRunning):
        m.set(h[0])
    m.mix(x[:, 1026:1500])
    m.set(h[0])
    assert np.array_equal(m.pending[1], d[1])


def test_random_data_within_the_chain_bound_of_fp64():
    """every fmaf rounds once: a chain of n = 32 K products is within n u sum|h x| of its exact value to first order, the sum of
    the groups adds one rounding each: (32 K + groups) 2^-24 sum|h x| per sample"""
    rng = np.random.default_rng(4)
    n_obj, taps, n = 200, 128, 300
    x = rng.standard_normal((n_obj, n)).astype(np.float32)
    h = (rng.standard_normal((C, n_obj, taps)) * np.exp(-np.arange(taps) / 30.0)).astype(np.float32)
    d = rng.integers(0, 40, n_obj).astype(np.int32)
    ts = np.arange(100, n)
    got = evaluate(x, 0, h, d, None, None, 0, 0, ts).astype(np.float64)
    want, mag = np.zeros((C, n)), np.zeros((C, n))
    for c in range(C):
        for o in range(n_obj):
            a, b = h[c, o].astype(np.float64), x[o].astype(np.float64)
            want[c, d[o]:] += np.convolve(b, a)[:n - d[o]]
            mag[c, d[o]:] += np.convolve(np.abs(b), np.abs(a))[:n - d[o]]
    bound = (32 * taps + (n_obj + 31) // 32) * 2.0 ** -24 * mag[:, ts]
    assert (np.abs(got - want[:, ts]) <= bound).all()
    assert np.abs(got - want[:, ts]).max() > 0           # (f32 after all)


def test_three_cuts_of_the_same_samples_give_the_same_bits():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, 1539)).astype(np.float32)
    h = [rng.standard_normal((C, N, K)).astype(np.float32) for _ in range(2)]
    d = [rng.integers(0, 91, N).astype(np.int32) for _ in range(2)]
    outs = []
    for cuts in ([0, 513, 1539], [0, 513, 1026, 1539], [0, 200, 513, 514, 1300, 1539]):
        m = Model(C, N, K, 90, 300)
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            if a == 0:
                m.set(h[0], d[0])
            if a == 513:
                m.set(h[1], d[1])
            parts.append(m.mix(x[:, a:b]))
        outs.append(np.concatenate(parts, axis=1))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
