"""The reference of the filter bank's tests (tests/cpp/scene_fir_bank_ref.c through tests/scene_fir_bank_model.py), checked
without a GPU: one pair with weight 1.f is the bank's filter itself, a padded (0, 0.f) pair changes nothing, and every chain equals
exact rational arithmetic rounded to f32 once per step."""
from fractions import Fraction

import numpy as np

from tests.scene_fir_bank_model import taps_from_bank


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def round_f32(x):
    """the f32 nearest to the Fraction x, ties to even: the nearest f64 first, then the choice among that value's f32
    neighbours made in exact arithmetic (the f64 on the way decides nothing)"""
    c = np.float32(float(x))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    cands = [v for v in cands if np.isfinite(v)]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - x), int(np.float32(v).view(np.uint32)) & 1))


def test_one_pair_of_weight_one_is_the_banks_filter():
    rng = np.random.default_rng(1)
    F, C, K, N = 5, 3, 17, 9
    bank = rng.standard_normal((F, C, K)).astype(np.float32)
    bank[2, 1, 3] = np.float32(1e-42)                                 # a subnormal tap comes through
    index = rng.integers(0, F, (N, 1)).astype(np.int32)
    index[:2, 0] = [0, F - 1]
    taps = taps_from_bank(bank, index, np.ones((N, 1), dtype=np.float32))
    want = np.ascontiguousarray(bank[index[:, 0]].transpose(1, 0, 2))  # [C][N][K]
    assert np.array_equal(_bits(taps), _bits(want))


def test_a_padded_pair_changes_nothing():
    rng = np.random.default_rng(2)
    F, C, K, N, J = 7, 2, 33, 11, 3
    bank = rng.standard_normal((F, C, K)).astype(np.float32)
    index = rng.integers(0, F, (N, J)).astype(np.int32)
    weight = rng.standard_normal((N, J)).astype(np.float32)
    weight[0] = [0.0, -1.5, 1.0]
    index[1] = [4, 4, 4]                                              # a repeated index
    taps = taps_from_bank(bank, index, weight)
    for pad in (1, 5):
        ip = np.concatenate([index, np.zeros((N, pad), dtype=np.int32)], axis=1)
        wp = np.concatenate([weight, np.zeros((N, pad), dtype=np.float32)], axis=1)
        assert np.array_equal(_bits(taps_from_bank(bank, ip, wp)), _bits(taps)), pad


def test_chains_equal_exact_rational_arithmetic_rounded_once_per_step():
    """2000 chains of J = 1 .. 8 steps: full mantissas, cancelling pairs, weights 0, 1 and negative, and products small enough
    to land among the subnormals"""
    rng = np.random.default_rng(3)
    n = 2000
    J = rng.integers(1, 9, n)
    scale = np.where(np.arange(n) % 10 == 0, 1e-20, 1.0)
    w = (rng.standard_normal((n, 8)) * scale[:, None]).astype(np.float32)
    b = (rng.standard_normal((n, 8)) * scale[:, None]).astype(np.float32)
    w[::7, 0], w[::11, 1], w[::13, 2] = 1.0, 0.0, -1.0
    b[::5, 1], w[::5, 1] = b[::5, 0], -w[::5, 0]                       # exact cancellation in step 2
    for i in range(n):
        # one object, one channel, one tap: bank filter j holds b[i][j]
        got = taps_from_bank(b[i, :J[i]].reshape(J[i], 1, 1), np.arange(J[i], dtype=np.int32).reshape(1, J[i]), w[i, :J[i]].reshape(1, J[i]))
        acc = Fraction(0)
        for j in range(J[i]):
            acc = Fraction(float(round_f32(Fraction(float(w[i, j])) * Fraction(float(b[i, j])) + acc)))
        want = np.float32(float(acc))
        assert got.shape == (1, 1, 1)
        if want == 0 and got[0, 0, 0] == 0:                           # (a Fraction has no signed zero: the value is the claim)
            continue
        assert _bits(got)[0, 0, 0] == _bits(want), (i, J[i], got[0, 0, 0], want)


def test_round_f32_itself_on_a_double_rounding_case():
    """1 + 2^-24 + 2^-60 lies just above the tie between 1 and 1 + 2^-23: the nearest f64 is the tie, which rounds to even"""
    x = Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)
    assert np.float32(float(x)) == np.float32(1.0)
    assert round_f32(x) == np.nextafter(np.float32(1.0), np.float32(2.0))
