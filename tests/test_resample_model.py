"""The reference of the resampler bus (tests/resample_model.py around tests/cpp/resample_ref.c) anchored, without a GPU, against an
independent fp64 numpy evaluation of the same taps:

- every f32 output is within (T + 1) 2^-24 sum_k |h[phi][k]| max|u| of the fp64 one, the standard bound of an f32 fmaf chain of
  T terms (gamma_T = T u / (1 - T u) with u = 2^-24, below (T + 1) u for T <= 256) plus nothing: the taps are the same f32 numbers
  in both;
- the model cut into steps equals the model in one piece, bit for bit;
- a 1 kHz sine from 44100 to 48000 stays within e64 plus that bound of the analytic sine delayed by (N - 1) / (2 L) input samples,
  e64 being the fp64 evaluation's own distance from the analytic sine, measured here (1.9e-5 at T = 32, beta 9, cutoff 0.9; a
  Kaiser window of beta 9 has about 90 dB, 3e-5, of ripple, and the test asks for e64 below 1e-4)."""
import numpy as np
import pytest

from tests import resample_model as rm

U24 = 2.0 ** -24
RATIOS = [(44100, 48000), (44100, 96000), (44100, 22050), (48000, 44100), (44100, 44100), (3, 2)]
# what tests/test_gpu_resample_windows.py leans on the reference for, (rates, taps, input samples): 2 / 95, 85 / 4079 and 84 / 4031 on
# both sides of the kernel's window limit, 30000 samples of them (about 630 outputs; 1500 samples would give 32), and 8 / 7 and 1 / 7
WINDOW_CASES = [((45600, 960), (172, 175, 176, 177), 30000), ((44869, 935), (50, 51, 52), 30000), ((44341, 924), (51, 52), 30000),
                ((44100, 50400), (4, 7), 1500), ((44100, 6300), (4, 7), 1500)]


def _signal(C, n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (C, n)).astype(np.float32)


def _cases(taps):
    """(rates, T, n): RATIOS x taps at 1500 samples, under the ids that two stacked parametrisations gave them, then WINDOW_CASES"""
    old = [pytest.param(r, T, 1500, id=f"{T}-rates{i}") for T in taps for i, r in enumerate(RATIOS)]
    return old + [pytest.param(r, T, n, id=f"{T}-{r[0]}to{r[1]}") for r, ts, n in WINDOW_CASES for T in ts]


@pytest.mark.parametrize("rates,T,n", _cases([1, 2, 7, 32, 256]))
def test_f32_chain_within_its_bound_of_the_fp64_evaluation(rates, T, n):
    L, M = rm.ratio(*rates)
    h = rm.design(L, M, T)
    u = _signal(2, n, 7 * T + L)
    y = rm.Model(2, L, M, h).process(u)
    y64, bound = rm.evaluate64(u, L, M, h)
    assert y.shape == y64.shape == (2, rm.ceil_div(n * L, M))
    err = np.abs(y.astype(np.float64) - y64)
    assert (err <= (T + 1) * U24 * bound).all(), (err / bound).max() / U24
    assert np.abs(y).max() > 1e-4                        # (not silence; the window of a one- or two-tap table is nearly shut)


@pytest.mark.parametrize("rates,T,n", _cases([1, 7, 32, 256]))
def test_cut_into_steps_equals_one_piece_bit_for_bit(rates, T, n):
    L, M = rm.ratio(*rates)
    h = rm.design(L, M, T)
    cuts = [1, 1, 3, 513, 2, 27, 1026, 5, 40]            # steps shorter than the history among them
    if n > 1500:
        cuts = cuts + [12312, 27, 1, 513, 15503, 26]     # at 47 : 1, two steps of more than 256 outputs among steps of 0 or 1
    n = sum(cuts)
    u = _signal(3, n, T + M)
    whole = rm.Model(3, L, M, h).process(u)
    m = rm.Model(3, L, M, h)
    parts, at = [], 0
    for c in cuts:
        want = m.n_out(c)
        parts.append(m.process(u[:, at:at + c]))
        assert parts[-1].shape[1] == want <= rm.ceil_div(c * L, M)
        at += c
    got = np.concatenate(parts, axis=1)
    assert got.shape == whole.shape and np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    assert (m.t, m.m) == (n, rm.ceil_div(n * L, M))


def test_counts_of_the_header():
    m = rm.Model(1, 160, 147, rm.design(160, 147, 4))
    assert m.n_out(513) == 559
    m.process(np.zeros((1, 513), dtype=np.float32))
    assert m.n_out(513) == 558 and m.p0 == 559 * 147 - 513 * 160


def test_one_khz_sine_to_48000_is_the_delayed_sine():
    L, M = rm.ratio(44100, 48000)
    T, f, n = 32, 1000.0, 8 * 513
    h = rm.design(L, M, T)
    t = np.arange(n, dtype=np.float64)
    u = np.sin(2.0 * np.pi * f * t / 44100.0).astype(np.float32)[None, :]
    y = rm.Model(1, L, M, h).process(u)[0].astype(np.float64)
    y64, bound = rm.evaluate64(u, L, M, h)
    delay = (L * T - 1) / (2.0 * L)                      # input samples
    m = np.arange(y.size, dtype=np.float64)
    want = np.sin(2.0 * np.pi * f * (m * M / L - delay) / 44100.0)
    settled = np.arange(y.size) * M // L >= T            # every tap reads a sample of the sine, none the silence before it
    # the fp64 evaluation reads the f32-rounded sine; that rounding, at most 2^-25 per sample through taps of sum |h| = bound, is part of e64
    e64 = np.abs(y64[0] - want)[settled].max()
    print(f"e64 = {e64:.3e}")
    assert e64 < 1e-4
    err = np.abs(y - want)[settled]
    assert (err <= e64 + (T + 1) * U24 * bound[0][settled]).all(), err.max()
    assert settled.sum() > 4000


def test_design_is_linear_phase_and_passes_dc():
    for (L, M, T) in ((160, 147, 32), (147, 160, 32), (1, 2, 7), (1, 1, 1)):
        g = rm.prototype(L, M, T)
        assert np.array_equal(g, g[::-1]) or np.abs(g - g[::-1]).max() < 1e-15
        h = rm.design(L, M, T, dtype=np.float64)
        if T >= 32:
            assert np.abs(h.sum(axis=1) - 1.0).max() < 1e-3
    assert rm.design(1, 1, 1)[0, 0] == np.float32(0.9)


def test_pcm_saturates():
    y = np.array([[0.0, 1.0, -1.0, 1.5, -7.0, 0.25, -0.5, 1e-40]], dtype=np.float32)
    want = np.array([0, 32767, -32767, 32767, -32767, 8192, -16384, 0], dtype=np.int16)      # 8191.75 -> 8192, -16383.5 -> -16384 (even)
    assert np.array_equal(rm.pcm16(y)[:, 0], want)
