"""The EQ bus's reference anchored, without a GPU: the model of tests/eq_model.py (tests/cpp/eq_ref.c inside) passes the identity
bit for bit, gives one stream however it is cut into steps, and its block form stays within 1e-8 of peak of the plain serial fp64
recurrence.  The figures this test prints are the table of DESIGN.md section 2, which decided PBSO_EQ_BLOCK."""
import numpy as np
import pytest

from tests import eq_model as em

RATE = 44100.0
# (name, kind, f0, Q, gain dB)
DESIGNS = [("high-pass 30 Hz Q 0.707", "highpass", 30.0, 0.707, 0.0),
           ("high-pass 20 Hz Q 2", "highpass", 20.0, 2.0, 0.0),
           ("high-pass 5 Hz Q 8", "highpass", 5.0, 8.0, 0.0),
           ("peak 100 Hz Q 4 +12 dB", "peak", 100.0, 4.0, 12.0),
           ("peak 1 kHz Q 2 -9 dB", "peak", 1000.0, 2.0, -9.0),
           ("high shelf 8 kHz +6 dB", "highshelf", 8000.0, 0.707, 6.0),
           ("low-pass 18 kHz", "lowpass", 18000.0, 0.707, 0.0)]


def noise(seed, rows, n):
    return np.random.default_rng(seed).standard_normal((rows, n)).astype(np.float32)


def same_bits(got, want, label):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, label
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (label, bad.size, bad[:4])


def stepped(model, x, cuts):
    out, at = [], 0
    for n in cuts:
        out.append(model.process(x[:, at:at + n]))
        at += n
    assert at == x.shape[1]
    return np.concatenate(out, axis=1)


def test_the_identity_passes_f32_input_bit_for_bit():
    x = noise(1, 3, 3 * 513)
    x[0, :5] = [1e-41, -1e-41, 3.4e38, -3.4e38, 0.0]                  # subnormals, the largest magnitudes
    m = em.Model(3, 4)
    same_bits(stepped(m, x, [513, 1026]), x, "identity")
    assert m.t == 3 * 513


def test_the_tables_of_the_identity_and_of_a_section():
    t = em.tables(em.identity(1, 1))[0, 0]
    assert t.shape == (5, em.P) and t[0, 0] == 1.0 and np.count_nonzero(t) == 1
    c = em.design("highpass", RATE, 30.0, 0.707)
    h, r, s, p, q = em.tables(c)
    assert (h[0], r[0], s[0], p[0], q[0]) == (c[0], c[1], c[2], -c[3], -c[4])
    # h is the impulse response: the serial recurrence on an impulse
    imp = np.zeros(em.P)
    imp[0] = 1.0
    assert np.array_equal(h, em.serial(c[None, :], imp))


@pytest.mark.parametrize("block", [32, 64])
def test_one_stream_however_it_is_cut(block):
    """cuts in buffers [1, 2, 1] and [4], and cuts at odd samples (inside blocks, shorter than a block, one sample)"""
    B, Cn, S = 513, 2, 3
    x = noise(2, Cn, 4 * B)
    sos = np.array([[em.design(k, RATE, f, q, g) for _, k, f, q, g in DESIGNS[c:c + S]] for c in range(Cn)])
    outs = []
    for cuts in ([B, 2 * B, B], [4 * B], [1, 62, 1, 1, 63, 200, 7, 4 * B - 335]):
        m = em.Model(Cn, S, block=block)
        m.set(sos)
        outs.append(stepped(m, x, cuts))
    same_bits(outs[1], outs[0], "[4] against [1, 2, 1]")
    same_bits(outs[2], outs[0], "sample-odd cuts against [1, 2, 1]")
    assert np.abs(outs[0]).max() > 0.1


def test_one_stream_through_fades_however_it_is_cut():
    """a first set at sample 0 (it fades from the identity) and a second at 2 * 513, R = 700: the fades cross a step edge in one
    cut and lie inside a step in another; the cuts share the two set points"""
    B, Cn, S, R = 513, 2, 2, 700
    x = noise(3, Cn, 5 * B)
    a = np.array([[em.design("highpass", RATE, 30.0, 0.707), em.design("peak", RATE, 1000.0, 2.0, -9.0)]] * Cn)
    b = np.array([[em.design("lowshelf", RATE, 200.0, 0.707, 6.0), em.design("lowpass", RATE, 18000.0, 0.707)]] * Cn)
    outs = []
    for first, second in (([B, B], [B, B, B]), ([2 * B], [3 * B]), ([100, 599, 1, 2 * B - 700], [698, 1, 1, 3 * B - 700])):
        m = em.Model(Cn, S, R)
        m.set(a)
        y0 = stepped(m, x[:, :2 * B], first)
        assert not m.fading() and m.fade_end() == m.t == 2 * B
        m.set(b)
        y1 = stepped(m, x[:, 2 * B:], second)
        outs.append(np.concatenate([y0, y1], axis=1))
    same_bits(outs[1], outs[0], "[2], [3] against [1, 1], [1, 1, 1]")
    same_bits(outs[2], outs[0], "sample cuts against buffers")
    # the first sample of a fade is From's but for w = 1 / R, and behind the fade the output is To alone
    m = em.Model(Cn, S, R)
    m.set(a)
    y = m.process(x[:, :B])
    assert m.fading() and m.fade_end() == R - 1
    assert np.abs(y[:, 0] - x[:, 0]).max() <= 2.0 * np.abs(x[:, 0]).max() / R + 1e-6


def test_the_block_form_against_the_serial_fp64_recurrence():
    """20 000 samples of seeded noise through each section alone, in both candidate block sizes; relative to the peak of the serial
    output.  The bar is 1e-8: the worst case measured without fused multiply-adds was 3e-10 (the 5 Hz high-pass of Q 8), so the bar
    leaves a factor of 30 over that and sits four orders below f32 resolution.  Measured again with them, as this test runs: 1.2e-10
    at P = 32 and 9.3e-11 at P = 64 for that section, 1.6e-11 and 3.5e-11 for the 30 and 20 Hz high-passes at P = 64, 1e-14 and
    below from 1 kHz up (DESIGN.md section 2 has the table)."""
    n = 20000
    x = np.random.default_rng(7).standard_normal(n)
    x32 = x.astype(np.float32)
    worst = {}
    for block in (32, 64):
        for name, kind, f0, q, g in DESIGNS:
            c = em.design(kind, RATE, f0, q, g)
            want = em.serial(c[None, :], x32.astype(np.float64))
            tab = em.tables(c, block)
            xx = np.concatenate([np.zeros(block + 2), x32.astype(np.float64)])
            yy = np.zeros_like(xx)
            em.block_section(tab, 0, xx, yy, block)
            err = np.abs(yy[block + 2:] - want).max() / np.abs(want).max()
            print(f"P = {block:2d}  {name:26s} max |block - serial| / peak = {err:.2e}")
            worst[(block, name)] = err
    assert max(worst.values()) < 1e-8, worst
    assert worst[(em.P, DESIGNS[4][0])] < 1e-13                        # (from 1 kHz up the two are rounding apart)
