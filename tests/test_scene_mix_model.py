"""The reference of the scene mix (tests/cpp/scene_mix_ref.c through tests/scene_mix_model.py) held to independent answers,
without a GPU: exact integer arithmetic where every operation is exact, an fp64 evaluation of the header's formula within the
derived rounding bound, the header's rules for set / reset on signals that read the parameters back, and independence of how
the samples are cut into steps."""
import numpy as np

from tests.scene_mix_model import Model

B = 513


def _exact_case(seed, n_obj, n_ch, max_delay, n):
    """integer rows |x| <= 1024, gains +-2^e (e = -2 .. 2), delays m or m + 0.5: x0 + 0.5 (x1 - x0) is a multiple of 1/2 below
    2^11, g v a multiple of 1/8 below 2^12, and 37 of them stay below 2^18 = 2^21 / 8: every f32 operation is exact"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1024, 1025, (n_obj, n)).astype(np.float32)
    g = (rng.choice([-1.0, 1.0], (n_ch, n_obj)) * 2.0 ** rng.integers(-2, 3, (n_ch, n_obj))).astype(np.float32)
    d2 = rng.integers(0, 2 * max_delay + 1, (n_ch, n_obj))           # the delay in half samples
    d2[0, :6] = [0, 2, 2 * max_delay, 2 * 600 + 1, 1, 2 * max_delay - 1]      # 0, 1, max_delay, 600.5 (> one buffer), 0.5
    return x, g, d2


def _exact_mix8(x, g, d2):
    """8 * out[c][t] in int64: sum_o (4 g) (x(i0) + x(i0 + 1)) for a half-sample delay, (4 g) 2 x(i0) for a whole one"""
    n_ch, n_obj = g.shape
    n = x.shape[1]
    xi = np.concatenate([np.zeros((n_obj, d2.max() + 2), dtype=np.int64), x.astype(np.int64)], axis=1)
    z = d2.max() + 2                                                 # xi[:, z + i] = x(i)
    out = np.zeros((n_ch, n), dtype=np.int64)
    t = np.arange(n)
    for c in range(n_ch):
        for o in range(n_obj):
            g4 = int(g[c, o] * 4)
            m, half = divmod(int(d2[c, o]), 2)
            if half:                                                 # t - m - 0.5 lies between x(t - m - 1) and x(t - m)
                out[c] += g4 * (xi[o, z + t - m - 1] + xi[o, z + t - m])
            else:
                out[c] += g4 * 2 * xi[o, z + t - m]
    return out


def test_exact_cases_equal_integer_arithmetic():
    """R = 0 over steps of 1, 2 and 1 buffers (delays reach across two steps back)"""
    n_obj, n_ch, max_delay = 37, 3, 700
    x, g, d2 = _exact_case(1, n_obj, n_ch, max_delay, 4 * B)
    m = Model(n_ch, n_obj, max_delay, 0)
    m.set(g, d2 / 2.0)
    got = np.concatenate([m.mix(x[:, a * B:b * B]) for a, b in ((0, 1), (1, 3), (3, 4))], axis=1)
    want8 = _exact_mix8(x, g, d2)
    assert np.abs(want8).max() > 8 * 1000
    assert (got.astype(np.float64) * 8 == want8).all()


def test_exact_cases_after_a_finished_ramp():
    """R = 300: the second set's ramp ends 300 samples into the second step; from there on the values are exact again"""
    n_obj, n_ch, max_delay, R = 37, 2, 700, 300
    x, g0, d0 = _exact_case(2, n_obj, n_ch, max_delay, 3 * B)
    _, g1, d1 = _exact_case(3, n_obj, n_ch, max_delay, 1)
    m = Model(n_ch, n_obj, max_delay, R)
    m.set(g0, d0 / 2.0)
    first = m.mix(x[:, :B])
    m.set(g1, d1 / 2.0)
    rest = m.mix(x[:, B:])
    assert (first.astype(np.float64) * 8 == _exact_mix8(x, g0, d0)[:, :B]).all()
    want8 = _exact_mix8(x, g1, d1)[:, B:]
    eq = rest.astype(np.float64) * 8 == want8
    assert eq[:, R - 1:].all()                                       # k = j + 1 >= R
    assert not eq[:, :R - 1].all()                                   # (and there was a ramp before)
    assert np.abs(want8).max() > 8 * 1000


class Fp64:
    """the header's formula per sample in fp64, written apart from the model: p = from + (to - from) k / R, a read at t - d
    split by floor, the object sum by numpy"""

    def __init__(self, n_ch, n_obj, max_delay, R):
        self.C, self.N, self.R, self.L = n_ch, n_obj, R, max_delay + 2
        self.frm, self.to = np.zeros((2, n_ch, n_obj)), np.zeros((2, n_ch, n_obj))
        self.t_set = np.zeros(2, dtype=np.int64)
        self.any, self.t = False, 0
        self.tail = np.zeros((n_obj, self.L))

    def at(self, kind, t):
        """[C][N][len(t)], and whether each t lies inside the ramp"""
        k = (np.asarray(t, dtype=np.int64) - self.t_set[kind] + 1).astype(np.float64)
        frm, to = self.frm[kind][..., None], self.to[kind][..., None]
        inside = k < self.R
        return np.where(inside, frm + (to - frm) * k / max(self.R, 1), to), inside

    def set(self, gain, delay=None):
        for kind, v in ((0, gain), (1, delay)):
            if v is None:
                continue
            v = np.asarray(v, dtype=np.float32).astype(np.float64)
            self.frm[kind] = self.at(kind, [self.t - 1])[0][..., 0] if self.any else v
            self.to[kind], self.t_set[kind] = v, self.t
        self.any = True

    def mix(self, rows):
        """-> out [C][n], mag [C][n] = sum_o |g| (|x0| + |x1|), inside [n] (a gain or delay ramp runs at that sample)"""
        n = rows.shape[1]
        xx = np.concatenate([self.tail, rows.astype(np.float64)], axis=1)     # xx[:, L + j] = x(t + j)
        t = np.arange(self.t, self.t + n)
        (g, ing), (d, ind) = self.at(0, t), self.at(1, t)
        out, mag = np.zeros((self.C, n)), np.zeros((self.C, n))
        for c in range(self.C):
            pos = t[None, :] - d[c]
            i0 = np.floor(pos)
            f = pos - i0
            j0 = (i0 - self.t + self.L).astype(np.int64)
            x0 = np.take_along_axis(xx, j0, 1)
            x1 = np.take_along_axis(xx, np.minimum(j0 + 1, xx.shape[1] - 1), 1)       # (past the end only with f = 0)
            out[c] = (g[c] * (x0 + f * (x1 - x0))).sum(axis=0)
            mag[c] = (np.abs(g[c]) * (np.abs(x0) + np.abs(x1))).sum(axis=0)
        self.tail = xx[:, -self.L:]
        self.t += n
        return out, mag, ing | ind


def test_random_data_within_the_derived_bound_of_fp64(capsys):
    """six roundings per term (g, f, x1 - x0, f *, x0 +, g *), at most 32 adds in a group and G adds of groups on top: to first
    order |ref - exact| <= (6 + 32 + G) u sum|g|(|x0| + |x1|) <= (40 + G) 2^-24 sum|g|(|x0| + |x1|).  Ramps of gains and delays
    cross step boundaries, the third set lands during the second's ramp."""
    n_obj, n_ch, max_delay, R = 37, 3, 1400, 700
    G = (n_obj + 31) // 32
    rng = np.random.default_rng(4)
    env = np.exp(-np.arange(4 * B) / 900.0)
    x = (rng.standard_normal((n_obj, 4 * B)) * env * rng.uniform(0.2, 1.0, (n_obj, 1))).astype(np.float32)
    ref, f64 = Model(n_ch, n_obj, max_delay, R), Fp64(n_ch, n_obj, max_delay, R)
    worst, inside, after = 0.0, 0, 0
    for k in range(4):
        if k < 3:
            g = rng.uniform(-1.5, 1.5, (n_ch, n_obj)).astype(np.float32)
            d = rng.uniform(0, max_delay, (n_ch, n_obj)).astype(np.float32)
            if k == 0:
                d[0, :5] = [0.0, 1.0, 513.25, 1400.0, 2.0 ** -30]
            ref.set(g, d)
            f64.set(g, d)
        rows = x[:, k * B:(k + 1) * B]
        got = ref.mix(rows)
        want, mag, ramping = f64.mix(rows)
        assert np.abs(got).max() > 0
        err = np.abs(got.astype(np.float64) - want)
        heard = mag > 0                                              # (the first samples of a channel with no delay below t: 0 <= 0)
        ratio = (err[heard] / mag[heard]).max() * 2.0 ** 24
        assert (err <= (40 + G) * 2.0 ** -24 * mag).all(), (k, ratio)
        worst = max(worst, ratio)
        if k > 0:
            inside += int(ramping.sum())
            after += int((~ramping).sum())
    assert inside > 0 and after > 0                                  # (the last step runs past the end of the last ramp)
    assert worst > 0                                                 # (f32 after all)
    with capsys.disabled():
        print(f"\nscene mix reference against fp64: largest |ref - fp64| = {worst:.3f} * 2^-24 * sum|g|(|x0| + |x1|)")


def _line(n_obj, a, b):
    """x_o(i) = i + 1 for every object: a unit gain and a delay d (d <= i) give back i + 1 - d, exactly"""
    return np.tile(np.arange(a + 1, b + 1, dtype=np.float32), (n_obj, 1))


def test_silence_before_the_first_set_and_no_ramp_at_the_first_set():
    m = Model(2, 3, 4, 8)
    assert not m.mix(np.ones((3, 10), dtype=np.float32)).any()
    m.set([[1, 2, 4], [0.5, 0.25, -1]])
    out = m.mix(np.ones((3, 10), dtype=np.float32))
    assert (out[0] == 7).all() and (out[1] == -0.25).all()           # at once, from the step's first sample


def test_a_set_is_replaced_before_its_step_and_a_set_during_a_ramp_starts_from_the_current_value():
    one = np.ones((1, 4), dtype=np.float32)
    m = Model(1, 1, 0, 8)
    m.set([[0.0]])
    m.mix(one)
    m.set([[100.0]])                                                 # replaced: never heard
    m.set([[8.0]])
    assert m.mix(one)[0].tolist() == [1, 2, 3, 4]                    # 0 + 8 k / 8, k = 1 ..
    m.set([[0.0]])                                                   # during the ramp: from p(t_set - 1) = 4
    assert m.p[0, 0, 0]["from"] == 4 and m.p[0, 0, 0]["t_set"] == 8 and m.p[0, 0, 0]["slope"] == -0.5
    assert np.concatenate([m.mix(one), m.mix(one), m.mix(one)])[:, 0].tolist() == [3.5, 1.5, 0]
    assert m.mix(one)[0].tolist() == [0, 0, 0, 0]
    # a ramp of R samples ends at its last sample: k = R gives p_to itself, not from + slope * R
    r = Model(1, 1, 0, 3)
    r.set([[1.0]])
    r.mix(one)
    r.set([[2.0]])
    got = r.mix(one)[0]
    assert got.tolist() == [np.float32(1 + 1 / 3.0), np.float32(1 + (1 / 3.0) * 2), 2, 2]


def test_delay_ramps_and_gains_only_sets():
    """on x(i) = i + 1 the output reads the delay back: out = t + 1 - d(t)"""
    m = Model(1, 2, 8, 4)
    m.set([[1, 1]], [[0, 8]])
    a = m.mix(_line(2, 0, 16))
    assert a[0, 8:].tolist() == [(t + 1) + (t + 1 - 8) for t in range(8, 16)]
    assert a[0, :8].tolist() == [t + 1 for t in range(8)]            # before sample 0 the second object is silent
    m.set([[1, 1]], [[2, 4]])                                        # d(t) = 0 + 2 k / 4 and 8 - 4 k / 4
    b = m.mix(_line(2, 16, 24))
    want_d = [(0.5, 7), (1, 6), (1.5, 5), (2, 4), (2, 4), (2, 4), (2, 4), (2, 4)]
    assert b[0].tolist() == [(t + 1 - d0) + (t + 1 - d1) for t, (d0, d1) in zip(range(16, 24), want_d)]
    before = m.p[:, :, 1].copy()
    m.set([[2, 0]])                                                  # gains only: the delay records stay as they are
    assert (m.p[:, :, 1] == before).all() and m.p[0, 0, 0]["t_set"] == 24 and m.p[0, 0, 1]["t_set"] == 16
    c = m.mix(_line(2, 24, 32))
    want_g = [(1.25, 0.75), (1.5, 0.5), (1.75, 0.25), (2, 0), (2, 0), (2, 0), (2, 0), (2, 0)]
    assert c[0].tolist() == [g0 * (t + 1 - 2) + g1 * (t + 1 - 4) for t, (g0, g1) in zip(range(24, 32), want_g)]


def test_reset_keeps_the_targets_clears_the_history_and_the_next_set_does_not_ramp():
    m = Model(1, 1, 4, 6)
    m.set([[1]], [[0]])
    m.mix(_line(1, 0, 8))
    m.set([[3]], [[4]])
    m.mix(_line(1, 8, 10))                                           # two samples into the ramp
    m.reset()
    assert m.t == 0 and not m.tail.any()
    q = m.p[0, 0]
    assert q["from"].tolist() == [3, 4] and q["to"].tolist() == [3, 4] and not q["t_set"].any() and not q["slope"].any()
    a = m.mix(_line(1, 0, 8))                                        # the values kept, ramps finished, silence before sample 0
    assert a[0].tolist() == [0, 0, 0, 0, 3, 6, 9, 12]
    m.set([[1]], [[1]])
    assert m.mix(_line(1, 8, 12))[0].tolist() == [8, 9, 10, 11]      # at once


def test_three_cuts_of_the_same_samples_give_the_same_bits():
    """after a common first buffer and a second set: 1 + 2 + 3 buffers against one step of 6 (a ramp of 700 samples crosses
    the first cut; a step that ends inside the ramp in one run lies in the middle of a step in the other)"""
    n_obj, n_ch, max_delay, R = 37, 3, 900, 700
    rng = np.random.default_rng(6)
    x = rng.standard_normal((n_obj, 7 * B)).astype(np.float32)
    sets = [(rng.uniform(-1, 1, (n_ch, n_obj)), rng.uniform(0, max_delay, (n_ch, n_obj))) for _ in range(2)]
    outs = []
    for cuts in ([1, 2, 3], [6]):
        m = Model(n_ch, n_obj, max_delay, R)
        m.set(*sets[0])
        parts, a = [m.mix(x[:, :B])], 1
        m.set(*sets[1])
        for nb in cuts:
            parts.append(m.mix(x[:, a * B:(a + nb) * B]))
            a += nb
        outs.append(np.concatenate(parts, axis=1))
    assert np.abs(outs[0]).max() > 0 and outs[0].shape == (n_ch, 7 * B)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
