"""The reference of the scene filter mix's delay stage (tests/cpp/scene_fir_delay_ref.c through tests/scene_fir_delay_model.py)
held to independent answers, without a GPU: exact shifts for integer delays, an fp64 evaluation of the same formula within the
rounding bound of the read, the rule of a set during a ramp, and independence of how the samples are cut into steps."""
import numpy as np

from tests.scene_fir_delay_model import DelayLine, Model, ramp_value

N = 37


def _rows(seed, n):
    return np.random.default_rng(seed).standard_normal((N, n)).astype(np.float32)


def _run(line, x, cuts, sets):
    """z of x cut at `cuts`; sets = {sample: delays}, each given before the step that starts there"""
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a in sets:
            line.set(sets[a])
        out.append(line.step(x[:, a:b]))
    return np.concatenate(out, axis=1)


def test_delay_zero_is_the_signal_itself():
    x = _rows(1, 1400)
    never = _run(DelayLine(N, 300, 200), x, [0, 513, 700, 1400], {})
    zeros = _run(DelayLine(N, 300, 200), x, [0, 513, 700, 1400], {0: np.zeros(N), 513: np.zeros(N)})
    assert np.array_equal(never.view(np.uint32), x.view(np.uint32)) and np.array_equal(zeros.view(np.uint32), x.view(np.uint32))


def test_integer_delays_shift_exactly():
    x = _rows(2, 1600)
    d = np.random.default_rng(2).integers(0, 601, N)
    d[:3] = [0, 600, 513]
    z = _run(DelayLine(N, 600, 0), x, [0, 513, 1026, 1600], {0: d})
    for o in range(N):
        want = np.concatenate([np.zeros(d[o], dtype=np.float32), x[o, :x.shape[1] - d[o]]])
        assert np.array_equal(z[o].view(np.uint32), want.view(np.uint32)), o


def _fp64(x, recs, R, n):
    """z in fp64 from the records [(t_set, PARAM array)] in force from t_set on: the header's formula, evaluated independently"""
    xx = np.concatenate([np.zeros((N, 2048)), x.astype(np.float64)], axis=1)
    z = np.empty((N, n))
    for k, (t_set, p) in enumerate(recs):
        end = recs[k + 1][0] if k + 1 < len(recs) else n
        for t in range(t_set, end):
            d = ramp_value(p, np.int64(t), R)
            pos = t - d                                              # the read position, fractional
            i0 = np.floor(pos).astype(np.int64)
            f = pos - i0
            o = np.arange(N)
            z[:, t] = xx[o, 2048 + i0] + f * (xx[o, 2048 + i0 + 1] - xx[o, 2048 + i0])
    return z


def test_fractional_and_ramped_delays_against_fp64():
    """three f32 roundings on magnitudes up to 2 max|x| and the rounding of f: within 8 * 2^-24 max|x|, stated as 1e-6 max|x|"""
    R, n = 600, 2100
    x = _rows(3, n)
    rng = np.random.default_rng(3)
    sets = {0: rng.uniform(0, 900, N), 513: rng.uniform(0, 900, N), 1026: rng.uniform(0, 900, N)}
    sets[513][:2] = [0.0, 900.0]
    line = DelayLine(N, 900, R)
    recs, out = [], []
    for a, b in ((0, 513), (513, 1026), (1026, 2100)):
        line.set(sets[a])
        out.append(line.step(x[:, a:b]))
        recs.append((a, line.p.copy()))
    z = np.concatenate(out, axis=1)
    err = np.abs(z.astype(np.float64) - _fp64(x, recs, R, n)).max()
    print("max |z - fp64| / max|x| =", err / np.abs(x).max())
    assert 0 < err <= 1e-6 * np.abs(x).max()


def test_a_set_during_a_ramp_starts_from_the_old_records_value():
    R = 600
    line = DelayLine(N, 900, R)
    rng = np.random.default_rng(4)
    a, b, c = (rng.uniform(0, 900, N).astype(np.float32) for _ in range(3))
    x = _rows(4, 1300)
    line.set(a)
    line.step(x[:, :513])
    assert (line.p["from"] == a).all() and (line.p["slope"] == 0).all() and line.ramp_end() == 513      # the first set: no ramp
    line.set(b)
    line.step(x[:, 513:713])
    old = line.p.copy()
    assert line.ramp_end() == 513 + R - 1 and (old["from"] == a).all() and (old["to"] == b).all()
    line.set(c)                                                      # 200 samples into the ramp of 600
    line.set(c)                                                      # (replaces itself: no step in between)
    line.step(x[:, 713:1300])
    want = old["from"] + old["slope"] * 200.0                        # p(t_set - 1), k = 712 - 513 + 1 = 200
    assert np.array_equal(line.p["from"], want) and (line.p["t_set"] == 713).all()
    assert np.array_equal(line.p["slope"], (c.astype(np.float64) - want) / 600.0)
    assert line.n_sets == 4 and line.ramp_end() == 713 + R - 1
    line.reset()
    assert (line.p["from"] == c).all() and (line.p["to"] == c).all() and line.t == 0 and line.ramp_end() == 0


def test_any_cut_gives_the_same_bits():
    R, n = 700, 2052
    x = _rows(5, n)
    rng = np.random.default_rng(5)
    sets = {0: rng.uniform(0, 500, N), 513: rng.uniform(0, 500, N), 1026: rng.uniform(0, 500, N)}
    outs = [_run(DelayLine(N, 500, R), x, cuts, sets) for cuts in
            ([0, 513, 1026, n], [0, 100, 513, 514, 1026, 1500, 1539, n], [0, 512, 513, 1025, 1026, 1027, n])]
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))


def test_the_filter_model_behind_the_line_sees_z():
    """one-hot taps: channel c of the whole model is z shifted by onset + k_c"""
    K, D = 8, 40
    x = _rows(6, 1200)
    d = np.random.default_rng(6).uniform(0, 300, N)
    h = np.zeros((2, N, K), dtype=np.float32)
    h[0, :, 0] = h[1, :, 5] = 1.0
    m = Model(2, N, K, 64, 0, 300, 100)
    m.set(h, np.full(N, D))
    m.set_delay(d)
    line = DelayLine(N, 300, 100)
    line.set(d)
    y = np.concatenate([m.mix(x[:, a:b]) for a, b in ((0, 513), (513, 1200))], axis=1)
    z = np.concatenate([line.step(x[:, a:b]) for a, b in ((0, 513), (513, 1200))], axis=1)
    for c, k in ((0, 0), (1, 5)):
        zs = np.concatenate([np.zeros((N, D + k), dtype=np.float32), z[:, :1200 - D - k]], axis=1)
        want = np.zeros(1200, dtype=np.float32)
        for g in range(0, N, 32):
            acc = np.zeros(1200, dtype=np.float32)
            for o in range(g, min(g + 32, N)):
                acc = acc + zs[o]
            want = want + acc
        assert np.array_equal(y[c].view(np.uint32), want.view(np.uint32)), c
