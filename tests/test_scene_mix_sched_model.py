"""The reference of the scene mix's schedule (tests/scene_mix_sched_model.py) anchored on the reference of the scene mix itself,
without a GPU: a schedule mixed in one piece equals, bit for bit, tests/scene_mix_model.Model fed the same rows cut exactly at
every t_set, with a plain set before each piece -- the header's statement of what a scheduled set is."""
import numpy as np
import pytest

from tests.scene_mix_model import Model
from tests.scene_mix_sched_model import SchedModel

B = 513


def _scene(seed, n_obj, n_ch, max_delay, n, n_sets):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n_obj, n)) * np.exp(-np.arange(n) / 1500.0)).astype(np.float32)
    g = rng.uniform(-1.5, 1.5, (n_sets, n_ch, n_obj)).astype(np.float32)
    d = rng.uniform(0, max_delay, (n_sets, n_ch, n_obj)).astype(np.float32)
    return x, g, d


def _cut_run(x, n_ch, max_delay, R, sets):
    """Model alone: the rows cut at every t_set, a plain set before each piece (sets: (t, gain, delay or None), ascending)"""
    m = Model(n_ch, x.shape[0], max_delay, R)
    edges = sorted({0, x.shape[1]} | {t for t, _, _ in sets})
    parts = []
    for a, b in zip(edges[:-1], edges[1:]):
        for t, g, d in sets:
            if t == a:
                m.set(g, d)
        parts.append(m.mix(x[:, a:b]))
    return np.concatenate(parts, axis=1), m


@pytest.mark.parametrize("R", [0, 1, 7, 513, 2000])
def test_a_schedule_in_one_piece_equals_plain_sets_between_cut_rows(R):
    """sets on and off the buffer grid: at sample 0, one sample in, around a multiple of 64, three samples apart, at a buffer's
    first and last sample, at the run's last sample; two of them of gains only, one of those during a delay ramp (R = 2000: every
    set lands during the ramp before it)"""
    n_obj, n_ch, max_delay, n = 5, 2, 700, 4 * B
    times = [0, 1, 63, 64, 65, 300, 303, B - 1, B, B + 17, 2 * B + 17, 3 * B, n - 1]
    x, g, d = _scene(10 + R, n_obj, n_ch, max_delay, n, len(times))
    sets = [(t, g[k], None if k in (5, 9) else d[k]) for k, t in enumerate(times)]
    want, cut = _cut_run(x, n_ch, max_delay, R, sets)
    m = SchedModel(n_ch, n_obj, max_delay, R)
    for t, gg, dd in sets:
        m.set_at(t, gg, dd)
    got = m.mix(x)
    assert np.abs(want).max() > 0
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not m.pending and m.t == n
    assert m.p.tobytes() == cut.p.tobytes()                          # and it leaves the records the cut run leaves


@pytest.mark.parametrize("R", [0, 7, 2000])
def test_sets_that_wait_for_a_later_step_and_any_cut_of_the_steps(R):
    """the same schedule given up front and stepped as 1 + 2 + 1 buffers, as 4 x 1 and as one piece: a set waits for the step that
    contains it, one lies exactly at a later step's first sample, and the cut changes no bit"""
    n_obj, n_ch, max_delay, n = 4, 3, 600, 4 * B
    times = [17, B + 5, 2 * B, 3 * B + 100]
    x, g, d = _scene(50 + R, n_obj, n_ch, max_delay, n, len(times))
    sets = [(t, g[k], d[k]) for k, t in enumerate(times)]
    want, _ = _cut_run(x, n_ch, max_delay, R, sets)
    for cuts in ([1, 2, 1], [1, 1, 1, 1], [4]):
        m = SchedModel(n_ch, n_obj, max_delay, R)
        m.schedule(times, g, d)
        parts, a = [], 0
        for nb in cuts:
            parts.append(m.mix(x[:, a * B:(a + nb) * B]))
            a += nb
        got = np.concatenate(parts, axis=1)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), cuts


def test_a_plain_set_after_a_drained_schedule_and_picked_samples():
    """a plain set continues mid-ramp from what the schedule left; samples picked from a step are the samples of the whole step"""
    n_obj, n_ch, max_delay, R, n = 3, 2, 300, 900, 3 * B
    x, g, d = _scene(77, n_obj, n_ch, max_delay, n, 3)
    sets = [(0, g[0], d[0]), (B + 200, g[1], d[1]), (2 * B, g[2], d[2])]
    want, _ = _cut_run(x, n_ch, max_delay, R, sets)
    m = SchedModel(n_ch, n_obj, max_delay, R)
    m.set_at(0, g[0], d[0])
    m.set_at(B + 200, g[1], d[1])
    pick = np.array([0, 5, B + 199, B + 200, B + 201, 2 * B - 1])
    first = m.mix(x[:, :2 * B], pick)
    m.set(g[2], d[2])                                                # 313 samples into the ramp of the set at B + 200
    last = m.mix(x[:, 2 * B:])
    assert np.array_equal(first.view(np.uint32), want[:, pick].view(np.uint32))
    assert np.array_equal(last.view(np.uint32), want[:, 2 * B:].view(np.uint32))


def test_reset_and_clear_drop_the_pending_sets():
    m = SchedModel(1, 1, 4, 8)
    one = np.ones((1, 4), dtype=np.float32)
    m.set_at(0, [[2.0]])
    m.set_at(100, [[5.0]])
    assert m.mix(one)[0].tolist() == [2, 2, 2, 2] and len(m.pending) == 1
    m.clear_schedule()
    assert not m.pending
    m.set_at(50, [[7.0]])
    m.reset()
    assert not m.pending and m.t == 0
    assert m.mix(one)[0].tolist() == [2, 2, 2, 2]                    # the target last in force, not a dropped one
