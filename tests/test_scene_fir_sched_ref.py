"""The reference of the filter mix's schedule anchored on itself, without a GPU: tests/scene_fir_sched_ref.py feeds the existing
models (tests/scene_fir_model.py, tests/scene_fir_delay_model.py) a step's rows cut at every t_set.  The models promise that the
cut into pieces does not matter; here the same schedule is run at two different cuts -- at the change points only, and at extra
points between them, in one step and in several -- and the bits must agree."""
import numpy as np
import pytest

from tests.scene_fir_sched_ref import Piecewise


def _run(delay, steps, cuts):
    C, N, K, max_onset, R, max_delay, Rd = 2, 5, 9, 40, 30, 50, 70
    rng = np.random.default_rng(11)
    n = 1200
    rows = rng.standard_normal((N, n)).astype(np.float32)
    ft = [0, 29, 300, 329, 700, 1199]                                 # (two pairs exactly R - 1 apart)
    dt = [3, 40, 60, 61, 690, 1100]
    taps = rng.standard_normal((len(ft), C, N, K)).astype(np.float32)
    onsets = rng.integers(0, max_onset + 1, (len(ft), N)).astype(np.int32)
    dl = rng.uniform(0, max_delay, (len(dt), N)).astype(np.float32)
    ref = Piecewise(C, N, K, max_onset, R, max_delay if delay else None, Rd)
    ref.schedule(ft[:3], taps[:3], onsets[:3])
    ref.schedule(ft[3:], taps[3:])                                    # onset None: the onsets of the set before
    if delay:
        ref.delay_schedule(dt, dl)
    outs, at = [], 0
    for m in steps:
        outs.append(ref.mix(rows[:, at:at + m], [c - at for c in cuts]))
        at += m
    assert at == n
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("delay", [False, True])
def test_the_piecewise_reference_does_not_depend_on_its_cuts(delay):
    a = _run(delay, [1200], [])
    b = _run(delay, [1200], [1, 17, 299, 301, 512, 1198])
    c = _run(delay, [400, 1, 799], [50, 450, 900])
    assert np.abs(a).max() > 0 and a.shape == (2, 1200)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
