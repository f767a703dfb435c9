"""The scene filter mix's bank through the device group (pbso_group_scene_fir_bank_create / _set_bank / _set_bank_at /
_bank_schedule): LOOPBACK worlds of 2 and 3 ranks with ragged shards, gathered with PBSO_GATHER_FIR.  Every rank holds the whole
bank and takes the pairs of its own objects; the result equals, bit for bit, the single engine's reference
(tests/scene_fir_sched_ref.py fed the taps tests/cpp/scene_fir_bank_ref.c builds) applied to each rank's objects, the ranks' results
added in rank order in f32 -- the group's stated sum."""
import numpy as np
import pytest

from openpbso_amd import capi
from openpbso_amd.solver import PbsoError
from tests.scene_fir_bank_model import taps_from_bank
from tests.scene_fir_sched_ref import Piecewise
from tests.test_gpu_group_scene_fir import _bits, _feed, _scene

pytestmark = pytest.mark.gpu

B = 513


@pytest.mark.parametrize("world,modes", [(2, [4096, 64, 64, 64]), (3, [300] * 7)])
def test_loopback_worlds_with_bank_sets_equal_the_reference_per_rank(world, modes):
    """[4096, 64, 64, 64] on two ranks is 1 + 3 objects, seven objects on three ranks 3 + 2 + 2.  Sets scheduled inside the steps
    (one call, onsets given), one at a later step's first sample, and a plain set_bank between two steps with onset None"""
    from openpbso_amd.group import Group
    steps = [2, 1, 2]
    C, K, F, J, max_onset, R = 2, 24, 11, 3, 300, 200
    n = len(modes)
    lams, hits, data = _scene(modes, sum(steps), 40 + world)
    rng = np.random.default_rng(40 + world)
    bank = (rng.standard_normal((F, C, K)) * np.exp(-np.arange(K) / 8.0)).astype(np.float32)
    times = [0, 300, B + 77, 2 * B]                                   # the last: pending across the first step's end
    index = rng.integers(0, F, (5, n, J)).astype(np.int32)
    weight = rng.standard_normal((5, n, J)).astype(np.float32)
    index[0, 0, :], weight[0, 0, :] = F - 1, [1.0, 0.0, -0.5]         # a repeated index on the first rank's object
    index[1, n - 1, 0], weight[1, n - 1, 0] = 0, 1.0
    onsets = rng.integers(0, max_onset + 1, (4, n)).astype(np.int32)
    with Group([0] * world, transport=capi.GROUP_LOOPBACK) as grp:
        _feed(None, grp, modes, lams, hits, data)
        spans = [grp.span(r) for r in range(world)]
        assert len({hi - lo for lo, hi in spans}) > 1 and all(hi > lo for lo, hi in spans)      # ragged, no rank empty
        refs = [Piecewise(C, hi - lo, K, max_onset, R) for lo, hi in spans]
        with pytest.raises(PbsoError) as ei:
            grp.scene_fir_bank_create(bank)                           # the group's filter mix is not enabled
        assert ei.value.status == capi.ERR_STATE
        grp.scene_fir_enable(C, K, max_onset, R)
        with pytest.raises(PbsoError) as ei:
            grp.scene_fir_set_bank(index[0], weight[0])               # no bank
        assert ei.value.status == capi.ERR_STATE
        grp.scene_fir_bank_create(bank)
        assert grp.scene_fir_bank_info()["n_filters"] == F
        bad = index[:4].copy()
        bad[3, n - 1, 2] = F                                          # the last rank's object: no rank takes a set
        with pytest.raises(PbsoError) as ei:
            grp.scene_fir_bank_schedule(times, bad, weight[:4], onsets)
        assert ei.value.status == capi.ERR_INVALID
        assert tuple(grp.scene_fir_schedule_info().values())[:3] == (0, 0, 0)
        grp.scene_fir_set_bank_at(times[0], index[0], weight[0], onsets[0])
        grp.scene_fir_bank_schedule(times[1:], index[1:4], weight[1:4], onsets[1:])
        for (lo, hi), ref in zip(spans, refs):
            ref.schedule(times, np.stack([taps_from_bank(bank, index[k, lo:hi], weight[k, lo:hi]) for k in range(4)]), onsets[:, lo:hi])
        assert tuple(grp.scene_fir_schedule_info().values())[:3] == (0, 4, 0)
        t = 0
        for k, nb in enumerate(steps):
            if k == 2:                                                # a plain bank set between two steps, the onsets kept
                grp.scene_fir_set_bank(index[4], weight[4])
                for (lo, hi), ref in zip(spans, refs):
                    ref.schedule([t], taps_from_bank(bank, index[4, lo:hi], weight[4, lo:hi])[None])
            grp.step(nb)
            grp.gather(capi.GATHER_FIR)
            want = np.zeros((C, nb * B), dtype=np.float32)
            for r, ref in enumerate(refs):
                want = want + ref.mix(grp.engine(r).audio())
            for r in range(world):
                _bits(grp.result(r), want, (k, r))
            t += nb * B
        assert tuple(grp.scene_fir_schedule_info().values())[:3] == (t, 0, 0)
        assert grp.scene_fir_bank_info()["sets"] == 5
