"""The delay stage of the scene filter mix through the device group (pbso_group_scene_fir_delay_enable / _set_delay; include/
openpbso_amd.h "device group"): the comparison of tests/test_gpu_group_scene_fir.py -- a LOOPBACK world of 2 ranks with ragged
shards against the reference applied to each rank's objects and the ranks' results added in rank order in f32, bit for bit --
with delays set by global object id and sliced per rank."""
import numpy as np
import pytest

from openpbso_amd import capi
from tests.scene_fir_delay_model import Model
from tests.test_gpu_group_scene_fir import _bits, _feed, _scene, _sets

pytestmark = pytest.mark.gpu

B = 513


def test_loopback_world_of_two_with_delays_equals_the_reference_per_rank():
    from openpbso_amd.group import Group
    from openpbso_amd.solver import PbsoError
    world, modes = 2, [4096, 64, 64, 64]                 # 1 + 3 objects
    steps = [2, 1, 1, 2]
    C, K, max_onset, R, max_delay, Rd = 2, 24, 800, 300, 700, 600
    n = len(modes)
    lams, hits, data = _scene(modes, sum(steps), world)
    sets = _sets(C, n, K, max_onset, world)
    rng = np.random.default_rng(7)
    delays = {0: rng.uniform(0, max_delay, n), 1: rng.uniform(0, max_delay, n), 2: rng.uniform(0, max_delay, n)}
    with Group([0] * world, transport=capi.GROUP_LOOPBACK) as grp:
        _feed(None, grp, modes, lams, hits, data)
        spans = [grp.span(r) for r in range(world)]
        with pytest.raises(PbsoError) as ei:
            grp.scene_fir_delay_enable(max_delay, Rd)        # the group's filter mix is not enabled
        assert ei.value.status == capi.ERR_STATE
        grp.scene_fir_enable(C, K, max_onset, R)
        with pytest.raises(PbsoError) as ei:
            grp.scene_fir_set_delay(delays[0])               # the delay stage is not enabled
        assert ei.value.status == capi.ERR_STATE
        with pytest.raises(PbsoError) as ei:
            grp.scene_fir_delay_enable(-1, Rd)
        assert ei.value.status == capi.ERR_INVALID
        grp.scene_fir_delay_enable(max_delay, Rd)
        bad = delays[0].copy()
        bad[n - 1] = max_delay + 1                           # the last rank's object: no rank takes the set
        with pytest.raises(PbsoError) as ei:
            grp.scene_fir_set_delay(bad)
        assert ei.value.status == capi.ERR_INVALID
        assert all(grp.engine(r).scene_fir_delay_info()["sets"] == 0 for r in range(world))
        models = [Model(C, hi - lo, K, max_onset, R, max_delay, Rd) for lo, hi in spans]
        for k, nb in enumerate(steps):
            if k in sets:
                h, d = sets[k]
                grp.scene_fir_set(h, d)
                for (lo, hi), m in zip(spans, models):
                    m.set(h[:, lo:hi], None if d is None else d[lo:hi])
            if k in delays:
                grp.scene_fir_set_delay(delays[k])
                for (lo, hi), m in zip(spans, models):
                    m.set_delay(delays[k][lo:hi])
            grp.step(nb)
            grp.gather(capi.GATHER_FIR)
            want = np.zeros((C, nb * B), dtype=np.float32)
            for r, m in enumerate(models):
                want = want + m.mix(grp.engine(r).audio())
            for r in range(world):
                _bits(grp.result(r), want, (k, r))
                assert grp.engine(r).scene_fir_delay_info() == models[r].info(), (k, r)
