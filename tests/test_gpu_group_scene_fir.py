"""PBSO_GATHER_FIR (include/openpbso_amd.h "device group"): every rank filters its own objects into C channels, the ranks
all-reduce the C rows.  A one-rank LOOPBACK group and a one-rank RCCL_ALWAYS group against a standalone engine; LOOPBACK worlds of
2 and 3 ranks with ragged shards and an empty rank against the reference applied to each rank's objects and the ranks' results
added in rank order in f32 -- all bit for bit; the once-per-step rule of the group."""
import numpy as np
import pytest

from openpbso_amd import ForceMessage, capi, synth
from tests.scene_fir_model import Model

pytestmark = pytest.mark.gpu

B = 513


def _scene(modes, nb_total, seed):
    rng = np.random.default_rng(seed)
    lams = [synth.eigenvalues(m, 700 + i) for i, m in enumerate(modes)]
    hits = sorted(((int(rng.integers(0, len(modes))), int(rng.integers(0, nb_total))) for _ in range(4 * len(modes))), key=lambda h: h[1])
    hits = [(o, 0) for o in range(len(modes))] + hits
    return lams, hits, [rng.standard_normal(modes[o]) * 1e-3 for o, _ in hits]


def _feed(eng, grp, modes, lams, hits, data):
    grp.plan(modes)
    for i in range(len(modes)):
        if eng is not None:
            eng.add_object(lams[i], synth.RHO, synth.ALPHA, synth.BETA)
        grp.add_object(i, lams[i], synth.RHO, synth.ALPHA, synth.BETA)
    if eng is not None:
        eng.finalize()
        for i in range(len(modes)):
            eng.set_use_transfer(i, False)
    grp.finalize()
    for r in grp.local_ranks():
        lo, hi = grp.span(r)
        for l in range(hi - lo):
            grp.engine(r).set_use_transfer(l, False)
    for (o, t), s in zip(hits, data):
        m = ForceMessage(data=s)
        assert grp.enqueue_force(o, m, t)
        if eng is not None:
            assert eng.enqueue_force(o, m, t)


def _sets(C, n, K, max_onset, seed):
    rng = np.random.default_rng(seed)
    taps = lambda: (rng.standard_normal((C, n, K)) * np.exp(-np.arange(K) / 8.0)).astype(np.float32)
    return {0: (taps(), rng.integers(0, max_onset + 1, n)), 1: (taps(), rng.integers(0, max_onset + 1, n)), 3: (taps(), None)}


def _bits(got, want, label):
    assert got.shape == want.shape and np.abs(want).max() > 0, label
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (label, np.abs(got - want).max())


@pytest.mark.parametrize("transport", [capi.GROUP_LOOPBACK, capi.GROUP_RCCL_ALWAYS])
def test_one_rank_group_equals_a_standalone_engine(transport):
    """the loopback sum of one rank, and the in-place ncclAllReduce of one rank's C rows: the filter mix of a separate engine fed
    the same messages and set calls"""
    from openpbso_amd import Engine
    from openpbso_amd.group import Group
    modes = [200] * 6 + [64, 333]
    steps = [2, 1, 3, 2]
    C, K, max_onset, R = 3, 24, 900, 400
    lams, hits, data = _scene(modes, sum(steps), 21)
    sets = _sets(C, len(modes), K, max_onset, 21)
    with Engine() as eng, Group([0], transport=transport) as grp:
        _feed(eng, grp, modes, lams, hits, data)
        eng.scene_fir_enable(C, K, max_onset, R)
        grp.scene_fir_enable(C, K, max_onset, R)
        for k, nb in enumerate(steps):
            if k in sets:
                eng.scene_fir_set(*sets[k])
                grp.scene_fir_set(*sets[k])
            eng.step(nb)
            eng.scene_fir()
            grp.step(nb)
            grp.gather(capi.GATHER_FIR)
            _bits(grp.result(0), eng.read_scene_fir(), k)


@pytest.mark.parametrize("world,modes", [(2, [4096, 64, 64, 64]), (3, [300] * 7), (3, [128, 128])])
def test_loopback_worlds_equal_the_reference_per_rank_added_in_rank_order(world, modes):
    """ragged shards ([4096, 64, 64, 64] on two ranks is 1 + 3 objects; two objects on three ranks leave a rank empty, which
    contributes silence); every step also gathered in the other modes, and a second GATHER_FIR refused"""
    from openpbso_amd.group import Group
    from openpbso_amd.solver import PbsoError
    steps = [2, 1, 1, 2]
    C, K, max_onset, R = 2, 24, 800, 300
    lams, hits, data = _scene(modes, sum(steps), world)
    sets = _sets(C, len(modes), K, max_onset, world)
    with Group([0] * world, transport=capi.GROUP_LOOPBACK) as grp:
        _feed(None, grp, modes, lams, hits, data)
        spans = [grp.span(r) for r in range(world)]
        models = [Model(C, hi - lo, K, max_onset, R) if hi > lo else None for lo, hi in spans]
        grp.scene_fir_enable(C, K, max_onset, R)
        for k, nb in enumerate(steps):
            if k in sets:
                h, d = sets[k]
                grp.scene_fir_set(h, d)
                for (lo, hi), m in zip(spans, models):
                    if m is not None:
                        m.set(h[:, lo:hi], None if d is None else d[lo:hi])
            grp.step(nb)
            grp.gather(capi.GATHER_ALL)                      # another mode of the same step first: allowed
            grp.gather(capi.GATHER_FIR)
            want = np.zeros((C, nb * B), dtype=np.float32)
            for r, m in enumerate(models):
                want = want + (m.mix(grp.engine(r).audio()) if m is not None else np.float32(0))
            for r in range(world):
                _bits(grp.result(r), want, (k, r))
            with pytest.raises(PbsoError) as ei:
                grp.gather(capi.GATHER_FIR)                  # once per step
            assert ei.value.status == capi.ERR_STATE
            for mode in (capi.GATHER_ALL, capi.GATHER_ROOT, capi.GATHER_MIX):
                grp.gather(mode)                             # the other modes still work for this step
            assert grp.result(0).shape == (nb * B,) or grp.result(0).shape == (1, nb * B)


def test_scene_gather_and_filter_gather_of_one_step():
    """both of a group's mixers enabled: modes 4 and 5 of the same step, each once"""
    from openpbso_amd.group import Group
    from openpbso_amd.solver import PbsoError
    modes = [64] * 5
    lams, hits, data = _scene(modes, 2, 4)
    with Group([0, 0], transport=capi.GROUP_LOOPBACK) as grp:
        _feed(None, grp, modes, lams, hits, data)
        grp.step(1)
        with pytest.raises(PbsoError):
            grp.gather(capi.GATHER_FIR)                      # not enabled
        for bad in ((0, 4, 10, 0), (2, 0, 10, 0), (2, 1025, 10, 0), (2, 4, -1, 0)):
            with pytest.raises(PbsoError):
                grp.scene_fir_enable(*bad)
        grp.scene_fir_enable(2, 4, 10, 0)
        grp.scene_mix_enable(3, 10, 0)
        with pytest.raises(PbsoError):
            grp.gather(capi.GATHER_FIR)                      # the step before the enable is not armed
        with pytest.raises(PbsoError):
            grp.scene_fir_set(np.ones((2, 5, 4)), np.full(5, 11))          # an onset above max_onset
        with pytest.raises(PbsoError):
            grp.scene_fir_set(np.full((2, 5, 4), np.nan))
        grp.scene_fir_set(np.ones((2, 5, 4)), np.full(5, 2))
        grp.scene_mix_set(np.ones((3, 5)))
        grp.step(2)
        grp.gather(capi.GATHER_SCENE)
        assert grp.result(1).shape == (3, 2 * B)
        grp.gather(capi.GATHER_FIR)
        p, rows, row = grp.result_ptr(0)
        assert p and rows == 2 and row == 2 * B and np.abs(grp.result(0)).max() > 0
