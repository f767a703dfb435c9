"""PBSO_GATHER_SCENE (include/openpbso_amd.h "device group"): every rank mixes its own objects into C channels, the ranks
all-reduce the C rows.  LOOPBACK worlds of 2, 3 and 4 ranks with ragged shards (and an empty rank) against one engine's scene mix
fed the same messages and the same set calls; a one-rank RCCL_ALWAYS group against its own engine, bit for bit; the once-per-step
rule of the group."""
import numpy as np
import pytest

from openpbso_amd import capi, synth

pytestmark = pytest.mark.gpu


def _scene(modes, nb_total, seed):
    rng = np.random.default_rng(seed)
    lams = [synth.eigenvalues(m, 900 + i) for i, m in enumerate(modes)]
    shapes = [synth.mode_shapes(m, 900 + i) for i, m in enumerate(modes)]
    nv = shapes[0].shape[1] // 3
    hits = sorted(((int(rng.integers(0, len(modes))), int(rng.integers(0, nv)), int(rng.integers(0, nb_total)))
                   for _ in range(6 * len(modes))), key=lambda h: h[2])
    return lams, shapes, hits, synth.unit_normals(len(hits), seed)


def _feed(eng, grp, modes, lams, shapes, hits, vns):
    from openpbso_amd import ForceMessage
    grp.plan(modes)
    for i in range(len(modes)):
        if eng is not None:
            eng.add_object(lams[i], synth.RHO, synth.ALPHA, synth.BETA, mode_shapes=shapes[i])
        grp.add_object(i, lams[i], synth.RHO, synth.ALPHA, synth.BETA, mode_shapes=shapes[i])
    if eng is not None:
        eng.finalize()
        for i in range(len(modes)):
            eng.set_use_transfer(i, False)
    grp.finalize()
    for r in grp.local_ranks():
        lo, hi = grp.span(r)
        for l in range(hi - lo):
            grp.engine(r).set_use_transfer(l, False)
    for (o, v, t), vn in zip(hits, vns):
        m = ForceMessage(vid=v, vn=vn)
        assert grp.enqueue_force(o, m, t)
        if eng is not None:
            assert eng.enqueue_force(o, m, t)


def _sets(C, n, max_delay, seed):
    rng = np.random.default_rng(seed)
    return {0: (rng.uniform(-1, 1, (C, n)), rng.uniform(0, max_delay, (C, n))),
            2: (rng.uniform(-1, 1, (C, n)), rng.uniform(0, max_delay, (C, n))),
            3: (rng.uniform(-1, 1, (C, n)), None)}


@pytest.mark.parametrize("world,modes", [(2, [4096, 64, 64, 64]), (3, [300] * 7), (4, [64] * 3 + [200] * 6), (3, [128, 128])])
def test_loopback_scene_gather_equals_the_single_engine(world, modes):
    """ragged shards ([4096, 64, 64, 64] on two ranks is 1 + 3 objects; two objects on three ranks leave a rank empty, which
    contributes silence); the ranks' mixes summed in rank order equal one engine's scene mix within f32 reassociation"""
    from openpbso_amd import Engine
    from openpbso_amd.group import Group
    from openpbso_amd.solver import PbsoError
    steps = [3, 1, 2, 4]
    C, max_delay, R = 2, 800, 600
    lams, shapes, hits, vns = _scene(modes, sum(steps), world)
    sets = _sets(C, len(modes), max_delay, world)
    with Engine() as eng, Group([0] * world, transport=capi.GROUP_LOOPBACK) as grp:
        _feed(eng, grp, modes, lams, shapes, hits, vns)
        eng.scene_mix_enable(C, max_delay, R)
        grp.scene_mix_enable(C, max_delay, R)
        xmax = np.zeros(len(modes))
        for k, nb in enumerate(steps):
            if k in sets:
                eng.scene_mix_set(*sets[k])
                grp.scene_mix_set(*sets[k])
            eng.step(nb)
            eng.scene_mix()
            want = eng.read_scene_mix().astype(np.float64)
            rows = eng.audio()
            grp.step(nb)
            grp.gather(capi.GATHER_ALL)                      # another mode of the same step first: allowed
            grp.gather(capi.GATHER_SCENE)
            # sum_o |g_co| max|x_o| over everything the mix can have read (gains during a ramp lie between two set values)
            xmax = np.maximum(xmax, np.abs(rows).max(axis=1))
            bound = np.abs(np.concatenate([s[0] for j, s in sets.items() if j <= k], axis=1)).max() * xmax.sum()
            for r in range(world):
                got = grp.result(r)
                assert got.shape == (C, nb * 513), (k, r)
                assert np.abs(got - want).max() <= 1e-5 * bound, (k, r, np.abs(got - want).max(), bound)
            assert np.abs(want).max() > 0
            with pytest.raises(PbsoError):
                grp.gather(capi.GATHER_SCENE)                # once per step
            grp.gather(capi.GATHER_MIX)                      # the other modes still work for this step


def test_one_rank_rccl_scene_gather_equals_a_standalone_engine():
    """PBSO_GROUP_RCCL_ALWAYS: the ncclAllReduce (in place) of one rank's C rows, bit for bit the scene mix of a separate engine fed
    the same messages and set calls -- not the rank engine's own output, which is the all-reduce's buffer"""
    from openpbso_amd import Engine
    from openpbso_amd.group import Group
    modes = [200] * 6 + [64, 333]
    steps = [4, 2, 3]
    C, max_delay, R = 3, 1200, 900
    lams, shapes, hits, vns = _scene(modes, sum(steps), 21)
    sets = _sets(C, len(modes), max_delay, 21)
    with Engine() as eng, Group([0], transport=capi.GROUP_RCCL_ALWAYS) as grp:
        _feed(eng, grp, modes, lams, shapes, hits, vns)
        eng.scene_mix_enable(C, max_delay, R)
        grp.scene_mix_enable(C, max_delay, R)
        for k, nb in enumerate(steps):
            if k in sets:
                eng.scene_mix_set(*sets[k])
                grp.scene_mix_set(*sets[k])
            eng.step(nb)
            eng.scene_mix()
            want = eng.read_scene_mix()
            grp.step(nb)
            grp.gather(capi.GATHER_SCENE)
            got = grp.result(0)
            assert got.shape == (C, nb * 513) and np.abs(want).max() > 0
            assert np.array_equal(got, want), k


def test_group_scene_mix_argument_and_state_checks():
    from openpbso_amd.group import Group
    from openpbso_amd.solver import PbsoError
    with Group([0], transport=capi.GROUP_LOOPBACK) as grp:
        grp.plan([64, 64])
        with pytest.raises(PbsoError):
            grp.scene_mix_enable(2, 10, 0)                   # before finalize
        for i in range(2):
            grp.add_object(i, synth.eigenvalues(64, 3 + i), synth.RHO, synth.ALPHA, synth.BETA)
        grp.finalize()
        grp.step(1)
        with pytest.raises(PbsoError):
            grp.gather(capi.GATHER_SCENE)                    # not enabled
        for bad in ((0, 10, 0), (9, 10, 0), (2, -1, 0)):
            with pytest.raises(PbsoError):
                grp.scene_mix_enable(*bad)
        grp.scene_mix_enable(2, 10, 0)
        with pytest.raises(PbsoError):
            grp.gather(capi.GATHER_SCENE)                    # the step before the enable is not armed
        with pytest.raises(PbsoError):
            grp.scene_mix_set(np.ones((2, 2)), np.full((2, 2), 11.0))      # a delay above max_delay
        with pytest.raises(PbsoError):
            grp.scene_mix_set(np.full((2, 2), np.nan))
        grp.scene_mix_set(np.ones((2, 2)), np.full((2, 2), 2.5))
        grp.step(2)
        grp.gather(capi.GATHER_SCENE)
        p, rows, row = grp.result_ptr(0)
        assert p and rows == 2 and row == 2 * 513
