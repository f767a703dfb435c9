"""K1b (kernels_block.hip), the stretch between two buffers' matrix pipelines: the per-lane accesses of the buffer loop go through a
uniform base and a 32-bit lane offset (the next buffer's coefficient, qnorm-matrix, force-gain and transfer rows, the qnorm row store,
the stores of a skipped buffer), and the combine reads sample 0 in the same pass as the block sums.  None of it changes a value: oracle parity at the block form's stated tolerances on the smallest scenes that
reach every one of those paths -- a quiet object, direct vertex hits, a transfer-row change, an explicit-data hit and a skipped buffer
in the headline instantiation (four modes per lane, two waves), its time-chunked twin, the builds of one and two modes per lane and a
team of four waves -- and a step cut into one-buffer launches equals the one launch bit for bit.
"""
import numpy as np
import pytest

from openpbso_amd import capi, synth
from tests.scenarios import ObjSpec, force_ev, rel_errors, run_engine, run_oracle

pytestmark = pytest.mark.gpu

TOL_MAX, TOL_L2 = 5e-4, 1e-3          # tests/test_gpu_parity.py, the block forms


def _check(got, want, qnorm=True):
    assert np.isfinite(got["audio"]).all()
    assert np.array_equal(got["emitted"], want["emitted"])
    mx, l2 = rel_errors(got["audio"], want["audio"])
    assert (mx <= TOL_MAX).all(), f"max-abs/peak {mx.max():.3e} > {TOL_MAX}"
    assert (l2 <= TOL_L2).all(), f"rel-L2 {l2.max():.3e} > {TOL_L2}"
    if qnorm:
        assert got["qnorm"].keys() >= want["qnorm"].keys()
        for key, w in want["qnorm"].items():
            assert np.abs(got["qnorm"][key] - w).max() <= 5e-4 * max(np.abs(w).max(), 1e-30) + 2e-6 * np.abs(want["audio"][key[0]]).max(), key
    for g, w in zip(got["state"], want["state"]):
        np.testing.assert_allclose(g[0], w[0], rtol=0, atol=5e-4 * max(np.abs(w[0]).max(), 1e-30))


NB = 6
SKIPPED = 3          # object 2's clearAllForces buffer


def _scene(n_modes=512):
    """object 0 quiet throughout; object 1 direct vertex hits in buffers 0, 1 and 4; object 2 hears through FFAT maps: its transfer
    row changes with the listener (buffers 0, 2 and 5), one hit by explicit data (buffer 1), one skipped buffer (clearAllForces)"""
    rng = np.random.default_rng(606)
    objs, evs = [], []
    for i in range(3):
        lam = synth.eigenvalues(n_modes, 2600 + i)
        maps = synth.ffat_maps(lam, 2600 + i, dim=4, cell_size=0.01) if i == 2 else None
        objs.append(ObjSpec(lam, shapes=synth.mode_shapes(n_modes, 2600 + i), maps=maps))
        if maps is None:
            evs.append(dict(t=0, obj=i, kind="use_transfer", use=False))
    nv = objs[1].shapes.shape[1] // 3
    vns = synth.unit_normals(NB, 2601)
    for b in (0, 1, 4):
        evs.append(force_ev(b, 1, vid=int(rng.integers(0, nv)), vn=vns[b]))
    dirs = np.array([[1, .2, .3], [.2, 1, .3], [.2, .3, 1]], dtype=float)
    for k, b in enumerate((0, 2, 5)):
        evs.append(dict(t=b, obj=2, kind="listener", pos=0.5 * dirs[k] / np.linalg.norm(dirs[k])))
    evs.append(force_ev(1, 2, data=rng.standard_normal(n_modes) * 1e-3))
    evs.append(force_ev(SKIPPED, 2, clear=True))
    return objs, evs


@pytest.fixture(scope="module")
def scene():
    objs, evs = _scene()
    return objs, evs, run_oracle(objs, evs, NB)


def _headline(info):
    assert info["modes_per_lane"] == 4 and info["waves_per_object"] == 2
    assert info["total_split_launches"] == 0 and info["total_sample_launches"] == 0


@pytest.mark.parametrize("form", [capi.FORM_BLOCK, capi.FORM_BLOCK_BF16])
@pytest.mark.parametrize("qnorm", [capi.QNORM_ALL, capi.QNORM_OFF])
def test_every_path_between_two_pipelines_one_launch(scene, qnorm, form, monkeypatch):
    monkeypatch.setenv("PBSO_SPLIT", "0")          # K1b for every launch
    objs, evs, want = scene
    got = run_engine(objs, evs, NB, form=form, qnorm=qnorm, modes_per_lane=4, team_waves=2, time_chunks=-1)
    _headline(got["info"])
    assert got["info"]["total_block_launches"] == 1 and got["info"]["total_time_chunk_launches"] == 0
    _check(got, want, qnorm=qnorm != capi.QNORM_OFF)
    assert not got["emitted"][2, SKIPPED] and got["emitted"].sum() == 3 * NB - 1
    assert not got["audio"][0].any() and not got["audio"][2, SKIPPED * 513:(SKIPPED + 1) * 513].any()
    assert np.abs(got["audio"][1]).max() > 0 and np.abs(got["audio"][2]).max() > 0


@pytest.mark.parametrize("cb", [1, 4])
def test_time_chunked_twin(scene, cb, monkeypatch):
    monkeypatch.setenv("PBSO_SPLIT", "0")
    objs, evs, want = scene
    got = run_engine(objs, evs, NB, form=capi.FORM_BLOCK, qnorm=capi.QNORM_ALL, modes_per_lane=4, team_waves=2, time_chunks=cb)
    _headline(got["info"])
    assert got["info"]["total_time_chunk_launches"] == got["info"]["total_block_launches"] == 1
    _check(got, want)


@pytest.mark.parametrize("n_modes,mpl,waves", [(64, 1, 1), (128, 2, 1), (1024, 4, 4)])
def test_other_team_shapes(n_modes, mpl, waves, monkeypatch):
    """one mode per lane (the half-ring combine, one barrier per group), two, and four waves of four (the combine adds the waves'
    rings in the order w = 0 .. 3); three buffers, one hit"""
    monkeypatch.setenv("PBSO_SPLIT", "0")
    rng = np.random.default_rng(n_modes)
    objs = [ObjSpec(synth.eigenvalues(n_modes, 2700 + n_modes))]
    evs = [dict(t=0, obj=0, kind="use_transfer", use=False), force_ev(1, 0, data=rng.standard_normal(n_modes) * 1e-3)]
    want = run_oracle(objs, evs, 3)
    got = run_engine(objs, evs, 3, form=capi.FORM_BLOCK, qnorm=capi.QNORM_ALL, modes_per_lane=mpl, team_waves=waves, time_chunks=-1)
    assert got["info"]["modes_per_lane"] == mpl and got["info"]["waves_per_object"] == waves
    assert got["info"]["total_block_launches"] == 1 and got["info"]["total_split_launches"] == 0
    _check(got, want)


def test_one_buffer_launches_equal_the_one_launch_bit_for_bit(scene, monkeypatch):
    """the end-of-launch state store and the first buffer's prefetch, six times instead of once"""
    monkeypatch.setenv("PBSO_SPLIT", "0")
    objs, evs, want = scene
    one = run_engine(objs, evs, NB, form=capi.FORM_BLOCK, qnorm=capi.QNORM_ALL, modes_per_lane=4, team_waves=2, time_chunks=-1)
    cut = run_engine(objs, evs, NB, split=[1] * NB, form=capi.FORM_BLOCK, qnorm=capi.QNORM_ALL, modes_per_lane=4, team_waves=2, time_chunks=-1)
    _headline(cut["info"])
    assert cut["info"]["total_block_launches"] == NB
    assert np.array_equal(one["audio"], cut["audio"]) and np.array_equal(one["emitted"], cut["emitted"])
    for key in one["qnorm"]:
        assert np.array_equal(one["qnorm"][key], cut["qnorm"][key]), key
    for sa, sb in zip(one["state"], cut["state"]):
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    _check(cut, want)
