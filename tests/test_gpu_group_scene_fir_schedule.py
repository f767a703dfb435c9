"""The scene filter mix's schedule through the device group (pbso_group_scene_fir_set_at / _schedule / _set_delay_at /
_delay_schedule / _clear_schedule): a LOOPBACK world of 2 ranks with ragged shards.  The schedule mixed in one step equals, bit for
bit, a second group driven with plain sets between steps cut at every change point (time_chunks = 1: the same rows for both)."""
import numpy as np
import pytest

from openpbso_amd import capi
from openpbso_amd.solver import PbsoError
from tests.test_gpu_group_scene_fir import _bits, _feed, _scene

pytestmark = pytest.mark.gpu

B = 513


def test_loopback_group_schedule_in_one_step_equals_cut_steps_with_plain_sets():
    from openpbso_amd.group import Group
    modes = [8, 4, 4, 4, 2]
    at = [0, 2, 3]                                                    # buffers of the filter sets; the delay sets one later
    at_d = [0, 3, 4]
    C, K, max_onset, R, max_delay, Rd, nb_total = 2, 24, 300, 400, 500, 700, 6
    n = len(modes)
    lams, hits, data = _scene(modes, nb_total, 71)
    rng = np.random.default_rng(71)
    taps = (rng.standard_normal((len(at), C, n, K)) * np.exp(-np.arange(K) / 8.0)).astype(np.float32)
    onsets = rng.integers(0, max_onset + 1, (len(at), n)).astype(np.int32)
    dl = rng.uniform(0, max_delay, (len(at_d), n)).astype(np.float32)
    with Group([0, 0], transport=capi.GROUP_LOOPBACK, time_chunks=1) as one, Group([0, 0], transport=capi.GROUP_LOOPBACK, time_chunks=1) as cut:
        for grp in (one, cut):
            _feed(None, grp, modes, lams, hits, data)
        with pytest.raises(PbsoError) as ei:
            one.scene_fir_set_at(0, taps[0], onsets[0])              # the group's filter mix is not enabled
        assert ei.value.status == capi.ERR_STATE
        for grp in (one, cut):
            grp.scene_fir_enable(C, K, max_onset, R)
        with pytest.raises(PbsoError) as ei:
            one.scene_fir_set_delay_at(0, dl[0])                     # ... nor its delay stage
        assert ei.value.status == capi.ERR_STATE
        for grp in (one, cut):
            grp.scene_fir_delay_enable(max_delay, Rd)
        bad = taps[1:].copy()
        bad[1, 1, n - 1, 3] = np.inf                                  # the last rank's object: no rank takes a set
        with pytest.raises(PbsoError) as ei:
            one.scene_fir_schedule([b * B for b in at[1:]], bad, onsets[1:])
        assert ei.value.status == capi.ERR_INVALID
        assert tuple(one.scene_fir_schedule_info().values())[:3] == (0, 0, 0)
        one.scene_fir_set_at(0, taps[0], onsets[0])
        one.scene_fir_schedule([b * B for b in at[1:]], taps[1:], onsets[1:])
        one.scene_fir_set_delay_at(0, dl[0])
        one.scene_fir_delay_schedule([b * B for b in at_d[1:]], dl[1:])
        assert tuple(one.scene_fir_schedule_info().values())[:3] == (0, 3, 3)
        one.step(nb_total)
        one.gather(capi.GATHER_ALL)
        rows_one = one.result(0)
        one.gather(capi.GATHER_FIR)
        assert tuple(one.scene_fir_schedule_info().values())[:3] == (nb_total * B, 0, 0)
        mixes, rows = [[], []], []
        edges = sorted(set(at + at_d + [nb_total]))
        for b0, b1 in zip(edges[:-1], edges[1:]):
            if b0 in at:
                cut.scene_fir_set(taps[at.index(b0)], onsets[at.index(b0)])
            if b0 in at_d:
                cut.scene_fir_set_delay(dl[at_d.index(b0)])
            cut.step(b1 - b0)
            cut.gather(capi.GATHER_ALL)
            rows.append(cut.result(0))
            cut.gather(capi.GATHER_FIR)
            for r in range(2):
                mixes[r].append(cut.result(r))
        assert np.array_equal(rows_one, np.concatenate(rows, axis=1))         # (the precondition: the same rows)
        for r in range(2):
            got = one.result(r)
            assert got.shape == (C, nb_total * B)
            _bits(got, np.concatenate(mixes[r], axis=1), r)
        one.scene_fir_set_at(nb_total * B + 900, taps[0], onsets[0])
        one.scene_fir_set_delay_at(nb_total * B + 9, dl[0])
        assert tuple(one.scene_fir_schedule_info().values())[1:3] == (1, 1)
        one.scene_fir_clear_schedule()
        assert tuple(one.scene_fir_schedule_info().values())[1:3] == (0, 0)
        with pytest.raises(PbsoError) as ei:
            one.scene_fir_set_at(nb_total * B - 1, taps[0])           # in the past: refused for the whole group
        assert ei.value.status == capi.ERR_INVALID
