"""tests/listener_mix_ref.py against tests/scenarios.py: the reference of the multi-listener mix and the reference of every
parity test are one -- a listener's row is what run_oracle gives for the same script with a `listener` event at that position."""
import numpy as np

from openpbso_amd import synth
from tests.listener_mix_ref import oracle_per_listener, oracle_rows
from tests.scenarios import B, ObjSpec, force_ev, oracle_map, run_oracle


def test_a_row_is_run_oracle_with_a_listener_event_at_stamp_0():
    n, nb = 70, 6
    lam = synth.eigenvalues(n, 611)
    o = ObjSpec(lam, shapes=synth.mode_shapes(n, 612, 5), maps=synth.ffat_maps(lam, 613, dim=4, cell_size=0.01))
    vn = synth.unit_normals(3, 614)
    rng = np.random.default_rng(615)
    evs = [force_ev(0, 0, vid=3, vn=vn[0]),
           force_ev(1, 0, vids=[0, 2, 4], coords=np.array([0.2, 0.5, 0.3]), vn=vn[1]),
           force_ev(1, 0, data=rng.standard_normal(n) * 1e-3),                          # the same stamp: dequeued a buffer later
           force_ev(3, 0, clear=True),
           force_ev(4, 0, vid=1, vn=vn[2])]
    pos = np.array([[0.3, -0.2, 0.4], [-0.5, 0.1, 0.2], [0.05, 0.45, -0.3]])
    rows = oracle_rows(o, evs, pos, nb)
    assert rows.shape == (3, nb * B)
    for l, p in enumerate(pos):
        want = run_oracle([o], evs + [dict(t=0, obj=0, kind="listener", pos=p)], nb)
        assert list(want["emitted"][0]) == [True, True, True, False, True, True]
        assert np.array_equal(rows[l], want["audio"][0]), l
        assert not rows[l, 3 * B:4 * B].any() and np.abs(rows[l, 4 * B:]).max() > 0
    assert not np.array_equal(rows[0], rows[1])                                       # the positions are heard apart


def test_the_unit_transfer_and_the_earlier_call_form():
    """without maps every listener hears the unit transfer (a `use_transfer` event with use = False in run_oracle); the form
    tests/test_gpu_listener_mix_edges.py calls -- explicit data by buffer, clears, oracle maps ready made -- gives the same rows"""
    n, nb = 33, 4
    lam = synth.eigenvalues(n, 711)
    rng = np.random.default_rng(712)
    hits = {0: rng.standard_normal(n) * 1e-3, 3: rng.standard_normal(n) * 1e-3}
    evs = [force_ev(0, 0, data=hits[0]), force_ev(2, 0, clear=True), force_ev(3, 0, data=hits[3])]
    pos = np.array([[0.3, -0.2, 0.4], [-0.5, 0.1, 0.2]])
    rows = oracle_rows(ObjSpec(lam), evs, pos, nb)
    want = run_oracle([ObjSpec(lam)], evs + [dict(t=0, obj=0, kind="use_transfer", use=False)], nb)["audio"][0]
    assert np.array_equal(rows[0], want) and np.array_equal(rows[1], want)
    assert np.array_equal(oracle_per_listener(lam, None, pos, nb, hits, clear_at=(2,)), rows)
    maps = synth.ffat_maps(lam, 713, dim=4, cell_size=0.01)
    a = oracle_per_listener(lam, [oracle_map(m) for m in maps], pos, nb, hits, clear_at=(2,))
    assert np.array_equal(a, oracle_rows(ObjSpec(lam, maps=maps), evs, pos, nb))
