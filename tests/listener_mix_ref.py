"""The reference of the multi-listener mix (pbso_listeners_enable / pbso_mix_listeners): what L independent fp64
ModalSolvers emit that were fed the same force messages, listener l's after computeTransfer(pos_l) (modal_solver.h:286-315).

oracle_rows takes the force events of tests/scenarios.py for ONE object -- explicit modal data, vertex / face hits projected with
the oracle's GetModalForceVertex / GetModalForceFace, clearAllForces, several messages on one stamp (the solver dequeues one per
step, modal_solver.h:184) -- and returns [L][n_buffers * 513] float64.  tests/test_listener_mix_ref.py shows that a row equals
scenarios.run_oracle with a `listener` event at that position, stamp 0, bit for bit."""
import numpy as np

from oracle import oracle_py as orc
from tests import scenarios

B = scenarios.B


def _modal_data(o, ev):
    n = o.n_modes
    if ev["data"] is not None:
        return np.asarray(ev["data"], dtype=np.float64)
    if ev["vid"] is not None:
        return orc.modal_force_vertex(o.shapes, ev["vid"], ev["vn"], n)
    if ev["vids"] is not None:
        return orc.modal_force_face(o.shapes, ev["vids"], ev["coords"], ev["vn"], n)
    return np.zeros(n)


def _rows(o, omaps, events, pos, nb):
    evs = sorted(events, key=lambda e: e["t"])
    assert all(e["kind"] == "force" for e in evs), "the listeners are the positions: force events only"
    msgs = [(e["t"], _modal_data(o, e), e) for e in evs]                 # (projected once, shared by the listeners)
    out = np.zeros((len(pos), nb * B))
    for l, p in enumerate(pos):
        s = orc.Solver(o.lam, o.rho, o.alpha, o.beta, n_modes=o.n_modes)
        if omaps is not None:
            s.read_ffat_maps(omaps)
            s.compute_transfer(p)
        else:
            s.set_use_transfer(False)
        i = 0
        for b in range(nb):
            while i < len(msgs) and msgs[i][0] <= b:
                _, data, e = msgs[i]
                i += 1
                assert s.enqueue_force(data, orc.make_force(e["force_type"], e["width"]), e["start"], e["end"], e["clear"])
            snd = s.step()
            if snd is not None:                                          # (None: clearAllForces, no buffer -- the engine writes zeros)
                out[l, b * B:(b + 1) * B] = snd[0]
        s.close()
    return out


def oracle_rows(o, events, pos, nb, obj=None):
    """o: a scenarios.ObjSpec (maps None: the unit transfer for every listener); events: scenarios.force_ev dicts, of object `obj`
    only when that is given; pos [L][3]"""
    evs = [e for e in events if obj is None or e["obj"] == obj]
    omaps = None if o.maps is None else [scenarios.oracle_map(m) for m in o.maps]
    return _rows(o, omaps, evs, np.asarray(pos, dtype=np.float64).reshape(-1, 3), nb)


def oracle_per_listener(lam, omaps, pos, nb, hits, clear_at=()):
    """the earlier form: explicit data `hits` {buffer: vector}, clearAllForces in the buffers `clear_at`, oracle maps ready made"""
    o = scenarios.ObjSpec(lam)                                           # (synth's material, as every caller of this form has)
    evs = [scenarios.force_ev(b, 0, clear=True) if b in clear_at else scenarios.force_ev(b, 0, data=hits[b])
           for b in sorted(set(hits) | set(clear_at))]
    return _rows(o, omaps, evs, np.asarray(pos, dtype=np.float64).reshape(-1, 3), nb)
