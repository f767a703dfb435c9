"""The scene of the pbso_set_material tests (tests/test_gpu_retune*.py): four ragged objects -- 1, 65, 200 and 1100 modes, the
last one several teams with split partial sums; the two in the middle have mode shapes of 5 vertices -- and one script of 5
buffers: vertex hits through the bank's own projection, a projected face hit, a Gaussian that lives three buffers, a sustained
AR stroke, explicit modal data; qnorm rows on.  One runner for the engine with a hook between its two steps, one for the oracle
with the integrator swapped at the same buffer."""
import ctypes as C

import numpy as np

from openpbso_amd import Engine, ForceMessage, capi, synth
from oracle import oracle_py as orc
from tests.scenarios import force_ev

MODES = [1, 65, 200, 1100]
N_VERTS = 5
MAT1 = (synth.RHO, synth.ALPHA, synth.BETA)
MAT2 = (1900.0, 25.0, 3e-7)                  # lighter and more damped: every mode under-damped, the highest at 20.6 kHz
OVERDAMPED = (synth.RHO, 1e5, synth.BETA)    # alpha / omega0 >> 1 for the low modes: sqrt of a negative number in modal_integrator.h:90
NB, CUT = 5, 2                               # buffers of the script; the retune point of the mid-run tests
LAMS = [synth.eigenvalues(n, 4100 + i) for i, n in enumerate(MODES)]
SHAPES = [None, synth.mode_shapes(65, 4101, N_VERTS), synth.mode_shapes(200, 4102, N_VERTS), None]


def events():
    rng = np.random.default_rng(41)
    vn = synth.unit_normals(8, 41)
    ev = [
        force_ev(0, 0, data=np.array([2e-3])),
        force_ev(0, 1, vid=3, vn=vn[0]),                                            # the bank's own projection
        force_ev(0, 2, vid=0, vn=vn[1]),
        force_ev(1, 2, vids=(1, 2, 4), coords=(0.2, 0.5, 0.3), vn=vn[2]),           # a projected face hit
        force_ev(0, 3, data=rng.standard_normal(1100) * 1e-3, force_type=capi.GAUSSIAN_FORCE, width=3400.0),   # ~3 buffers
        force_ev(3, 3, data=rng.standard_normal(1100) * 1e-3),
        # a sustained AR stroke over buffers 1 .. 3, its contact point moved once
        force_ev(1, 1, vids=(0, 1, 2), coords=(0.6, 0.3, 0.1), vn=vn[3], force_type=capi.AUTOREGRESSIVE_FORCE, start=True),
        force_ev(2, 1, vids=(2, 3, 4), coords=(0.1, 0.1, 0.8), vn=vn[4], force_type=capi.AUTOREGRESSIVE_FORCE),
        force_ev(4, 1, force_type=capi.AUTOREGRESSIVE_FORCE, end=True),
        force_ev(3, 2, vid=4, vn=vn[5]),
        force_ev(4, 0, data=np.array([-1e-3])),
    ]
    return sorted(ev, key=lambda e: e["t"])


def _msg(ev):
    return ForceMessage(data=ev["data"], forceType=ev["force_type"], gaussianWidth=ev["width"], sustainedForceStart=ev["start"],
                        sustainedForceEnd=ev["end"], clearAllForces=ev["clear"], vid=ev["vid"], vids=ev["vids"], coords=ev["coords"],
                        vn=ev["vn"])


def build_engine(mats, **kw):
    """mats: one (density, alpha, beta) for all objects or one per object"""
    if not isinstance(mats[0], tuple):
        mats = [mats] * len(MODES)
    eng = Engine(**kw)
    for lam, sh, m in zip(LAMS, SHAPES, mats):
        eng.add_object(lam, m[0], m[1], m[2], mode_shapes=sh)
    eng.finalize()
    for i in range(len(MODES)):
        eng.set_use_transfer(i, False)
    return eng


def enqueue_all(eng):
    for ev in events():
        assert eng.enqueue_force(ev["obj"], _msg(ev), ev["t"])


def collect(eng, nb, out, done):
    out["audio"].append(eng.audio().copy())
    for oi in range(len(MODES)):
        for b in range(nb):
            out["qnorm"][(oi, done + b)] = eng.qnorm(oi, b).copy()


def run(mats, before=None, between=None, enqueue_first=False, chunks=(CUT, NB - CUT), **kw):
    """The script on an engine built with `mats`.  before(eng): called after finalize, behind the enqueue calls when enqueue_first
    (else in front of them); between(eng): called between the steps of `chunks` (after the first).  Returns audio [4][NB * B],
    the qnorm rows, the final state and the engine's last material stats."""
    eng = build_engine(mats, **kw)
    try:
        if enqueue_first:
            enqueue_all(eng)
        if before:
            before(eng)
        if not enqueue_first:
            enqueue_all(eng)
        out = dict(audio=[], qnorm={})
        done = 0
        for k, nb in enumerate(chunks):
            eng.step(nb)
            collect(eng, nb, out, done)
            done += nb
            if k == 0 and between:
                between(eng)
        out["audio"] = np.concatenate(out["audio"], axis=1)
        out["state"] = [eng.state(i) for i in range(len(MODES))]
        out["stats"] = eng.material_stats()
        out["material"] = [eng.material(i) for i in range(len(MODES))]
        return out
    finally:
        eng.close()


def same_run(a, b, rows=None):
    """audio, qnorm rows and state agree bit for bit (for the objects `rows`)"""
    rows = range(len(MODES)) if rows is None else rows
    for i in rows:
        assert np.array_equal(a["audio"][i], b["audio"][i]), ("audio", i, np.abs(a["audio"][i].astype(np.float64) - b["audio"][i]).max())
        for bb in range(NB):
            assert np.array_equal(a["qnorm"][(i, bb)], b["qnorm"][(i, bb)]), ("qnorm", i, bb)
        for w in range(2):
            assert np.array_equal(a["state"][i][w], b["state"][i][w]), ("state", i, w)
    assert max(np.abs(a["audio"][i]).max() for i in rows) > 0


def retune_to(mat, ids=None, keep=True):
    ids = list(range(len(MODES))) if ids is None else ids
    return lambda eng: eng.set_material(ids, mat[0], mat[1], mat[2], keep_state=keep)


# ---- the oracle, with ModalSolver::setIntegrator at a buffer ------------------------------------------------------------------
def oracle_swap(s, lam, mat, keep):
    """or_integrator_build + or_solver_set_integrator on a live oracle solver; keep: the old integrator's (q_{k-1}, q_{k-2}) are
    copied into the new one through the pointers or_solver_state returns"""
    l = s._l
    q1, q2 = s.state()
    om = np.ascontiguousarray(lam, dtype=np.float64)
    it = l.or_integrator_build(mat[0], om.ctypes.data_as(C.POINTER(C.c_double)), om.size, mat[1], mat[2], l.h, s.n)
    assert it
    l.or_solver_set_integrator(s._s, it)
    if keep:
        for which, q in ((0, q1), (1, q2)):
            dst = np.ctypeslib.as_array(l.or_solver_state(s._s, which), shape=(s.n,))
            dst[:] = q


def run_oracle(mat, swap=None, only=None):
    """swap: None or (buffer, material, keep) -- the integrator of every object swapped before that buffer's step.
    Returns audio [n][NB * B] f64, qnorm rows, state."""
    ids = list(range(len(MODES))) if only is None else list(only)
    evs = events()
    out = dict(audio=np.zeros((len(MODES), NB * 513)), qnorm={}, state=[None] * len(MODES))
    for oi in ids:
        s = orc.Solver(LAMS[oi], mat[0], mat[1], mat[2])
        s.set_use_transfer(False)
        mine = [e for e in evs if e["obj"] == oi]
        ei = 0
        for b in range(NB):
            if swap and b == swap[0]:
                oracle_swap(s, LAMS[oi], swap[1], swap[2])
            while ei < len(mine) and mine[ei]["t"] <= b:
                ev = mine[ei]
                ei += 1
                n = MODES[oi]
                if ev["data"] is not None:
                    data = np.asarray(ev["data"], dtype=np.float64)
                elif ev["vid"] is not None:
                    data = orc.modal_force_vertex(SHAPES[oi], ev["vid"], ev["vn"], n)
                elif ev["vids"] is not None:
                    data = orc.modal_force_face(SHAPES[oi], ev["vids"], ev["coords"], ev["vn"], n)
                else:
                    data = np.zeros(n)
                assert s.enqueue_force(data, orc.make_force(ev["force_type"], ev["width"]), ev["start"], ev["end"], ev["clear"])
            r = s.step()
            assert r is not None
            out["audio"][oi, b * 513:(b + 1) * 513] = r[0]
            out["qnorm"][(oi, b)] = r[1].copy()
        out["state"][oi] = s.state()
        s.close()
    return out
