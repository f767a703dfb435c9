"""The scene of tests/test_gpu_scan_borders.py: 150 buffers whose events sit on the borders of the time-axis scan (kernels_scan.hip).

The scan decodes its buffers in batches (lane = buffer): 64 per batch in the serial kernel, 32 in the segmented one and 16 in its DENSE
build; it requests hit rows HB = 16 at a time, steps in unrolled groups of G = 8 whose gains are fetched two groups ahead, and carries the
transfer row in force from batch to batch.  The positions P are the first and last lanes of groups, of both segmented batch sizes and
of the serial batches 0, 1 and 2; every event kind is put there on an object that still rings from a hit at most two buffers earlier, so
that a skipped step, a lost gain, a mark one buffer off or a wrong transfer row is an error of the order of the peak.

What sits where (objects by index into SIZES):
  * the four force kinds -- explicit-data impulse, vertex hit, face hit, clear -- at every position of P, rotated over the objects that
    are free there (the rotation runs backwards, so that the object that was cleared at p is the idle one at p + 1 where five are free);
  * object 3 (300 modes, FFAT maps with one psi zeroed; the only one with use_transfer) is the one cleared at CLEAR3, the launch-local
    lanes 15, 16, 31, 32, 63, 64 and the run's last buffer, and takes a listener move at every position of LISTENER_AT: stamped on a
    cleared buffer the move is the kind "listener_clear" and its row waits for the next buffer that steps (the moves at 63 and 64
    take effect at 65).  No move lies in 66 .. 139: cut [2, 148] makes 66 .. 129 serial batch 1, and the row in force at the chunk
    starts of batch 2 is then the one set in batch 0; the move at LATE_MOVE = 140 ends the stretch;
  * object 4 (600 modes) is hit on every buffer of RUN = [64, 104), vertex / explicit / face in turn: 40 hits in serial batch 1, three
    windows of HB.  It has no other hit in 14 .. 60 and 104 .. 127, which is what lets HIT_CUTS count 16, 17, 33 and 40 hits in one batch;
  * object 2 has a clear on every buffer of CLEAR_RUN = [76, 95): chunk 4 of the segmented scan at 19 buffers per chunk steps nothing;
  * dense events (dense=True only): a Gaussian of three buffers on object 2 from 62 (alive across 63 | 64) and on object 3 from 126
    (across 127 | 128), a sustained AR stroke on object 1 from 60 to 70 with data updates and an arprm at 63 and at 64 (the only buffers
    an arprm may lie on: outside a sustained stroke nobody takes it from its one-slot queue), and a plain AR force on object 1 at 129,
    which lives to the end of the run.  Object 1 takes no other message in 60 .. 70 in either variant, so both variants share BORDERS.

One force message per (object, buffer): ModalSolver::step takes one from the queue per buffer (modal_solver.h:184).
"""
import numpy as np

from openpbso_amd import synth
from tests.scenarios import ObjSpec, force_ev

NB = 150
SIZES = (1, 64, 65, 300, 600)
P = (0, 7, 8, 15, 16, 17, 23, 24, 31, 32, 33, 47, 48, 62, 63, 64, 65, 71, 72, 127, 128, 129, 149)
FORCE_KINDS = ("impulse", "vertex", "face", "clear")
KINDS = FORCE_KINDS + ("listener", "listener_clear", "arprm")
HIT_KINDS = ("impulse", "vertex", "face")

MAPS_OBJ, RUN_OBJ, CLEAR_OBJ, STROKE_OBJ = 3, 4, 2, 1
RUN = range(64, 104)                      # object 4: a hit on every buffer
CLEAR_RUN = range(76, 95)                 # object 2: a clear on every buffer
CLEAR3 = (15, 16, 31, 32, 63, 64, 149)    # object 3 cleared (with a listener move on the same stamp)
LISTENER_AT = tuple(p for p in P if p not in (17, 33) and not 65 <= p <= 129)      # (17, 33, 65: behind two cleared buffers)
LATE_MOVE = 140                           # object 3: one more listener move, on no border, behind 74 buffers without one
STROKE = (60, 70)                         # object 1: sustained AR contact, start and end message
STROKE_DATA = (62, 65, 67)                # ... its data updates
ARPRM_AT = (63, 64)
GAUSS = {62: 2, 126: 3}                   # first buffer -> object; alive for GAUSS_BUFFERS buffers
GAUSS_WIDTH_US = 2800.0                   # 123 samples wide, cut off after 1230: three buffers of 513
GAUSS_BUFFERS = 3
DENSE_AMP = 5e-5                          # dense data against the impulses' 1e-3: a profile of hundreds of samples, the same peak
AR_AT, AR_OBJ = 129, 1                    # a plain AutoregressiveForce: never removed (forces.h:119-128)

# cuts of the run that put 40, 33, 17 hits of object 4 into ONE 64-buffer batch of the serial scan, and the prefix whose batch 1 has 16:
# (launch lengths, index of the launch, batch of that launch, hits).  Object 4 is hit at 61, 62, 63 and on RUN, so the batch
# [30, 94) holds 3 + 30 and [14, 78) holds 3 + 14.
HIT_CUTS = (([NB], 0, 1, 40), ([30, 120], 1, 0, 33), ([14, 136], 1, 0, 17), ([80], 0, 1, 16))


def _free_objects(p):
    """the objects that may take one of the four force kinds at position p"""
    free = [0, 1, 2, 3, 4]
    if STROKE[0] <= p <= STROKE[1] + 1 or p == AR_AT:      # (+ 1: no room for the hit that must come before)
        free.remove(STROKE_OBJ)
    if p in GAUSS and GAUSS[p] in free:
        free.remove(GAUSS[p])
    if p in (17, 33, 65):
        free.remove(MAPS_OBJ)
    if 14 <= p <= 60 or 104 <= p <= 128:
        free.remove(RUN_OBJ)
    return free


def _run_kind(b):
    return ("vertex", "impulse", "face")[(b - RUN[0]) % 3]


def _placement():
    """{(kind, position): object} of the four force kinds"""
    table = {}
    r = 0
    for p in P:
        free = _free_objects(p)
        kinds = list(FORCE_KINDS)
        if p in CLEAR3:
            table[("clear", p)] = MAPS_OBJ
            free.remove(MAPS_OBJ)
            kinds.remove("clear")
        if p in RUN:
            table[(_run_kind(p), p)] = RUN_OBJ
            free.remove(RUN_OBJ)
            kinds.remove(_run_kind(p))
        # a Gaussian is alive on its object until GAUSS_BUFFERS are over: no clear there
        no_clear = {o for b0, o in GAUSS.items() if b0 <= p < b0 + GAUSS_BUFFERS}
        for _ in range(len(free)):
            got = {k: free[(i + r) % len(free)] for i, k in enumerate(kinds[:len(free)])}
            if got.get("clear") not in no_clear:
                break
            r -= 1
        for k, o in got.items():
            table[(k, p)] = o
        r -= 1
    return table


def _borders():
    table = _placement()
    for p in LISTENER_AT:
        table[("listener_clear" if table.get(("clear", p)) == MAPS_OBJ else "listener", p)] = MAPS_OBJ
    for p in ARPRM_AT:
        table[("arprm", p)] = STROKE_OBJ
    return table


BORDERS = _borders()                      # {(kind, position): object}; the "arprm" entries exist in the dense variant only


def borders(dense=True):
    return {k: o for k, o in BORDERS.items() if dense or k[0] != "arprm"}


_LISTENER_DIRS = np.array([[1, .2, .3], [.2, 1, .3], [.2, .3, 1], [-1, .2, .3], [.3, -1, .2]], dtype=float)


def build(dense=True):
    """(objs, events) for scenarios.run_engine / run_oracle"""
    rng = np.random.default_rng(150150)
    objs, shapes = [], []
    for i, m in enumerate(SIZES):
        lam = synth.eigenvalues(m, 2900 + i)
        shp = synth.mode_shapes(m, 2900 + i)
        maps = None
        if i == MAPS_OBJ:
            maps = synth.ffat_maps(lam, 2900 + i, dim=4, cell_size=0.01)
            for mm in maps:
                mm["psi"] = np.array(mm["psi"], dtype=np.float64)
            maps[7]["psi"][:] = 0.0
        objs.append(ObjSpec(lam, shapes=shp, maps=maps))
        shapes.append(shp)
    nv = synth.N_VERTS
    vns = [synth.unit_normals(NB, 2900 + i) for i in range(len(SIZES))]

    def hit(kind, b, o):
        if kind == "impulse":
            return force_ev(b, o, data=rng.standard_normal(SIZES[o]) * 1e-3)
        if kind == "vertex":
            return force_ev(b, o, vid=int(rng.integers(0, nv)), vn=vns[o][b])
        if kind == "face":
            bary = rng.random(3) + 0.1
            return force_ev(b, o, vids=[int(v) for v in rng.choice(nv, 3, replace=False)], coords=list(bary / bary.sum()), vn=vns[o][b])
        assert kind == "clear"
        return force_ev(b, o, clear=True)

    msgs = {}                             # (object, buffer) -> kind of its one force message
    for (kind, p), o in sorted(BORDERS.items(), key=lambda kv: (kv[0][1], kv[1], kv[0][0])):
        if kind in FORCE_KINDS:
            assert (o, p) not in msgs
            msgs[(o, p)] = kind
    for b in RUN:
        msgs[(RUN_OBJ, b)] = _run_kind(b)
    for b in CLEAR_RUN:
        msgs[(CLEAR_OBJ, b)] = "clear"
    dense_msgs = {}
    for b in (STROKE[0],) + STROKE_DATA + (STROKE[1],):
        dense_msgs[(STROKE_OBJ, b)] = "stroke"
    for b0, o in GAUSS.items():
        dense_msgs[(o, b0)] = "gauss"
    dense_msgs[(AR_OBJ, AR_AT)] = "ar"
    assert not set(msgs) & set(dense_msgs)
    # primers: whatever a border event acts on rings from a hit at most two buffers earlier (in both variants: a dense message is not
    # counted as one; an arprm acts on the stroke itself)
    targets = sorted({(o, p) for (kind, p), o in BORDERS.items() if kind != "arprm"} | {(CLEAR_OBJ, CLEAR_RUN[0]), (STROKE_OBJ, STROKE[0]), (AR_OBJ, AR_AT)}
                     | {(o, b0) for b0, o in GAUSS.items()} | {(MAPS_OBJ, LATE_MOVE)}, key=lambda t: (t[1], t[0]))
    for o, p in targets:
        if p == 0 or any(msgs.get((o, q)) in HIT_KINDS for q in (p - 1, p - 2) if q >= 0):
            continue
        for q in (p - 1, p - 2):
            blocked = o == STROKE_OBJ and STROKE[0] <= q <= STROKE[1]
            if q >= 0 and (o, q) not in msgs and (o, q) not in dense_msgs and not blocked:
                msgs[(o, q)] = "vertex"
                break
        else:
            raise AssertionError(f"no room for a primer in front of object {o}, buffer {p}")

    evs = [dict(t=0, obj=i, kind="use_transfer", use=False) for i in range(len(SIZES)) if i != MAPS_OBJ]
    for (o, b), kind in sorted(msgs.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        evs.append(hit(kind, b, o))
    for k, p in enumerate(LISTENER_AT + (LATE_MOVE,)):
        d = _LISTENER_DIRS[k % len(_LISTENER_DIRS)]
        evs.append(dict(t=p, obj=MAPS_OBJ, kind="listener", pos=(0.35 + 0.05 * (k % 4)) * d / np.linalg.norm(d)))
    if dense:
        o = STROKE_OBJ
        evs.append(force_ev(STROKE[0], o, data=rng.standard_normal(SIZES[o]) * DENSE_AMP, force_type=2, start=True))
        for b in STROKE_DATA:
            evs.append(force_ev(b, o, data=rng.standard_normal(SIZES[o]) * DENSE_AMP, force_type=2))
        evs.append(force_ev(STROKE[1], o, force_type=2, end=True))
        for k, b in enumerate(ARPRM_AT):
            evs.append(dict(t=b, obj=o, kind="arprm", a=[0.5 - 0.1 * k, 0.3], sigma=0.004 + 0.002 * k, mu=0.2 + 0.1 * k))
        for b0, go in GAUSS.items():
            evs.append(force_ev(b0, go, data=rng.standard_normal(SIZES[go]) * DENSE_AMP, force_type=1, width=GAUSS_WIDTH_US))
        evs.append(force_ev(AR_AT, AR_OBJ, data=rng.standard_normal(SIZES[AR_OBJ]) * DENSE_AMP, force_type=2))
    return objs, evs


def script_rows(events, dense=True):
    """what the script says of every (object, buffer), by ModalSolver::step's rules (modal_solver.h:184-240): `kind` [n_obj][NB] of
    's' (skipped: a clear), 'h' (an impulse: a PointForce's one sample), 'd' (a dense profile: a Gaussian alive, an AR force) or '.'"""
    kind = np.full((len(SIZES), NB), ".", dtype="<U1")
    for o in range(len(SIZES)):
        by_buf = {}
        for e in events:
            if e["obj"] == o and e["kind"] == "force":
                assert e["t"] not in by_buf, "one force message per (object, buffer)"
                by_buf[e["t"]] = e
        gauss_left, ar, sustained = 0, False, False
        for b in range(NB):
            e = by_buf.get(b)
            point = False
            if e is not None:
                if e["clear"]:
                    assert not sustained, "a clear inside a sustained stroke trips the reference's assert"
                    gauss_left, ar = 0, False
                    kind[o, b] = "s"
                    continue
                if e["start"]:
                    gauss_left, ar, sustained = 0, True, True
                elif not sustained:
                    if e["force_type"] == 0:
                        point = True
                    elif e["force_type"] == 1:
                        gauss_left = GAUSS_BUFFERS
                    else:
                        ar = True
                if e["end"]:
                    gauss_left, ar, sustained, point = 0, False, False, False
            if gauss_left or ar:
                kind[o, b] = "d"
            elif point:
                kind[o, b] = "h"
            gauss_left = max(0, gauss_left - 1)
    return kind


def hits_in_batch(kind_row, cut, launch, batch, width=64):
    """hits (the scan's hit mask: live && (amp != 0 || !impulse)) of one object in batch `batch` of launch `launch` of a cut"""
    lo = sum(cut[:launch]) + width * batch
    hi = min(lo + width, sum(cut[:launch + 1]))
    return int(np.isin(kind_row[lo:hi], ("h", "d")).sum())


def dense_rows(kind, lo, hi):
    """dense (object, buffer) rows of the launch [lo, hi)"""
    return int((kind[:, lo:hi] == "d").sum())
