"""The CPU anchor of tests/scan_border_scene.py (no GPU): the border table covers what it claims, the built events sit where it says,
the hit counts per scan batch are the ones the hit-window cases need, every border event acts on a ringing object, and the oracle's run
of the scene is pinned, so that an edit of the scene shows here before it shows as a changed GPU figure."""
import copy
import hashlib

import numpy as np
import pytest

from tests import scan_border_scene as S
from tests.scenarios import B, run_oracle

EXACT_LANES = (15, 16, 31, 32, 63, 64)


def position_classes():
    """the classes of launch-local position the issue names, as {class: positions of P in it}"""
    cls = {"first lane of a group": [p for p in S.P if p % 8 == 0], "last lane of a group": [p for p in S.P if p % 8 == 7],
           "last buffer of the run": [S.NB - 1]}
    for lane in EXACT_LANES:
        cls[f"lane {lane}"] = [lane]
    return cls


@pytest.fixture(scope="module", params=[True, False], ids=["dense", "plain"])
def scene(request):
    objs, evs = S.build(dense=request.param)
    return dict(dense=request.param, objs=objs, evs=evs, want=run_oracle(objs, evs, S.NB))


def check_table(evs, table):
    """every (kind, position) of the table is an event of that kind on that object at that buffer"""
    force = {(e["obj"], e["t"]): e for e in evs if e["kind"] == "force"}
    other = {(e["kind"], e["obj"], e["t"]) for e in evs if e["kind"] != "force"}
    for (kind, p), o in table.items():
        e = force.get((o, p))
        where = (kind, p, o)
        if kind in S.FORCE_KINDS:
            assert e is not None and e["force_type"] == 0 and not e["start"] and not e["end"], where
            assert e["clear"] == (kind == "clear"), where
            assert (e["data"] is not None) == (kind == "impulse") and (e["vid"] is not None) == (kind == "vertex"), where
            assert (e["vids"] is not None) == (kind == "face"), where
        elif kind in ("listener", "listener_clear"):
            assert ("listener", o, p) in other and o == S.MAPS_OBJ, where
            assert (e is not None and e["clear"]) == (kind == "listener_clear"), where
        else:
            assert kind == "arprm" and ("arprm", o, p) in other, where
            assert S.STROKE[0] <= p < S.STROKE[1] and o == S.STROKE_OBJ, where


def test_the_table_covers_every_kind_at_every_class_of_position():
    assert len(S.P) == len(set(S.P)) and max(S.P) == S.NB - 1 and set(k for k, _ in S.BORDERS) == set(S.KINDS)
    classes = position_classes()
    for name, pos in classes.items():
        assert pos and set(pos) <= set(S.P), name
        for p in pos:
            # the four force kinds: at EVERY position of every class
            for kind in S.FORCE_KINDS:
                assert (kind, p) in S.BORDERS, (kind, name, p)
    # every force kind on at least four different objects (the rotation)
    for kind in S.HIT_KINDS:
        assert len({o for (k, _), o in S.BORDERS.items() if k == kind}) >= 4, kind
    assert len({o for (k, _), o in S.BORDERS.items() if k == "clear"}) >= 4
    # listener moves: one object has maps, so a position holds EITHER a move on a stepped buffer or one on a cleared buffer.  The move
    # on a cleared buffer (the row must wait for the next buffer that steps: across the batch border at 15 | 16, 31 | 32, 63 | 64)
    # takes the exact lanes and the last buffer, the plain move first and last lanes of groups; together every class, and every
    # position of P outside 65 .. 129 (66 .. 139 have no move, so that cut [2, 148] has a serial batch without one) and behind a double clear
    moves = {p: k for (k, p) in S.BORDERS if k in ("listener", "listener_clear")}
    assert set(moves) == set(S.LISTENER_AT) == {p for p in S.P if not 65 <= p <= 129 and p not in (17, 33)}
    for name, pos in classes.items():
        assert any(p in moves for p in pos), name
    for p in EXACT_LANES + (S.NB - 1,):
        assert moves[p] == "listener_clear", p
    assert {p % 8 for p, k in moves.items() if k == "listener"} >= {0, 7}
    # an arprm is taken from its one-slot queue by a sustained AR buffer only (modal_solver.h:225-231): legal inside the stroke, and
    # there it sits on lane 63 (last of a group, last of serial batch 0) and lane 64 (first of a group, first of batch 1)
    assert {p for (k, p) in S.BORDERS if k == "arprm"} == {63, 64}
    assert "arprm" not in {k for k, _ in S.borders(dense=False)} and len(S.borders(False)) == len(S.BORDERS) - 2


def test_the_events_sit_where_the_table_says(scene):
    check_table(scene["evs"], S.borders(scene["dense"]))
    kind = S.script_rows(scene["evs"])
    for (k, p), o in S.borders(scene["dense"]).items():
        if k in S.HIT_KINDS:
            assert kind[o, p] in ("h", "d"), (k, p, o)         # ('d': the hit falls on a buffer a Gaussian or an AR force is alive on)
        elif k in ("clear", "listener_clear"):
            assert kind[o, p] == "s", (k, p, o)
        elif k == "arprm":
            assert kind[o, p] == "d", (k, p, o)
    # the oracle agrees with the script's reading of which buffers step
    assert np.array_equal(scene["want"]["emitted"], kind != "s")
    assert (kind[S.RUN_OBJ, S.RUN[0]:S.RUN[-1] + 1] == "h").all() and (kind[S.CLEAR_OBJ, S.CLEAR_RUN[0]:S.CLEAR_RUN[-1] + 1] == "s").all()
    if scene["dense"]:
        assert "".join(kind[2, 61:66]) == "hdddh" and "".join(kind[3, 125:130]) == "hdddh"       # the Gaussians: alive across 63 | 64 and 127 | 128
        assert (kind[S.STROKE_OBJ, 60:70] == "d").all() and kind[S.STROKE_OBJ, 70] == "." and (kind[S.AR_OBJ, S.AR_AT:] == "d").all()
        assert S.dense_rows(kind, 0, S.NB) == 3 + 3 + 10 + 21
    else:
        assert S.dense_rows(kind, 0, S.NB) == 0


@pytest.mark.parametrize("what", ["hit", "clear", "listener", "arprm"])
def test_a_moved_event_fails_the_table(what):
    """the coverage check is not vacuous: one event moved one buffer off its border fails it"""
    _, evs = S.build(dense=True)
    evs = copy.deepcopy(evs)
    pick = {"hit": lambda e: e["kind"] == "force" and e["obj"] == S.BORDERS[("face", 63)] and e["t"] == 63,
            "clear": lambda e: e["kind"] == "force" and e["obj"] == S.MAPS_OBJ and e["t"] == 64,
            "listener": lambda e: e["kind"] == "listener" and e["t"] == 62,
            "arprm": lambda e: e["kind"] == "arprm" and e["t"] == 64}[what]
    moved = [e for e in evs if pick(e)]
    assert len(moved) == 1
    check_table(evs, S.BORDERS)
    moved[0]["t"] += 1 if what != "clear" else 2
    with pytest.raises(AssertionError):
        check_table(evs, S.BORDERS)


def test_hit_counts_of_one_batch(scene):
    """the hit-window cases: 16 hits fill one window of HB = 16 exactly, 17 need a second one, 33 a third, 40 is the whole run.  The
    issue's cuts [41, 109] and [57, 93] leave all 40 hits of [64, 104) in one batch ([41, 105) and [57, 121): 43 with 61 .. 63), so the
    cuts are [30, 120] and [14, 136]: with the three hits of object 4 at 61 .. 63 the batches [30, 94) and [14, 78) hold 33 and 17"""
    row = S.script_rows(scene["evs"])[S.RUN_OBJ]
    got = [S.hits_in_batch(row, cut, launch, batch) for cut, launch, batch, _ in S.HIT_CUTS]
    assert got == [n for *_, n in S.HIT_CUTS] == [40, 33, 17, 16]
    assert [cut for cut, *_ in S.HIT_CUTS] == [[150], [30, 120], [14, 136], [80]]
    assert S.hits_in_batch(row, [41, 109], 1, 0) == 43 and S.hits_in_batch(row, [57, 93], 1, 0) == 43


def test_every_border_event_acts_on_a_ringing_object(scene):
    """a hit at most two buffers earlier, and audio in the last buffer before the event that was emitted (a cleared buffer emits
    nothing: where the buffer before is one, the one before that) of at least 5e-3 of the object's peak -- ten times the audio bar"""
    want, kind = scene["want"], S.script_rows(scene["evs"])
    audio = want["audio"].reshape(len(S.SIZES), S.NB, B)
    peak = np.abs(audio).max(axis=(1, 2))
    for (k, p), o in S.borders(scene["dense"]).items():
        if p == 0:
            continue
        assert any(q >= 0 and kind[o, q] in ("h", "d") for q in (p - 1, p - 2)), (k, p, o)
        q = p - 1 if want["emitted"][o, p - 1] else p - 2
        assert want["emitted"][o, q] and np.abs(audio[o, q]).max() >= 5e-3 * peak[o], (k, p, o, np.abs(audio[o, q]).max() / peak[o])
    # ... and the events themselves are audible: a hit changes the buffer it falls on
    assert (np.abs(audio).max(axis=2)[kind == "h"] > 0).all()


def layout_digest(evs):
    """the script's layout -- kinds, objects, buffers, vertex ids: integers only -- as a digest"""
    rows = sorted((e["t"], e["obj"], e["kind"], int(e.get("force_type") or 0), bool(e.get("clear")), bool(e.get("start")), bool(e.get("end")),
                   -1 if e.get("vid") is None else int(e["vid"]), tuple(int(v) for v in (e.get("vids") or ()))) for e in evs)
    return hashlib.sha256(repr(rows).encode()).hexdigest()[:16]


PINNED = {True: dict(n_events=213, digest="a595c86a51353cc4", peaks=[24350.717708, 3802748.6382, 123090879.81, 200171708.07, 24141471.408]),
          False: dict(n_events=203, digest="80d286796f048aaa", peaks=[24350.717708, 3051165.3319, 3590748.6414, 17503662.697, 24141471.408])}


def test_the_oracle_run_is_pinned(scene):
    """deterministic: two builds and two oracle runs give the same bits; and pinned: the layout digest and the per-object peaks and
    energies of the oracle's audio are written down here, so that any edit of the scene shows (the GPU figures in DESIGN section 2
    were measured on THIS scene)"""
    objs, evs = S.build(dense=scene["dense"])
    again = run_oracle(objs, evs, S.NB)
    assert np.array_equal(again["audio"], scene["want"]["audio"]) and np.array_equal(again["emitted"], scene["want"]["emitted"])
    for a, b in zip(again["state"], scene["want"]["state"]):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    pin = PINNED[scene["dense"]]
    peaks = np.abs(scene["want"]["audio"]).max(axis=1)
    assert len(evs) == pin["n_events"] and layout_digest(evs) == pin["digest"]
    np.testing.assert_allclose(peaks, pin["peaks"], rtol=1e-9)       # (the pins are written to eleven digits)
