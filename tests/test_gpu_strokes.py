"""Contact strokes as one script (pbso_enqueue_strokes) against the same entries through pbso_enqueue_force one by one.

Equality means np.array_equal on audio, emitted, every qnorm row and the final (q1, q2) state: both feeds hand the kernels the
same numbers, so there is no tolerance to choose.  The fast path (one record per object from the host, the per-buffer tables
from stroke_expand_kernel) is REQUIRED where every object is eligible: stroke_stats() must report every entry as taken
directly.  One-buffer steps keep the host path and engines with time_chunks forced take the fast path too; both are held to
equality only.  Against the oracle the bar is the one the project applies to dense-profile scenes, 5e-4 of peak."""
import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from tests.scenarios import B, ObjSpec, force_ev, rel_errors, run_oracle

pytestmark = pytest.mark.gpu
START, END, ZERO = capi.STROKE_START, capi.STROKE_END, capi.STROKE_ZERO
AR = capi.AUTOREGRESSIVE_FORCE
TOL_MAX = 5e-4


def _scene(sizes, seed):
    return [(synth.eigenvalues(m, seed + i), synth.mode_shapes(m, seed + i)) for i, m in enumerate(sizes)]


def _entries(n_obj, stamps_of, seed, end_at=None):
    """per object: a dummy start at its first stamp, a face entry per further stamp, optionally an end entry (face data) at end_at;
    returns a list of (obj, stamp, flags, vids, coords, vn) in object order"""
    rng = np.random.default_rng(seed)
    out = []
    for o in range(n_obj):
        st = list(stamps_of(o))
        for k, t in enumerate(st):
            bary = rng.random(3)
            bary /= bary.sum()
            vn = rng.standard_normal(3)
            vn /= np.linalg.norm(vn)
            fl = (START | ZERO) if k == 0 else 0
            out.append((o, int(t), fl, rng.integers(0, synth.N_VERTS, 3), bary, vn))
        if end_at is not None:
            vn = rng.standard_normal(3)
            out.append((o, int(end_at), END, rng.integers(0, synth.N_VERTS, 3), np.array([0.2, 0.3, 0.5]), vn / np.linalg.norm(vn)))
    return out


def _as_message(e, force_type):
    o, t, fl, vids, coords, vn = e
    if fl & ZERO:
        return ForceMessage(forceType=force_type, sustainedForceStart=bool(fl & START), sustainedForceEnd=bool(fl & END))
    return ForceMessage(forceType=force_type, sustainedForceStart=bool(fl & START), sustainedForceEnd=bool(fl & END),
                        vids=vids, coords=coords, vn=vn)


def _feed(eng, entries, strokes, force_type):
    if not entries:
        return
    if strokes:
        n = eng.enqueue_strokes([e[0] for e in entries], np.array([e[3] for e in entries]), np.array([e[4] for e in entries]),
                                np.array([e[5] for e in entries]), [e[1] for e in entries], np.array([e[2] for e in entries], dtype=np.uint8),
                                force_type)
        assert n == len(entries)
    else:
        for e in entries:
            assert eng.enqueue_force(e[0], _as_message(e, force_type), e[1])


def _run(scene, entries, split, strokes, force_type=AR, extra=None, busy=None, per_step=True, **engine_kw):
    """the steps of `split`, each fed its own entries just before it (per_step) or the whole script before the first step;
    extra(eng) adds other calls after finalize; busy: an object that gets a Gaussian message first"""
    eng = Engine(**engine_kw)
    try:
        for lam, shapes in scene:
            eng.add_object(lam, synth.RHO, synth.ALPHA, synth.BETA, mode_shapes=shapes)
        eng.finalize()
        for i in range(len(scene)):
            eng.set_use_transfer(i, False)
        if busy is not None:
            g = np.random.default_rng(5).standard_normal(len(scene[busy][0])) * 1e-3
            assert eng.enqueue_force(busy, ForceMessage(data=g, forceType=capi.GAUSSIAN_FORCE, gaussianWidth=1500.0), 0)
        if extra is not None:
            extra(eng)
        audio, emitted, qn = [], [], []
        done = 0
        if not per_step:
            _feed(eng, entries, strokes, force_type)
        for nb in split:
            if per_step:
                _feed(eng, [e for e in entries if done <= e[1] < done + nb], strokes, force_type)
            eng.step(nb)
            audio.append(eng.audio().copy())
            emitted.append(eng.emitted().copy())
            qn += [eng.qnorm(o, b).copy() for o in range(len(scene)) for b in range(nb)]
            done += nb
        return dict(audio=np.concatenate(audio, axis=1), emitted=np.concatenate(emitted, axis=1), qnorm=qn,
                    state=[eng.state(i) for i in range(len(scene))], stats=eng.stroke_stats(), info=eng.info())
    finally:
        eng.close()


def _assert_equal(a, b):
    assert np.array_equal(a["audio"], b["audio"])
    assert np.array_equal(a["emitted"], b["emitted"])
    assert len(a["qnorm"]) == len(b["qnorm"]) and all(np.array_equal(x, y) for x, y in zip(a["qnorm"], b["qnorm"]))
    for (p1, p2), (q1, q2) in zip(a["state"], b["state"]):
        assert np.array_equal(p1, q1) and np.array_equal(p2, q2)
    assert np.abs(a["audio"]).max() > 0


def _bench_shape(n_obj, nb):
    """dummy start at 0, one face entry per buffer, an end entry, a few free buffers behind it"""
    return _entries(n_obj, lambda o: range(0, nb - 5), 11, end_at=nb - 5)


def _gaps_and_bursts(n_obj, nb):
    """stamps with gaps (buffers that keep the old data row) and bursts (three entries on one stamp, consumed one per buffer);
    no burst spills over a multiple of 10 buffers, so steps of 10 see only their own entries"""
    base = [0, 1, 4, 4, 4, 8, 12, 13, 13, 13, 17, 20, 25, 25, 25, 29, 31, 36, 36, 36]
    return _entries(n_obj, lambda o: [t for t in base if t < nb], 12)


CASES = {
    "bench": (lambda: _scene([130] * 3, 900), lambda: _bench_shape(3, 24), [24]),
    "bench_split": (lambda: _scene([130] * 3, 900), lambda: _bench_shape(3, 60), [1, 7, 40, 12]),
    "gaps_bursts": (lambda: _scene([130] * 2, 910), lambda: _gaps_and_bursts(2, 40), [10, 10, 10, 10]),
    "mixed_sizes": (lambda: _scene([64, 512, 4096], 920), lambda: _bench_shape(3, 16), [8, 8]),
}


@pytest.mark.parametrize("form", [capi.FORM_BLOCK, capi.FORM_VELOCITY])
@pytest.mark.parametrize("case", sorted(CASES))
def test_stroke_script_equals_message_by_message(case, form):
    scene, entries, split = (f() if callable(f) else f for f in CASES[case])
    a = _run(scene, entries, split, True, form=form)
    b = _run(scene, entries, split, False, form=form)
    _assert_equal(a, b)
    assert b["stats"] == dict(direct=0, queued=0, dropped=0, kernel_launches=0)


@pytest.mark.parametrize("opts", ["submit_thread=1", "time_chunks=2", "chunk_buffers=5"])
@pytest.mark.parametrize("case", ["bench", "gaps_bursts", "mixed_sizes"])
def test_stroke_script_equals_messages_on_pinned_paths(case, opts, monkeypatch):
    """the second submitting thread, time chunks forced on, launches shorter than the step (the stroke cut over several launches)"""
    monkeypatch.setenv("PBSO_ENGINE_OPTS", opts)
    scene, entries, split = (f() if callable(f) else f for f in CASES[case])
    _assert_equal(_run(scene, entries, split, True), _run(scene, entries, split, False))


def test_whole_script_before_the_first_step_and_ar_parameters_mid_stroke():
    """the script handed over once, stepped in pieces (entries beyond a step wait in the queue), and an AR-parameter message stamped
    mid-stroke; parameters already in the slot when the stroke starts"""
    scene, entries = _scene([130] * 2, 930), _bench_shape(2, 30)

    def extra(eng):
        eng.enqueue_arprm(0, [0.5, 0.3], 0.004, 0.2, 0)
        eng.enqueue_arprm(1, [0.6, 0.2], 0.003, 0.1, 9)

    for per_step in (True, False):
        a = _run(scene, entries, [6, 10, 14], True, extra=extra, per_step=per_step)
        b = _run(scene, entries, [6, 10, 14], False, extra=extra, per_step=per_step)
        _assert_equal(a, b)


def test_point_force_face_hits_without_sustained_flags():
    scene = _scene([130] * 2, 940)
    entries = [(o, t, 0, v, c, n) for (o, t, _, v, c, n) in _gaps_and_bursts(2, 20)]
    a = _run(scene, entries, [20], True, force_type=capi.POINT_FORCE)
    b = _run(scene, entries, [20], False, force_type=capi.POINT_FORCE)
    _assert_equal(a, b)


@pytest.mark.parametrize("engine_kw", [dict(form=capi.FORM_BLOCK), dict(form=capi.FORM_VELOCITY), dict(submit_thread=1)])
@pytest.mark.parametrize("case", ["bench", "gaps_bursts", "mixed_sizes"])
def test_the_fast_path_ran(case, engine_kw):
    """every object of these cases is eligible in every step (steps of at least two buffers): all entries direct, none queued or
    dropped, at least one stroke-kernel launch per step -- a silent fall-back fails here"""
    scene, entries, split = (f() if callable(f) else f for f in CASES[case])
    a = _run(scene, entries, split, True, **engine_kw)
    assert a["stats"]["direct"] == len(entries) and a["stats"]["queued"] == 0 and a["stats"]["dropped"] == 0, a["stats"]
    assert a["stats"]["kernel_launches"] >= len(split), a["stats"]
    _assert_equal(a, _run(scene, entries, split, False, **engine_kw))


def test_fallback_is_the_same_audio():
    """object 1 has a Gaussian message in its queue: its entries take the queue, the others the records"""
    scene, entries = _scene([130] * 3, 950), _bench_shape(3, 20)
    a = _run(scene, entries, [20], True, busy=1)
    b = _run(scene, entries, [20], False, busy=1)
    _assert_equal(a, b)
    per_obj = len(entries) // 3
    assert a["stats"]["queued"] == per_obj and a["stats"]["direct"] == 2 * per_obj and a["stats"]["dropped"] == 0, a["stats"]


@pytest.mark.parametrize("case", ["bench", "gaps_bursts"])
def test_against_the_oracle(case):
    scene, entries, split = (f() if callable(f) else f for f in CASES[case])
    nb = sum(split)
    got = _run(scene, entries, split, True)
    objs = [ObjSpec(lam, shapes=shapes) for lam, shapes in scene]
    evs = [dict(t=0, obj=i, kind="use_transfer", use=False) for i in range(len(scene))]
    for o, t, fl, vids, coords, vn in entries:
        if fl & ZERO:
            evs.append(force_ev(t, o, force_type=2, start=bool(fl & START), end=bool(fl & END)))
        else:
            evs.append(force_ev(t, o, vids=vids, coords=coords, vn=vn, force_type=2, start=bool(fl & START), end=bool(fl & END)))
    want = run_oracle(objs, evs, nb)
    mx, l2 = rel_errors(got["audio"], want["audio"])
    print(f"strokes vs oracle ({case}): max|gpu - oracle| / peak = {mx.max():.3e}, relative L2 = {l2.max():.3e}")
    assert np.array_equal(got["emitted"], want["emitted"])
    assert (mx <= TOL_MAX).all(), mx


def test_overflow_and_validation():
    scene = _scene([130] * 2, 960)
    n = 1100
    rng = np.random.default_rng(3)
    vids, coords, vns = rng.integers(0, synth.N_VERTS, (n, 3)), np.full((n, 3), 1.0 / 3), synth.unit_normals(n, 4)
    with Engine() as eng:
        with pytest.raises(PbsoError) as ei:                                    # before finalize
            eng.enqueue_strokes([0], vids[:1], coords[:1], vns[:1], [0])
        assert ei.value.status == capi.ERR_STATE
        for lam, shapes in scene:
            eng.add_object(lam, synth.RHO, synth.ALPHA, synth.BETA, mode_shapes=shapes)
        eng.add_object(scene[0][0], synth.RHO, synth.ALPHA, synth.BETA)          # object 2: no mode shapes
        eng.finalize()
        for i in range(3):
            eng.set_use_transfer(i, False)
        for bad in (lambda: eng.enqueue_strokes([1, 0], vids[:2], coords[:2], vns[:2], [0, 0]),              # descending ids
                    lambda: eng.enqueue_strokes([0], [[0, 1, synth.N_VERTS]], coords[:1], vns[:1], [0]),     # vertex id beyond n_dof / 3
                    lambda: eng.enqueue_strokes([2], vids[:1], coords[:1], vns[:1], [0]),                    # no mode shapes
                    lambda: eng.enqueue_strokes([0], vids[:1], coords[:1], vns[:1], [0], force_type=capi.GAUSSIAN_FORCE)):
            with pytest.raises(PbsoError) as ei:
                bad()
            assert ei.value.status == capi.ERR_INVALID
        # a busy object (a Gaussian message in its queue) and more entries than its queue holds: the surplus is dropped and counted
        g = rng.standard_normal(130) * 1e-3
        assert eng.enqueue_force(0, ForceMessage(data=g, forceType=capi.GAUSSIAN_FORCE, gaussianWidth=1500.0), 0)
        flags = np.zeros(n, dtype=np.uint8)
        flags[0] = START
        assert eng.enqueue_strokes(np.zeros(n, dtype=np.int32), vids, coords, vns, np.arange(n), flags) == n
        for second in (lambda: eng.enqueue_strokes([1], vids[:1], coords[:1], vns[:1], [0]),
                       lambda: eng.enqueue_vertex_hits([1], [3], vns[:1], [0])):
            with pytest.raises(PbsoError) as ei:                                # one script per step, of either kind
                second()
            assert ei.value.status == capi.ERR_STATE
        eng.step(4)
        stats, info = eng.stroke_stats(), eng.info()
        assert stats["dropped"] == n - 1022 == info["total_dropped_hits"] and stats["queued"] == 1022 and stats["direct"] == 0, (stats, info)


def test_a_stroke_interrupted_by_clear_all_fails_like_the_message_feed():
    """sustained, but the force list emptied by a clearAllForces message: the next data message makes pbso_step return
    PBSO_ERR_ASSERT ("sustained force list is empty") -- the same status from the same step when that entry comes as a stroke"""
    scene = _scene([130], 970)
    ents = _entries(1, lambda o: range(0, 4), 13)
    late = _entries(1, lambda o: [4, 5], 14)[1:]          # a data entry for the buffer right behind the clearAllForces message
    status = []
    for strokes in (True, False):
        with Engine() as eng:
            eng.add_object(scene[0][0], synth.RHO, synth.ALPHA, synth.BETA, mode_shapes=scene[0][1])
            eng.finalize()
            eng.set_use_transfer(0, False)
            _feed(eng, ents, strokes, AR)
            eng.step(4)
            assert eng.enqueue_force(0, ForceMessage(clearAllForces=True), 4)
            eng.step(1)                                      # (the clearing step returns early: nothing is asserted in it)
            _feed(eng, late, strokes, AR)
            with pytest.raises(PbsoError) as ei:
                eng.step(4)
            status.append(ei.value.status)
            assert "sustained force list is empty" in str(ei.value)
    assert status == [capi.ERR_ASSERT, capi.ERR_ASSERT]
