"""Track forces (pbso_track_create / pbso_enqueue_track_force) on the device against the fp64 model of tests/track_model.py,
which tests/test_track_model.py anchors to the C oracle.

Tolerance against the model: the bar the project states for dense-profile scenes and test_gpu_strokes.py
uses -- max |d| <= 5e-4 of peak and relative L2 <= 1e-3 -- for audio, qnorm rows and the final state.  Where a test says EQUAL it
means np.array_equal on audio, emitted, every qnorm row and the state: both runs hand the kernels the same numbers."""
import functools

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from tests.scenarios import B, ObjSpec, force_ev, rel_errors, run_oracle
from tests.track_model import EngineRefused, run_engine, run_model, track_ev

pytestmark = pytest.mark.gpu
TOL_MAX, TOL_L2 = 5e-4, 1e-3
START, END, ZERO = capi.STROKE_START, capi.STROKE_END, capi.STROKE_ZERO


# ---------------------------------------------------------------------------
def _unit(n):
    return [dict(t=0, obj=i, kind="use_transfer", use=False) for i in range(n)]


def _hit(rng, kind, n_modes):
    """the spatial part of a message: vertex / face / explicit data"""
    vn = rng.standard_normal(3)
    vn /= np.linalg.norm(vn)
    if kind == "vertex":
        return dict(vid=int(rng.integers(0, synth.N_VERTS)), vn=vn)
    if kind == "face":
        bary = rng.random(3)
        return dict(vids=rng.integers(0, synth.N_VERTS, 3), coords=bary / bary.sum(), vn=vn)
    return dict(data=rng.standard_normal(n_modes) * 1e-3)


def _check(got, want, what, only=None):
    """tolerance on audio, qnorm rows and the final state; prints the figures before it asserts"""
    ids = list(range(len(want["state"]))) if only is None else list(only)
    ga = got["audio"][ids]
    assert np.isfinite(ga).all()
    assert np.array_equal(got["emitted"][ids], want["emitted"])
    mx, l2 = rel_errors(ga, want["audio"])
    qerr = 0.0
    for (k, b), w in want["qnorm"].items():
        if (ids[k], b) in got["qnorm"]:
            qerr = max(qerr, np.abs(got["qnorm"][(ids[k], b)] - w).max() / max(np.abs(w).max(), 1e-30))
    serr = 0.0
    for k, (w1, w2) in enumerate(want["state"]):
        g1, g2 = got["state"][ids[k]]
        scale = max(np.abs(w1).max(), 1e-300)
        serr = max(serr, np.abs(g1 - w1).max() / scale, np.abs(g2 - w2).max() / scale)
    print(f"{what}: audio max|d|/peak {mx.max():.3e}, relative L2 {l2.max():.3e}; qnorm rows {qerr:.3e}; state {serr:.3e}")
    assert np.abs(want["audio"]).max() > 0
    assert (mx <= TOL_MAX).all(), (what, mx)
    assert (l2 <= TOL_L2).all(), (what, l2)
    assert qerr <= TOL_MAX, (what, qerr)
    assert serr <= TOL_MAX, (what, serr)
    return mx.max(), l2.max()


def _assert_equal(a, b, only=None):
    ids = slice(None) if only is None else list(only)
    assert np.array_equal(a["audio"][ids], b["audio"][ids])
    assert np.array_equal(a["emitted"][ids], b["emitted"][ids])
    keys = [k for k in a["qnorm"] if only is None or k[0] in only]
    assert len(a["qnorm"]) == len(b["qnorm"]) and all(np.array_equal(a["qnorm"][k], b["qnorm"][k]) for k in keys)
    for i, ((p1, p2), (q1, q2)) in enumerate(zip(a["state"], b["state"])):
        if only is None or i in only:
            assert np.array_equal(p1, q1) and np.array_equal(p2, q2)
    assert np.abs(a["audio"][ids]).max() > 0


def _engine(objs, tracks, evs, split, **kw):
    try:
        return run_engine(objs, tracks, evs, split, **kw)
    except EngineRefused as e:
        pytest.skip(f"the engine refuses this combination: {e}")


# ---------------------------------------------------------------------------
# 1. random tracks, rate 1, integral first: every form and every path a dense row can take
@functools.lru_cache(maxsize=None)
def _scene1():
    rng = np.random.default_rng(1201)
    sizes = [64, 130, 512, 1024, 4096]
    kinds = ["explicit", "vertex", "face", "vertex", "explicit"]
    objs = []
    for i, m in enumerate(sizes):
        lam = synth.eigenvalues(m, 1201 + i)
        maps = synth.ffat_maps(lam, 1300 + i, dim=8) if i in (1, 2) else None
        objs.append(ObjSpec(lam, shapes=synth.mode_shapes(m, 1201 + i), maps=maps))
    tracks = [rng.standard_normal(int(n)).astype(np.float32) for n in (300, 777, 1500, 2600, 5000)]
    evs = []
    for i in range(len(sizes)):
        if objs[i].maps is None:
            evs.append(dict(t=0, obj=i, kind="use_transfer", use=False))
        else:
            evs.append(dict(t=0, obj=i, kind="listener", pos=[0.31 + 0.05 * i, -0.22, 0.27]))
        for j, t in enumerate((1 + i % 3, 9 + i, 17)):
            trk = int(rng.integers(0, len(tracks)))
            evs.append(track_ev(t, i, trk, first=float(rng.integers(0, 200)), start_sample=int(rng.integers(0, B)) if j else 0,
                                **_hit(rng, kinds[i], sizes[i])))
    nb = 24
    want = run_model(objs, tracks, evs, nb, per_sample=False)
    return objs, tracks, evs, nb, want


PATHS = {
    "default": {},
    "time_chunks_1": dict(time_chunks=1),
    "time_chunks_3": dict(time_chunks=3),
    "pipe_4": dict(bank_kernel=capi.BANK_PIPE, pipe_consumers=4),
    "pipe_2": dict(bank_kernel=capi.BANK_PIPE, pipe_consumers=2),
    "dense_launches_2": dict(dense_launches=2),
    "forced_block_off": dict(forced_block=-1),
    "submit_thread": dict(submit_thread=1),
}
FORMS = {"block": capi.FORM_BLOCK, "block_bf16": capi.FORM_BLOCK_BF16, "velocity": capi.FORM_VELOCITY}


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("form", sorted(FORMS))
def test_random_tracks_against_the_model_on_every_path(form, path):
    objs, tracks, evs, nb, want = _scene1()
    got = _engine(objs, tracks, evs, [nb], form=FORMS[form], qnorm=capi.QNORM_ALL, **PATHS[path])
    _check(got, want, f"random tracks, {form}, {path}")
    assert got["track_stats"][0] == len(tracks) and got["track_stats"][1] == sum(len(t) for t in tracks)
    assert got["track_stats"][2] == 15 and got["track_stats"][3] == want["track_rows"], (got["track_stats"], want["track_rows"])


@pytest.mark.parametrize("form", sorted(FORMS))
def test_random_tracks_without_qnorm_rows(form):
    objs, tracks, evs, nb, want = _scene1()
    got = _engine(objs, tracks, evs, [nb], form=FORMS[form], qnorm=capi.QNORM_OFF)
    _check(got, want, f"random tracks, {form}, qnorm off")


# ---------------------------------------------------------------------------
# 2. fractional first, rates, gains, loop, n_samples shorter and longer than the track, start samples
@functools.lru_cache(maxsize=None)
def _scene2():
    rng = np.random.default_rng(1202)
    tracks = [rng.standard_normal(int(n)).astype(np.float32) for n in (300, 901, 2000)]
    combos = [(rate, loop, ns, s) for rate in (0.37, 1.0, 2.5) for loop in (False, True) for ns in ("short", "long", 0)
              for s in (0, 1, 256, 512)]
    objs, evs = [], []
    for i, (rate, loop, ns, s) in enumerate(combos):
        m = 64 + 2 * (i % 34)
        objs.append(ObjSpec(synth.eigenvalues(m, 2000 + i), shapes=synth.mode_shapes(m, 2000 + i)))
        trk = i % len(tracks)
        played = len(tracks[trk]) / rate                    # output samples until the read position leaves the track
        n_samples = {"short": max(2, int(0.4 * played)), "long": int(1.7 * played) + 3, 0: 0}[ns]
        evs.append(track_ev(1 + i % 2, i, trk, first=float(rng.random() * 40.0), rate=rate, gain=float(0.25 + 1.5 * rng.random()) * (-1) ** i,
                            n_samples=n_samples, start_sample=s, loop=loop, **_hit(rng, ("vertex", "face", "explicit")[i % 3], m)))
    nb = 14
    evs += _unit(len(objs))
    return objs, tracks, evs, nb, run_model(objs, tracks, evs, nb, per_sample=False)


def test_rates_gains_loops_lengths_and_start_samples():
    objs, tracks, evs, nb, want = _scene2()
    got = _engine(objs, tracks, evs, [nb])
    _check(got, want, "rates / gains / loop / n_samples / start_sample")
    assert got["track_stats"][2] == len(objs)
    assert got["track_stats"][3] == want["track_rows"], (got["track_stats"], want["track_rows"])


# ---------------------------------------------------------------------------
# 3. + 4.  sample-accurate onsets; the two oracle equivalences on the device
def _delta_case():
    m = 130
    lam = synth.eigenvalues(m, 1203)
    objs = [ObjSpec(lam, shapes=synth.mode_shapes(m, 1203))]
    hit = dict(vid=7, vn=synth.unit_normals(1, 1203)[0])
    return objs, hit


@pytest.mark.parametrize("s", [0, 1, 17, 256, 512])
def test_one_sample_track_is_a_hit_at_that_sample(s):
    """against the engine's own PointForce run delayed by s samples, and against the oracle's (audio only, transfer off);
    s = 0: the delta track against the oracle's PointForce"""
    objs, hit = _delta_case()
    nb = 5
    point = _unit(1) + [force_ev(1, 0, **hit)]
    got = _engine(objs, [np.array([1.0], dtype=np.float32)], _unit(1) + [track_ev(1, 0, 0, start_sample=s, **hit)], [nb])
    own = _engine(objs, [], point, [nb], direct_hits=-1)["audio"][0].astype(np.float64)
    want = run_oracle(objs, point, nb)["audio"][0]
    for name, ref in (("the engine's PointForce", own), ("the oracle's PointForce", want)):
        delayed = np.concatenate([np.zeros(s), ref[:nb * B - s]])[None]
        mx, l2 = rel_errors(got["audio"], delayed)
        print(f"delta track at start_sample {s} against {name} delayed: max|d|/peak {mx.max():.3e}, relative L2 {l2.max():.3e}")
        assert (mx <= TOL_MAX).all() and (l2 <= TOL_L2).all(), (name, mx, l2)
    assert got["track_stats"][2:] == (1, 1)


def _stroke_case(nb=12):
    m, mu = 130, 0.140625
    lam = synth.eigenvalues(m, 1204)
    objs = [ObjSpec(lam, shapes=synth.mode_shapes(m, 1204))]
    rng = np.random.default_rng(1204)
    faces = [_hit(rng, "face", m) for _ in range(nb - 4)]

    def script(first, **kw):
        evs = [first(0, start=True)]
        evs += [force_ev(1 + k, 0, **f, **kw) for k, f in enumerate(faces)]
        return evs + [force_ev(nb - 3, 0, end=True, **kw)]
    ar = _unit(1) + [dict(t=0, obj=0, kind="arprm", a=[0.783, 0.116], sigma=0.0, mu=mu)]
    ar += script(lambda t, **k: force_ev(t, 0, force_type=2, **k), force_type=2)
    tr = _unit(1) + script(lambda t, **k: track_ev(t, 0, 0, loop=True, **k))
    return objs, [np.array([mu], dtype=np.float32)], ar, tr, nb


def test_constant_looping_track_is_the_ar_force_with_sigma_zero():
    """against the oracle's AR(sigma = 0) stroke within the tolerance, and EQUAL to the engine's own AR(sigma = 0) run of the same
    script: both hand the bank the same f32 rows"""
    objs, tracks, ar, tr, nb = _stroke_case()
    want = run_oracle(objs, ar, nb)
    got = _engine(objs, tracks, tr, [nb])
    _check(got, want, "constant looping track against the oracle's AR(sigma = 0)")

    def feed_ar(eng, ids):
        eng.enqueue_arprm(0, [0.783, 0.116], 0.0, 0.140625, 0)
    own = _engine(objs, [], [e for e in ar if e["kind"] != "arprm"], [nb], extra=feed_ar)
    _assert_equal(got, own)


# ---------------------------------------------------------------------------
# 5. every producer of rows gives the same row
def _scene5(with_ar):
    rng = np.random.default_rng(1205)
    sizes = [130, 64, 512]
    objs = [ObjSpec(synth.eigenvalues(m, 1500 + i), shapes=synth.mode_shapes(m, 1500 + i)) for i, m in enumerate(sizes)]
    tracks = [rng.standard_normal(n).astype(np.float32) for n in (1400, 3100)]
    evs = _unit(3)
    # live samples reach beyond sample 0 in every buffer they touch: plays of fixed lengths that end mid-buffer
    evs.append(track_ev(0, 0, 0, first=3.25, rate=0.81, gain=1.7, n_samples=3 * B + 100, start_sample=40, **_hit(rng, "face", 130)))
    evs.append(force_ev(2, 0, **_hit(rng, "vertex", 130)))                                     # a PointForce hit beside it
    evs.append(track_ev(5, 0, 1, first=0.5, rate=2.5, gain=-0.6, n_samples=2 * B + 7, start_sample=500, **_hit(rng, "explicit", 130)))
    evs.append(track_ev(1, 2, 1, rate=1.0, loop=True, n_samples=6 * B + 250, start_sample=256, **_hit(rng, "vertex", 512)))
    if with_ar:                                             # an AR stroke on object 1: the launches have AR uses
        evs.append(force_ev(0, 1, force_type=2, start=True))
        evs += [force_ev(t, 1, force_type=2, **_hit(rng, "face", 64)) for t in range(1, 9)]
        evs.append(force_ev(9, 1, force_type=2, end=True))
    else:
        evs.append(track_ev(3, 1, 0, first=10.0, rate=0.37, n_samples=4 * B + 31, **_hit(rng, "face", 64)))
    return objs, tracks, evs, 12


PIN = dict(bank_kernel=capi.BANK_BLOCK, time_chunks=-1)     # one bank path whatever K2 form runs (the policy looks at it)
PRODUCERS = {
    "rows": {},
    "chain": dict(profile_kernel=1),
    "chain_serial": dict(profile_kernel=2),
    "margin_50": dict(profile_margin_pct=50),
    "host": dict(device_profiles=-1),
    "no_fusion": dict(fuse_short_launches=-1),
}


@pytest.mark.parametrize("split", ["one_step", "one_buffer_steps"])
def test_every_producer_of_rows_gives_the_same_row(split):
    objs, tracks, evs, nb = _scene5(False)
    cut = [nb] if split == "one_step" else [1] * nb
    base = _engine(objs, tracks, evs, cut, **PIN)
    _check(base, run_model(objs, tracks, evs, nb, per_sample=False), f"producers scene, {split}")
    for name, kw in PRODUCERS.items():
        if name == "rows":
            continue
        other = _engine(objs, tracks, evs, cut, **PIN, **kw)
        _assert_equal(base, other)
        assert other["track_stats"] == base["track_stats"], name


def test_fused_and_combined_kernels_give_the_same_row():
    """one-buffer steps with an AR stroke on another object of the launch (the launch has AR uses: the fused + combine kernel)
    against the separate kernels; the track objects also against the chain kernel and the host profiles (whose AR rows differ
    from the row-parallel form's in the last place, by design)"""
    objs, tracks, evs, nb = _scene5(True)
    base = _engine(objs, tracks, evs, [1] * nb, **PIN)
    _assert_equal(base, _engine(objs, tracks, evs, [1] * nb, fuse_short_launches=-1, **PIN))
    _assert_equal(base, _engine(objs, tracks, evs, [1] * nb, profile_margin_pct=50, **PIN))
    for kw in (dict(profile_kernel=1), dict(profile_kernel=2), dict(device_profiles=-1)):
        _assert_equal(base, _engine(objs, tracks, evs, [1] * nb, **PIN, **kw), only=[0, 2])


def test_a_row_whose_only_live_sample_is_sample_zero():
    """the corner the producers may take differently (an impulse descriptor on the host path, a dense row on the device path):
    within the tolerance of the model on both"""
    objs, hit = _delta_case()
    tracks = [np.array([0.75], dtype=np.float32)]
    evs = _unit(1) + [track_ev(1, 0, 0, **hit)]
    want = run_model(objs, tracks, evs, 4)
    for kw in ({}, dict(device_profiles=-1)):
        _check(_engine(objs, tracks, evs, [4], **kw), want, f"one sample at sample 0, {kw}")


# ---------------------------------------------------------------------------
# 6. step cuts
@pytest.mark.parametrize("pinned", [False, True])
def test_step_cuts_and_feeding_orders(pinned):
    objs, tracks, evs, nb, want = _scene1()
    kw = dict(time_chunks=1) if pinned else {}
    runs = []
    for cut in ([24], [1] * 24, [5, 7, 12]):
        for per_step in (False, True):
            got = _engine(objs, tracks, evs, cut, per_step=per_step, **kw)
            _check(got, want, f"cut {cut if len(cut) < 5 else '[1] * 24'}, fed {'step by step' if per_step else 'before the first step'}, {kw}")
            runs.append(got)
    if pinned:
        for other in runs[1:]:
            _assert_equal(runs[0], other)


# ---------------------------------------------------------------------------
# 7. bookkeeping
def test_bookkeeping_against_the_model():
    rng = np.random.default_rng(1207)
    m = 96
    n_obj = 6
    objs = [ObjSpec(synth.eigenvalues(m, 1700 + i), shapes=synth.mode_shapes(m, 1700 + i)) for i in range(n_obj)]
    tracks = [rng.standard_normal(n).astype(np.float32) for n in (900, 1300, 200)]
    h = lambda kind="vertex": _hit(rng, kind, m)                                                    # noqa: E731
    evs = _unit(n_obj)
    # 0: a track and a Gaussian alive in one buffer (the product of sums), then two tracks at once
    evs += [track_ev(1, 0, 0, rate=0.9, **h()), force_ev(2, 0, force_type=1, width=3000.0, **h("face")),
            track_ev(6, 0, 1, start_sample=100, **h("explicit")), track_ev(7, 0, 0, first=5.5, gain=0.5, start_sample=7, **h())]
    # 1: a track cut short by clearAllForces (no buffer emitted), a hit afterwards
    evs += [track_ev(1, 1, 1, **h()), force_ev(3, 1, clear=True), force_ev(5, 1, **h())]
    # 2: a track removed by a sustainedForceStart; the sustained force a looping track, its data replaced by face messages, ended
    evs += [track_ev(0, 2, 0, loop=True, **h()), track_ev(2, 2, 1, loop=True, rate=1.3, start=True)]
    evs += [track_ev(t, 2, 2, gain=9.0, **h("face")) for t in range(3, 9)]                      # (their play records are dropped)
    evs += [force_ev(9, 2, end=True, **h("face"))]
    # 3: an exhausted track under sustained contact: silence, the force still in the list, data messages keep arriving
    evs += [track_ev(1, 3, 2, start=True, start_sample=300, **h())] + [force_ev(t, 3, **h("face")) for t in (2, 3, 4, 5)]
    evs += [force_ev(8, 3, end=True), force_ev(10, 3, **h())]
    # 4: a zero-length play is rejected at once (first beyond the track), a hit in the same buffer's successor
    evs += [track_ev(1, 4, 2, first=200.0, **h()), force_ev(2, 4, **h())]
    # 5: n_samples beyond the track without loop: zeros, alive until N
    evs += [track_ev(1, 5, 2, n_samples=3 * B, **h()), force_ev(3, 5, **h("face"))]
    nb = 13
    want = run_model(objs, tracks, evs, nb)
    assert not want["emitted"].all()
    for kw in ({}, dict(device_profiles=-1), dict(time_chunks=2)):
        got = _engine(objs, tracks, evs, [nb], **kw)
        _check(got, want, f"bookkeeping, {kw}")
        assert got["track_stats"][3] == want["track_rows"], (kw, got["track_stats"], want["track_rows"])


def test_a_track_message_behind_a_full_queue_is_refused():
    objs, hit = _delta_case()
    tracks = [np.ones(10, dtype=np.float32)]
    evs = _unit(1) + [force_ev(2, 0, **hit) for _ in range(1023)] + [track_ev(2, 0, 0, **hit)]
    got = _engine(objs, tracks, evs, [4])
    want = run_model(objs, tracks, evs, 4)
    assert got["accepted"] == [True] + want["accepted"][0] and want["accepted"][0][-1] is False and all(want["accepted"][0][:-1])
    _check(got, want, "a full queue")
    assert got["track_stats"][2:] == (0, 0)


def test_strokes_on_an_object_with_a_live_track_force_go_through_the_queue():
    m = 130
    objs = [ObjSpec(synth.eigenvalues(m, 1208 + i), shapes=synth.mode_shapes(m, 1208 + i)) for i in range(2)]
    rng = np.random.default_rng(1208)
    tracks = [rng.standard_normal(4000).astype(np.float32)]
    nb = 10
    entries = []                                            # (obj, stamp, flags, vids, coords, vn): a stroke on both objects
    for o in range(2):
        for k, t in enumerate(range(2, 8)):
            bary = rng.random(3)
            entries.append((o, t, (START | ZERO) if k == 0 else (END if t == 7 else 0), rng.integers(0, synth.N_VERTS, 3), bary / bary.sum(),
                            synth.unit_normals(1, 50 + t)[0]))
    hit = _hit(rng, "vertex", m)

    def run(strokes):
        def extra(eng, ids):
            assert eng.enqueue_track_force(1, ForceMessage(**hit), ids[0], rate=0.7)      # object 1: a live track force from buffer 0 on
            if strokes:
                eng.enqueue_strokes([e[0] for e in entries], np.array([e[3] for e in entries]), np.array([e[4] for e in entries]),
                                    np.array([e[5] for e in entries]), [e[1] for e in entries],
                                    np.array([e[2] for e in entries], dtype=np.uint8), capi.AUTOREGRESSIVE_FORCE)
            else:
                for o, t, fl, vids, coords, vn in entries:
                    kw = {} if fl & ZERO else dict(vids=vids, coords=coords, vn=vn)
                    assert eng.enqueue_force(o, ForceMessage(forceType=2, sustainedForceStart=bool(fl & START),
                                                             sustainedForceEnd=bool(fl & END), **kw), t)
        return _engine(objs, tracks, _unit(2), [nb], extra=extra)
    a, b = run(True), run(False)
    _assert_equal(a, b)
    per_obj = len(entries) // 2
    assert a["stroke_stats"]["queued"] == per_obj and a["stroke_stats"]["direct"] == per_obj, a["stroke_stats"]


# ---------------------------------------------------------------------------
# 8. validation
def test_validation():
    m = 64
    lam = synth.eigenvalues(m, 1209)
    msg = ForceMessage(vid=3, vn=[0.0, 0.0, 1.0])
    with Engine() as eng:
        eng.add_object(lam, synth.RHO, synth.ALPHA, synth.BETA, mode_shapes=synth.mode_shapes(m, 1209))
        trk = eng.create_track(np.linspace(-1, 1, 500))               # before finalize
        assert trk == 0
        with pytest.raises(PbsoError) as ei:
            eng.enqueue_track_force(0, msg, trk)
        assert ei.value.status == capi.ERR_STATE
        eng.finalize()
        eng.set_use_transfer(0, False)
        assert eng.create_track(np.ones(3)) == 1                      # ... and after
        bad_tracks = (np.array([0.0, np.nan, 1.0]), np.array([np.inf]), np.zeros(0))
        for t in bad_tracks:
            with pytest.raises(PbsoError) as ei:
                eng.create_track(t)
            assert ei.value.status == capi.ERR_INVALID
        assert eng.track_stats()[:2] == (2, 503)
        bad = dict(track=[dict(track=2), dict(track=-1)], start_sample=[dict(start_sample=-1), dict(start_sample=513)],
                   n_samples=[dict(n_samples=-1)], first=[dict(first=-0.5), dict(first=float("nan")), dict(first=float("inf"))],
                   rate=[dict(rate=0.0), dict(rate=-1.0), dict(rate=float("nan")), dict(rate=float("inf"))],
                   gain=[dict(gain=float("nan")), dict(gain=float("inf"))])
        for field, cases in bad.items():
            for kw in cases:
                args = dict(track=trk)
                args.update(kw)
                with pytest.raises(PbsoError) as ei:
                    eng.enqueue_track_force(0, msg, **args)
                assert ei.value.status == capi.ERR_INVALID and field in str(ei.value), (kw, str(ei.value))
        cm = msg.to_c()
        cm.force_type = capi.TRACK_FORCE
        import ctypes as C
        lib = capi.lib()
        assert lib.pbso_enqueue_force(eng._h, 0, C.byref(cm), 0) == capi.ERR_INVALID          # a track force without a play record
        play = capi.TrackPlay(trk, 0, 0, 7, 0, 0.0, 1.0, 1.0)
        assert lib.pbso_enqueue_track_force(eng._h, 0, C.byref(cm), C.byref(play), 0) == capi.ERR_INVALID and \
            b"reserved" in lib.pbso_last_error(eng._h)
        cm.force_type = capi.POINT_FORCE
        play.reserved = 0
        assert lib.pbso_enqueue_track_force(eng._h, 0, C.byref(cm), C.byref(play), 0) == capi.ERR_INVALID
        # ... and the engine still steps
        assert eng.enqueue_track_force(0, msg, trk, rate=0.5, gain=2.0)
        eng.step(3)
        assert np.isfinite(eng.audio()).all() and np.abs(eng.audio()).max() > 0
        assert eng.track_stats() == (2, 503, 1, 2)                                               # 500 / 0.5 = 1000 samples: two buffers


# ---------------------------------------------------------------------------
# 9. size
def test_128_objects_under_sustained_looping_tracks_and_a_track_created_between_steps():
    n_obj, m, nb = 128, 512, 86
    rng = np.random.default_rng(1210)
    objs = [ObjSpec(synth.eigenvalues(m, 3000 + i), shapes=synth.mode_shapes(m, 3000 + i)) for i in range(n_obj)]
    tracks = [(0.142 + 0.05 * rng.standard_normal(int(rng.integers(300, 5000)))).astype(np.float32) for _ in range(n_obj)]
    evs = _unit(n_obj)
    for i in range(n_obj):
        evs.append(track_ev(0, i, i, loop=True, rate=0.5 + 1.5 * float(rng.random()), first=float(rng.random() * 100), start=True))
        evs += [force_ev(t, i, **_hit(rng, "face", m)) for t in range(1, nb, 1 + i % 4)]
    sampled = [0, 17, 31, 64, 65, 99, 126, 127]
    want = run_model(objs, tracks, evs, nb, only=sampled, per_sample=False)
    late = (0.3 * rng.standard_normal(1000)).astype(np.float32)
    out = {}

    def second_step(eng, ids):
        eng.step(nb)
        out["audio"], out["emitted"] = eng.audio().copy(), eng.emitted().copy()
        out["state"] = [eng.state(i) for i in range(n_obj)]
        out["rows"] = eng.track_stats()[3]
        tid = eng.create_track(late)                          # created between two steps, used in the next one
        assert tid == n_obj
        for i in sampled:
            assert eng.enqueue_force(i, ForceMessage(sustainedForceEnd=True))
        assert eng.enqueue_track_force(5, ForceMessage(sustainedForceEnd=True), tid)
        assert eng.enqueue_track_force(5, ForceMessage(**_hit(np.random.default_rng(5), "vertex", m)), tid, rate=1.25, start_sample=33)
    tail = _engine(objs, tracks, evs, [3], extra=second_step, qnorm=capi.QNORM_OFF)
    got = dict(audio=out["audio"], emitted=out["emitted"].astype(bool), qnorm={}, state=out["state"])
    _check(got, want, "128 x 512 x 86 under sustained looping tracks", only=sampled)
    assert out["emitted"].all() and out["rows"] == n_obj * nb
    # the three buffers behind it: object 5 plays the late track (against the model continued from the first step's script)
    evs2 = evs + [force_ev(nb, 5, end=True), track_ev(nb, 5, n_obj, rate=1.25, start_sample=33, **_hit(np.random.default_rng(5), "vertex", m))]
    want2 = run_model(objs, tracks + [late], evs2, nb + 3, only=[5], per_sample=False)
    mx, l2 = rel_errors(tail["audio"][5:6], want2["audio"][:, nb * B:])
    print(f"a track created between two steps: max|d|/peak {mx.max():.3e}, relative L2 {l2.max():.3e}")
    assert (mx <= TOL_MAX).all() and (l2 <= TOL_L2).all()
