"""Buffer lengths and sample rates other than the reference's 513 / 44100 (pbso_engine_desc::frames_per_buffer, ::sample_rate).

Every comparison with an oracle is with the variant library compiled for that (frames, rate) pair (oracle_py.lib(frames=, rate=),
anchored by tests/test_oracle_variants.py).  The bar is the project's own (tests/test_gpu_parity.py):
max |d| <= 5e-4 of peak and relative L2 <= 1e-3 for the velocity form on audio, on every qnorm row (against that row's own peak)
and on the final state; 2e-2 / 3e-2 for the reference-literal direct form, whose bar was set at 44100 Hz and is applied at that
rate; the fuzz file's qnorm rule for the random scripts.  emitted flags and the FFAT transfer rows (`latest`) are compared bit for
bit.  Where a test says EQUAL it means np.array_equal on audio, emitted, every qnorm row and the final state.

Lengths: 27 (one tile: a ring of two slots, the one-tile lag has no tile in front of it in its buffer), 54, 270, 513 with the
velocity form (the control), 540 (longer than 513; rows padded to 544) and 864 (32 tiles: all-ones tile masks, and a team of 16
waves would not fit the LDS).  Rates: 22050 (band cut at 9 kHz), 48000, 96000."""
import functools

import numpy as np
import pytest
import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from oracle import oracle_py as orc
from tests import track_model
from tests.scenarios import ObjSpec, force_ev, rel_errors, run_engine, run_oracle
from tests.test_gpu_fuzz import _run_seed
from tests.test_gpu_strokes import CASES as STROKE_CASES, _assert_equal as _strokes_equal, _run as _stroke_run
from tests.track_model import track_ev

pytestmark = pytest.mark.gpu

TOL_MAX, TOL_L2 = 5e-4, 1e-3
VEL = capi.FORM_VELOCITY
LENGTHS = [27, 54, 270, 513, 540, 864]
PAIRS = [(f, 44100) for f in LENGTHS] + [(f, r) for r in (22050, 48000, 96000) for f in (270, 513)] + [(864, 96000)]
THREE = [27, 270, 864]


def _f_hi(rate):
    return dict(f_hi=9000.0) if rate < 40000 else {}


def _n_buffers(frames):
    """enough buffers for the long Gaussian (12 buffers) and what follows it; short buffers get more, so forces still span many"""
    return {27: 60, 54: 24}.get(frames, 18)


# ---------------------------------------------------------------------------
# 1. the scripted scene
def _scripted(frames, rate, sizes=(1, 37, 64, 65, 200), maps_modes=100):
    """ragged objects without maps and one with FFAT maps whose listener moves every buffer.  Forces: point hits, a Gaussian narrower
    than one sample at this rate (5 us), one that lives 12 buffers (width 1.2 buffers), a sustained AR stroke with a parameter
    change, plain AR forces, clearAllForces holes, two messages stamped for one buffer."""
    nb = _n_buffers(frames)
    k = 3 if frames == 27 else 1                                # stamps spread over the longer run
    rng = np.random.default_rng(1000 * frames + rate // 50)
    objs = [ObjSpec(synth.eigenvalues(m, 3100 + i, **_f_hi(rate))) for i, m in enumerate(sizes)]
    n_plain = len(objs)
    if maps_modes:
        lam = synth.eigenvalues(maps_modes, 3200, **_f_hi(rate))
        objs.append(ObjSpec(lam, maps=synth.ffat_maps(lam, 3201, dim=4)))
    long_us = 1.2 * frames / rate * 1e6
    assert int(5.0 * 1e-6 * rate) == 0 and 10 * int(long_us * 1e-6 * rate) >= 10 * frames

    def d(o):
        return rng.standard_normal(objs[o].n_modes) * 1e-3
    evs = [dict(t=0, obj=i, kind="use_transfer", use=False) for i in range(n_plain)]
    # object 0: hits, the narrow Gaussian, two messages on one stamp (the second is consumed a buffer later)
    evs += [force_ev(0, 0, data=d(0)), force_ev(2 * k, 0, data=d(0), force_type=1, width=5.0), force_ev(5 * k, 0, data=d(0)),
            force_ev(5 * k, 0, data=d(0))]
    if n_plain > 1:
        # object 1: the long Gaussian with a hit and the narrow one on top of it
        evs += [force_ev(1, 1, data=d(1), force_type=1, width=long_us), force_ev(3, 1, data=d(1)),
                force_ev(4, 1, data=d(1), force_type=1, width=5.0)]
    if n_plain > 2:
        # object 2: a plain AR force (lives until the clear), a hole, hits behind it
        evs += [force_ev(1, 2, data=d(2), force_type=2), force_ev(2, 2, data=d(2)), force_ev(8 * k, 2, clear=True),
                force_ev(10 * k, 2, data=d(2)), force_ev(12 * k, 2, data=d(2)), force_ev(12 * k, 2, data=d(2))]
    if n_plain > 3:
        # object 3: a sustained stroke: new contact data, new AR parameters, the end; a hit behind it
        evs += [force_ev(1, 3, data=d(3), force_type=2, start=True), force_ev(3, 3, data=d(3), force_type=2),
                dict(t=4 * k, obj=3, kind="arprm", a=[0.6, 0.1], sigma=2e-3, mu=0.2), force_ev(6 * k, 3, data=d(3), force_type=2),
                force_ev(9 * k, 3, force_type=2, end=True), force_ev(11 * k, 3, data=d(3))]
    if n_plain > 4:
        # object 4: everything at once, a hole, then the long Gaussian cut off by the end of the run
        evs += [force_ev(0, 4, data=d(4)), force_ev(2, 4, data=d(4), force_type=1, width=400.0), force_ev(5, 4, data=d(4), force_type=2),
                force_ev(9 * k, 4, clear=True), force_ev(10 * k, 4, data=d(4), force_type=1, width=long_us)]
    if maps_modes:
        m = n_plain
        evs += [force_ev(0, m, data=d(m)), force_ev(4 * k, m, data=d(m)), force_ev(7 * k, m, data=d(m), force_type=1, width=5.0),
                force_ev(9 * k, m, data=d(m), force_type=2)]
        for b in range(nb):
            p = rng.standard_normal(3)
            evs.append(dict(t=b, obj=m, kind="listener", pos=p / np.linalg.norm(p) * rng.uniform(0.2, 2.0) + 1e-3))
    return objs, evs, nb


@functools.lru_cache(maxsize=None)
def _scripted_ref(frames, rate):
    objs, evs, nb = _scripted(frames, rate)
    want = run_oracle(objs, evs, nb, frames=frames, rate=rate)
    assert not want["emitted"].all() and np.abs(want["audio"]).max(axis=1).min() > 0
    return objs, evs, nb, want


def _figures(got, want):
    """(audio max / peak, audio relative L2, qnorm rows max / row peak, qnorm rows relative L2, state max / peak of q1)"""
    mx, l2 = rel_errors(got["audio"], want["audio"])
    qmx = ql2 = smx = 0.0
    for key, w in want["qnorm"].items():
        g = got["qnorm"][key].astype(np.float64)
        qmx = max(qmx, np.abs(g - w).max() / max(np.abs(w).max(), 1e-300))
        ql2 = max(ql2, np.linalg.norm(g - w) / max(np.linalg.norm(w), 1e-300))
    for (g1, g2), (w1, w2) in zip(got["state"], want["state"]):
        scale = max(np.abs(w1).max(), 1e-300)
        smx = max(smx, np.abs(g1 - w1).max() / scale, np.abs(g2 - w2).max() / scale)
    return mx.max(), l2.max(), qmx, ql2, smx


def _check(got, want, what, tol_max=TOL_MAX, tol_l2=TOL_L2):
    assert np.isfinite(got["audio"]).all()
    fig = _figures(got, want)
    print(f"{what}: audio max|d|/peak {fig[0]:.3e} relL2 {fig[1]:.3e}; qnorm rows {fig[2]:.3e} relL2 {fig[3]:.3e}; state {fig[4]:.3e}")
    assert np.array_equal(got["emitted"].astype(bool), want["emitted"])
    for a, w in zip(got["latest"], want["latest"]):
        assert np.array_equal(a, w)
    assert fig[0] <= tol_max and fig[1] <= tol_l2, (what, "audio", fig)
    assert fig[2] <= tol_max and fig[3] <= tol_l2, (what, "qnorm", fig)
    assert fig[4] <= tol_max, (what, "state", fig)
    return fig


def _equal(a, b):
    assert np.array_equal(a["audio"], b["audio"]) and np.array_equal(a["emitted"], b["emitted"])
    assert a["qnorm"].keys() == b["qnorm"].keys() and all(np.array_equal(a["qnorm"][k], b["qnorm"][k]) for k in a["qnorm"])
    for (p1, p2), (q1, q2) in zip(a["state"], b["state"]):
        assert np.array_equal(p1, q1) and np.array_equal(p2, q2)
    assert np.abs(a["audio"]).max() > 0


@pytest.mark.parametrize("mpl", [0, 1, 2, 3, 4, 8])
@pytest.mark.parametrize("frames,rate", PAIRS)
def test_scripted_scene_against_the_variant_oracle(frames, rate, mpl):
    objs, evs, nb, want = _scripted_ref(frames, rate)
    for qn in (capi.QNORM_ALL, capi.QNORM_CLOSED):
        got = run_engine(objs, evs, nb, frames=frames, rate=rate, form=VEL, modes_per_lane=mpl, qnorm=qn)
        assert got["info"]["frames_per_buffer"] == frames and got["info"]["recurrence_form"] == VEL
        assert got["audio"].shape == (len(objs), nb * frames)
        _check(got, want, f"{frames} / {rate}, {mpl} modes per lane, qnorm mode {qn}")


@functools.lru_cache(maxsize=None)
def _large_ref(frames, rate):
    objs, evs, nb = _scripted(frames, rate, sizes=(1100, 1000, 65), maps_modes=0)
    return objs, evs, nb, run_oracle(objs, evs, nb, frames=frames, rate=rate)


@pytest.mark.parametrize("team_waves", [16, 0])
@pytest.mark.parametrize("frames,rate", PAIRS)
def test_object_of_1100_modes_as_one_team_and_under_the_policy(frames, rate, team_waves):
    """team_waves = 16 asks for the largest teams: at one mode per lane 1100 modes (18 waves) are two teams of 9, and 1000 modes
    (16 waves) one team of 16 -- whose tile ring no longer fits the LDS from 702 frames on: the engine cuts it in two (the cap is
    14 waves at 864 frames).  The policy spreads one-wave teams."""
    objs, evs, nb, want = _large_ref(frames, rate)
    for mpl in (1, 0):
        got = run_engine(objs, evs, nb, frames=frames, rate=rate, form=VEL, modes_per_lane=mpl, team_waves=team_waves)
        info = got["info"]
        assert info["lds_bytes_per_workgroup"] <= 160 * 1024
        if team_waves == 16 and mpl == 1:
            assert info["waves_per_object"] == (16 if frames < 702 else 9)
        _check(got, want, f"1100 modes, {frames} / {rate}, team_waves {team_waves}, {mpl} modes per lane (W = {info['waves_per_object']})")


@pytest.mark.parametrize("form", [capi.FORM_BLOCK, capi.FORM_BLOCK_BF16])
@pytest.mark.parametrize("frames", [27, 270, 540, 864])
def test_block_forms_fall_back_to_the_velocity_form(frames, form):
    """a length the block forms cannot tile: the engine says so in info() and runs the velocity form's arithmetic, bit for bit"""
    objs, evs, nb, want = _scripted_ref(frames, 44100)
    vel = run_engine(objs, evs, nb, frames=frames, form=VEL)
    blk = run_engine(objs, evs, nb, frames=frames, form=form)
    assert blk["info"]["recurrence_form"] == VEL and vel["info"]["recurrence_form"] == VEL
    _equal(vel, blk)
    for a, b in zip(vel["latest"], blk["latest"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("frames", THREE)
def test_direct_form_at_its_own_bar(frames):
    """the reference-literal recurrence in fp32: 2e-2 of peak / 3e-2 relative L2 (tests/test_gpu_parity.py), at the rate that bar
    was set at"""
    objs, evs, nb, want = _scripted_ref(frames, 44100)
    got = run_engine(objs, evs, nb, frames=frames, form=capi.FORM_DIRECT)
    assert got["info"]["recurrence_form"] == capi.FORM_DIRECT
    _check(got, want, f"direct form, {frames} / 44100", 2e-2, 3e-2)


# ---------------------------------------------------------------------------
# 2. random scripts (tests/test_gpu_fuzz.py).  The seeds are the first twelve per pair whose script the oracle accepts (a
# clearAllForces while a stroke is sustained trips a live assert of the reference): chosen on the CPU, so nothing here skips.
FUZZ_SEEDS = {
    (27, 44100): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],
    (270, 48000): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],
    (864, 96000): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11],
}
FUZZ_BASE = {(27, 44100): 300000, (270, 48000): 310000, (864, 96000): 320000}
FUZZ_SIZES = [5, 64, 200, 1100]


def fuzz_args(frames, rate, seed):
    """(seed of the scene, keyword arguments of _run_seed)"""
    i = seed
    kw = dict(form=VEL, modes_per_lane=[0, 1, 2, 3, 4, 8][i % 6], qnorm=capi.QNORM_CLOSED if i % 2 else capi.QNORM_ALL,
              chunk_buffers=[1, 5, 128][i % 3], device_profiles=-1 if i % 4 >= 2 else 0, team_waves=16 if i % 5 == 0 else 0)
    return FUZZ_BASE[(frames, rate)] + seed, dict(engine_kw=kw, projected_hits=bool(i % 2), frames=frames, rate=rate,
                                                  nb_range=(20, 60) if frames == 27 else (6, 16))


@pytest.mark.parametrize("frames,rate,seed", [(f, r, s) for (f, r), seeds in FUZZ_SEEDS.items() for s in seeds])
def test_random_scripts_match_the_variant_oracle(frames, rate, seed):
    scene_seed, kw = fuzz_args(frames, rate, seed)
    _run_seed(scene_seed, FUZZ_SIZES, kw.pop("engine_kw"), **kw)


# ---------------------------------------------------------------------------
# 3. bit-exact properties, no oracle
def _property_scene(frames):
    sizes = [37, 64, 200, 1100]
    rng = np.random.default_rng(4400 + frames)
    objs = [ObjSpec(synth.eigenvalues(m, 4400 + i), shapes=synth.mode_shapes(m, 4400 + i)) for i, m in enumerate(sizes)]
    data = [rng.standard_normal(m) * 1e-3 for m in sizes]
    off = [dict(t=0, obj=i, kind="use_transfer", use=False) for i in range(len(sizes))]
    return objs, data, off


@pytest.mark.parametrize("frames", THREE)
def test_bit_exact_properties(frames):
    """the same run twice; a step cut into launches and into steps; a shift by two whole buffers; x 4; planner threads"""
    objs, data, off = _property_scene(frames)
    nb, n = 16, len(objs)
    gauss = [force_ev(5, 1, data=data[1], force_type=1, width=1.5 * frames / 44100 * 1e6)]       # a dense profile over several buffers
    evs = [force_ev(i % 4, i, data=data[i]) for i in range(n)] + gauss + off
    kw = dict(frames=frames, form=VEL)
    a = run_engine(objs, evs, nb, chunk_buffers=1000, **kw)
    _equal(a, run_engine(objs, evs, nb, chunk_buffers=1000, **kw))
    for cb in (1, 4):
        _equal(a, run_engine(objs, evs, nb, chunk_buffers=cb, **kw))
    _equal(a, run_engine(objs, evs, nb, split=[3, 5, 1, 7], **kw))
    _equal(a, run_engine(objs, evs, nb, plan_threads=4, **kw))
    _equal(a, run_engine(objs, evs, nb, plan_threads=1, **kw))
    shifted = [dict(e, t=e["t"] + 2) if e["kind"] == "force" else e for e in evs]
    s = run_engine(objs, shifted, nb, **kw)["audio"]
    assert np.array_equal(s[:, 2 * frames:], a["audio"][:, :-2 * frames]) and not s[:, :2 * frames].any()
    times4 = [dict(e, data=4.0 * e["data"]) if e["kind"] == "force" else e for e in evs]
    assert np.array_equal(run_engine(objs, times4, nb, **kw)["audio"], 4.0 * a["audio"])


@pytest.mark.parametrize("frames", THREE)
def test_projection_on_the_device_equals_explicit_data(frames):
    """vertex and face hits projected on the device in fp64 (direct_hits = -1: not from the bank's f32 table) against the same
    messages with the oracle's projection as explicit data: EQUAL"""
    objs, _, off = _property_scene(frames)
    rng = np.random.default_rng(77)
    dev, host = [], []
    for i, o in enumerate(objs):
        vn = synth.unit_normals(2, 500 + i)
        vid, vids = int(rng.integers(0, synth.N_VERTS)), rng.integers(0, synth.N_VERTS, 3)
        bary = rng.random(3)
        bary /= bary.sum()
        dev += [force_ev(i % 3, i, vid=vid, vn=vn[0]), force_ev(4 + i, i, vids=vids, coords=bary, vn=vn[1])]
        host += [force_ev(i % 3, i, data=orc.modal_force_vertex(o.shapes, vid, vn[0])),
                 force_ev(4 + i, i, data=orc.modal_force_face(o.shapes, vids, bary, vn[1]))]
    a = run_engine(objs, dev + off, 10, frames=frames, form=VEL, direct_hits=-1)
    b = run_engine(objs, host + off, 10, frames=frames, form=VEL, direct_hits=-1)
    _equal(a, b)


# ---------------------------------------------------------------------------
# 4. requests only the 513-frame block forms can honour.  Engine::finalize builds the time-chunk tables only if is_block()
# (tc_ok_), the pipeline table only if is_block() (split_ok_), step_chunk cuts in time only if is_block(), and
# mix_listeners refuses unless is_block(): at another length all three must leave the velocity run untouched / return a status.
@pytest.mark.parametrize("frames", THREE)
def test_requests_of_the_block_forms_at_other_lengths(frames):
    objs, evs, nb, _ = _scripted_ref(frames, 44100)
    plain = run_engine(objs, evs, nb, frames=frames, form=VEL)
    for kw in (dict(time_chunks=2), dict(bank_kernel=capi.BANK_PIPE), dict(bank_kernel=capi.BANK_PIPE, modes_per_lane=1)):
        got = run_engine(objs, evs, nb, frames=frames, form=capi.FORM_BLOCK, **kw)
        assert got["info"]["recurrence_form"] == VEL
        if "modes_per_lane" not in kw:
            _equal(plain, got)
        else:
            _equal(run_engine(objs, evs, nb, frames=frames, form=VEL, modes_per_lane=1), got)
    with Engine(form=capi.FORM_BLOCK, frames_per_buffer=frames) as eng:
        lam = synth.eigenvalues(64, 5)
        eng.add_object(lam, synth.RHO, synth.ALPHA, synth.BETA)
        eng.set_ffat_maps(0, synth.ffat_maps(lam, 6, dim=4))
        eng.finalize()
        with pytest.raises(PbsoError) as e:
            eng.listeners_enable(0)
        assert e.value.status == capi.ERR_STATE
        eng.enqueue_force(0, ForceMessage(data=np.ones(64) * 1e-3))
        eng.step(2)
        with pytest.raises(PbsoError) as e:
            eng.mix_listeners(0, np.array([[0.3, 0.2, 0.5], [0.1, -0.4, 0.2]]))
        assert e.value.status == capi.ERR_STATE
        assert np.abs(eng.audio()).max() > 0                # and the engine goes on


# ---------------------------------------------------------------------------
# 5. strokes and tracks
@pytest.mark.parametrize("case", ["bench", "gaps_bursts"])
@pytest.mark.parametrize("frames,rate", [(270, 48000), (864, 96000)])
def test_stroke_script_equals_message_by_message(frames, rate, case):
    scene, entries, split = STROKE_CASES[case][0](), STROKE_CASES[case][1](), STROKE_CASES[case][2]
    kw = dict(form=VEL, frames_per_buffer=frames, sample_rate=rate)
    a = _stroke_run(scene, entries, split, True, **kw)
    b = _stroke_run(scene, entries, split, False, **kw)
    assert a["audio"].shape[1] == sum(split) * frames
    _strokes_equal(a, b)
    assert b["stats"] == dict(direct=0, queued=0, dropped=0, kernel_launches=0)


def _delta_case():
    m = 130
    lam = synth.eigenvalues(m, 1203)
    objs = [ObjSpec(lam, shapes=synth.mode_shapes(m, 1203))]
    vn = np.array([0.36, -0.48, 0.8])
    return objs, dict(vid=123, vn=vn), [dict(t=0, obj=0, kind="use_transfer", use=False)]


@pytest.mark.parametrize("frames,rate", [(270, 48000), (864, 96000)])
def test_one_sample_track_is_a_hit_at_that_sample(frames, rate):
    """start_sample 0, 1 and frames - 1 against the engine's own PointForce run delayed by that many samples and against the variant
    oracle's (the bar of tests/test_gpu_track_force.py); start_sample = frames is refused"""
    objs, hit, unit = _delta_case()
    nb = 5
    point = unit + [force_ev(1, 0, **hit)]
    kw = dict(frames=frames, rate=rate, form=VEL)
    own = track_model.run_engine(objs, [], point, [nb], direct_hits=-1, **kw)["audio"][0].astype(np.float64)
    want = run_oracle(objs, point, nb, frames=frames, rate=rate)["audio"][0]
    for s in (0, 1, frames - 1):
        got = track_model.run_engine(objs, [np.array([1.0], dtype=np.float32)], unit + [track_ev(1, 0, 0, start_sample=s, **hit)], [nb], **kw)
        for name, ref in (("the engine's PointForce", own), ("the oracle's PointForce", want)):
            delayed = np.concatenate([np.zeros(s), ref[:nb * frames - s]])[None]
            mx, l2 = rel_errors(got["audio"], delayed)
            print(f"{frames} / {rate}: delta track at start_sample {s} against {name} delayed: max|d|/peak {mx.max():.3e}, relative L2 {l2.max():.3e}")
            assert (mx <= TOL_MAX).all() and (l2 <= TOL_L2).all(), (name, s, mx, l2)
        assert got["track_stats"][2:] == (1, 1)
    with pytest.raises(PbsoError) as e:
        track_model.run_engine(objs, [np.array([1.0], dtype=np.float32)], unit + [track_ev(1, 0, 0, start_sample=frames, **hit)], [nb], **kw)
    assert e.value.status == capi.ERR_INVALID


@pytest.mark.parametrize("frames,rate", [(270, 48000), (864, 96000)])
def test_looping_track_at_rate_0_37_against_the_model(frames, rate):
    objs, hit, unit = _delta_case()
    nb = 8
    trk = np.random.default_rng(9).standard_normal(211).astype(np.float32)
    evs = unit + [track_ev(1, 0, 0, first=3.25, rate=0.37, gain=0.8, n_samples=4 * frames + 11, start_sample=frames // 3, loop=True, **hit)]
    want = track_model.run_model(objs, [trk], evs, nb, per_sample=False, frames=frames, rate=rate)
    got = track_model.run_engine(objs, [trk], evs, [nb], frames=frames, rate=rate, form=VEL)
    got["latest"], want["latest"] = [], []
    _check(got, want, f"looping track at rate 0.37, {frames} / {rate}")


# ---------------------------------------------------------------------------
# 6. ways out of the engine: pbso_step_to_host, the row read-backs and pbso_mix_objects against audio()
@pytest.mark.parametrize("nb", [3, 4])
@pytest.mark.parametrize("frames", [27, 135, 270, 864])
def test_ways_out_of_the_engine(frames, nb):
    """135 frames and an odd buffer count give odd row lengths: pbso_mix_objects' paired loads must not be taken.  The mix is the f32
    sum in object order (one group: fewer than 32 objects), bit for bit."""
    sizes = [1, 37, 64, 65, 200]
    rng = np.random.default_rng(frames + nb)

    def make():
        eng = Engine(form=VEL, frames_per_buffer=frames)
        for i, m in enumerate(sizes):
            eng.add_object(synth.eigenvalues(m, 6100 + i), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        r = np.random.default_rng(61)
        for i, m in enumerate(sizes):
            eng.set_use_transfer(i, False)
            for t in (0, 1 + i % 2, nb + 1):
                assert eng.enqueue_force(i, ForceMessage(data=r.standard_normal(m) * 1e-3), t)
        return eng
    a, b = make(), make()
    try:
        mono = torch.zeros(nb * frames, dtype=torch.float32, device="cuda")
        host = b.host_buffer(nb)
        torch.cuda.synchronize()
        for k in range(2):
            a.step(nb)
            a.mix_objects(mono.data_ptr())
            a.sync()
            audio = a.audio()
            assert audio.shape == (len(sizes), nb * frames) and (np.abs(audio).max(axis=1) > 0).all()
            rows = [int(x) for x in rng.permutation(len(sizes))[:3]]
            assert np.array_equal(a.audio_rows(rows), audio[rows])
            want = np.zeros(nb * frames, dtype=np.float32)
            for o in range(len(sizes)):
                want = want + audio[o]
            assert np.array_equal(mono.cpu().numpy(), want), k
            b.step_to_host(nb, host)
            b.host_wait()
            assert np.array_equal(host.reshape(len(sizes), nb * frames), audio), k
    finally:
        a.close()
        b.close()
