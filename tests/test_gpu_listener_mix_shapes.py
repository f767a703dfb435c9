"""The multi-listener mix (pbso_listeners_enable / pbso_mix_listeners) on every team shape the block kernel builds.

pbso_listeners_enable switches the whole bank launch to the DUMP instantiations of iir_block_kernel (kernels_block.hip,
launch_one<R, 2, PROJ, true>): the f32 projection then steps with coarse2 instead of the headline's vburst_pk, every slice writes its
block-start states and a scale row (dump_state / dump_scale), qnorm rows are always on -- and listener_mix_kernel rebuilds the
listeners' audio from those states.  The older listener tests use scenes that the policy gives ONE mode per lane (the HALF variant:
a one-group ring, two combines per buffer); here are the builds at two and four modes per lane, both projections, objects cut into
several teams (team.col0 != 0), dead slices, vertex hits through the bank's own projection, several enabled objects, listener
counts around MIX_TILE = 8, launch cuts, and the settings that must fall back to the walk in buffer order.

Reference: one fp64 ModalSolver per listener (tests/listener_mix_ref.py).  Bars, all the project's own: 5e-4 of the row's peak
against the oracle, 1e-4 of the peak between the mix row at the engine's own listener position and the engine's
own audio() (test_multi_listener_mix_matches_independent_solvers).  Every case asserts through info() that it ran what it names."""
import functools

import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError
from tests.listener_mix_ref import oracle_rows
from tests.scenarios import B, ObjSpec, force_ev

pytestmark = pytest.mark.gpu

ORACLE_BAR = 5e-4           # max|mix - oracle| <= 5e-4 peak, per listener row
AUDIO_BAR = 1e-4            # max|mix row at the engine's listener - audio()| <= 1e-4 peak
N_VERTS = 5


def _spec(n, seed, maps=True):
    lam = synth.eigenvalues(n, seed)
    return ObjSpec(lam, shapes=synth.mode_shapes(n, seed, N_VERTS),
                   maps=synth.ffat_maps(lam, seed + 1, dim=4, cell_size=0.01) if maps else None)


def _positions(n, seed):
    """outside the maps' 0.04 m cube, no two alike, none on an axis"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, 3))
    return p / np.linalg.norm(p, axis=1, keepdims=True) * (0.3 + 0.3 * rng.random((n, 1)))


def _engine(objs, **kw):
    kw.setdefault("team_waves", 0)
    kw.setdefault("form", capi.FORM_BLOCK)
    eng = Engine(**kw)
    for o in objs:
        oid = eng.add_object(o.lam, o.rho, o.alpha, o.beta, o.n_modes, o.shapes)
        if o.maps is not None:
            eng.set_ffat_maps(oid, o.maps)
    eng.finalize()
    for i, o in enumerate(objs):
        if o.maps is None:
            eng.set_use_transfer(i, False)
    return eng


def _enqueue(eng, events, t0=0, t1=1 << 60):
    """the force events with t0 <= t < t1, in stamp order (the force queue is a FIFO)"""
    for ev in sorted(events, key=lambda e: e["t"]):
        if t0 <= ev["t"] < t1:
            m = ForceMessage(data=ev["data"], forceType=ev["force_type"], gaussianWidth=ev["width"], clearAllForces=ev["clear"],
                             vid=ev["vid"], vids=ev["vids"], coords=ev["coords"], vn=ev["vn"])
            assert eng.enqueue_force(ev["obj"], m, ev["t"])


def _ran(info, mpl, block_launches):
    assert info["modes_per_lane"] == mpl, info["modes_per_lane"]
    assert info["total_sample_launches"] == 0
    assert info["total_block_launches"] == block_launches, info["total_block_launches"]


def _err(got, want):
    """max|got - want| / peak(want) per row"""
    got, want = np.atleast_2d(np.asarray(got, dtype=np.float64)), np.atleast_2d(want)
    return np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)


def _check_mix(mix, want, tag):
    mix = mix.astype(np.float64)
    assert mix.shape == want.shape, (mix.shape, want.shape)
    assert np.isfinite(mix).all(), tag
    assert (np.abs(mix).max(axis=1) > 0).all(), tag                                    # no listener hears silence
    e = _err(mix, want)
    print(f"{tag}: max|mix - oracle| / peak = {e.max():.3e}")
    assert (e <= ORACLE_BAR).all(), (tag, e)
    return e.max()


# ---- 1. team shapes ------------------------------------------------------------------------------------------------------------
S1_MODES, S1_BYSTANDER, S1_NB, S1_L, S1_OWN, S1_CLEAR = (65, 600, 1100), 300, 5, 9, 4, 1
S1_CLEAR_AT = 2


@functools.lru_cache(maxsize=None)
def _scene1():
    """three objects to enable -- 65 modes (at four modes per lane: dead slices), 600 and 1100 (at team_waves = 2: several teams,
    partial sums) -- and a 300-mode bystander without maps.  Five buffers in launches of 2 + 2 + 1.  Per object: an explicit-data
    impulse, a face hit and a second message on its stamp (dequeued a buffer later, modal_solver.h:184), a quiet buffer, and a
    vertex hit on the idle object (DESC_DIRECT: the bank's own projection) -- in the LAST launch, which then has no force row at
    all.  Object 1 has a clearAllForces buffer in the middle launch instead."""
    objs = [_spec(n, 8100 + i) for i, n in enumerate(S1_MODES)] + [_spec(S1_BYSTANDER, 8109, maps=False)]
    rng = np.random.default_rng(81)
    vn = synth.unit_normals(16, 82)
    data = lambda i: rng.standard_normal(objs[i].n_modes) * 1e-3
    evs = []
    for i in (0, 2):
        evs += [force_ev(0, i, data=data(i)),
                force_ev(1, i, vids=[0, 2, 3 + i // 2], coords=np.array([0.2, 0.5, 0.3]), vn=vn[i]), force_ev(1, i, data=data(i)),
                force_ev(4, i, vid=1 + i, vn=vn[4 + i])]                                # (buffer 3 is quiet)
    evs += [force_ev(0, 1, data=data(1)), force_ev(0, 1, vids=[4, 1, 0], coords=np.array([0.6, 0.1, 0.3]), vn=vn[8]),
            force_ev(S1_CLEAR_AT, 1, clear=True), force_ev(3, 1, vid=2, vn=vn[9])]      # (buffer 4 is quiet)
    evs += [force_ev(0, 3, data=data(3)), force_ev(3, 3, vid=0, vn=vn[10])]
    pos = _positions(S1_L, 83)
    want = [oracle_rows(objs[i], evs, pos, S1_NB, obj=i) for i in range(3)]
    want.append(oracle_rows(objs[3], evs, pos[:1], S1_NB, obj=3))
    for w in want:
        w.setflags(write=False)
    return objs, evs, pos, want


def _run_scene1(enabled, **kw):
    objs, evs, pos, _ = _scene1()
    with _engine(objs, chunk_buffers=2, **kw) as eng:
        for i in enabled:
            eng.listeners_enable(i)
        for i in range(3):
            eng.compute_transfer(i, pos[S1_OWN], 0)
        _enqueue(eng, evs)
        eng.step(S1_NB)
        audio = eng.audio().astype(np.float64)
        emitted = eng.emitted()
        mixes = {i: eng.mix_listeners(i, pos) for i in enabled}
        return audio, emitted, mixes, eng.info()


@pytest.mark.parametrize("team_waves", [0, 2, 16], ids=["policy", "tw2", "tw16"])
@pytest.mark.parametrize("form", [capi.FORM_BLOCK, capi.FORM_BLOCK_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mpl", [1, 2, 4])
def test_team_shapes(mpl, form, team_waves):
    objs, evs, pos, want = _scene1()
    audio, emitted, mixes, info = _run_scene1((0, 1, 2), form=form, modes_per_lane=mpl, team_waves=team_waves)
    _ran(info, mpl, 3)                                                                 # 5 buffers in launches of 2 + 2 + 1
    assert info["last_step_forced_rows"] == 0           # the last launch's vertex hits went through the bank's projection: no force row
    assert emitted[S1_CLEAR].tolist() == [b != S1_CLEAR_AT for b in range(S1_NB)] and emitted[[0, 2, 3]].all()
    worst = own = 0.0
    for i in range(3):
        tag = f"team shapes R={mpl} form={form} team_waves={team_waves} object {i} ({objs[i].n_modes} modes)"
        worst = max(worst, _check_mix(mixes[i], want[i], tag))
        d = np.abs(mixes[i][S1_OWN] - audio[i]).max() / np.abs(want[i][S1_OWN]).max()
        own = max(own, d)
        assert d <= AUDIO_BAR, (tag, d)
    e = _err(audio, np.array([w[S1_OWN] for w in want[:3]] + [want[3][0]]))
    print(f"team shapes R={mpl} form={form} team_waves={team_waves}: worst mix row {worst:.3e}, audio() against the oracle {e.max():.3e}, "
          f"mix row at the engine's listener against audio() {own:.3e}")
    assert (e <= ORACLE_BAR).all(), e
    cl = slice(S1_CLEAR_AT * B, (S1_CLEAR_AT + 1) * B)
    assert not mixes[S1_CLEAR][:, cl].any() and not audio[S1_CLEAR, cl].any()           # clearAllForces: exactly zero, every listener


# ---- 5. listeners on against listeners off ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("time_chunks", [0, -1], ids=["policy", "walk"])
def test_listeners_on_against_listeners_off(time_chunks):
    """ADVICE.md (round 6): the DUMP builds kept the four-instruction coarse step while the headline build steps with vburst_pk
    (P22 - 1 formed in f32 on the device, D' = fma(P22 - 1, D, fma(P21, Q, D))), so enabling listeners changes the audio bits of a
    scene.  The scene of test_team_shapes at four modes per lane, f32 projection: nobody enabled against the 600-mode object
    enabled -- every object's audio(), the bystander's included, within the bar the suite uses between a mix row and audio().
    `walk` pins both runs to the walk in buffer order (the builds differ in DUMP alone); `policy` is what a caller gets.
    Measured on an MI355X: see DESIGN.md section 2."""
    objs, evs, pos, want = _scene1()
    ref = np.array([w[S1_OWN] for w in want[:3]] + [want[3][0]])
    kw = dict(form=capi.FORM_BLOCK, modes_per_lane=4, time_chunks=time_chunks)
    off, _, _, info_off = _run_scene1((), **kw)
    on, _, mixes, info_on = _run_scene1((1,), **kw)
    _ran(info_off, 4, 3)
    _ran(info_on, 4, 3)
    assert info_on["total_time_chunk_launches"] == 0 and (time_chunks == 0 or info_off["total_time_chunk_launches"] == 0)
    _check_mix(mixes[1], want[1], "on/off, the enabled object")
    e_off, e_on = _err(off, ref), _err(on, ref)
    d = np.abs(on - off).max(axis=1) / np.abs(ref).max(axis=1)
    print(f"listeners on/off ({'policy' if time_chunks == 0 else 'walk'}): off vs oracle {e_off.max():.3e}, on vs oracle {e_on.max():.3e}, "
          f"on vs off {d.max():.3e} of peak, rows with other bits {int((on != off).any(axis=1).sum())} of {len(on)}")
    assert (e_off <= ORACLE_BAR).all() and (e_on <= ORACLE_BAR).all(), (e_off, e_on)
    assert (d <= AUDIO_BAR).all(), d


# ---- 2. listener counts around the accumulator tile -------------------------------------------------------------------------------
S2_COUNTS = (1, 7, 8, 9, 16, 17)


@functools.lru_cache(maxsize=None)
def _run2():
    """one 130-mode object at two modes per lane, 3 buffers, ONE step mixed for every listener count.  Position 12 of the 17 is
    also listener 0 of 1 and listener 7 of 8."""
    o = _spec(130, 8200)
    pos = _positions(17, 84)
    sets = {L: pos[:L] for L in S2_COUNTS}
    sets[1] = pos[12:13]
    sets[8] = np.concatenate([pos[:7], pos[12:13]])
    rng = np.random.default_rng(85)
    evs = [force_ev(0, 0, data=rng.standard_normal(130) * 1e-3), force_ev(2, 0, vid=3, vn=synth.unit_normals(1, 86)[0])]
    with _engine([o], modes_per_lane=2) as eng:
        eng.listeners_enable(0)
        _enqueue(eng, evs)
        eng.step(3)
        mixes = {L: eng.mix_listeners(0, p) for L, p in sets.items()}
        info = eng.info()
    want = oracle_rows(o, evs, pos, 3)
    idx = {L: list(range(L)) for L in S2_COUNTS}
    idx[1], idx[8] = [12], list(range(7)) + [12]
    return mixes, {L: want[idx[L]] for L in S2_COUNTS}, info


@pytest.mark.parametrize("L", S2_COUNTS)
def test_listener_counts_around_the_accumulator_tile(L):
    mixes, want, info = _run2()
    _ran(info, 2, 1)
    _check_mix(mixes[L], want[L], f"L={L}")


def test_a_listener_row_does_not_depend_on_the_other_listeners():
    """every listener has its own accumulators and its own fmaf chain in listener_mix_kernel: the same position gives the same
    bits as listener 0 of 1, 7 of 8 and 12 of 17"""
    mixes, _, _ = _run2()
    assert np.array_equal(mixes[1][0], mixes[8][7]) and np.array_equal(mixes[1][0], mixes[17][12])
    assert np.array_equal(mixes[7], mixes[17][:7]) and np.array_equal(mixes[16], mixes[17][:16]) and np.array_equal(mixes[9], mixes[16][:9])


# ---- 3. mode counts around the wave and slab edges --------------------------------------------------------------------------------
@pytest.mark.parametrize("mpl", [1, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 4096])
def test_mode_counts_around_the_wave_and_slab_edges(n, mpl):
    """L = 3, 3 buffers; FFAT maps and the engine's own listener at position 1, for 4096 modes the unit transfer (no maps: every
    listener hears the engine's output).  Combinations pbso_finalize refuses: none -- the block form takes 1, 2 and 4 modes per
    lane at any mode count (4096 at one mode per lane is 64 waves in several teams), so nothing is skipped."""
    o = _spec(n, 8300 + n % 1000, maps=n != 4096)
    pos = _positions(3, 87)
    rng = np.random.default_rng(88)
    vn = synth.unit_normals(2, 89)
    evs = [force_ev(0, 0, vid=4, vn=vn[0]), force_ev(1, 0, data=rng.standard_normal(n) * 1e-3)]
    with _engine([o], modes_per_lane=mpl) as eng:
        eng.listeners_enable(0)
        if o.maps is not None:
            eng.compute_transfer(0, pos[1], 0)
        _enqueue(eng, evs)
        eng.step(3)
        audio = eng.audio()[0].astype(np.float64)
        mix = eng.mix_listeners(0, pos)
        _ran(eng.info(), mpl, 1)
    want = oracle_rows(o, evs, pos, 3)
    _check_mix(mix, want, f"n={n} R={mpl}")
    assert np.abs(mix[1] - audio).max() <= AUDIO_BAR * np.abs(want[1]).max()
    assert _err(audio, want[1])[0] <= ORACLE_BAR


# ---- 4. several enabled objects, enabled at different times -----------------------------------------------------------------------
@pytest.mark.parametrize("mpl", [2, 4])
def test_objects_enabled_at_different_times(mpl):
    """enable A, step 3, mix A; enable B (d_wtab32_ grows and keeps A's table), step 5 (the state buffers grow), mix A and B.  The
    second step's mixes have the same bits on an engine that never mixed in between, and on one where B was enabled first (the
    dump rows swapped) and both from the start: the mix of A depends neither on B's row nor on when B was enabled."""
    objs = [_spec(130, 8400), _spec(600, 8401), _spec(70, 8402, maps=False)]
    pos = _positions(5, 90)
    rng = np.random.default_rng(91)
    vn = synth.unit_normals(6, 92)
    evs = []
    for i in range(3):
        n = objs[i].n_modes
        evs += [force_ev(0, i, data=rng.standard_normal(n) * 1e-3), force_ev(2, i, vid=i, vn=vn[i]),
                force_ev(3, i, data=rng.standard_normal(n) * 1e-3), force_ev(6, i, vid=4 - i, vn=vn[3 + i])]

    def run(order, mix_between):
        """order: (object, step before which it is enabled)"""
        with _engine(objs, modes_per_lane=mpl) as eng:
            first = None
            for step, (t0, nb) in enumerate(((0, 3), (3, 5))):
                for i, when in order:
                    if when == step:
                        eng.listeners_enable(i)
                _enqueue(eng, evs, t0, t0 + nb)
                eng.step(nb)
                if step == 0 and mix_between:
                    first = eng.mix_listeners(0, pos)
            return first, eng.mix_listeners(0, pos), eng.mix_listeners(1, pos), eng.audio(), eng.info()

    a1, a2, b2, audio, info = run(((0, 0), (1, 1)), True)
    _ran(info, mpl, 2)
    want = [oracle_rows(objs[i], evs, pos, 8, obj=i) for i in range(2)]
    _check_mix(a1, want[0][:, :3 * B], f"A, first step, R={mpl}")
    _check_mix(a2, want[0][:, 3 * B:], f"A, second step, R={mpl}")
    _check_mix(b2, want[1][:, 3 * B:], f"B, second step, R={mpl}")
    _, a2n, b2n, audio_n, info = run(((0, 0), (1, 1)), False)
    _ran(info, mpl, 2)
    assert np.array_equal(a2, a2n) and np.array_equal(b2, b2n) and np.array_equal(audio, audio_n)
    _, a2s, b2s, audio_s, info = run(((1, 0), (0, 0)), False)                           # B has dump row 0, A row 1, from the start
    _ran(info, mpl, 2)
    assert np.array_equal(a2, a2s) and np.array_equal(b2, b2s) and np.array_equal(audio, audio_s)


# ---- 6. settings that must fall back to the walk ------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["time_chunks", "pipeline"])
def test_settings_that_fall_back_to_the_walk(setting):
    """an engine told time_chunks = 3, or bank_kernel = PBSO_BANK_PIPE, runs its launches cut in time / on the pipeline kernel until
    an object is enabled; from then on choose_time_chunks returns false and use_split() is false: the walk in buffer order, on the
    DUMP build.  The audio across the switch is one oracle run; with submit_thread = 1 every bit is the same."""
    kw = dict(time_chunks=3) if setting == "time_chunks" else dict(bank_kernel=capi.BANK_PIPE)
    counter = "total_time_chunk_launches" if setting == "time_chunks" else "total_split_launches"
    objs = [_spec(130, 8600), _spec(300, 8601, maps=False)]
    pos = _positions(3, 93)
    rng = np.random.default_rng(94)
    vn = synth.unit_normals(4, 95)
    evs = []
    for i in range(2):
        n = objs[i].n_modes
        evs += [force_ev(0, i, data=rng.standard_normal(n) * 1e-3), force_ev(2, i, vid=1 + i, vn=vn[i]),
                force_ev(4, i, vid=3, vn=vn[2 + i]), force_ev(5, i, data=rng.standard_normal(n) * 1e-3)]

    def run(submit_thread):
        with _engine(objs, form=capi.FORM_BLOCK, modes_per_lane=1, submit_thread=submit_thread, **kw) as eng:
            eng.compute_transfer(0, pos[2], 0)
            _enqueue(eng, evs, 0, 4)
            eng.step(4)
            before = eng.info()
            first = eng.audio().copy()
            eng.listeners_enable(0)
            _enqueue(eng, evs, 4, 8)
            eng.step(4)
            return before, eng.info(), np.concatenate([first, eng.audio()], axis=1), eng.mix_listeners(0, pos)

    before, after, audio, mix = run(0)
    assert before[counter] == 1 and before["total_block_launches"] == 1, before
    assert after[counter] == 1 and after["total_time_chunk_launches"] + after["total_split_launches"] == 1, after
    _ran(after, 1, 2)
    want = oracle_rows(objs[0], evs, pos, 8, obj=0)
    _check_mix(mix, want[:, 4 * B:], f"after the switch from {setting}")
    ref = np.array([want[2], oracle_rows(objs[1], evs, pos[:1], 8, obj=1)[0]])
    e = _err(audio, ref)
    assert (e <= ORACLE_BAR).all(), e
    assert np.abs(mix[2] - audio[0, 4 * B:]).max() <= AUDIO_BAR * np.abs(want[2, 4 * B:]).max()
    before_t, after_t, audio_t, mix_t = run(1)
    assert before_t[counter] == 1 and after_t[counter] == 1
    _ran(after_t, 1, 2)
    assert np.array_equal(audio, audio_t) and np.array_equal(mix, mix_t)


# ---- 7. refusals at the untested shapes ---------------------------------------------------------------------------------------------
def test_a_gaussian_that_lives_two_buffers_is_refused_at_four_modes_per_lane():
    """a Gaussian of 1850 us is 9 x 81 samples long (forces.h:40-45: cutoff 5): a dense force profile in buffers 0 and 1, no block
    states there -- PBSO_ERR_STATE for that step, the next, clean step mixes again"""
    o = _spec(600, 8700)
    pos = _positions(3, 96)
    rng = np.random.default_rng(97)
    # (1e-5: the Gaussian's 200 samples' worth of force rings about as loud as the clean step's impulses)
    evs = [force_ev(0, 0, data=rng.standard_normal(600) * 1e-5, force_type=capi.GAUSSIAN_FORCE, width=1850.0),
           force_ev(4, 0, vid=2, vn=synth.unit_normals(1, 98)[0]), force_ev(5, 0, data=rng.standard_normal(600) * 1e-3)]
    with _engine([o], modes_per_lane=4, team_waves=2) as eng:
        eng.listeners_enable(0)
        eng.compute_transfer(0, pos[0], 0)
        _enqueue(eng, evs, 0, 4)
        eng.step(4)
        with pytest.raises(PbsoError) as ei:
            eng.mix_listeners(0, pos)
        assert ei.value.status == capi.ERR_STATE
        first = eng.audio()[0].astype(np.float64)
        _enqueue(eng, evs, 4, 7)
        eng.step(3)
        mix = eng.mix_listeners(0, pos)
        audio = np.concatenate([first, eng.audio()[0].astype(np.float64)])
        _ran(eng.info(), 4, 2)
    want = oracle_rows(o, evs, pos, 7)
    assert np.abs(want[0, B:2 * B]).max() > 0 and np.isfinite(audio).all()              # the Gaussian did reach into buffer 1
    _check_mix(mix, want[:, 4 * B:], "after a refused Gaussian step")
    assert _err(audio, want[0])[0] <= ORACLE_BAR


def test_one_wave_of_one_team_outside_the_scaled_state_range_is_refused():
    """600 modes at four modes per lane and team_waves = 2: teams of 2 waves (columns 0 .. 511, 128 lanes) and 1 wave.  Mode 100 is
    lane 100 of slice 0: wave 1 of team 0.  Its FFAT map is all zero, so under the engine's own listener that wave alone leaves the
    scaled-state representation (weight 0 < 2^-20) and steps per sample beside a wave on the block path: its scale rows say 0,
    PBSO_ERR_STATE.  Under the unit transfer, before and after, the step mixes (the LISTENERS' weight 0 is just a silent mode)."""
    lam = synth.eigenvalues(600, 8701)
    maps = synth.ffat_maps(lam, 8702, dim=4, cell_size=0.01)
    maps[100]["psi"] = np.zeros_like(np.asarray(maps[100]["psi"], dtype=np.float64))
    o = ObjSpec(lam, shapes=synth.mode_shapes(600, 8701, N_VERTS), maps=maps)
    pos = _positions(3, 99)
    rng = np.random.default_rng(100)
    nb = 3
    evs = [force_ev(0, 0, data=rng.standard_normal(600) * 1e-3), force_ev(3, 0, data=rng.standard_normal(600) * 1e-3),
           force_ev(6, 0, vid=1, vn=synth.unit_normals(1, 101)[0]), force_ev(7, 0, data=rng.standard_normal(600) * 1e-3)]
    with _engine([o], modes_per_lane=4, team_waves=2) as eng:
        eng.listeners_enable(0)
        mixes = []
        for step in range(3):
            if step == 1:
                eng.compute_transfer(0, pos[0], nb)                  # the engine's own listener: mode 100 gets weight 0
            if step == 2:
                eng.set_use_transfer(0, False, 2 * nb)               # the unit transfer again
            _enqueue(eng, evs, step * nb, (step + 1) * nb)
            eng.step(nb)
            assert np.isfinite(eng.audio()).all() and np.abs(eng.audio()).max() > 0
            if step == 1:
                with pytest.raises(PbsoError) as ei:
                    eng.mix_listeners(0, pos)
                assert ei.value.status == capi.ERR_STATE
            else:
                mixes.append(eng.mix_listeners(0, pos))
        _ran(eng.info(), 4, 3)
    want = oracle_rows(o, evs, pos, 3 * nb)
    _check_mix(mixes[0], want[:, :nb * B], "before the refused step")
    _check_mix(mixes[1], want[:, 2 * nb * B:], "after the refused step")


# ---- 8. a step longer than a launch by default ------------------------------------------------------------------------------------
def test_a_step_longer_than_a_default_launch():
    """130 buffers with the default chunk_buffers: launches of 128 + 2 -- dump_b = qn_b0 + b across the launch cut (hits on both
    sides of it, and in the two buffers of the second launch)"""
    n, nb = 64, 130
    o = _spec(n, 8800)
    pos = _positions(2, 102)
    rng = np.random.default_rng(103)
    vn = synth.unit_normals(3, 104)
    evs = [force_ev(0, 0, data=rng.standard_normal(n) * 1e-3), force_ev(60, 0, vid=0, vn=vn[0]), force_ev(127, 0, vid=3, vn=vn[1]),
           force_ev(128, 0, data=rng.standard_normal(n) * 1e-3), force_ev(129, 0, vid=2, vn=vn[2])]
    with _engine([o]) as eng:
        eng.listeners_enable(0)
        eng.compute_transfer(0, pos[1], 0)
        _enqueue(eng, evs)
        eng.step(nb)
        audio = eng.audio()[0].astype(np.float64)
        mix = eng.mix_listeners(0, pos)
        _ran(eng.info(), 1, 2)                                       # (the policy's shape for one 64-mode object: one mode per lane)
    want = oracle_rows(o, evs, pos, nb)
    _check_mix(mix, want, "130 buffers")
    assert (np.abs(want[:, 128 * B:]).max(axis=1) > 0.1 * np.abs(want).max(axis=1)).all()      # the second launch is not lost in the row's peak
    assert np.abs(mix[1] - audio).max() <= AUDIO_BAR * np.abs(want[1]).max()
