"""pbso_set_material (include/openpbso_amd.h "retune"): a new material for objects of a finalized engine, every coefficient table of
theirs rebuilt on the device (csrc/kernels_retune.hip, csrc/mode_tables.h).  The scene and its runners: tests/retune_scene.py.
Device tables are pinned to finalize's host tables THROUGH THE AUDIO: a retuned engine equals a fresh engine of the new material bit
for bit, a retune to the material in force changes nothing, objects not named keep their rows; the reference's setIntegrator
(through the oracle) bounds the mid-run cases."""
import numpy as np
import pytest

from openpbso_amd import capi, synth
from tests import retune_scene as rs
from tests.scenarios import rel_errors

# recurrence form, frames per buffer, further descriptor fields
FORMS = [
    pytest.param(capi.FORM_BLOCK, 0, {}, id="block"),
    pytest.param(capi.FORM_BLOCK_BF16, 0, {}, id="block_bf16"),
    pytest.param(capi.FORM_VELOCITY, 0, {}, id="velocity"),
    pytest.param(capi.FORM_DIRECT, 0, {}, id="direct"),
    pytest.param(capi.FORM_BLOCK, 0, dict(time_chunks=1), id="block-tc1"),
    pytest.param(capi.FORM_BLOCK, 0, dict(time_chunks=3), id="block-tc3"),
    pytest.param(capi.FORM_BLOCK, 0, dict(forced_block=1), id="block-forced"),
    pytest.param(capi.FORM_VELOCITY, 27, {}, id="velocity-27"),
    pytest.param(capi.FORM_VELOCITY, 864, {}, id="velocity-864"),
]
MAIN_FORMS = FORMS[:4]


def _kw(form, frames, sel):
    kw = dict(form=form, **sel)
    if frames:
        kw["frames_per_buffer"] = frames
    return kw


_fresh = {}


def fresh(mat, form, frames=0, sel=None):
    """the un-retuned run of a material, computed once per build and shared"""
    sel = sel or {}
    key = (mat, form, frames, tuple(sorted(sel.items())))
    if key not in _fresh:
        _fresh[key] = rs.run(mat, **_kw(form, frames, sel))
    return _fresh[key]


# ---- without a GPU: the oracle's side of the mid-run comparison ------------------------------------------------------------------
def test_oracle_swap_to_the_same_material_with_the_state_copied_is_a_no_op():
    """or_integrator_build + or_solver_set_integrator after two buffers, the old (q_{k-1}, q_{k-2}) copied into the new integrator
    through or_solver_state's pointers, reproduces the unswapped oracle run bit for bit: the copy is a valid keep_state reference.
    Without the copy (keep_state = 0's reference) the run differs."""
    plain = rs.run_oracle(rs.MAT1)
    kept = rs.run_oracle(rs.MAT1, swap=(rs.CUT, rs.MAT1, True))
    assert np.array_equal(plain["audio"], kept["audio"])
    for i in range(len(rs.MODES)):
        assert np.array_equal(plain["state"][i][0], kept["state"][i][0]) and np.array_equal(plain["state"][i][1], kept["state"][i][1])
        for b in range(rs.NB):
            assert np.array_equal(plain["qnorm"][(i, b)], kept["qnorm"][(i, b)])
    zeroed = rs.run_oracle(rs.MAT1, swap=(rs.CUT, rs.MAT1, False))
    assert not np.array_equal(plain["audio"], zeroed["audio"])
    assert np.array_equal(plain["audio"][:, :rs.CUT * 513], zeroed["audio"][:, :rs.CUT * 513])


# ---- 3: equals a fresh engine ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form,frames,sel", FORMS)
def test_retuned_before_the_first_step_equals_a_fresh_engine_bit_for_bit(form, frames, sel):
    a = rs.run(rs.MAT1, before=rs.retune_to(rs.MAT2), **_kw(form, frames, sel))
    b = fresh(rs.MAT2, form, frames, sel)
    rs.same_run(a, b)
    assert a["material"] == [rs.MAT2] * 4 and b["material"] == [rs.MAT2] * 4
    # ... and the two materials do sound different (the comparison is not vacuous)
    assert not np.array_equal(b["audio"], fresh(rs.MAT1, form, frames, sel)["audio"])


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [True, False])
def test_messages_enqueued_before_the_retune_take_the_new_material(keep):
    """every message of the script is in the queues when the material changes: nothing computed from c3 was kept at enqueue time"""
    a = rs.run(rs.MAT1, before=rs.retune_to(rs.MAT2, keep=keep), enqueue_first=True, form=capi.FORM_BLOCK)
    rs.same_run(a, fresh(rs.MAT2, capi.FORM_BLOCK))


# ---- 4: a retune to the material in force -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form,frames,sel", FORMS)
def test_retune_to_the_material_in_force_mid_run_is_a_no_op(form, frames, sel):
    a = rs.run(rs.MAT1, between=rs.retune_to(rs.MAT1, keep=True), **_kw(form, frames, sel))
    rs.same_run(a, fresh(rs.MAT1, form, frames, sel))
    assert a["stats"][:3] == (1, 4, sum(rs.MODES))


# ---- 5: only the named objects ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form,frames,sel", MAIN_FORMS + [FORMS[5]])
def test_only_the_named_objects_change(form, frames, sel):
    named, others = [3, 1], [0, 2]                          # the split object among them, not in id order
    a = rs.run(rs.MAT1, before=rs.retune_to(rs.MAT2, ids=named), **_kw(form, frames, sel))
    rs.same_run(a, fresh(rs.MAT1, form, frames, sel), rows=others)
    rs.same_run(a, fresh(rs.MAT2, form, frames, sel), rows=named)
    assert a["material"] == [rs.MAT1, rs.MAT2, rs.MAT1, rs.MAT2]
    # g32 elements: object 1 alone has shapes among the named (15 dof x padded modes, whole waves of 64)
    assert a["stats"][:3] == (1, 2, 1100 + 65) and a["stats"][3] > 0 and a["stats"][3] % (15 * 64) == 0


# ---- 6: against the oracle, mid-run -----------------------------------------------------------------------------------------------
TOL_MAX, TOL_L2 = 5e-4, 1e-3              # max|d| <= 5e-4 peak, relative L2 <= 1e-3
# The reference-literal direct form in fp32 fails that tolerance WITHOUT any retune (1.3e-2, SURVEY B-4: q0 - q_prev
# cancels in fp32); tests/test_gpu_parity.py holds it to 2e-2 / 3e-2 against the oracle, and so does this file.
TOL_DIRECT_MAX, TOL_DIRECT_L2 = 2e-2, 3e-2


def _against_oracle(got, want, what, tol=(TOL_MAX, TOL_L2)):
    worst = [0.0, 0.0]
    mx, l2 = rel_errors(got["audio"], want["audio"])
    print(f"{what}: audio max/peak {mx.max():.3e}  L2 {l2.max():.3e}")
    worst = [max(worst[0], mx.max()), max(worst[1], l2.max())]
    for i in range(len(rs.MODES)):
        rows = np.array([got["qnorm"][(i, b)] for b in range(rs.NB)], dtype=np.float64)
        wrows = np.array([want["qnorm"][(i, b)] for b in range(rs.NB)])
        # the rows of one object against the object's largest row entry; the state likewise
        peak = np.abs(wrows).max() or 1.0
        qm = np.abs(rows - wrows).max() / peak
        ql = np.linalg.norm(rows - wrows) / max(np.linalg.norm(wrows), 1e-300)
        sg = np.concatenate(got["state"][i]).astype(np.float64)
        sw = np.concatenate(want["state"][i])
        sm = np.abs(sg - sw).max() / (np.abs(sw).max() or 1.0)
        sl = np.linalg.norm(sg - sw) / max(np.linalg.norm(sw), 1e-300)
        print(f"{what}: object {i}: qnorm max/peak {qm:.3e} L2 {ql:.3e}   state max/peak {sm:.3e} L2 {sl:.3e}")
        worst = [max(worst[0], qm, sm), max(worst[1], ql, sl)]
    assert worst[0] <= tol[0] and worst[1] <= tol[1], (what, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [False, True], ids=["zero", "keep"])
@pytest.mark.parametrize("form,frames,sel", MAIN_FORMS)
def test_mid_run_retune_against_the_oracles_set_integrator(form, frames, sel, keep):
    """after two buffers: the engine gets pbso_set_material, the oracle solver or_integrator_build + or_solver_set_integrator
    (keep: with the old state copied in, the copy the CPU test above validates)"""
    key = ("oracle", keep)
    if key not in _fresh:
        _fresh[key] = rs.run_oracle(rs.MAT1, swap=(rs.CUT, rs.MAT2, keep))
    got = rs.run(rs.MAT1, between=rs.retune_to(rs.MAT2, keep=keep), **_kw(form, frames, sel))
    tol = (TOL_DIRECT_MAX, TOL_DIRECT_L2) if form == capi.FORM_DIRECT else (TOL_MAX, TOL_L2)
    _against_oracle(got, _fresh[key], f"form {form} keep {int(keep)}", tol)


# ---- 7: state carried on, against a restored engine --------------------------------------------------------------------------------
# pbso_read_state -> pbso_write_state is an exact round trip for the form listed here (established with ONE material and two
# engines: test_state_round_trip_mid_run below).  The per-sample kernel keeps (scale x state, scale) and write_state stores scale 1,
# so a restored engine rounds differently from the next sample on, by an ulp of f32: the velocity and direct forms, and the
# split-bf16 block form, whose dense-profile launches of this script run on the per-sample kernel.  Tolerance of test 6 there
# (measured: round trip 8e-7 ... 9e-6, restored 4e-7 ... 2.5e-5 of peak).
EXACT_ROUND_TRIP = (capi.FORM_BLOCK,)


def _restore_from(src):
    def hook(eng):
        for i in range(len(rs.MODES)):
            eng.set_state(i, *src[i])
    return hook


def _compare_restored(a, c, form, what):
    if form in EXACT_ROUND_TRIP:
        rs.same_run(a, c)
    else:
        _against_oracle(a, dict(audio=c["audio"].astype(np.float64), qnorm=c["qnorm"], state=c["state"]), what)


@pytest.mark.gpu
@pytest.mark.parametrize("form,frames,sel", MAIN_FORMS)
def test_state_round_trip_mid_run(form, frames, sel):
    """one material, two engines: the second one gets its own state written back after two buffers"""
    grabbed = {}
    a = rs.run(rs.MAT1, between=lambda eng: grabbed.update(s=[eng.state(i) for i in range(4)]), **_kw(form, frames, sel))
    c = rs.run(rs.MAT1, between=_restore_from(grabbed["s"]), **_kw(form, frames, sel))
    _compare_restored(a, c, form, f"round trip, form {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form,frames,sel", MAIN_FORMS)
def test_kept_state_continues_as_a_restored_engine_of_the_new_material(form, frames, sel):
    """A: material 1, retuned to 2 with keep_state after two buffers.  C: material 2 from the start (the same force bookkeeping),
    given A's state at that point.  Bit for bit in the f32 block form, within the oracle tolerance in the forms whose state round
    trip is not exact (block_bf16, velocity, direct: see EXACT_ROUND_TRIP)."""
    grabbed = {}

    def at_cut(eng):
        before = [eng.state(i) for i in range(4)]
        eng.set_material([0, 1, 2, 3], *rs.MAT2, keep_state=True)
        after = [eng.state(i) for i in range(4)]
        for i in range(4):                                  # what pbso_read_state returns is the same before and after the call
            assert np.array_equal(before[i][0], after[i][0]) and np.array_equal(before[i][1], after[i][1])
        assert max(np.abs(s[0]).max() for s in before) > 0
        grabbed["s"] = before
    a = rs.run(rs.MAT1, between=at_cut, **_kw(form, frames, sel))
    c = rs.run(rs.MAT2, between=_restore_from(grabbed["s"]), **_kw(form, frames, sel))
    # from the retune point on: C's first two buffers ran with material 2, A's with material 1
    cut = rs.CUT * 513
    a["audio"], c["audio"] = a["audio"][:, cut:].copy(), c["audio"][:, cut:].copy()
    for i in range(4):
        for b in range(rs.CUT):
            a["qnorm"][(i, b)] = c["qnorm"][(i, b)] = np.zeros(rs.MODES[i], dtype=np.float32)
    assert np.abs(a["audio"]).max() > 0
    _compare_restored(a, c, form, f"restored, form {form}")


@pytest.mark.gpu
@pytest.mark.parametrize("form,frames,sel", MAIN_FORMS)
def test_keep_state_zero_clears_the_named_objects_only(form, frames, sel):
    seen = {}

    def at_cut(eng):
        before = [eng.state(i) for i in range(4)]
        eng.set_material([1, 3], *rs.MAT2, keep_state=False)
        after = [eng.state(i) for i in range(4)]
        seen.update(before=before, after=after)
    rs.run(rs.MAT1, between=at_cut, **_kw(form, frames, sel))
    for i in (1, 3):
        assert np.abs(seen["before"][i][0]).max() > 0 and not seen["after"][i][0].any() and not seen["after"][i][1].any()
    for i in (0, 2):
        assert np.array_equal(seen["before"][i][0], seen["after"][i][0]) and np.array_equal(seen["before"][i][1], seen["after"][i][1])


# ---- 8: the multi-listener mix ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("enable_first", [True, False])
def test_listener_mix_after_a_retune_equals_the_fresh_engines(enable_first):
    """pbso_listeners_enable builds the object's f32 operand table from the HOST's c1 / c2: enabled after the retune it must see the
    new ones, enabled before it the table is rebuilt with the others"""
    from openpbso_amd import Engine, ForceMessage
    from openpbso_amd.solver import PbsoError
    lam = synth.eigenvalues(65, 4200)
    shapes = synth.mode_shapes(65, 4200, rs.N_VERTS)
    maps = synth.ffat_maps(lam, 4243, dim=4, cell_size=0.01)
    pos = synth.listener_path(3, radius=0.4)
    vn = synth.unit_normals(2, 5)
    mixes = []
    for retune in (True, False):
        with Engine(form=capi.FORM_BLOCK) as eng:
            m = rs.MAT1 if retune else rs.MAT2
            oid = eng.add_object(lam, *m, mode_shapes=shapes)
            eng.set_ffat_maps(oid, maps)
            eng.finalize()
            if retune and enable_first:
                eng.listeners_enable(oid)
                eng.enqueue_force(oid, ForceMessage(vid=1, vn=vn[0]), 0)
                eng.step(1)
                eng.mix_listeners(oid, pos)
                eng.set_material([oid], *rs.MAT2, keep_state=False)
                with pytest.raises(PbsoError):            # the last step's states were stepped with the old material
                    eng.mix_listeners(oid, pos)
            elif retune:
                eng.set_material([oid], *rs.MAT2)
                eng.listeners_enable(oid)
            else:
                eng.listeners_enable(oid)
            stamp = 1 if (retune and enable_first) else 0
            eng.enqueue_force(oid, ForceMessage(vid=2, vn=vn[1]), stamp)
            eng.enqueue_force(oid, ForceMessage(vid=4, vn=vn[0]), stamp + 2)
            eng.step(3)
            mixes.append((eng.mix_listeners(oid, pos).copy(), eng.audio().copy()))
    assert np.array_equal(mixes[0][0], mixes[1][0]) and np.array_equal(mixes[0][1], mixes[1][1])
    assert np.abs(mixes[0][0]).max() > 0


# ---- 9: errors and atomicity -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_calls_change_nothing():
    import ctypes as C
    from openpbso_amd import Engine
    from openpbso_amd.solver import PbsoError, material_array
    with Engine(form=capi.FORM_BLOCK) as eng:
        eng.add_object(rs.LAMS[1], *rs.MAT1)
        with pytest.raises(PbsoError) as ei:
            eng.set_material([0], *rs.MAT2)
        assert ei.value.status == capi.ERR_STATE            # before finalize
    want = fresh(rs.MAT1, capi.FORM_BLOCK)
    nan, inf = float("nan"), float("inf")
    bad = [
        ([4], rs.MAT2), ([-1], rs.MAT2), ([0, 1, 0], rs.MAT2),                     # out of range, named twice
        ([1], (nan, 25.0, 3e-7)), ([1], (1900.0, inf, 3e-7)), ([1], (1900.0, 25.0, nan)),
        ([2], (0.0, 25.0, 3e-7)), ([2], (-1900.0, 25.0, 3e-7)),
        ([0, 3], rs.OVERDAMPED),                             # an over-damped mode: c1 / c3 not finite
        ([0, 1, 2, 3], ([1900.0, 1900.0, 1900.0, -1.0], 25.0, 3e-7)),              # the LAST of four is bad: the first three stay too
    ]

    def refused(eng):
        lib, h = eng._l, eng._h
        ip = C.POINTER(C.c_int)
        one = np.zeros(1, dtype=np.int32)
        mats = material_array([0], *rs.MAT2)
        assert lib.pbso_set_material(h, -1, one.ctypes.data_as(ip), mats, 1) == capi.ERR_INVALID
        assert lib.pbso_set_material(h, 1, None, mats, 1) == capi.ERR_INVALID
        assert lib.pbso_set_material(h, 1, one.ctypes.data_as(ip), None, 1) == capi.ERR_INVALID
        for ids, m in bad:
            with pytest.raises(PbsoError) as ei:
                eng.set_material(ids, *m, keep_state=False)
            assert ei.value.status == capi.ERR_INVALID, (ids, m)
        assert [eng.material(i) for i in range(4)] == [rs.MAT1] * 4
        assert eng.material_stats() == (0, 0, 0, 0)
        eng.set_material([], *rs.MAT2)                      # n == 0: accepted, nothing to do
        assert eng.material_stats() == (1, 0, 0, 0)
    a = rs.run(rs.MAT1, before=refused, between=refused_mid(bad), form=capi.FORM_BLOCK)
    rs.same_run(a, want)


def refused_mid(bad):
    from openpbso_amd.solver import PbsoError

    def hook(eng):
        for ids, m in bad:
            with pytest.raises(PbsoError):
                eng.set_material(ids, *m, keep_state=False)
    return hook


@pytest.mark.gpu
def test_material_stats_count_as_documented():
    eng = rs.build_engine(rs.MAT1, form=capi.FORM_BLOCK)
    try:
        m_pad = eng.info()["modes_padded"]
        eng.set_material([1, 2], *rs.MAT2)
        assert eng.material_stats() == (1, 2, 265, 2 * 15 * m_pad)
        eng.set_material([0, 3], [1000.0, 3000.0], 10.0, [1e-7, 2e-7], keep_state=False)      # scalars broadcast
        assert eng.material_stats() == (2, 4, 265 + 1101, 2 * 15 * m_pad)
        assert eng.material(0) == (1000.0, 10.0, 1e-7) and eng.material(3) == (3000.0, 10.0, 2e-7) and eng.material(1) == rs.MAT2
    finally:
        eng.close()


# ---- 10: run-ahead ---------------------------------------------------------------------------------------------------------------------
def _run_ahead(submit_thread, long_launch):
    """several steps with nothing read in between, a retune, more steps; the audio of the last steps and the final state"""
    from openpbso_amd import ForceMessage
    eng = rs.build_engine(rs.MAT1, form=capi.FORM_BLOCK, submit_thread=submit_thread, qnorm=capi.QNORM_OFF, chunk_buffers=256)
    try:
        rs.enqueue_all(eng)
        for _ in range(3):
            eng.step(1)
        if long_launch:
            eng.step(256)                                   # the start-gate path: a launch of >= 256 buffers in flight at the call
        eng.set_material([0, 1, 2, 3], *rs.MAT2, keep_state=True)
        eng.enqueue_force(2, ForceMessage(vid=1, vn=(0.0, 0.6, 0.8)), 0)
        out = []
        for _ in range(3):
            eng.step(1)
            out.append(eng.audio().copy())
        return np.concatenate(out, axis=1), [eng.state(i) for i in range(4)]
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("long_launch", [False, True])
def test_retune_behind_run_ahead_steps_equals_the_direct_path(long_launch):
    a, sa = _run_ahead(1, long_launch)
    b, sb = _run_ahead(0, long_launch)
    assert np.array_equal(a, b) and np.abs(a).max() > 0
    for i in range(4):
        assert np.array_equal(sa[i][0], sb[i][0]) and np.array_equal(sa[i][1], sb[i][1])


# ---- 11: the device group ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_group_set_material_in_a_loopback_group_equals_the_engine():
    from openpbso_amd.group import Group
    from openpbso_amd.solver import PbsoError
    want = fresh(rs.MAT1, capi.FORM_BLOCK)
    single = rs.run(rs.MAT1, between=rs.retune_to(rs.MAT2, ids=[3, 0, 1], keep=False), form=capi.FORM_BLOCK)
    assert not np.array_equal(single["audio"], want["audio"])
    with Group([0, 0], transport=capi.GROUP_LOOPBACK, form=capi.FORM_BLOCK) as grp:
        grp.plan(rs.MODES)
        assert grp.span(0)[1] < 4                           # both ranks own objects
        for i in range(4):
            grp.add_object(i, rs.LAMS[i], *rs.MAT1, mode_shapes=rs.SHAPES[i])
        grp.finalize()
        for r in range(2):
            lo, hi = grp.span(r)
            for i in range(hi - lo):
                grp.engine(r).set_use_transfer(i, False)
        for ev in rs.events():
            assert grp.enqueue_force(ev["obj"], rs._msg(ev), ev["t"])
        got = []
        rows = [grp.owner(i) for i in range(4)]
        cmax = max(grp.span(r)[1] - grp.span(r)[0] for r in range(2))      # the gathered block: [world][cmax] rows

        def gathered():
            grp.gather(capi.GATHER_ALL)
            res = grp.result(0)
            return np.array([res[r * cmax + l] for r, l in rows])
        grp.step(rs.CUT)
        got.append(gathered())
        with pytest.raises(PbsoError):                      # the bad id belongs to rank 1: rank 0's object is not retuned either
            grp.set_material([0, 3], [1900.0, -1.0], 25.0, 3e-7)
        with pytest.raises(PbsoError):
            grp.set_material([0, 4], *rs.MAT2)
        assert grp.engine(0).material(0) == rs.MAT1
        grp.set_material([3, 0, 1], *rs.MAT2, keep_state=False)
        grp.step(rs.NB - rs.CUT)
        got.append(gathered())
    assert np.array_equal(np.concatenate(got, axis=1), single["audio"])
