"""The product boundary of the scene filter mix's schedule, without a GPU: the eleven entry points in the header, in capi.EXPORTS and
in the built library; the unchanged ABI version; the refusal of every call without an engine; the header's rules for a scheduled
set; the Python methods.  (An engine needs a device, so what a call refuses on an enabled mixer -- descending times, a t_set
before the clock, the spacing rule, a NaN tap, an onset out of range, a delay schedule without the stage -- is in
tests/test_gpu_scene_fir_schedule.py, and the spacing arithmetic itself in tests/test_fir_schedule_check.py.)"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_CALLS = ("pbso_scene_fir_set_at", "pbso_scene_fir_schedule", "pbso_scene_fir_set_delay_at", "pbso_scene_fir_delay_schedule",
                "pbso_scene_fir_clear_schedule", "pbso_scene_fir_schedule_info")
GROUP_CALLS = ("pbso_group_scene_fir_set_at", "pbso_group_scene_fir_schedule", "pbso_group_scene_fir_set_delay_at",
               "pbso_group_scene_fir_delay_schedule", "pbso_group_scene_fir_clear_schedule")


def _capi():
    from openpbso_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi


def test_entry_points_in_header_exports_and_library():
    capi = _capi()
    hdr = open(os.path.join(ROOT, "include", "openpbso_amd.h")).read()
    declared = set(re.findall(r"\b(pbso_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.lib()
    for name in ENGINE_CALLS + GROUP_CALLS:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def test_every_call_refuses_a_missing_engine_or_group():
    capi = _capi()
    lib = capi.lib()
    t = (C.c_int64 * 2)(0, 5)
    taps, onset, out = (C.c_float * 2)(1.0, 1.0), (C.c_int * 2)(0, 0), (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.pbso_scene_fir_set_at(None, 0, taps, onset) == capi.ERR_STATE
    assert lib.pbso_scene_fir_schedule(None, 2, t, taps, None) == capi.ERR_STATE
    assert lib.pbso_scene_fir_set_delay_at(None, 0, taps) == capi.ERR_STATE
    assert lib.pbso_scene_fir_delay_schedule(None, 2, t, taps) == capi.ERR_STATE
    assert lib.pbso_scene_fir_clear_schedule(None) == capi.ERR_STATE
    assert lib.pbso_scene_fir_schedule_info(None, out) == capi.ERR_STATE and list(out) == [7, 7, 7, 7]
    assert lib.pbso_group_scene_fir_set_at(None, 0, taps, onset) == capi.ERR_STATE
    assert lib.pbso_group_scene_fir_schedule(None, 2, t, taps, None) == capi.ERR_STATE
    assert lib.pbso_group_scene_fir_set_delay_at(None, 0, taps) == capi.ERR_STATE
    assert lib.pbso_group_scene_fir_delay_schedule(None, 2, t, taps) == capi.ERR_STATE
    assert lib.pbso_group_scene_fir_clear_schedule(None) == capi.ERR_STATE


def test_header_states_the_rules_of_a_scheduled_set():
    hdr = " ".join(open(os.path.join(ROOT, "include", "openpbso_amd.h")).read().replace(" * ", " ").split())
    for phrase in ("with t_set given by the caller", "fades in from the set in force at t_set - 1",
                   "onset == NULL keeps the onsets of the set before it", "from p(t_set - 1) of the record in force at t_set - 1",
                   "z(tau) uses the record in force at tau", "takes effect without a fade or ramp, whichever call made it",
                   "cut at every t_set with pbso_scene_fir_set / pbso_scene_fir_set_delay before each piece",
                   "strictly greater than the last pending set's of its kind", "t_set - t_prev + 1 >= R",
                   "whenever there is a predecessor and R >= 2", "delay sets may follow each other at any spacing",
                   "validate all of their sets before they take any", "n_sets == 0 is accepted",
                   "At most 4096 filter sets and 65 536 delay sets", "PBSO_ERR_NOMEM and nothing has changed",
                   "S + 2 padded filter sets", "K_d + 1 blocks of",
                   "While scheduled sets of its kind are pending the plain set returns PBSO_ERR_STATE", "mid-ramp included",
                   "drops the pending filter AND delay sets not yet in force", "the reset keeps the delays last IN FORCE",
                   "out[3] = the smallest t_set the next scheduled filter set may have"):
        assert phrase in hdr, phrase


def test_python_methods_exist():
    from openpbso_amd.group import Group
    from openpbso_amd.solver import Engine
    for m in ("scene_fir_set_at", "scene_fir_schedule", "scene_fir_set_delay_at", "scene_fir_delay_schedule", "scene_fir_clear_schedule",
              "scene_fir_schedule_info"):
        assert callable(getattr(Engine, m)), m
        assert callable(getattr(Group, m)), m
