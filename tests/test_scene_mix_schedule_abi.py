"""The product boundary of the scene mix's schedule, without a GPU: the seven entry points in the header, in capi.EXPORTS and in the
built library; the unchanged ABI version; the header's rules for a scheduled set; the Python methods."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_scene_mix_set_at", "pbso_scene_mix_schedule", "pbso_scene_mix_clear_schedule", "pbso_scene_mix_info",
                "pbso_group_scene_mix_set_at", "pbso_group_scene_mix_schedule", "pbso_group_scene_mix_clear_schedule")


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
    for name in ENTRY_POINTS:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def test_header_states_the_rules_of_a_scheduled_set():
    hdr = " ".join(open(os.path.join(ROOT, "include", "openpbso_amd.h")).read().replace(" * ", " ").split())
    for phrase in ("with t_set given by the caller", "the record in force at t_set - 1", "divided once",
                   "takes effect without a ramp, whichever call made it", "delay == NULL leaves the delay records untouched",
                   "the record in force is that of the latest set with t_set <= t", "strictly greater than the last pending scheduled set's",
                   "validates all of its sets before it takes any", "stays pending until the step that contains it",
                   "At most 65 536 sets", "PBSO_ERR_NOMEM and nothing has changed",
                   "While scheduled sets are pending pbso_scene_mix_set returns PBSO_ERR_STATE", "mid-ramp included",
                   "the reset keeps the targets last IN FORCE", "out[1] = scheduled sets still pending"):
        assert phrase in hdr, phrase


def test_python_methods_exist():
    from openpbso_amd.group import Group
    from openpbso_amd.solver import Engine
    for m in ("scene_mix_set_at", "scene_mix_schedule", "scene_mix_clear_schedule", "scene_mix_info"):
        assert callable(getattr(Engine, m)), m
        assert callable(getattr(Group, m)), m
