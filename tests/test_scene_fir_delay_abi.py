"""The product boundary of the scene filter mix's delay stage, without a GPU: the five entry points in the header, in capi.EXPORTS
and in the built library; the unchanged ABI version; the header's statement of the delay's arithmetic; the Python methods."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_scene_fir_delay_enable", "pbso_scene_fir_set_delay", "pbso_scene_fir_delay_info",
                "pbso_group_scene_fir_delay_enable", "pbso_group_scene_fir_set_delay")


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


def test_header_states_the_delays_arithmetic():
    hdr = open(os.path.join(ROOT, "include", "openpbso_amd.h")).read()
    for phrase in ("i0 = tau - (long)floor(d) - (fr != 0)", "(float)(1.0 - fr)", "record in force at",
                   "x_o(i0) + f * (x_o(i0 + 1) - x_o(i0))", "three rounded f32 operations, none fused"):
        assert phrase in hdr, phrase


def test_python_methods_exist():
    from openpbso_amd.group import Group
    from openpbso_amd.solver import Engine
    for m in ("scene_fir_delay_enable", "scene_fir_set_delay", "scene_fir_delay_info"):
        assert callable(getattr(Engine, m)), m
    for m in ("scene_fir_delay_enable", "scene_fir_set_delay"):
        assert callable(getattr(Group, m)), m
