"""The scene filter mix's product boundary, without a GPU: the eight entry points in the header, in capi.EXPORTS and in the built
library; the gather mode; the unchanged ABI version; the Python methods."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_scene_fir_enable", "pbso_scene_fir_set", "pbso_scene_fir", "pbso_read_scene_fir", "pbso_scene_fir_reset",
                "pbso_scene_fir_info", "pbso_group_scene_fir_enable", "pbso_group_scene_fir_set")


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
    assert re.search(r"PBSO_GATHER_FIR\s*=\s*5\b", hdr)
    assert capi.GATHER_FIR == 5
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def test_header_states_the_order_of_arithmetic():
    hdr = open(os.path.join(ROOT, "include", "openpbso_amd.h")).read()
    for phrase in ("fmaf(h[k], x(t - D - k), acc)", "k = K-1 down to 0", "group of 32 consecutive objects", "three separately rounded",
                   "w(t) = (float)((double)(t - t_set + 1) / (double)R)"):
        assert phrase in hdr, phrase


def test_python_methods_exist():
    from openpbso_amd.group import Group
    from openpbso_amd.solver import Engine
    for m in ("scene_fir_enable", "scene_fir_set", "scene_fir", "read_scene_fir", "scene_fir_reset", "scene_fir_info"):
        assert callable(getattr(Engine, m)), m
    for m in ("scene_fir_enable", "scene_fir_set"):
        assert callable(getattr(Group, m)), m
