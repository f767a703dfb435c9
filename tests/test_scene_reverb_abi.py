"""The scene reverb's product boundary, without a GPU: the six entry points in the header, in capi.EXPORTS and in the built
library; the segment length; the unchanged ABI version; the stated order of arithmetic; the Python methods."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_scene_reverb_enable", "pbso_scene_reverb_set", "pbso_scene_reverb", "pbso_read_scene_reverb",
                "pbso_scene_reverb_reset", "pbso_scene_reverb_info")


def _capi():
    from openpbso_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi


def _header():
    return open(os.path.join(ROOT, "include", "openpbso_amd.h")).read()


def test_entry_points_in_header_exports_and_library():
    capi = _capi()
    hdr = _header()
    declared = set(re.findall(r"\b(pbso_[a-z_0-9]+)\s*\(", hdr))
    lib = capi.lib()
    for name in ENTRY_POINTS:
        assert name in declared and name in capi.EXPORTS and hasattr(lib, name), name
    assert re.search(r"#define\s+PBSO_SCENE_REVERB_SEGMENT\s+2048\b", hdr)
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def test_header_states_the_order_of_arithmetic():
    hdr = _header()
    for phrase in ("for k = min(K, (j+1) S) - 1 down to j S :  acc = fmaf(r_ci[k], u_i(t - k), acc)",
                   "for i ascending, for j ascending :          y = y + p_cij(t)",
                   "out_c(t) = Yfrom_c(t) + w(t) * (Yto_c(t) - Yfrom_c(t))", "three separately rounded",
                   "out_c(t) = add_c(t) + out_c(t)", "w(t) = (float)((double)(t - t_set + 1) / (double)R)",
                   "S is part of the definition", "Subnormals are kept", "within K + 15 samples"):
        assert phrase in hdr, phrase


def test_the_segment_of_the_kernels_and_the_reference_is_the_headers():
    from tests.scene_reverb_model import SEGMENT
    kh = open(os.path.join(ROOT, "openpbso_amd", "csrc", "kernels.h")).read()
    ref = open(os.path.join(ROOT, "tests", "cpp", "scene_reverb_ref.c")).read()
    assert SEGMENT == 2048
    assert re.search(r"SCENE_REVERB_SEGMENT\s*=\s*2048\b", kh) and re.search(r"#define\s+S\s+2048\b", ref)


def test_python_methods_exist():
    from openpbso_amd.solver import Engine
    for m in ("scene_reverb_enable", "scene_reverb_set", "scene_reverb", "read_scene_reverb", "scene_reverb_reset", "scene_reverb_info"):
        assert callable(getattr(Engine, m)), m
