"""The stroke entry points at the product boundary (no GPU): pbso_enqueue_strokes and pbso_stroke_stats are declared in the
header, listed in capi.EXPORTS and exported by the built library -- and the two things other tests pin did not move: the ABI
version is still 6 and pbso_engine_info keeps its layout (the stroke counters have a call of their own for that reason)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbso_enqueue_strokes", "pbso_stroke_stats")
ENGINE_INFO_BYTES = 232              # ctypes.sizeof(capi.EngineInfo) before the stroke entry points were added


def _capi():
    from openpbso_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi


def test_header_declares_and_library_exports_the_stroke_entry_points():
    capi = _capi()
    hdr = open(os.path.join(ROOT, "include", "openpbso_amd.h")).read()
    declared = set(re.findall(r"^int (pbso_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    lib = capi.lib()
    for name in NAMES:
        assert name in declared, name
        assert name in capi.EXPORTS, name
        assert hasattr(lib, name), name
    for flag in ("PBSO_STROKE_START 1u", "PBSO_STROKE_END 2u", "PBSO_STROKE_ZERO 4u"):
        assert "#define " + flag in hdr
    assert (capi.STROKE_START, capi.STROKE_END, capi.STROKE_ZERO) == (1, 2, 4)


def test_abi_version_and_engine_info_layout_did_not_move():
    capi = _capi()
    assert capi.lib().pbso_abi_version() == 6 == capi.ABI_VERSION
    assert C.sizeof(capi.EngineInfo) == ENGINE_INFO_BYTES


def test_stroke_calls_refuse_a_null_engine():
    capi = _capi()
    lib = capi.lib()
    out = (C.c_int64 * 4)()
    assert lib.pbso_stroke_stats(None, out) == capi.ERR_STATE
    assert lib.pbso_enqueue_strokes(None, 0, None, None, None, None, None, None, capi.AUTOREGRESSIVE_FORCE) == capi.ERR_STATE
