"""The force-track entry points at the product boundary (no GPU): pbso_track_create, pbso_enqueue_track_force and
pbso_track_stats are declared in the header, listed in capi.EXPORTS and exported by the built library; PBSO_TRACK_FORCE is 3;
pbso_track_play has the layout capi.TrackPlay mirrors -- and what other tests pin did not move: the ABI version is still 6 and
pbso_engine_info keeps its layout (the track counters have a call of their own for that reason)."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbso_track_create", "pbso_enqueue_track_force", "pbso_track_stats")
ENGINE_INFO_BYTES = 232
TRACK_PLAY_BYTES = 48                # four ints, one int64, three doubles


def _capi():
    from openpbso_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi


def test_header_declares_and_library_exports_the_track_entry_points():
    capi = _capi()
    hdr = open(os.path.join(ROOT, "include", "openpbso_amd.h")).read()
    declared = set(re.findall(r"^int (pbso_[a-z_0-9]+)\s*\(", hdr, flags=re.M))
    lib = capi.lib()
    for name in NAMES:
        assert name in declared, name
        assert name in capi.EXPORTS, name
        assert hasattr(lib, name), name
    assert re.search(r"PBSO_TRACK_FORCE\s*=\s*3\b", hdr)
    assert capi.TRACK_FORCE == 3


def test_track_play_layout(tmp_path):
    """sizeof and every field offset of pbso_track_play as the C compiler sees the header, against the ctypes mirror"""
    capi = _capi()
    assert C.sizeof(capi.TrackPlay) == TRACK_PLAY_BYTES
    fields = [n for n, _ in capi.TrackPlay._fields_]
    assert fields == ["track", "loop", "start_sample", "reserved", "n_samples", "first", "rate", "gain"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "openpbso_amd.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(pbso_track_play));\n'
                   + "".join(f'    printf(" %zu", offsetof(pbso_track_play, {n}));\n' for n in fields)
                   + '    printf(" %d\\n", (int)PBSO_TRACK_FORCE);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [TRACK_PLAY_BYTES] + [getattr(capi.TrackPlay, n).offset for n in fields] + [3], got


def test_abi_version_and_engine_info_layout_did_not_move():
    capi = _capi()
    assert capi.lib().pbso_abi_version() == 6 == capi.ABI_VERSION
    assert C.sizeof(capi.EngineInfo) == ENGINE_INFO_BYTES


def test_track_calls_refuse_a_null_engine():
    capi = _capi()
    lib = capi.lib()
    out = (C.c_int64 * 4)()
    tid = C.c_int(-1)
    samples = (C.c_float * 4)(0.0, 1.0, 0.0, -1.0)
    msg, play = capi.ForceMsg(), capi.TrackPlay()
    msg.force_type = capi.TRACK_FORCE
    assert lib.pbso_track_stats(None, out) == capi.ERR_STATE
    assert lib.pbso_track_create(None, samples, 4, C.byref(tid)) == capi.ERR_STATE
    assert lib.pbso_enqueue_track_force(None, 0, C.byref(msg), C.byref(play), 0) == capi.ERR_STATE


def test_python_wrapper_has_the_track_methods():
    _capi()
    from openpbso_amd import Engine
    for name in ("create_track", "enqueue_track_force", "track_stats"):
        assert callable(getattr(Engine, name)), name
    assert sys.modules["openpbso_amd.solver"].TRACK_FORCE == 3
