"""pbso_set_material's product boundary, without a GPU: the entry points in the header, in capi.EXPORTS and in the built library; the
unchanged ABI version; the 24-byte material record in C and in Python; the Python methods; the semantics the header states; the
retune kernels built without scratch; the headless tool's refusals of bad --retune lines."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_set_material", "pbso_get_material", "pbso_material_stats", "pbso_group_set_material")


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
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def test_the_material_record_is_24_bytes_in_c_and_python(tmp_path):
    capi = _capi()
    assert C.sizeof(capi.Material) == 24
    assert [(n, getattr(capi.Material, n).offset) for n, _ in capi.Material._fields_] == [("density", 0), ("alpha", 8), ("beta", 16)]
    assert re.search(r"typedef struct pbso_material \{ double density, alpha, beta; \} pbso_material;", _header())
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include "openpbso_amd.h"\n'
                   "_Static_assert(sizeof(pbso_material) == 24, \"24 bytes\");\n"
                   "_Static_assert(offsetof(pbso_material, alpha) == 8 && offsetof(pbso_material, beta) == 16, \"layout\");\n"
                   "int main(void) { return 0; }\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "size")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_methods_exist():
    from openpbso_amd.group import Group
    from openpbso_amd.solver import Engine
    for m in ("set_material", "material", "material_stats"):
        assert callable(getattr(Engine, m)), m
    assert callable(Group.set_material)


def test_header_states_the_semantics():
    hdr = " ".join(_header().split())
    for phrase in ("It takes effect at the first sample of the next step, for every sample of that step on",
                   "keep_state != 0: the state pbso_read_state returns is the same immediately before and after the call",
                   "keep_state == 0: q_{k-1} = q_{k-2} = 0 for the named objects",
                   "Everything is validated before the device is touched; on any error nothing has changed",
                   "all or nothing within the ranks of this process",
                   "the maps were computed for the material they were loaded with",
                   "The mode count of an object stays as given to pbso_add_object",
                   "it costs a device synchronisation"):
        assert phrase.replace(" * ", " ") in hdr.replace(" * ", " "), phrase


def test_retune_kernels_build_without_scratch():
    """the resource listing the build writes beside kernels_retune.o (as for kernels_master.o)"""
    _capi()
    path = os.path.join(ROOT, "openpbso_amd", "csrc", "kernels_retune.resources.txt")
    if not os.path.exists(path):
        b = subprocess.run(["make", "-C", os.path.dirname(path), "-B", "kernels_retune.o"], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr
    txt = open(path).read()
    names = re.findall(r"Function Name: (\S+)", txt)
    assert any("retune_tables_kernel" in n for n in names) and any("retune_g32_kernel" in n for n in names)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", txt)]
    assert len(scratch) == len(names) == 2 and scratch == [0, 0]


def test_headless_refuses_bad_retune_lines_before_it_needs_a_device(tmp_path):
    _capi()
    from tests.test_headless_cli import EXE, make_data_dir
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    mat = d / "bowl_material.txt"
    cases = {
        "missing.txt": (f"1 0 {tmp_path / 'nowhere.txt'}\n", "cannot read material file"),
        "negative.txt": (f"-1 0 {mat}\n", "outside buffers"),
        "late.txt": (f"2 0 {mat}\n", "outside buffers"),
        "word.txt": (f"1 0 {mat} melt\n", "keep or zero"),
        "copy.txt": (f"1 1 {mat} keep\n", "copy that does not exist"),
        "short.txt": ("1 0\n", "bad retune line"),
        "empty.txt": ("# nothing\n", "no lines"),
    }
    base = [EXE, "-d", str(d), "--buffers", "2", "--out", str(tmp_path / "o.wav")]
    for name, (text, msg) in cases.items():
        (tmp_path / name).write_text(text)
        r = subprocess.run(base + ["--retune", str(tmp_path / name)], capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (name, r.stderr)
    r = subprocess.run(base + ["--retune", str(tmp_path / "not_there.txt")], capture_output=True, text=True)
    assert r.returncode != 0 and "cannot read" in r.stderr
    r = subprocess.run(base + ["--retune"], capture_output=True, text=True)
    assert r.returncode != 0 and "missing value" in r.stderr
    assert not (tmp_path / "o.wav").exists()
