"""The product boundary of the scene filter mix's bank, without a GPU: the nine entry points in the header, in capi.EXPORTS and in
the built library; the unchanged ABI version; the refusal of every call without an engine or group; the header's rules for a bank
set; the Python methods.  (An engine needs a device, so what a call refuses on an enabled mixer -- an index out of range, a
non-finite weight, the overflow bound, J of 0 or 9, the spacing rule, no bank -- is in tests/test_gpu_scene_fir_bank.py, and the
chain itself in tests/test_scene_fir_bank_ref.py.)"""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_CALLS = ("pbso_scene_fir_bank_create", "pbso_scene_fir_bank_info", "pbso_scene_fir_set_bank", "pbso_scene_fir_set_bank_at",
                "pbso_scene_fir_bank_schedule")
GROUP_CALLS = ("pbso_group_scene_fir_bank_create", "pbso_group_scene_fir_set_bank", "pbso_group_scene_fir_set_bank_at",
               "pbso_group_scene_fir_bank_schedule")


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
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)       # entry points were added, none changed
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def test_every_call_refuses_a_missing_engine_or_group():
    capi = _capi()
    lib = capi.lib()
    t = (C.c_int64 * 2)(0, 5)
    taps, index, weight = (C.c_float * 2)(1.0, 1.0), (C.c_int * 2)(0, 0), (C.c_float * 2)(1.0, 1.0)
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.pbso_scene_fir_bank_create(None, 1, taps) == capi.ERR_STATE
    assert lib.pbso_scene_fir_bank_info(None, out) == capi.ERR_STATE and list(out) == [7, 7, 7, 7]
    assert lib.pbso_scene_fir_set_bank(None, 1, index, weight, None) == capi.ERR_STATE
    assert lib.pbso_scene_fir_set_bank_at(None, 0, 1, index, weight, index) == capi.ERR_STATE
    assert lib.pbso_scene_fir_bank_schedule(None, 2, t, 1, index, weight, None) == capi.ERR_STATE
    assert lib.pbso_group_scene_fir_bank_create(None, 1, taps) == capi.ERR_STATE
    assert lib.pbso_group_scene_fir_set_bank(None, 1, index, weight, None) == capi.ERR_STATE
    assert lib.pbso_group_scene_fir_set_bank_at(None, 0, 1, index, weight, index) == capi.ERR_STATE
    assert lib.pbso_group_scene_fir_bank_schedule(None, 2, t, 1, index, weight, None) == capi.ERR_STATE


def test_header_states_the_rules_of_a_bank_set():
    hdr = " ".join(open(os.path.join(ROOT, "include", "openpbso_amd.h")).read().replace(" * ", " ").split())
    for phrase in ("acc = 0.f; for j = 0 .. J-1 ascending: acc = fmaf(weight[o][j], bank[index[o][j]][c][k], acc); h_co[k] = acc",
                   "1 <= J <= 8", "a bank set IS the plain or scheduled set with those taps",
                   "J = 1 with weight 1.f is the bank's filter itself", "The same index may occur twice for one object",
                   "Bank sets and taps sets are one ordered kind", "either may follow the other",
                   "VALIDATION, ALL OR NOTHING, before anything is taken", "Every index in [0, F), every weight finite",
                   # (the line joiner above eats " * ": the product's sign is the one token not looked for)
                   "sum_j |weight[o][j]|", "A <= FLT_MAX in fp64, A = max |bank tap| computed once at creation",
                   "a call before the enable or without a bank is PBSO_ERR_STATE", "1 <= F <= 1 << 20",
                   "returns PBSO_ERR_NOMEM and the mixer is as it was",
                   "A second create replaces the bank; it is PBSO_ERR_STATE while bank sets are pending",
                   "Sets already taken by a mix are materialised taps and are not affected", "pbso_scene_fir_reset keeps the bank",
                   "A new pbso_scene_fir_enable drops the bank", "out[3] = device bytes of the bank",
                   "object-major, so every rank takes a contiguous slice"):
        assert phrase in hdr, phrase


def test_python_methods_exist():
    from openpbso_amd.group import Group
    from openpbso_amd.solver import Engine
    for m in ("scene_fir_bank_create", "scene_fir_bank_info", "scene_fir_set_bank", "scene_fir_set_bank_at", "scene_fir_bank_schedule"):
        assert callable(getattr(Engine, m)), m
        assert callable(getattr(Group, m)), m
