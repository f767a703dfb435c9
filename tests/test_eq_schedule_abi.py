"""The EQ bus's schedule at the product boundary, without a GPU: the four entry points in the header, in capi.EXPORTS and in the
built library; the unchanged ABI version; the Python methods; the SCHEDULE block's rules; the new kernels' resource listing; the
host arithmetic of csrc/eq_schedule.h through its check program (built with the host compiler under ASan + UBSan and run as a
program of its own); the headless tool's refusals."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("pbso_eq_set_at", "pbso_eq_schedule", "pbso_eq_clear_schedule", "pbso_eq_schedule_info")
KERNELS = ("eq_sched_tables_kernel", "eq_sched_input_kernel", "eq_sched_forward_kernel", "eq_sched_chain_kernel", "eq_sched_finish_kernel",
           "eq_sched_output_kernel")


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
        assert getattr(lib, name).argtypes, name
    assert re.search(r"#define\s+PBSO_ABI_VERSION\s+6\b", hdr)
    assert capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def test_python_methods_exist():
    _capi()
    from openpbso_amd.solver import Engine
    for m in ("eq_set_at", "eq_schedule", "eq_clear_schedule", "eq_schedule_info"):
        assert callable(getattr(Engine, m)), m


def test_header_states_the_schedule():
    hdr = _header()
    at = hdr.index("The EQ bus's SCHEDULE")
    assert at > hdr.index("int pbso_eq_design(")          # behind the EQ block, which stays as it is
    block = hdr[at:hdr.index("int pbso_eq_schedule_info(")]
    flat = " ".join(block.replace("\n *", " ").split())
    for phrase in ("EFFECT.", "VALIDATION, ALL OR NOTHING.", "LIFETIME.", "WITH pbso_eq_set.",
                   "A scheduled set does exactly what pbso_eq_set does, with t_set given by the caller",
                   "block origins are t_set + g * P", "for t < t_set every one of its signals is the value of the cascade in force at t",
                   "From keeps running on its own grid through t_set + R - 2", "three f32 operations",
                   "bit for bit, the same input cut at every t_set with pbso_eq_set before each piece",
                   "t_set must be >= the next processed sample", "strictly greater than the last pending set's",
                   "counts as pending at the next processed sample", "No set while a fade runs",
                   "t_set - t_prev + 1 >= R whenever R >= 2", "the identity installed by enable or reset is a predecessor with t_set = 0",
                   "validated as pbso_eq_set validates them", "PBSO_ERR_INVALID", "validates all of its sets before it takes any",
                   "PBSO_ERR_STATE before the enable", "n_sets == 0 is accepted", "stays pending until the step that contains it",
                   "At most 65 536 sets may be pending", "At most 4096 sets may take effect inside one processed step",
                   "n_sets_in_step * C * S * 5 * P doubles", "PBSO_ERR_NOMEM and nothing has changed",
                   "launched exactly as without a schedule", "While scheduled sets are pending pbso_eq_set returns PBSO_ERR_STATE",
                   "mid-fade included", "pbso_eq_clear_schedule drops the sets not yet in force",
                   "pbso_eq_reset and a new pbso_eq_enable drop them too", "out[0] = t of the next processed sample",
                   "out[1] = scheduled sets pending", "out[2] = the smallest t_set the next scheduled set may have",
                   "out[3] = the number of sets that took effect inside the last processed step",
                   "pbso_eq_info out[3] counts every set of a pbso_eq_schedule call",
                   "pbso_eq_tables returns the tables of the last set that has taken effect"):
        assert phrase in flat, phrase


def test_kernels_use_no_scratch():
    _capi()
    path = os.path.join(ROOT, "openpbso_amd", "csrc", "kernels_eq_schedule.resources.txt")
    if not os.path.exists(path):                         # (a library from another build of the tree: make the listing)
        subprocess.run(["make", "-C", os.path.dirname(path), "kernels_eq_schedule.o"], check=True, capture_output=True)
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) == len(KERNELS)
    for kernel in KERNELS:
        assert sum(kernel in n for n in names) == 1, kernel
    assert all(s == 0 for s in scratch), list(zip(names, scratch))
    assert "warning" not in text
    # built as kernels_eq.o is: no contraction, no fast-math or denormal flag
    rule = re.search(r"^kernels_eq_schedule\.o:.*\n\t(.*)$", open(os.path.join(os.path.dirname(path), "Makefile")).read(), re.M).group(1)
    assert "-ffp-contract=off" in rule and "-Rpass-analysis=kernel-resource-usage" in rule
    assert not re.search(r"fast-math|denorm|-Ofast", rule)


def test_the_check_program_passes_under_the_sanitizers():
    csrc = os.path.join(ROOT, "openpbso_amd", "csrc")
    b = subprocess.run(["make", "-C", csrc, "eq_schedule_check"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    rule = re.search(r"^eq_schedule_check:.*\n\t(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M).group(1)
    assert rule.startswith("g++") and "-fsanitize=address,undefined" in rule and "-ffp-contract=off" in rule
    r = subprocess.run([os.path.join(ROOT, "openpbso_amd", "eq_schedule_check")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "eq_schedule_check: all ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "FAIL" not in r.stdout
    # what it pins: the pair positions of a block cut at k = 0, 1, P - 2, P - 1, and the scenarios of the hazards
    for k, L in ((0, 64), (1, 1), (62, 62), (63, 63)):
        assert re.search(rf"cut at k={k}: block o=\d+ L={L} ", r.stdout), k
    for name in ("70 one-sample sets at a step end", "27 frames", "first and last sample", "tail at the step end", "spacing R-1",
                 "predecessor offset"):
        for R in (0, 2) if name.startswith("70") else (0, 1, 2, 3, 64, 67, 200):
            assert re.search(rf"scenario {re.escape(name)} S=\d R={R} .* ok", r.stdout), (name, R)


def test_headless_refuses_bad_eq_schedule_flags_before_it_needs_a_device(tmp_path):
    _capi()
    from tests.test_headless_cli import EXE, make_data_dir
    d = tmp_path / "data"
    d.mkdir()
    make_data_dir(d)
    (tmp_path / "pan.txt").write_text("0 0 1.0 0.0 0.5 10.0\n")
    (tmp_path / "eq.txt").write_text("1 0 highpass 30 0.707 0\n2 1 peak 1000 2 -9\n")
    (tmp_path / "early.txt").write_text("0 0 highpass 30 0.707 0\n2 1 peak 1000 2 -9\n")
    base = [EXE, "-d", str(d), "--buffers", "4", "--out", str(tmp_path / "o.wav")]
    mixed = ["--channels", "2", "--pan", str(tmp_path / "pan.txt")]
    for extra, msg in ((mixed + ["--eq-schedule"], "--eq-schedule needs --eq"),
                       (["--eq-schedule"], "--eq-schedule needs --eq"),
                       # buffers 1 and 2 are 513 samples apart: a fade of 515 needs 514
                       (mixed + ["--eq", str(tmp_path / "eq.txt"), "--eq-schedule", "--eq-xfade", "515"], "closer to their predecessor than the fade allows"),
                       # the identity is a predecessor at sample 0
                       (mixed + ["--eq", str(tmp_path / "early.txt"), "--eq-schedule", "--eq-xfade", "2"], "closer to their predecessor than the fade allows")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    assert not (tmp_path / "o.wav").exists()
