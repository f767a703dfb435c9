"""The per-lane bodies of the retune kernels (csrc/mode_tables.h: retune_lane, retune_g32_lane -- what csrc/kernels_retune.hip runs per
lane) against the vector builders of csrc/engine_tables.h (what finalize uploads), bit for bit, on the host alone:
tests/cpp/retune_tables_check.cpp is built with the host compiler, -ffp-contract=off and -fsanitize=address,undefined and run as a
program of its own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_retune_lane_bodies_equal_the_host_builders_under_asan_and_ubsan():
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "openpbso_amd", "csrc"), "retune_tables_check"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "openpbso_amd", "retune_tables_check")], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "retune tables check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
