"""What Engine::finalize computes and what a launch decides (csrc/engine_tables.h: team tables, coefficient tables;
csrc/launch_policy.h: which kernel, which cut, which hand-over) against their rules, on the host alone:
tests/cpp/engine_tables_check.cpp is built with the host compiler and -fsanitize=address,undefined and run as a program of its
own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_engine_tables_and_launch_policy_under_asan_and_ubsan():
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "openpbso_amd", "csrc"), "engine_tables_check"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "openpbso_amd", "engine_tables_check")], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and "engine tables check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
