"""The work-strip table and the validation arithmetic of the scene filter mix's schedule (csrc/fir_schedule.h: integers only, what
scene_fir.cpp builds a step's launch from and the kernels of kernels_fir.hip read) against a per-sample labelling of the step:
tests/cpp/fir_schedule_check.cpp is built with the host compiler and -fsanitize=address,undefined and run as a program of its own.
No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fir_schedule_under_asan_and_ubsan():
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "openpbso_amd", "csrc"), "fir_schedule_check"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "openpbso_amd", "fir_schedule_check")], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and "fir schedule check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
