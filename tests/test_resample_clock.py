"""The host arithmetic of the resampler bus (csrc/resample_clock.h: the reduction to L / M with its limits, the output range of a
call and the advance of p0, the prototype design) against the rules of include/openpbso_amd.h, on the host alone:
tests/cpp/resample_clock_check.cpp is built with the host compiler and -fsanitize=address,undefined and run as a program of its
own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resample_clock_under_asan_and_ubsan():
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "openpbso_amd", "csrc"), "resample_clock_check"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "openpbso_amd", "resample_clock_check")], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "resample clock check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
