"""The record a scheduled set of the scene mix leaves (ramp_next of csrc/scene_ramp.h: the body of pbso_scene_mix_set on the host and
of scene_schedule_expand_kernel on the device), chained over random schedules as a thread of that kernel chains it, against the
chain of plain sets it stands for, every field bitwise: tests/cpp/scene_schedule_check.cpp is built with the host compiler and
-fsanitize=address,undefined and run as a program of its own.  No GPU, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scene_schedule_under_asan_and_ubsan():
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "openpbso_amd", "csrc"), "scene_schedule_check"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(ROOT, "openpbso_amd", "scene_schedule_check")], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and "scene schedule check ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
