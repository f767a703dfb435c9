"""The scene filter mix's kernels (kernels_fir.hip) against the f32 matrix rate at three shapes: the headline step (1024 x 512,
860 buffers, C = 2, K = 128), the real-time step (the same scene, one buffer per call) and a small scene with eight channels
(64 x 256, 86 buffers, K = 32) -- each in the steady state and with every measured step entirely inside a cross-fade (both filter
sets computed).

  python scripts/scene_fir_roofline.py --shape headline          the workload alone: steps, each followed by its filter mix
  python scripts/scene_fir_roofline.py --profile OUT_DIR          every shape under rocprofv3 --kernel-trace --stats (one child
                                                                  process each, under its own time limit), then the kernels' time
                                                                  per call and the fraction of the flop floor

  python scripts/scene_fir_roofline.py --shape headline --delay steady|moving
                                                                  the same behind the delay stage (the same file): delays
                                                                  set once (ramp 441, none running in a timed step: the
                                                                  steady path), or newly set before every step with a ramp
                                                                  longer than the step (every staged sample evaluates it)
  python scripts/scene_fir_roofline.py --shape headline --alternate
                                                                  three engines in one process -- no delay stage, steady, moving --
                                                                  mixed in turn step after step: the delay stage's cost beside the
                                                                  undelayed mix of the same build, host-timed around a sync

The floor is the formulation's own work, 2 C N (K + 15) n flop per mix (twice that inside a fade), at the 155 Tflop/s measured for
v_mfma_f32_16x16x4_f32.  The first mix of a run (the first set takes effect without a fade) is left out of the averages.  Needs
the GPU: there is no CPU path."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 513
MFMA_F32_TFLOPS = 155.0
XFADE = 1 << 20                                           # longer than every measured run of the fade shapes
SHAPES = {"headline": dict(n_obj=1024, modes=512, nb=860, C=2, K=128, steps=3),
          "headline_fade": dict(n_obj=1024, modes=512, nb=860, C=2, K=128, steps=3, fade=True),
          "realtime": dict(n_obj=1024, modes=512, nb=1, C=2, K=128, steps=200),
          "realtime_fade": dict(n_obj=1024, modes=512, nb=1, C=2, K=128, steps=200, fade=True),
          "small8": dict(n_obj=64, modes=256, nb=86, C=8, K=32, steps=40),
          "small8_fade": dict(n_obj=64, modes=256, nb=86, C=8, K=32, steps=20, fade=True)}
KERNELS = ("scene_fir_stage1", "scene_fir_stage2", "fir_history_kernel")


def mix_flop(n_obj, nb, C, K, fade=False, **_):
    return 2.0 * C * n_obj * (K + 15) * nb * B * (2 if fade else 1)


DELAY_RAMP = 1 << 20                                      # longer than every measured step: a delay set anew before each never settles


def make_scene(s, delay):
    """an engine of shape s with its filter mix enabled, behind the delay stage for delay = "steady" / "moving" """
    import numpy as np
    from openpbso_amd import Engine, ForceMessage, synth
    rng = np.random.default_rng(1)
    eng = Engine(chunk_buffers=max(128, s["nb"]))
    for i in range(s["n_obj"]):
        eng.add_object(synth.eigenvalues(s["modes"], 100 + i), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    for i in range(s["n_obj"]):
        eng.set_use_transfer(i, False)
        assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(s["modes"]) * 1e-3), 0)
    eng.scene_fir_enable(s["C"], s["K"], 2048, XFADE)
    if delay:
        # moving: a ramp longer than a step, so that every staged sample evaluates its ramp; steady: a usual ramp, and mix_step
        # asserts that none runs in what it times
        eng.scene_fir_delay_enable(2048, DELAY_RAMP if delay == "moving" else 441)
    return eng, rng


def mix_step(eng, rng, s, k, delay):
    """step k of a run: the sets that belong before it, the step, and the host time of its filter mix"""
    if k == 0 or (k == 1 and s.get("fade")):
        eng.scene_fir_set(rng.standard_normal((s["C"], s["n_obj"], s["K"])), rng.integers(0, 2049, s["n_obj"]))
    if delay and (k == 0 or delay == "moving"):
        eng.scene_fir_set_delay(rng.uniform(0, 2048, s["n_obj"]))
    eng.step(s["nb"])
    eng.sync()
    if delay == "steady":                                # what is timed is the steady path: no ramp runs at the step's first sample
        assert eng.scene_fir_delay_info()["ramp_end"] == eng.scene_fir_info()["t"]
    t0 = time.perf_counter()
    eng.scene_fir()
    eng.sync()
    return time.perf_counter() - t0


def run_shape(name, delay=None):
    import numpy as np
    s = SHAPES[name]
    assert not s.get("fade") or (s["steps"] - 1) * s["nb"] * B < XFADE
    assert s["nb"] * B < DELAY_RAMP                      # (every set restarts the ramp: a moving delay is inside it for the whole step)
    eng, rng = make_scene(s, delay)
    try:
        t_mix = [mix_step(eng, rng, s, k, delay) for k in range(s["steps"])]
        out = eng.read_scene_fir()
        assert np.isfinite(out).all() and np.abs(out).max() > 0
        t = sorted(t_mix[1:])
        print(json.dumps(dict(shape=name, delay=delay, **s, host_ms_median=1e3 * t[len(t) // 2], host_ms_min=1e3 * t[0], flop=mix_flop(**s))))
    finally:
        eng.close()


def run_alternating(name):
    import numpy as np
    s = SHAPES[name]
    modes = (None, "steady", "moving")
    scenes = {m: make_scene(s, m) for m in modes}
    try:
        t_mix = {m: [] for m in modes}
        for k in range(s["steps"]):
            for m in modes:
                t_mix[m].append(mix_step(*scenes[m], s, k, m))
        for m in modes:
            out = scenes[m][0].read_scene_fir()
            assert np.isfinite(out).all() and np.abs(out).max() > 0
            t = sorted(t_mix[m][1:])
            print(json.dumps(dict(shape=name, delay=m, nb=s["nb"], steps=s["steps"], host_ms_median=1e3 * t[len(t) // 2], host_ms_min=1e3 * t[0])),
                  flush=True)
    finally:
        for eng, _ in scenes.values():
            eng.close()


def per_call_ns(d):
    """average duration per kernel over all calls but each kernel's first, from the kernel trace"""
    ns = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        calls = {}
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in row["Kernel_Name"]:
                    calls.setdefault(k, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
        for k, c in calls.items():
            c = sorted(c)[1:]
            ns[k] = sum(e - b for b, e in c) / max(len(c), 1)
    return ns


def profile(out_dir, shapes):
    os.makedirs(out_dir, exist_ok=True)
    rows = []
    for name in shapes:
        s = SHAPES[name]
        d = os.path.join(out_dir, name)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", name, "--", sys.executable, os.path.abspath(__file__),
               "--shape", name]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        with open(os.path.join(out_dir, name + ".log"), "w") as f:
            f.write(r.stdout + r.stderr)
        if r.returncode != 0:
            print(f"{name}: rocprofv3 exit {r.returncode} (see {name}.log)")
            return r.returncode
        ns = per_call_ns(d)
        flop = mix_flop(**s)
        ms = sum(ns.values()) / 1e6
        floor_ms = flop / (MFMA_F32_TFLOPS * 1e12) * 1e3
        rows.append(dict(shape=name, n_obj=s["n_obj"], modes=s["modes"], nb=s["nb"], C=s["C"], K=s["K"], fade=bool(s.get("fade")),
                         kernel_us={k: v / 1e3 for k, v in ns.items()}, mix_ms=ms, flop=flop, floor_ms=floor_ms,
                         stage1_tflops=flop / (ns["scene_fir_stage1"] * 1e-9) / 1e12, fraction_of_floor=floor_ms / ms))
        print(json.dumps(rows[-1]), flush=True)
    with open(os.path.join(out_dir, "scene_fir_roofline.json"), "w") as f:
        json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--profile", metavar="OUT_DIR")
    ap.add_argument("--only", nargs="*", choices=sorted(SHAPES), help="with --profile: these shapes only")
    ap.add_argument("--delay", choices=("steady", "moving"), help="with --shape: behind the delay stage")
    ap.add_argument("--alternate", action="store_true", help="with --shape: no delay stage, steady and moving delays in turn")
    a = ap.parse_args()
    if a.profile:
        sys.exit(profile(a.profile, a.only or list(SHAPES)))
    if a.alternate:
        run_alternating(a.shape or "headline")
    else:
        run_shape(a.shape or "headline", a.delay)
