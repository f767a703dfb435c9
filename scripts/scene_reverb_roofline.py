"""The scene reverb's kernels (kernels_reverb.hip) against the f32 matrix rate at three shapes: the headline step (860 buffers, one
bus, C = 2, K = 65536) in the steady state and with every measured step entirely inside a cross-fade (both tap sets computed); the
real-time step (the same reverb, one buffer per call, 200 calls); and a small wide one (86 buffers, 2 inputs, 8 outputs, K = 16384).

  python scripts/scene_reverb_roofline.py --shape headline         the workload alone: steps, each followed by its reverb call
  python scripts/scene_reverb_roofline.py --profile OUT_DIR         every shape under rocprofv3 --kernel-trace --stats (one child
                                                                    process each, under its own time limit; no counters in the
                                                                    same run), then the kernels' time per call and the fraction of
                                                                    the flop floor

The floor is the formulation's own work, 2 n_out n_in (K + 15 J) n flop per call (twice that inside a fade), at the 155 Tflop/s
measured for v_mfma_f32_16x16x4_f32.  The engine behind the reverb is one object of 64 modes: the input is a random device tensor.
The first call of a run (the first set takes effect without a fade) is left out of the averages.  The call-to-completion time of the
host (the real-time shape's figure against the 11.6 ms buffer deadline) is taken without a profiler too: --shape.  Needs the GPU:
there is no CPU path."""
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
SEGMENT = 2048
MFMA_F32_TFLOPS = 155.0
XFADE = 1 << 20                                           # longer than every measured run of the fade shape
SHAPES = {"headline": dict(nb=860, n_in=1, n_out=2, K=65536, steps=4),
          "headline_fade": dict(nb=860, n_in=1, n_out=2, K=65536, steps=3, fade=True),
          "realtime": dict(nb=1, n_in=1, n_out=2, K=65536, steps=201),
          "small_wide": dict(nb=86, n_in=2, n_out=8, K=16384, steps=20)}
KERNELS = ("scene_reverb_stage1", "scene_reverb_stage2", "reverb_history_kernel")


def call_flop(nb, n_in, n_out, K, fade=False, **_):
    J = (K + SEGMENT - 1) // SEGMENT
    return 2.0 * n_out * n_in * (K + 15 * J) * nb * B * (2 if fade else 1)


def run_shape(name):
    import numpy as np
    import torch
    from openpbso_amd import Engine, synth
    s = SHAPES[name]
    assert not s.get("fade") or (s["steps"] - 1) * s["nb"] * B < XFADE
    rng = np.random.default_rng(1)
    eng = Engine(chunk_buffers=max(128, s["nb"]))
    try:
        eng.add_object(synth.eigenvalues(64, 100), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        eng.scene_reverb_enable(s["n_in"], s["n_out"], s["K"], XFADE if s.get("fade") else 0)
        shape = (s["n_out"], s["n_in"], s["K"])
        x = torch.randn((s["n_in"], s["nb"] * B), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t_call = []
        for k in range(s["steps"]):
            if k == 0 or (k == 1 and s.get("fade")):
                eng.scene_reverb_set(rng.standard_normal(shape) * np.exp(-np.arange(s["K"]) / (s["K"] / 6.0)))
            eng.step(s["nb"])
            eng.sync()
            t0 = time.perf_counter()
            eng.scene_reverb(x.data_ptr())
            eng.sync()
            t_call.append(time.perf_counter() - t0)
        out = eng.read_scene_reverb()
        assert np.isfinite(out).all() and np.abs(out).max() > 0
        t = sorted(t_call[1:])
        print(json.dumps(dict(shape=name, **s, host_ms_median=1e3 * t[len(t) // 2], host_ms_min=1e3 * t[0], host_ms_max=1e3 * t[-1],
                              flop=call_flop(**s))))
    finally:
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
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
        with open(os.path.join(out_dir, name + ".log"), "w") as f:
            f.write(r.stdout + r.stderr)
        if r.returncode != 0:
            print(f"{name}: rocprofv3 exit {r.returncode} (see {name}.log)")
            return r.returncode
        ns = per_call_ns(d)
        flop = call_flop(**s)
        ms = sum(ns.values()) / 1e6
        floor_ms = flop / (MFMA_F32_TFLOPS * 1e12) * 1e3
        host = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"shape"')]
        rows.append(dict(shape=name, **{k: s[k] for k in ("nb", "n_in", "n_out", "K")}, fade=bool(s.get("fade")),
                         kernel_us={k: v / 1e3 for k, v in ns.items()}, call_ms=ms, flop=flop, floor_ms=floor_ms,
                         stage1_tflops=flop / (ns["scene_reverb_stage1"] * 1e-9) / 1e12, fraction_of_floor=floor_ms / ms,
                         stage1_fraction_of_rate=flop / (ns["scene_reverb_stage1"] * 1e-9) / 1e12 / MFMA_F32_TFLOPS,
                         host_ms_median_under_profiler=host[0]["host_ms_median"] if host else None))
        print(json.dumps(rows[-1]), flush=True)
    with open(os.path.join(out_dir, "scene_reverb_roofline.json"), "w") as f:
        json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--profile", metavar="OUT_DIR")
    ap.add_argument("--only", nargs="*", choices=sorted(SHAPES), help="with --profile: these shapes only")
    a = ap.parse_args()
    if a.profile:
        sys.exit(profile(a.profile, a.only or list(SHAPES)))
    run_shape(a.shape or "headline")
