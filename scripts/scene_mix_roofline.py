"""The scene mix's kernels (kernels_mix.hip) against HBM at three shapes: the headline step (1024 x 512, 860 buffers, C = 2), the
real-time step (1024 x 512, one buffer, C = 2) and a small scene with eight channels (64 x 256, 86 buffers); and the real-time
step of a moving scene (new gains and delays before every step, ramped over 441 samples: most of each step is inside a ramp).

  python scripts/scene_mix_roofline.py --shape headline          the workload alone: steps, each followed by its scene mix
  python scripts/scene_mix_roofline.py --profile OUT_DIR          every shape under rocprofv3 --kernel-trace --stats (one child
                                                                  process each), then the mix kernels' time and bytes/s

Bytes are counted from the shapes: the step's rows once, the history (stage 1 reads at most H samples per object, the update
reads and writes H), the partial rows written and read back, the output.  Needs the GPU: there is no CPU path."""
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
HBM_TBS = 6.29                                            # measured copy rate of the MI355X (MI355X_MICROARCH: float4 copy)
SHAPES = {"headline": dict(n_obj=1024, modes=512, nb=860, C=2, steps=4, max_delay=2048),
          "realtime": dict(n_obj=1024, modes=512, nb=1, C=2, steps=300, max_delay=2048),
          "small8": dict(n_obj=64, modes=256, nb=86, C=8, steps=60, max_delay=2048),
          "realtime_moving": dict(n_obj=1024, modes=512, nb=1, C=2, steps=300, max_delay=2048, set_every=1)}
KERNELS = ("scene_mix_stage1", "scene_mix_stage2", "scene_history_kernel")


def mix_bytes(n_obj, nb, C, max_delay, **_):
    """bytes the mix has to move at least (each read once)"""
    n, H, groups = nb * B, max_delay + 1, (n_obj + 31) // 32
    return {"rows": 4 * n_obj * n, "history": 4 * n_obj * H * 3, "partials": 4 * 2 * C * groups * n, "output": 4 * C * n}


def run_shape(name):
    import numpy as np
    from openpbso_amd import Engine, ForceMessage, synth
    s = SHAPES[name]
    rng = np.random.default_rng(1)
    eng = Engine(chunk_buffers=max(128, s["nb"]))
    try:
        for i in range(s["n_obj"]):
            eng.add_object(synth.eigenvalues(s["modes"], 100 + i), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        for i in range(s["n_obj"]):
            eng.set_use_transfer(i, False)
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(s["modes"]) * 1e-3), 0)
        eng.scene_mix_enable(s["C"], s["max_delay"], 441)
        shape = (s["C"], s["n_obj"])
        eng.scene_mix_set(rng.uniform(-1, 1, shape), rng.uniform(0, 1000, shape))
        t_mix = []
        for k in range(s["steps"]):
            if k == s["steps"] // 2 or (s.get("set_every") and k % s["set_every"] == 0):
                eng.scene_mix_set(rng.uniform(-1, 1, shape), rng.uniform(0, 1000, shape))     # a ramp
            eng.step(s["nb"])
            eng.sync()
            t0 = time.perf_counter()
            eng.scene_mix()
            eng.sync()
            t_mix.append(time.perf_counter() - t0)
        out = eng.read_scene_mix()
        assert np.isfinite(out).all()
        t = sorted(t_mix[1:])
        print(json.dumps(dict(shape=name, **s, host_ms_median=1e3 * t[len(t) // 2], host_ms_min=1e3 * t[0],
                              bytes=mix_bytes(**s))))
    finally:
        eng.close()


def profile(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    rows = []
    for name, s in SHAPES.items():
        d = os.path.join(out_dir, name)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-f", "csv", "-d", d, "-o", name, "--", sys.executable, os.path.abspath(__file__),
               "--shape", name]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=400)
        with open(os.path.join(out_dir, name + ".log"), "w") as f:
            f.write(r.stdout + r.stderr)
        if r.returncode != 0:
            print(f"{name}: rocprofv3 exit {r.returncode} (see {name}.log)")
            return r.returncode
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        ns = {}
        for row in csv.DictReader(open(stats[0])):
            for k in KERNELS:
                if k in row["Name"]:
                    ns[k] = ns.get(k, 0.0) + float(row["AverageNs"])
        by = mix_bytes(**s)
        total = sum(by.values())
        ms = sum(ns.values()) / 1e6
        rows.append(dict(shape=name, n_obj=s["n_obj"], modes=s["modes"], nb=s["nb"], C=s["C"], kernel_us={k: v / 1e3 for k, v in ns.items()},
                         mix_ms=ms, bytes=total, tb_per_s=total / (ms * 1e-3) / 1e12, floor_ms=total / (HBM_TBS * 1e12) * 1e3))
        print(json.dumps(rows[-1]))
    with open(os.path.join(out_dir, "scene_mix_roofline.json"), "w") as f:
        json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--profile", metavar="OUT_DIR")
    a = ap.parse_args()
    if a.profile:
        sys.exit(profile(a.profile))
    run_shape(a.shape or "headline")
