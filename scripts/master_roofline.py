"""The master bus's kernels (kernels_master.hip) against their byte floor at four shapes: the headline step (860 buffers, C = 2,
L = 64), a wide one (860 buffers, C = 8, L = 4096), and the real-time step (one buffer per call, 200 calls, C = 2) at L = 64 and at
L = 4096.

  python scripts/master_roofline.py --shape headline          the workload alone: steps, each followed by its master call
  python scripts/master_roofline.py --all                     every shape without a profiler, one child process each under its own
                                                              time limit: the call-to-completion time of the host
  python scripts/master_roofline.py --profile OUT_DIR         every shape under rocprofv3 --kernel-trace --stats (one child process
                                                              each, under its own time limit; no counters in the same run), then the
                                                              kernels' time per call beside the byte floor

The floor is the stage's own traffic -- 4 C n bytes in and out and 12 n bytes of r / a / g -- at the 6.29 TB/s measured for a
device copy; the n L fmaf are listed beside it.  The engine behind the stage is one object of 64 modes: the input is a random
device tensor of unit scale against a ceiling of 0.7, so the limiter works in every call.  The first call of a run is left out of
the averages.  A child that fails or runs into its limit ends the run: nothing is started behind it.  Needs the GPU: there is no
CPU path."""
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
COPY_TBPS = 6.29
SHAPES = {"headline": dict(nb=860, C=2, L=64, H=0, steps=6),
          "wide": dict(nb=860, C=8, L=4096, H=0, steps=6),
          "realtime_64": dict(nb=1, C=2, L=64, H=0, steps=201),
          "realtime_4096": dict(nb=1, C=2, L=4096, H=0, steps=201)}
KERNELS = ("master_prepare_kernel", "master_min_lds_kernel", "master_min_pass_kernel", "master_gain_kernel", "master_apply_kernel",
           "master_history_kernel")


def call_bytes(nb, C, **_):
    n = nb * B
    return 2 * 4.0 * C * n + 12.0 * n


def call_fmaf(nb, L, **_):
    return float(nb * B) * L


def run_shape(name):
    import numpy as np
    import torch
    from openpbso_amd import Engine, synth
    s = SHAPES[name]
    eng = Engine(chunk_buffers=max(128, s["nb"]))
    try:
        eng.add_object(synth.eigenvalues(64, 100), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        eng.master_enable(s["C"], 0.7, s["L"], s["H"], 0)
        x = torch.randn((s["C"], s["nb"] * B), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t_call = []
        for k in range(s["steps"]):
            eng.step(s["nb"])
            eng.sync()
            t0 = time.perf_counter()
            eng.master(x.data_ptr())
            eng.sync()
            t_call.append(time.perf_counter() - t0)
        out = eng.read_master()
        assert np.isfinite(out).all() and 0 < np.abs(out).max() <= np.float32(0.7)
        t = sorted(t_call[1:])
        print(json.dumps(dict(shape=name, **s, host_ms_median=1e3 * t[len(t) // 2], host_ms_min=1e3 * t[0], host_ms_max=1e3 * t[-1],
                              bytes=call_bytes(**s), fmaf=call_fmaf(**s))))
    finally:
        eng.close()


def per_call_ns(d):
    """duration per kernel and call (a kernel launched several times in a call: their sum) over all calls but the first"""
    ns = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        calls, n_calls = {}, 0
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in row["Kernel_Name"]:
                    calls.setdefault(k, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
        n_calls = len(calls.get("master_apply_kernel", []))
        if n_calls < 2:
            continue
        for k, c in calls.items():
            per = len(c) // n_calls                      # launches of this kernel in one call
            c = sorted(c)[per:]
            ns[k] = sum(e - b for b, e in c) / (n_calls - 1)
    return ns


def all_shapes(shapes):
    for name in shapes:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", name], cwd=ROOT, capture_output=True, text=True, timeout=180)
        print(r.stdout.strip() or r.stderr[-2000:], flush=True)
        if r.returncode != 0:
            print(f"{name}: exit {r.returncode}")
            return r.returncode
    return 0


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
        us = sum(ns.values()) / 1e3
        floor_us = call_bytes(**s) / (COPY_TBPS * 1e12) * 1e6
        host = [json.loads(l) for l in r.stdout.splitlines() if l.startswith('{"shape"')]
        rows.append(dict(shape=name, **{k: s[k] for k in ("nb", "C", "L", "H")}, kernel_us={k: round(v / 1e3, 2) for k, v in ns.items()},
                         call_us=round(us, 2), bytes=call_bytes(**s), fmaf=call_fmaf(**s), byte_floor_us=round(floor_us, 3),
                         host_ms_median_under_profiler=host[0]["host_ms_median"] if host else None))
        print(json.dumps(rows[-1]), flush=True)
    with open(os.path.join(out_dir, "master_roofline.json"), "w") as f:
        json.dump(rows, f, indent=1)
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--profile", metavar="OUT_DIR")
    ap.add_argument("--only", nargs="*", choices=sorted(SHAPES), help="with --profile / --all: these shapes only")
    a = ap.parse_args()
    if a.profile:
        sys.exit(profile(a.profile, a.only or list(SHAPES)))
    if a.all:
        sys.exit(all_shapes(a.only or list(SHAPES)))
    run_shape(a.shape or "headline")
