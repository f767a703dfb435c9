#!/usr/bin/env python3
"""The scraping scene of `bench.py --scenario scraping` (same generators and seeds, the same engine options, stepped the same
way, message feed), once under AutoregressiveForce strokes -- the yardstick, on a build of the PARENT commit when --parent-lib
names one (PBSO_LIB selects the library a process loads) -- and once with the same messages under LOOPING TRACK forces: the
dummy start message of every object is a PBSO_TRACK_FORCE that loops a track of the object's own (a noise signal around the AR
force's mean), the per-buffer face messages that replace the spatial vector are the same arrays in both legs.

Every leg runs in a fresh child process; the two legs alternate, --runs repeats each (at least five for a figure worth keeping).
Per run: ms_per_step (host clock around the timed steps, ending in a device synchronise), the engine's last_step_kernel_ms,
total_host_plan_ms and total_host_submit_ms per step, the caller's enqueue time per step.  One JSON line per run and the ranges
at the end.  The K2 kernels' own time per launch comes from a separate run of one leg under
`rocprofv3 --kernel-trace --stats -- python scripts/track_feed.py --leg track` (force_rows_kernel and its companions).

    python scripts/track_feed.py --objects 1024 --modes 512 --buffers 86 --steps 20 --warmup 5 --runs 5 --parent-lib /path/to/parent.so
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TRACK_SAMPLES = 4096


def run(args, leg):
    import torch

    import bench
    from openpbso_amd import Engine, ForceMessage, capi, synth
    args.scenario = "scraping"
    n_obj, nb = args.objects, args.buffers
    n_steps = args.warmup + args.steps
    lam, shapes, scripts = bench.build_inputs(args, list(range(n_obj)), n_steps * nb)
    eng = Engine(qnorm=capi.QNORM_OFF, chunk_buffers=max(128, nb), submit_thread=bench.submit_thread_of(args))
    for i in range(n_obj):
        eng.add_object(lam[i], synth.RHO, synth.ALPHA, synth.BETA, mode_shapes=shapes[i])
    eng.finalize()
    fo = np.repeat(np.arange(n_obj, dtype=np.int32), nb)
    feeds = []
    for k in range(n_steps):
        b0 = k * nb
        t = np.tile(np.arange(b0, b0 + nb, dtype=np.int64), n_obj)
        vids = np.concatenate([scripts[i]["fids"][b0:b0 + nb] for i in range(n_obj)]).astype(np.int32)
        bary = np.concatenate([scripts[i]["bary"][b0:b0 + nb] for i in range(n_obj)])
        vns = np.concatenate([scripts[i]["vns"][b0:b0 + nb] for i in range(n_obj)])
        keep = t > 0 if k == 0 else np.ones(t.size, dtype=bool)               # (buffer 0 is the dummy start message, below)
        # (under sustained contact only the spatial vector of these messages is used: the same arrays in both legs)
        feeds.append(eng.hit_messages(fo[keep], vids[keep], vns[keep], t[keep], coords=bary[keep], force_type=capi.AUTOREGRESSIVE_FORCE))
    t_create = time.perf_counter()
    if leg == "track":
        rng = np.random.default_rng(77)
        ids = [eng.create_track((0.142 + 0.00148 * rng.standard_normal(TRACK_SAMPLES)).astype(np.float32)) for _ in range(n_obj)]
    t_create = time.perf_counter() - t_create
    for i in range(n_obj):
        eng.set_use_transfer(i, False)
        if leg == "track":
            assert eng.enqueue_track_force(i, ForceMessage(sustainedForceStart=True), ids[i], loop=True)
        else:
            assert eng.enqueue_force(i, ForceMessage(forceType=capi.AUTOREGRESSIVE_FORCE, sustainedForceStart=True), 0)
    audio = torch.zeros((n_obj, nb * 513), dtype=torch.float32, device="cuda")
    enqueue_s = [0.0]

    def hand_over(k):
        if k >= n_steps:
            return
        t0 = time.perf_counter()
        took = eng.enqueue_force_batch(*feeds[k])
        enqueue_s[0] += time.perf_counter() - t0
        assert took == feeds[k][0].size

    hand_over(0)
    for k in range(args.warmup):
        eng.step(nb, into=audio.data_ptr())
        hand_over(k + 1)
    eng.sync()
    i0 = eng.info()
    enqueue_s[0] = 0.0
    t0 = time.perf_counter()
    for k in range(args.warmup, n_steps):
        eng.step(nb, into=audio.data_ptr())
        hand_over(k + 1)
    eng.sync()
    wall = time.perf_counter() - t0
    i1 = eng.info()
    track_stats = list(eng.track_stats()) if leg == "track" else None
    checksum = float(audio.double().abs().sum().item())
    eng.close()
    ms_step = 1e3 * wall / args.steps
    return dict(leg=leg, lib=os.environ.get("PBSO_LIB", "this build"), ms_per_step=round(ms_step, 4),
                x_real_time=round(nb * 513 / 44100.0 / (ms_step * 1e-3), 1), last_step_kernel_ms=round(i1["last_step_kernel_ms"], 4),
                host_plan_ms_per_step=round((i1["total_host_plan_ms"] - i0["total_host_plan_ms"]) / args.steps, 4),
                host_submit_ms_per_step=round((i1["total_host_submit_ms"] - i0["total_host_submit_ms"]) / args.steps, 4),
                enqueue_call_ms_per_step=round(1e3 * enqueue_s[0] / args.steps, 4), track_create_ms=round(1e3 * t_create, 3),
                track_stats=track_stats, audio_abs_sum=checksum)


KEYS = ("ms_per_step", "last_step_kernel_ms", "host_plan_ms_per_step", "host_submit_ms_per_step", "enqueue_call_ms_per_step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=1024)
    ap.add_argument("--modes", type=int, default=512)
    ap.add_argument("--buffers", type=int, default=86)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libopenpbso_amd.so built from the parent commit: the AR leg loads it")
    ap.add_argument("--leg", choices=["ar", "track"], default=None, help="run ONE leg in this process (what the children do)")
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds a child may take")
    args = ap.parse_args()
    if args.leg is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("track_feed.py needs the GPU: there is nothing to time without one")
        print(json.dumps(run(args, args.leg)), flush=True)
        return
    results = {"ar": [], "track": []}
    base = [sys.executable, os.path.abspath(__file__)] + [f"--{k}={getattr(args, k)}" for k in ("objects", "modes", "buffers", "steps", "warmup")]
    for r in range(args.runs):
        for leg in ("ar", "track"):
            env = dict(os.environ)
            env.pop("PBSO_LIB", None)
            if leg == "ar" and args.parent_lib:
                env["PBSO_LIB"] = os.path.abspath(args.parent_lib)
            out = subprocess.run(base + ["--leg", leg], env=env, capture_output=True, text=True, timeout=args.timeout)
            if out.returncode != 0:                       # a leg that failed ends the run: nothing more is started on the device
                sys.stderr.write(out.stderr)
                sys.exit(f"leg {leg} of run {r} ended with status {out.returncode}")
            res = json.loads(out.stdout.strip().splitlines()[-1])
            res["run"] = r
            results[leg].append(res)
            print(json.dumps(res), flush=True)
    summary = {leg: {k: [min(x[k] for x in rs), max(x[k] for x in rs)] for k in KEYS} for leg, rs in results.items() if rs}
    print(json.dumps({"ranges_over_runs": summary, "objects": args.objects, "modes": args.modes, "buffers": args.buffers, "steps": args.steps,
                      "warmup": args.warmup, "runs": args.runs, "ar_leg_library": args.parent_lib or "this build"}), flush=True)


if __name__ == "__main__":
    main()
