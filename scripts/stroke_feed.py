#!/usr/bin/env python3
"""The scraping scene of `bench.py --scenario scraping` (same generators and seeds, the same engine options, stepped the same
way: the next step's input is handed over while the device runs the current one), fed once as messages
(pbso_enqueue_force_batch, what bench.py does) and once as strokes (pbso_enqueue_strokes), three runs of each, alternating.

Per run: ms_per_step (host clock around the timed steps, ending in a device synchronise), the engine's last_step_kernel_ms,
total_host_plan_ms and total_host_submit_ms per step, the time of the caller's enqueue call per step, and -- strokes only -- the
stroke kernel's own time per launch from HIP events (--host-profile: PBSO_HOST_PROFILE=1 makes the engine record them; its lines
go to stderr when the engine closes and are picked up from there).  Prints one JSON line per run and the ranges at the end.

    python scripts/stroke_feed.py --objects 1024 --modes 512 --buffers 86 --steps 20 --warmup 5
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(args, inputs, feed, host_profile):
    import torch

    import bench
    from openpbso_amd import Engine, ForceMessage, capi, synth
    lam, shapes, scripts = inputs
    n_obj, nb = args.objects, args.buffers
    n_steps = args.warmup + args.steps
    # the engine's diagnostics (stroke kernel time) are printed to stderr when it closes: keep them in a file
    err_file = tempfile.TemporaryFile(mode="w+b")
    saved_fd = os.dup(2)
    if host_profile:
        os.environ["PBSO_HOST_PROFILE"] = "1"
        os.dup2(err_file.fileno(), 2)
    try:
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
            if feed == "strokes":
                flags = np.zeros(n_obj * nb, dtype=np.uint8)
                if k == 0:
                    flags[::nb] = capi.STROKE_START | capi.STROKE_ZERO          # the dummy start message of buffer 0
                feeds.append(eng.prepare_strokes(fo, vids, bary, vns, t, flags))
            else:
                keep = t > 0 if k == 0 else np.ones(t.size, dtype=bool)           # (buffer 0 is the dummy start message, below)
                feeds.append(eng.hit_messages(fo[keep], vids[keep], vns[keep], t[keep], coords=bary[keep],
                                              force_type=capi.AUTOREGRESSIVE_FORCE))
        for i in range(n_obj):
            eng.set_use_transfer(i, False)
            if feed == "messages":
                assert eng.enqueue_force(i, ForceMessage(forceType=capi.AUTOREGRESSIVE_FORCE, sustainedForceStart=True), 0)
        audio = torch.zeros((n_obj, nb * 513), dtype=torch.float32, device="cuda")
        enqueue_s = [0.0]

        def hand_over(k):
            if k >= n_steps:
                return
            t0 = time.perf_counter()
            if feed == "strokes":
                took, want = eng.enqueue_prepared_strokes(feeds[k]), feeds[k][0]
            else:
                took, want = eng.enqueue_force_batch(*feeds[k]), feeds[k][0].size
            enqueue_s[0] += time.perf_counter() - t0
            assert took == want

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
        stats = eng.stroke_stats()
        checksum = float(audio.double().abs().sum().item())
        eng.close()
    finally:
        if host_profile:
            os.dup2(saved_fd, 2)
            os.environ.pop("PBSO_HOST_PROFILE", None)
        os.close(saved_fd)
    err_file.seek(0)
    err_text = err_file.read().decode(errors="replace")
    err_file.close()
    sys.stderr.write(err_text)
    m = re.search(r"pbso stroke kernel: ([0-9.]+) ms per launch", err_text)
    ms_step = 1e3 * wall / args.steps
    return dict(feed=feed, ms_per_step=round(ms_step, 4), x_real_time=round(nb * 513 / 44100.0 / (ms_step * 1e-3), 1),
                last_step_kernel_ms=round(i1["last_step_kernel_ms"], 4),
                host_plan_ms_per_step=round((i1["total_host_plan_ms"] - i0["total_host_plan_ms"]) / args.steps, 4),
                host_submit_ms_per_step=round((i1["total_host_submit_ms"] - i0["total_host_submit_ms"]) / args.steps, 4),
                enqueue_call_ms_per_step=round(1e3 * enqueue_s[0] / args.steps, 4),
                stroke_kernel_ms_per_launch=float(m.group(1)) if m else None, stroke_stats=stats, audio_abs_sum=checksum,
                host_profile=err_text.strip().splitlines() if host_profile else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=1024)
    ap.add_argument("--modes", type=int, default=512)
    ap.add_argument("--buffers", type=int, default=86)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--feeds", default="messages,strokes")
    ap.add_argument("--host-profile", action="store_true", help="PBSO_HOST_PROFILE=1: host stages and the stroke kernel's HIP-event time")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("stroke_feed.py needs the GPU: there is nothing to time without one")
    import bench
    args.scenario = "scraping"
    inputs = bench.build_inputs(args, list(range(args.objects)), (args.warmup + args.steps) * args.buffers)
    results = {}
    for r in range(args.runs):
        for feed in args.feeds.split(","):
            res = run(args, inputs, feed, args.host_profile)
            res["run"] = r
            results.setdefault(feed, []).append(res)
            print(json.dumps(res), flush=True)
    summary = {}
    for feed, rs in results.items():
        summary[feed] = {k: [min(x[k] for x in rs), max(x[k] for x in rs)]
                         for k in ("ms_per_step", "last_step_kernel_ms", "host_plan_ms_per_step", "host_submit_ms_per_step",
                                   "enqueue_call_ms_per_step")}
        sk = [x["stroke_kernel_ms_per_launch"] for x in rs if x["stroke_kernel_ms_per_launch"] is not None]
        if sk:
            summary[feed]["stroke_kernel_ms_per_launch"] = [min(sk), max(sk)]
        summary[feed]["audio_abs_sum"] = sorted({x["audio_abs_sum"] for x in rs})
    print(json.dumps({"ranges_over_runs": summary, "objects": args.objects, "modes": args.modes, "buffers": args.buffers,
                      "steps": args.steps, "warmup": args.warmup}), flush=True)


if __name__ == "__main__":
    main()
