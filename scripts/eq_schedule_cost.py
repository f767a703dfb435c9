#!/usr/bin/env python3
"""What automating the EQ bus costs: C = 2 channels, ten seconds (n = 860 * 513 samples), S = 1, 4 and 8 sections, a cross-fade of
R = 256 samples, a new coefficient set every buffer (a swept peaking band).  Timed as scripts/eq_cost.py times: HIP events on the
engine's stream around the EQ calls, warm, the median of --calls (20).

    (a) scheduled   all 859 sets scheduled up front, the ten seconds in ONE step (pbso_eq_schedule, one pbso_eq)
    (b) cut         the same sets in the same process as 860 one-buffer steps with pbso_eq_set before each (a pair of events
                    around every eq_set + eq, summed: the engine's own steps are outside them, as in the other legs)
    (c) no set      the ten-second step with no set inside it: the plain path (compare scripts/eq_cost.py on the parent commit)

and the number of kernel launches of a scheduled step with 1 set and with 859, read from the engine's PBSO_HOST_PROFILE line in a
child process.  One JSON line per case.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHAIN = [("highpass", 30.0, 0.707, 0.0), ("lowshelf", 120.0, 0.707, 3.0), ("peak", 250.0, 1.4, -4.0), ("peak", 1000.0, 2.0, 2.0),
         ("peak", 3200.0, 2.0, -3.0), ("peak", 6500.0, 3.0, 1.5), ("highshelf", 9000.0, 0.707, 4.0), ("lowpass", 18000.0, 0.707, 0.0)]
R = 256


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def sweep(capi, rate, C, S, k):
    """the cascade at buffer k: the chain of eq_cost.py with its first section a peaking band that moves"""
    rows = [capi.eq_design("peak", rate, 200.0 + 10.0 * k, 1.0, 6.0)] + [capi.eq_design(kd, rate, f0, q, g) for kd, f0, q, g in CHAIN[1:S]]
    return [rows] * C


def count_launches(nb, S):
    """a child with PBSO_HOST_PROFILE=1: a step with one scheduled set, then a step with a set every buffer"""
    env = dict(os.environ, PBSO_HOST_PROFILE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--buffers", str(nb), "--sections", str(S)], env=env,
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit(r.stderr[-2000:])
    return [(int(a), int(b)) for a, b in re.findall(r"eq: scheduled step: (\d+) sets, (\d+) kernel launches", r.stderr)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, default=860)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--sections", type=int, nargs="*", default=[1, 4, 8])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

    from openpbso_amd import Engine, capi, synth
    stream = torch.cuda.Stream()
    eng = Engine(stream=stream.cuda_stream, chunk_buffers=max(128, a.buffers))
    try:
        eng.add_object(synth.eigenvalues(64, 100), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        C, nb, B, rate = a.channels, a.buffers, eng.B, float(eng.sample_rate)
        n = nb * B
        x = torch.randn((C, n), dtype=torch.float32, device="cuda") * 0.25
        torch.cuda.synchronize()
        if a.child:
            S = a.sections[0]
            eng.eq_enable(C, S, R)
            eng.eq_set_at(B, sweep(capi, rate, C, S, 1))
            eng.step(nb)
            eng.eq(x.data_ptr())
            t = eng.eq_info()["t"]
            eng.eq_schedule([t + k * B for k in range(1, nb)], np.array([sweep(capi, rate, C, S, k) for k in range(1, nb)]))
            eng.step(nb)
            eng.eq(x.data_ptr())
            eng.sync()
            return
        for S in a.sections:
            sets = np.array([sweep(capi, rate, C, S, k) for k in range(nb)])

            def timed(prepare, call):
                ms = []
                for k in range(a.warmup + a.calls):
                    prepare()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call()
                    e1.record(stream)
                    e1.synchronize()
                    if k >= a.warmup:
                        ms.append(e0.elapsed_time(e1))
                return ms

            # (a) every set but the first scheduled (the first one is a plain set before the step: t_set = its first sample)
            eng.eq_enable(C, S, R)

            def prepare_a():
                t = eng.eq_info()["t"]
                eng.eq_set(sets[0])
                eng.eq_schedule([t + k * B for k in range(1, nb)], sets[1:])
                eng.step(nb)

            ms_a = timed(prepare_a, lambda: eng.eq(x.data_ptr()))
            y_a = eng.read_eq()
            assert eng.eq_schedule_info()["sets_in_step"] == nb

            # (b) the same sets, the run cut at every buffer
            eng.eq_enable(C, S, R)
            parts = [x[:, k * B:(k + 1) * B].contiguous() for k in range(nb)]
            torch.cuda.synchronize()
            outs = [torch.empty((C, B), dtype=torch.float32, device="cuda") for _ in range(nb)]
            ms_b = []
            for rep in range(a.warmup + a.calls):
                ev = []
                for k in range(nb):
                    eng.step(1)                           # (outside the events, as the step of the other legs)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    eng.eq_set(sets[k])
                    eng.eq(parts[k].data_ptr(), outs[k].data_ptr())
                    e1.record(stream)
                    ev.append((e0, e1))
                ev[-1][1].synchronize()
                if rep >= a.warmup:
                    ms_b.append(sum(e0.elapsed_time(e1) for e0, e1 in ev))
            torch.cuda.synchronize()
            y_b = torch.cat(outs, dim=1).cpu().numpy()
            # the same bits: the last timed pass of either leg began at a multiple of n samples with the same sets
            same = bool(np.array_equal(y_a.view(np.uint32), y_b.view(np.uint32)))

            # (c) no set inside the step
            eng.eq_enable(C, S, R)
            eng.eq_set(sets[0])
            ms_c = timed(lambda: eng.step(nb), lambda: eng.eq(x.data_ptr()))
            launches = count_launches(nb, S)
            print(json.dumps(dict(stage="eq_schedule", S=S, C=C, n=n, R=R, sets=nb, a_scheduled_ms=median(ms_a), a_min=min(ms_a), a_max=max(ms_a),
                                  b_cut_ms=median(ms_b), b_min=min(ms_b), b_max=max(ms_b), c_no_set_ms=median(ms_c), c_min=min(ms_c),
                                  c_max=max(ms_c), a_equals_b_bits=same, launches_sets=launches, plain_launches=2 + 3 * S)), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
