#!/usr/bin/env python3
"""What the loudness bus costs: C = 2 channels, a ten-second step (n = 860 * 513 samples) and a one-buffer step, with the true peak
on and off, timed with HIP events on the engine's stream around pbso_loudness, warm, the median of --calls calls (20).  Beside it, in
the same run and the same way, on the same input: pbso_eq at S = 2 (the K-weighting is that cascade: what is left over is the two
kernels of the stage) and pbso_master at a look-ahead of 64, the yardstick of the other cost scripts.

    python scripts/loudness_cost.py                      one JSON line per case
    python scripts/loudness_cost.py --buffers 86         another step length

The engine behind the stage is one object of 64 modes: the input is a random device tensor.  Every step is followed by one call of
the stage (the rule that every step is processed exactly once); the step itself is outside the events.  The log is reset before it
fills.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, nargs="*", default=[860, 1])
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

    from openpbso_amd import Engine, capi, synth
    stream = torch.cuda.Stream()
    eng = Engine(stream=stream.cuda_stream, chunk_buffers=max(128, max(a.buffers)))
    try:
        eng.add_object(synth.eigenvalues(64, 100), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        C = a.channels
        hop = eng.sample_rate // 10
        for nb in a.buffers:
            n = nb * eng.B
            x = torch.randn((C, n), dtype=torch.float32, device="cuda") * 0.25
            torch.cuda.synchronize()

            def timed(call):
                ms = []
                for k in range(a.warmup + a.calls):
                    eng.step(nb)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    call()
                    e1.record(stream)
                    e1.synchronize()
                    if k >= a.warmup:
                        ms.append(e0.elapsed_time(e1))
                return ms

            eng.master_enable(C, 0.7, 64, 0, 0)
            ms = timed(lambda: eng.master(x.data_ptr()))
            master = median(ms)
            print(json.dumps(dict(stage="master", lookahead=64, C=C, n=n, ms_median=master, ms_min=min(ms), ms_max=max(ms))), flush=True)
            eng.eq_enable(C, 2, 0)
            eng.eq_set([capi.loudness_design(float(eng.sample_rate))] * C)
            ms = timed(lambda: eng.eq(x.data_ptr()))
            eq = median(ms)
            print(json.dumps(dict(stage="eq", S=2, C=C, n=n, ms_median=eq, ms_min=min(ms), ms_max=max(ms))), flush=True)
            for true_peak in (True, False):
                eng.loudness_enable(C, None, (a.warmup + a.calls) * n // hop + 1, true_peak)
                ms = timed(lambda: eng.loudness(x.data_ptr()))
                r = eng.loudness_report()
                assert r["n_blocks"] == (a.warmup + a.calls) * n // hop and (r["n_blocks"] < 4 or np.isfinite(r["integrated"]))
                print(json.dumps(dict(stage="loudness", true_peak=true_peak, C=C, n=n, sub_blocks=n / hop, ms_median=median(ms), ms_min=min(ms),
                                      ms_max=max(ms), ms_beyond_eq=median(ms) - eq, times_eq=median(ms) / eq, times_master=median(ms) / master,
                                      integrated=r["integrated"], true_peak_linear=r["true_peak"])), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
