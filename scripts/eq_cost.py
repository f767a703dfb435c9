#!/usr/bin/env python3
"""What the EQ bus costs: C = 2 channels, a ten-second step (n = 860 * 513 samples) at S = 1, 4 and 8 sections, and a one-buffer step
at the same S, timed with HIP events on the engine's stream around pbso_eq, warm, the median of --calls calls (20).  Beside it, in
the same run and the same way, pbso_master at a look-ahead of 64 on the same input: the yardstick, a stage of the same kind whose
cost is known.

    python scripts/eq_cost.py                      one JSON line per case
    python scripts/eq_cost.py --buffers 86         another step length

The engine behind the stage is one object of 64 modes: the input is a random device tensor.  Every step is followed by one call of
each stage (the rule that every step is processed exactly once); the step itself is outside the events.  The sections are the
cascade a master chain would carry: a 30 Hz high-pass, a low shelf, peaking bands, a high shelf.  Needs the GPU: there is no CPU
path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CHAIN = [("highpass", 30.0, 0.707, 0.0), ("lowshelf", 120.0, 0.707, 3.0), ("peak", 250.0, 1.4, -4.0), ("peak", 1000.0, 2.0, 2.0),
         ("peak", 3200.0, 2.0, -3.0), ("peak", 6500.0, 3.0, 1.5), ("highshelf", 9000.0, 0.707, 4.0), ("lowpass", 18000.0, 0.707, 0.0)]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, nargs="*", default=[860, 1])
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--sections", type=int, nargs="*", default=[1, 4, 8])
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
            assert 0 < np.abs(eng.read_master()).max() <= np.float32(0.7)
            master = median(ms)
            print(json.dumps(dict(stage="master", lookahead=64, C=C, n=n, ms_median=master, ms_min=min(ms), ms_max=max(ms))), flush=True)
            for S in a.sections:
                eng.eq_enable(C, S, 0)
                eng.eq_set([[capi.eq_design(k, float(eng.sample_rate), f0, q, g) for k, f0, q, g in CHAIN[:S]]] * C)
                ms = timed(lambda: eng.eq(x.data_ptr()))
                y = eng.read_eq()
                assert y.shape == (C, n) and np.isfinite(y).all() and np.abs(y).max() > 0
                blocks = (n + capi.EQ_BLOCK - 1) // capi.EQ_BLOCK
                print(json.dumps(dict(stage="eq", P=capi.EQ_BLOCK, S=S, C=C, n=n, launches=2 + 3 * S, ms_median=median(ms), ms_min=min(ms),
                                      ms_max=max(ms), ms_per_section=(median(ms)) / S, serial_fma_per_section=2 * blocks,
                                      fma=float(n) * C * S * (capi.EQ_BLOCK / 2 + 4.5), times_master=median(ms) / master)), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
