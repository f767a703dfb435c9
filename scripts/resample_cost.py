#!/usr/bin/env python3
"""What the resampler bus costs at the headline step's shape: C = 2 channels, n = 860 * 513 input samples (ten seconds), 44100 ->
48000 Hz (160 / 147), at T = 32 and at T = 256 taps per output sample, timed with HIP events on the engine's stream around
pbso_resample, warm, the median of --calls calls (20).  Beside it, in the same run and the same way, pbso_master at a look-ahead of
64 on the same input: the yardstick, a stage of the same kind (a few maps over [C][n]) whose cost is known.

    python scripts/resample_cost.py                     one JSON line per stage and the ratio at the end
    python scripts/resample_cost.py --buffers 1         the real-time step

The engine behind the stages is one object of 64 modes: the input is a random device tensor.  Every step is followed by one call
of each stage (the rule that every step is processed exactly once); the step itself is outside the events.  The floor printed
beside the resampler is its own traffic, 4 C (n + n_out) bytes, at the 6.29 TB/s measured for a device copy; its n_out T C fmaf
are listed too.  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_TBPS = 6.29


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--buffers", type=int, default=860)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rate-out", type=int, default=48000)
    ap.add_argument("--taps", type=int, nargs="*", default=[32, 256])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import numpy as np
    import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

    from openpbso_amd import Engine, synth
    stream = torch.cuda.Stream()
    eng = Engine(stream=stream.cuda_stream, chunk_buffers=max(128, a.buffers))
    try:
        eng.add_object(synth.eigenvalues(64, 100), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        C, n = a.channels, a.buffers * eng.B
        x = torch.randn((C, n), dtype=torch.float32, device="cuda") * 0.25
        torch.cuda.synchronize()

        def timed(call):
            ms = []
            for k in range(a.warmup + a.calls):
                eng.step(a.buffers)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call()
                e1.record(stream)
                e1.synchronize()
                if k >= a.warmup:
                    ms.append(e0.elapsed_time(e1))
            return ms

        results = {}
        eng.master_enable(C, 0.7, 64, 0, 0)
        ms = timed(lambda: eng.master(x.data_ptr()))
        assert 0 < np.abs(eng.read_master()).max() <= np.float32(0.7)
        results["master"] = median(ms)
        print(json.dumps(dict(stage="master", lookahead=64, C=C, n=n, ms_median=median(ms), ms_min=min(ms), ms_max=max(ms))), flush=True)
        for T in a.taps:
            eng.resample_enable(a.rate_out, C, T)
            i = eng.resample_info()
            ms = timed(lambda: eng.resample(x.data_ptr()))
            i = eng.resample_info()
            y = eng.read_resample()
            assert y.shape == (C, i["n_out"]) and np.isfinite(y).all() and np.abs(y).max() > 0
            n_out = i["n_out"]
            results[T] = median(ms)
            print(json.dumps(dict(stage="resample", L=i["L"], M=i["M"], T=T, C=C, n=n, n_out=n_out, ms_median=median(ms), ms_min=min(ms),
                                  ms_max=max(ms), fmaf=float(n_out) * T * C, bytes=4.0 * C * (n + n_out),
                                  byte_floor_ms=4.0 * C * (n + n_out) / (COPY_TBPS * 1e12) * 1e3,
                                  times_master=median(ms) / results["master"])), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
