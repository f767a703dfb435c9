"""A moving scene at the headline shape (1024 x 512, C = 2, max_delay 2048, ramp 513): new gains and delays for all objects every
buffer, ten seconds of audio (860 buffers) per repetition.

  --mode one         one 860-buffer step + one mix with the 860 sets scheduled (pbso_scene_mix_schedule)
  --mode cut         860 one-buffer steps, a pbso_scene_mix_set before each: the only way without the schedule
  --mode per_sample  86 buffers, a set every 48 samples -- every 64-sample tile has a set inside it, so the whole step takes the
                     per-sample path of the schedule-aware stage 1 -- beside the same step with nothing scheduled

Wall time of a repetition on a synchronised host clock: from before the first set call to after the sync behind the last mix;
the set calls' own host time is reported beside it.  One JSON line.  --mode cut runs on a library without the schedule too
(PBSO_LIB).  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 513


def main():
    import numpy as np
    from openpbso_amd import Engine, ForceMessage, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("one", "cut", "per_sample"), default="one")
    ap.add_argument("--objects", type=int, default=1024)
    ap.add_argument("--modes", type=int, default=512)
    ap.add_argument("--buffers", type=int, default=860)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    C, max_delay, R = 2, 2048, 513
    nb = 86 if a.mode == "per_sample" else a.buffers
    rng = np.random.default_rng(1)
    eng = Engine(chunk_buffers=max(128, nb))
    try:
        for i in range(a.objects):
            eng.add_object(synth.eigenvalues(a.modes, 100 + i), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        for i in range(a.objects):
            eng.set_use_transfer(i, False)
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(a.modes) * 1e-3), 0)
        eng.scene_mix_enable(C, max_delay, R)
        every = 48 if a.mode == "per_sample" else B
        K = nb * B // every if a.mode == "per_sample" else nb
        g = rng.uniform(-1, 1, (K, C, a.objects)).astype(np.float32)
        d = rng.uniform(0, 1000, (K, C, a.objects)).astype(np.float32)
        total, sets, mix, plain_mix = [], [], [], []
        t_abs = 0
        for rep in range(a.warmup + a.reps):
            eng.sync()
            t0 = time.perf_counter()
            if a.mode == "cut":
                t_sets = 0.0
                for b in range(nb):
                    s0 = time.perf_counter()
                    eng.scene_mix_set(g[b], d[b])
                    t_sets += time.perf_counter() - s0
                    eng.step(1)
                    eng.scene_mix()
                eng.sync()
                t1 = time.perf_counter()
            else:
                eng.scene_mix_schedule(t_abs + every * np.arange(K, dtype=np.int64), g, d)
                t_sets = time.perf_counter() - t0
                eng.step(nb)
                if a.mode == "per_sample":
                    eng.sync()
                m0 = time.perf_counter()
                eng.scene_mix()
                eng.sync()
                t1 = time.perf_counter()
                mix.append(t1 - m0)
            t_abs += nb * B
            total.append(t1 - t0)
            sets.append(t_sets)
            if a.mode == "per_sample":                               # the same step with nothing scheduled, for comparison
                eng.step(nb)
                eng.sync()
                m0 = time.perf_counter()
                eng.scene_mix()
                eng.sync()
                plain_mix.append(time.perf_counter() - m0)
                t_abs += nb * B
        out = eng.read_scene_mix()
        assert np.isfinite(out).all() and np.abs(out).max() > 0
        ms = lambda v: [round(1e3 * x, 3) for x in v[a.warmup:]]
        res = dict(mode=a.mode, lib=os.environ.get("PBSO_LIB", "built"), objects=a.objects, modes=a.modes, buffers=nb, sets=K, C=C,
                   max_delay=max_delay, ramp=R, total_ms=ms(total), set_calls_ms=ms(sets))
        if a.mode == "per_sample":
            res.update(mix_ms=ms(mix), plain_mix_ms=ms(plain_mix), set_every=every)
        print(json.dumps(res))
    finally:
        eng.close()


if __name__ == "__main__":
    main()
