"""A source field moving past a listener at the filter mix's headline shape (1024 x 512, C = 2, K = 128, max_onset 64, xfade 441,
max_delay 2048, delay ramp 513): new head-related filters AND new delays for all objects every buffer, ten seconds of audio (860
buffers) per repetition.

  --mode one    one 860-buffer step + one mix with the 860 filter sets and 860 delay sets scheduled (pbso_scene_fir_schedule /
                pbso_scene_fir_delay_schedule)
  --mode cut    860 one-buffer steps, a pbso_scene_fir_set and a pbso_scene_fir_set_delay before each: the only way without the
                schedule
  --mode plain  one 860-buffer step + one mix with nothing scheduled and nothing set since the first buffer: the unscheduled
                pbso_scene_fir, which runs on a library without the schedule too (PBSO_LIB)
  --no-delay    without the delay stage (filter sets only): the difference to the run with it is the delay stage's cost

Wall time of a repetition on a synchronised host clock (sync, clock, work, sync, clock): from before the first set call to after
the sync behind the last mix; the set calls' own host time and the mix alone (HIP events around pbso_scene_fir on the engine's
stream are not exposed, so: sync, clock, mix, sync, clock) beside it.  Medians of the timed repetitions, every value listed.  One
JSON line.  A set is 1 MB of taps: --sets-per-call N schedules them N at a time just before the step (default: all at once, 860 MB
of taps pending on the host).  Needs the GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 513


def main():
    import numpy as np
    from openpbso_amd import Engine, ForceMessage, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("one", "cut", "plain"), default="one")
    ap.add_argument("--objects", type=int, default=1024)
    ap.add_argument("--modes", type=int, default=512)
    ap.add_argument("--buffers", type=int, default=860)
    ap.add_argument("--taps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-delay", action="store_true")
    ap.add_argument("--sets-per-call", type=int, default=0)
    a = ap.parse_args()
    C, K, max_onset, xfade, max_delay, Rd = 2, a.taps, 64, 441, 2048, 513
    nb, N = a.buffers, a.objects
    rng = np.random.default_rng(1)
    eng = Engine(chunk_buffers=max(128, nb))
    try:
        for i in range(N):
            eng.add_object(synth.eigenvalues(a.modes, 100 + i), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        for i in range(N):
            eng.set_use_transfer(i, False)
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(a.modes) * 1e-3), 0)
        eng.scene_fir_enable(C, K, max_onset, xfade)
        if not a.no_delay:
            eng.scene_fir_delay_enable(max_delay, Rd)
        # eight distinct sets used in turn (a set per buffer of 1 MB each: the values do not change what is measured)
        h8 = (rng.standard_normal((8, C, N, K)) * np.exp(-np.arange(K) / 32.0)).astype(np.float32)
        on8 = rng.integers(0, max_onset + 1, (8, N)).astype(np.int32)
        d8 = rng.uniform(0, 1000, (8, N)).astype(np.float32)
        pick = np.arange(nb) % 8
        if a.mode == "one":                                          # the caller's arrays as it would hold them: built outside the timed region
            h_all, on_all, d_all = np.ascontiguousarray(h8[pick]), np.ascontiguousarray(on8[pick]), np.ascontiguousarray(d8[pick])
        total, sets, mix = [], [], []
        t_abs = 0
        for rep in range(a.warmup + a.reps):
            eng.sync()
            t0 = time.perf_counter()
            if a.mode == "cut":
                t_sets = t_mix = 0.0
                for b in range(nb):
                    s0 = time.perf_counter()
                    eng.scene_fir_set(h8[pick[b]], on8[pick[b]])
                    if not a.no_delay:
                        eng.scene_fir_set_delay(d8[pick[b]])
                    t_sets += time.perf_counter() - s0
                    eng.step(1)
                    eng.scene_fir()
                eng.sync()
                t1 = time.perf_counter()
            else:
                if a.mode == "one":
                    per = a.sets_per_call or nb
                    for b0 in range(0, nb, per):
                        b1 = min(b0 + per, nb)
                        ts = t_abs + B * np.arange(b0, b1, dtype=np.int64)
                        eng.scene_fir_schedule(ts, h_all[b0:b1], on_all[b0:b1])
                        if not a.no_delay:
                            eng.scene_fir_delay_schedule(ts, d_all[b0:b1])
                elif rep == 0:
                    eng.scene_fir_set(h8[0], on8[0])
                    if not a.no_delay:
                        eng.scene_fir_set_delay(d8[0])
                t_sets = time.perf_counter() - t0
                eng.step(nb)
                eng.sync()
                m0 = time.perf_counter()
                eng.scene_fir()
                eng.sync()
                t1 = time.perf_counter()
                t_mix = t1 - m0
            t_abs += nb * B
            total.append(t1 - t0)
            sets.append(t_sets)
            mix.append(t_mix)
        out = eng.read_scene_fir()
        assert np.isfinite(out).all() and np.abs(out).max() > 0
        ms = lambda v: [round(1e3 * x, 3) for x in v[a.warmup:]]
        med = lambda v: round(1e3 * statistics.median(v[a.warmup:]), 3)
        res = dict(mode=a.mode, lib=os.environ.get("PBSO_LIB", "built"), objects=N, modes=a.modes, buffers=nb, C=C, taps=K, xfade=xfade,
                   delay=not a.no_delay, total_ms=ms(total), total_median_ms=med(total), set_calls_ms=ms(sets))
        if a.mode != "cut":
            res.update(mix_ms=ms(mix), mix_median_ms=med(mix))
        print(json.dumps(res), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
