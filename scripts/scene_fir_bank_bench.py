"""A source field moving past a listener at the filter mix's headline shape (1024 x 512, C = 2, K = 128, max_onset 64, xfade 441),
its filters blended from a bank of F = 1024 directions with J = 3 weights per object: a new set for all objects every buffer, ten
seconds of audio (860 buffers, 860 sets in one step) per repetition.  In ONE process, alternating, warm:

  taps   pbso_scene_fir_schedule fed the blend built on the host (860 x 1 MB of taps; the blend itself is built outside the timed
         region: the caller's cost of computing it is not counted against this run)
  bank   pbso_scene_fir_bank_schedule fed the indices and weights (860 x 24 KB), the bank uploaded once before

each followed by one 860-buffer step and one mix.  Per run the wall time of the schedule call and of the mix alone (sync, clock,
call, sync, clock), medians of the timed repetitions with every value listed; then the same again with the delay stage enabled
(max_delay 2048, ramp 513, a delay set every buffer, scheduled outside the timed calls: it is the same for both runs).  The sets of
the two runs stand for the same taps up to the rounding of the host's blend (numpy, pair by pair in f32); that the mixes agree bit
for bit when the blend is the stated fmaf chain is what tests/test_gpu_scene_fir_bank.py checks, not this script.  One JSON line per configuration.  Needs the GPU: there
is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B = 513


def run(a, delay):
    import numpy as np
    from openpbso_amd import Engine, ForceMessage, synth
    C, K, F, J, max_onset, xfade, max_delay, Rd = 2, a.taps, a.filters, a.pairs, 64, 441, 2048, 513
    nb, N = a.buffers, a.objects
    rng = np.random.default_rng(1)
    eng = Engine(chunk_buffers=max(128, nb))
    try:
        for i in range(N):
            eng.add_object(synth.eigenvalues(a.modes, 100 + i), synth.RHO, synth.ALPHA, synth.BETA)
        eng.finalize()
        for i in range(N):
            eng.set_use_transfer(i, False)
        eng.scene_fir_enable(C, K, max_onset, xfade)
        if delay:
            eng.scene_fir_delay_enable(max_delay, Rd)
        bank = (rng.standard_normal((F, C, K)) * np.exp(-np.arange(K) / 32.0)).astype(np.float32)
        eng.scene_fir_bank_create(bank)
        # eight distinct sets used in turn (the values do not change what is measured)
        ix8 = rng.integers(0, F, (8, N, J)).astype(np.int32)
        w8 = rng.dirichlet(np.ones(J), (8, N)).astype(np.float32)
        # the host's blend [8][C][N][K], pair by pair in f32 (its last bit does not matter to the timing)
        h8 = np.zeros((8, C, N, K), dtype=np.float32)
        for j in range(J):
            h8 += w8[:, None, :, j, None] * bank[ix8[:, :, j]].transpose(0, 2, 1, 3)
        on8 = rng.integers(0, max_onset + 1, (8, N)).astype(np.int32)
        d8 = rng.uniform(0, 1000, (8, N)).astype(np.float32)
        pick = np.arange(nb) % 8
        # the caller's arrays as it would hold them: built outside the timed region
        h_all, on_all, d_all = np.ascontiguousarray(h8[pick]), np.ascontiguousarray(on8[pick]), np.ascontiguousarray(d8[pick])
        ix_all, w_all = np.ascontiguousarray(ix8[pick]), np.ascontiguousarray(w8[pick])
        t = {k: {"schedule": [], "mix": []} for k in ("taps", "bank")}
        for rep in range(a.warmup + a.reps):
            for kind in ("taps", "bank"):
                eng.scene_fir_reset()                                 # both runs from t = 0 and silence, with the same sets
                for i in range(N):
                    assert eng.enqueue_force(i, ForceMessage(data=np.random.default_rng(7 + i).standard_normal(a.modes) * 1e-3))
                ts = B * np.arange(nb, dtype=np.int64)
                if delay:
                    eng.scene_fir_delay_schedule(ts, d_all)
                eng.sync()
                s0 = time.perf_counter()
                if kind == "taps":
                    eng.scene_fir_schedule(ts, h_all, on_all)
                else:
                    eng.scene_fir_bank_schedule(ts, ix_all, w_all, on_all)
                s1 = time.perf_counter()
                eng.step(nb)
                eng.sync()
                m0 = time.perf_counter()
                eng.scene_fir()
                eng.sync()
                m1 = time.perf_counter()
                t[kind]["schedule"].append(s1 - s0)
                t[kind]["mix"].append(m1 - m0)
                out = eng.read_scene_fir()
                assert np.isfinite(out).all() and np.abs(out).max() > 0
        ms = lambda v: [round(1e3 * x, 3) for x in v[a.warmup:]]
        med = lambda v: round(1e3 * statistics.median(v[a.warmup:]), 3)
        res = dict(objects=N, modes=a.modes, buffers=nb, C=C, taps=K, filters=F, J=J, xfade=xfade, delay=delay)
        for kind in ("taps", "bank"):
            res[kind] = dict(schedule_ms=ms(t[kind]["schedule"]), schedule_median_ms=med(t[kind]["schedule"]), mix_ms=ms(t[kind]["mix"]),
                             mix_median_ms=med(t[kind]["mix"]),
                             total_median_ms=round(med(t[kind]["schedule"]) + med(t[kind]["mix"]), 3))
        res["bytes_per_set"] = dict(taps=4 * C * N * K, bank=8 * N * J)
        print(json.dumps(res), flush=True)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=1024)
    ap.add_argument("--modes", type=int, default=512)
    ap.add_argument("--buffers", type=int, default=860)
    ap.add_argument("--taps", type=int, default=128)
    ap.add_argument("--filters", type=int, default=1024)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    for delay in (False, True):
        run(a, delay)


if __name__ == "__main__":
    main()
