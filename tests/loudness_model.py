"""The reference of the loudness bus's tests: tests/cpp/loudness_ref.c (the stated arithmetic in plain C with fma() and fmaf(), and
the plain serial fp64 recurrence) compiled with the host compiler into a temporary directory, and a model around it that keeps the
clock, the histories of the K-weighting's signals, the 64 accumulators, the 11 input samples and the running maxima as the engine
does, so that it can be stepped in cuts.  design() is the header's K-weighting in numpy scalars; taps() is the header's prototype
rule in numpy (tests/resample_model.py); report() is the header's gating in numpy, in the stated order of the sums."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

from tests import resample_model as rm

_HERE = os.path.dirname(os.path.abspath(__file__))
BLOCK = np.dtype([("energy", "<f8"), ("true_peak", "<f4"), ("sample_peak", "<f4")])
P = 64                                                   # PBSO_EQ_BLOCK
LANES, TAPS, TAIL = 64, 12, 11
_lib = None
_tmp = None


def ref_lib():
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="loudness_ref_")
        so = os.path.join(_tmp.name, "libloudness_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-march=native", "-shared", "-fPIC",
                        os.path.join(_HERE, "cpp", "loudness_ref.c"), "-o", so, "-lm"], check=True)
        _lib = C.CDLL(so)
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        _lib.loud_ref_serial.argtypes = [dp, C.c_long, dp, dp, dp]
        _lib.loud_ref_tables.argtypes = [dp, C.c_int, dp]
        _lib.loud_ref_block.argtypes = [dp, C.c_int, C.c_long, C.c_long, dp, dp]
        _lib.loud_ref_energy.argtypes = [dp, C.c_long, C.c_long, C.c_long, dp, dp]
        _lib.loud_ref_peak.argtypes = [fp, C.c_long, C.c_long, C.c_long, fp, C.c_int, fp, fp, fp]
        for f in (_lib.loud_ref_serial, _lib.loud_ref_tables, _lib.loud_ref_block):
            f.restype = None
        _lib.loud_ref_energy.restype = _lib.loud_ref_peak.restype = C.c_long
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def hop(rate):
    assert rate % 10 == 0 and rate // 10 >= 256
    return rate // 10


def oversampling(rate):
    return 4 if rate < 80000 else 2


def design(rate):
    """the header's K-weighting, line by line, in fp64: [2][5] = b0 b1 b2 a1 a2"""
    f = np.float64
    one, two, rate = f(1.0), f(2.0), f(rate)
    f0, G, Q = f(1681.974450955533), f(3.999843853973347), f(0.7071752369554196)
    K = f(math.tan(f(math.pi) * f0 / rate))
    Vh = f(math.pow(10.0, G / f(20.0)))
    Vb = f(math.pow(Vh, 0.4996667741545416))
    a0 = one + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, two * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, two * (K * K - one) / a0,
             (one - K / Q + K * K) / a0]
    f0, Q = f(38.13547087602444), f(0.5003270373238773)
    K = f(math.tan(f(math.pi) * f0 / rate))
    a0 = one + K / Q + K * K
    highpass = [one, -two, one, two * (K * K - one) / a0, (one - K / Q + K * K) / a0]
    return np.array([shelf, highpass], dtype=np.float64)


def taps(rate):
    """the true peak's phase table h[O][12] float32: the resampler's prototype rule with L = O, M = 1, beta = 8, cutoff = 1"""
    return rm.design(oversampling(rate), 1, TAPS, 8.0, 1.0)


def tables(sos):
    """sos [S][5] -> [S][5][P] = h r s p q, by the C reference's recurrence"""
    sos = np.ascontiguousarray(sos, dtype=np.float64).reshape(-1, 5)
    out = np.empty((sos.shape[0], 5, P))
    for i in range(sos.shape[0]):
        ref_lib().loud_ref_tables(_dp(sos[i]), P, _dp(out[i]))
    return out


def serial(sos, x):
    """x [n] through the cascade sos [S][5] by the plain fp64 recurrence, from silence"""
    y = np.ascontiguousarray(x, dtype=np.float64)
    for c in np.ascontiguousarray(sos, dtype=np.float64).reshape(-1, 5):
        out, st = np.empty_like(y), np.zeros(4)
        ref_lib().loud_ref_serial(_dp(c), y.size, _dp(y), _dp(st), _dp(out))
        y = out
    return y


def lufs(w):
    return -0.691 + 10.0 * math.log10(w) if w > 0.0 else -math.inf


def _window(E, G, hs, W):
    """w_i for i >= W - 1 over E [n][C]: per channel the energies summed left to right, / (W hs), the channels in ascending c"""
    n, Cn = E.shape
    if n < W:
        return np.empty(0)
    m = n - W + 1
    w = np.zeros(m)
    for c in range(Cn):
        e = E[0:m, c].copy()
        for k in range(1, W):
            e = e + E[k:k + m, c]
        w = w + np.float64(G[c]) * (e / (np.float64(W) * np.float64(hs)))
    return w


def _mean(w):
    return np.cumsum(w)[-1] / np.float64(w.size)        # (cumsum adds in ascending order, one by one)


def report(blocks, hs, weight=None):
    """the header's gating over blocks [n][C] (BLOCK records): a dict with the fields of pbso_loudness_summary"""
    blocks = np.asarray(blocks)
    n, Cn = blocks.shape
    G = np.ones(Cn) if weight is None else np.asarray(weight, dtype=np.float64)
    E = np.ascontiguousarray(blocks["energy"], dtype=np.float64)
    r = {k: -math.inf for k in ("integrated", "momentary", "short_term", "max_momentary", "max_short_term", "relative_threshold")}
    r["true_peak"] = float(blocks["true_peak"].max()) if blocks.size else 0.0
    r["sample_peak"] = float(blocks["sample_peak"].max()) if blocks.size else 0.0
    r["n_blocks"], r["n_gated"] = n, 0
    w = _window(E, G, hs, 4)
    l = np.array([lufs(v) for v in w])
    if l.size:
        r["momentary"], r["max_momentary"] = float(l[-1]), float(l.max())
    ws = _window(E, G, hs, 30)
    if ws.size:
        ls = np.array([lufs(v) for v in ws])
        r["short_term"], r["max_short_term"] = float(ls[-1]), float(ls.max())
    A = l > -70.0
    if A.any():
        gamma = lufs(_mean(w[A])) - 10.0
        r["relative_threshold"] = gamma
        Gt = A & (l > gamma)
        r["n_gated"] = int(Gt.sum())
        if Gt.any():
            r["integrated"] = lufs(_mean(w[Gt]))
    return r


class Model:
    """the stage at `rate` on C channels: process(u [C][n] float32) appends the records of the sub-blocks that end in the step"""

    def __init__(self, rate, n_channels, weight=None, true_peak=True, taps_=None):
        self.rate, self.C, self.hs, self.O = rate, n_channels, hop(rate), oversampling(rate)
        self.weight = np.ones(n_channels) if weight is None else np.asarray(weight, dtype=np.float64)
        self.true_peak = true_peak
        self.h = np.ascontiguousarray(taps(rate) if taps_ is None else taps_, dtype=np.float32)
        assert self.h.shape == (self.O, TAPS)
        self.tab = tables(design(rate))                  # [2][5][P]
        self.reset()

    def reset(self):
        self.t = 0
        self.hist = np.zeros((self.C, 3, P + 2))         # the last P + 2 samples of signals 0, 1, 2
        self.acc = np.zeros((self.C, LANES))
        self.tail = np.zeros((self.C, TAIL), dtype=np.float32)
        self.run = np.zeros((self.C, 2), dtype=np.float32)
        self.records = np.zeros((0, self.C), dtype=BLOCK)

    def weighted(self, u):
        """z [C][n] float64 of the step u [C][n]; the histories move on"""
        n = u.shape[1]
        k0 = self.t % P
        z = np.empty((self.C, n))
        for c in range(self.C):
            x = np.concatenate([self.hist[c, 0], u[c].astype(np.float64)])
            self.hist[c, 0] = x[n:]
            for s in range(2):
                y = np.concatenate([self.hist[c, s + 1], np.zeros(n)])
                ref_lib().loud_ref_block(_dp(np.ascontiguousarray(self.tab[s])), P, k0, n, _dp(x), _dp(y))
                self.hist[c, s + 1] = y[n:]
                x = y
            z[c] = x[P + 2:]
        return z

    def process(self, input):
        u = np.ascontiguousarray(input, dtype=np.float32).reshape(self.C, -1)
        n = u.shape[1]
        k0 = self.t % self.hs
        done = (k0 + n) // self.hs
        rec = np.zeros((done, self.C), dtype=BLOCK)
        z = self.weighted(u)
        for c in range(self.C):
            e = np.zeros(max(done, 1))
            acc = np.ascontiguousarray(self.acc[c])
            assert ref_lib().loud_ref_energy(_dp(np.ascontiguousarray(z[c])), n, k0, self.hs, _dp(acc), _dp(e)) == done
            self.acc[c] = acc
            rec["energy"][:, c] = e[:done]
            if self.true_peak:
                x = np.ascontiguousarray(np.concatenate([self.tail[c], u[c]]))
                tp, sp = np.zeros(max(done, 1), dtype=np.float32), np.zeros(max(done, 1), dtype=np.float32)
                run = np.ascontiguousarray(self.run[c])
                assert ref_lib().loud_ref_peak(_fp(x), n, k0, self.hs, _fp(self.h), self.O, _fp(run), _fp(tp), _fp(sp)) == done
                self.run[c] = run
                self.tail[c] = x[n:]
                rec["true_peak"][:, c], rec["sample_peak"][:, c] = tp[:done], sp[:done]
        self.records = np.concatenate([self.records, rec])
        self.t += n
        return rec

    def report(self):
        return report(self.records, self.hs, self.weight)
