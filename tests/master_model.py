"""The reference of the master bus's tests: tests/cpp/master_ref.c (the stated order of arithmetic in a page of C) compiled with the
host compiler into a temporary directory, and a model around it that keeps the history of v, the gain with its ramp and t as the
engine does, and computes the meters of every buffer.  The window's taps are an input: no test depends on a cos.  The C file has
the sliding minimum twice: in linear time (master_ref, what every test runs against) and as the header's double loop
(master_ref_literal: evaluate(..., literal=True), Model(..., literal=True)); tests/test_master_model.py holds the two bit-equal."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
B = 513                                  # the default buffer length (Model(frames=...) takes any other)
METER_DTYPE = np.dtype([("in_peak", np.float32), ("out_peak", np.float32), ("min_gain", np.float32), ("n_limited", np.int32),
                        ("sumsq", np.float64)])
_lib = None
_tmp = None


def ref_lib():
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="master_ref_")
        so = os.path.join(_tmp.name, "libmaster_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-march=native", "-shared", "-fPIC",
                        os.path.join(_HERE, "cpp", "master_ref.c"), "-o", so, "-lm"], check=True)
        _lib = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        for f in (_lib.master_ref, _lib.master_ref_literal):
            f.argtypes = [fp, C.c_int, C.c_long, C.c_int, C.c_int, C.c_float, fp, fp, fp, C.POINTER(C.c_long)]
            f.restype = None
    return _lib


def window(L):
    """the engine's formula in numpy: fp64 raised cosine, summed in ascending k, rounded to f32 once"""
    h = 1.0 - np.cos(2.0 * np.pi * (np.arange(L, dtype=np.float64) + 1.0) / (L + 1.0))
    s = 0.0
    for x in h:
        s += float(x)
    return (h / s).astype(np.float32)


def evaluate(v, L, H, T, w, literal=False):
    """v [C][2 L + H + n] float32: the history in front of the step -> y [C][n], g [n], number of chains that ended above 1.f
    (literal: the sliding minimum by the header's double loop, O(n (L + H)), instead of in linear time)"""
    fp = C.POINTER(C.c_float)
    v = np.ascontiguousarray(v, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    assert w.shape == (L,)
    n = v.shape[1] - (2 * L + H)
    y, g, cnt = np.empty((v.shape[0], n), dtype=np.float32), np.empty(n, dtype=np.float32), C.c_long(0)
    master_ref = ref_lib().master_ref_literal if literal else ref_lib().master_ref
    master_ref(v.ctypes.data_as(fp), v.shape[0], n, L, H, C.c_float(T), w.ctypes.data_as(fp), y.ctypes.data_as(fp),
               g.ctypes.data_as(fp), C.byref(cnt))
    return y, g, cnt.value


class Model:
    def __init__(self, n_channels, ceiling, lookahead, hold, ramp, w=None, frames=B, literal=False):
        self.literal = literal
        self.B = frames                                                    # the meters' buffer length
        self.C, self.T, self.L, self.H, self.R = n_channels, float(np.float32(ceiling)), lookahead, hold, ramp
        self.HL = 2 * lookahead + hold
        self.w = window(lookahead) if w is None else np.asarray(w, dtype=np.float32)
        self.tail = np.zeros((n_channels, self.HL), dtype=np.float32)      # v(t - HL) .. v(t - 1)
        self.t = 0
        self.frm = self.to = 1.0                                           # the gain: fp64 from, to, slope; t_set
        self.slope, self.t_set = 0.0, 0
        self.n_acc_above_one = 0
        self.meters = self.gains = None

    def _p(self, t):
        """p(t) for an array (or one) of absolute samples, in fp64: to once t - t_set + 1 >= R, else from + slope * k"""
        k = np.asarray(t, dtype=np.int64) - self.t_set + 1
        ramp = np.float64(self.frm) + np.float64(self.slope) * k.astype(np.float64)
        return np.where((self.R == 0) | (k >= self.R), np.float64(self.to), ramp)

    def ramp_end(self):
        return self.t_set + self.R - 1 if self.frm != self.to and self.t - self.t_set + 1 < self.R else self.t

    def set_gain(self, gain):
        self.frm = float(self._p(self.t - 1))
        self.to = float(np.float32(gain))
        self.t_set = self.t
        self.slope = (self.to - self.frm) / float(self.R) if self.R else 0.0

    def reset(self):
        self.tail[:] = 0
        self.t, self.frm, self.slope, self.t_set = 0, self.to, 0.0, 0

    def process(self, input):
        """input [C][n] float32, the next step (n a multiple of the buffer length for the meters) -> y [C][n]; self.meters [n // B][C]"""
        u = np.asarray(input, dtype=np.float32).reshape(self.C, -1)
        n = u.shape[1]
        p = self._p(self.t + np.arange(n)).astype(np.float32)
        v = p[None, :] * u                                                 # one rounded f32 multiplication
        vv = np.concatenate([self.tail, v], axis=1)
        y, g, cnt = evaluate(vv, self.L, self.H, self.T, self.w, self.literal)
        self.n_acc_above_one += cnt
        self.tail = np.ascontiguousarray(vv[:, vv.shape[1] - self.HL:])
        self.t += n
        self.gains = g
        B = self.B
        if n % B == 0:
            nb = n // B
            m = np.zeros((nb, self.C), dtype=METER_DTYPE)
            gb = g.reshape(nb, B)
            for c in range(self.C):
                m["in_peak"][:, c] = np.abs(v[c]).reshape(nb, B).max(axis=1)
                m["out_peak"][:, c] = np.abs(y[c]).reshape(nb, B).max(axis=1)
                m["min_gain"][:, c] = gb.min(axis=1)
                m["n_limited"][:, c] = (gb < np.float32(1)).sum(axis=1)
                sq = y[c].astype(np.float64).reshape(nb, B) ** 2
                m["sumsq"][:, c] = np.cumsum(sq, axis=1)[:, -1]            # the ascending sum
            self.meters = m
        return y


def pcm16(y):
    """interleaved [n][C] int16: (int16_t)lrintf(y * 32767.f) -- one rounded f32 multiplication, then to nearest, ties to even"""
    x = np.asarray(y, dtype=np.float32) * np.float32(32767.0)
    return np.ascontiguousarray(np.rint(x).astype(np.int16).T)
