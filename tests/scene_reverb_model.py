"""The reference of the scene reverb's tests: tests/cpp/scene_reverb_ref.c (the stated order of arithmetic in about 30 lines of C)
compiled with the host compiler into a temporary directory, and a model around it that keeps from / to / t_set and a tail of
past input samples as the engine does, and evaluates any list of output samples of a step."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
SEGMENT = 2048
_lib = None
_tmp = None


def ref_lib():
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="scene_reverb_ref_")
        so = os.path.join(_tmp.name, "libscene_reverb_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-march=native", "-shared", "-fPIC",
                        os.path.join(_HERE, "cpp", "scene_reverb_ref.c"), "-o", so, "-lm"], check=True)
        _lib = C.CDLL(so)
        fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_long)
        _lib.scene_reverb_ref.argtypes = [fp, C.c_int, C.c_long, C.c_long, fp, fp, C.c_int, C.c_int, C.c_long, C.c_int, lp, C.c_int, fp, fp]
        _lib.scene_reverb_ref.restype = None
    return _lib


def evaluate(u, base, r_to, r_from, t_set, R, ts, add=None, shape=None):
    """out [n_out][len(ts)] float32 at the absolute samples ts; u [n_in][L] float32 holds samples base .. base + L - 1; r_* [n_out][n_in][K]
    (r_to None: nothing set, shape = (n_out, n_in, K)); add [n_out][len(ts)] or None"""
    fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_long)
    ptr = lambda a: None if a is None else a.ctypes.data_as(fp)
    u = np.ascontiguousarray(u, dtype=np.float32)
    r_to = None if r_to is None else np.ascontiguousarray(r_to, dtype=np.float32)
    r_from = None if r_from is None else np.ascontiguousarray(r_from, dtype=np.float32)
    n_out, n_in, K = shape if r_to is None else r_to.shape
    assert u.shape[0] == n_in and (r_from is None or r_from.shape == (n_out, n_in, K))
    ts = np.ascontiguousarray(ts, dtype=np.int64).astype(C.c_long)
    add = None if add is None else np.ascontiguousarray(add, dtype=np.float32)
    assert add is None or add.shape == (n_out, ts.size)
    out = np.empty((n_out, ts.size), dtype=np.float32)
    ref_lib().scene_reverb_ref(ptr(u), n_in, u.shape[1], int(base), ptr(r_to), ptr(r_from), n_out, K, int(t_set), int(R),
                               ts.ctypes.data_as(lp), ts.size, ptr(add), ptr(out))
    return out


class FadeRunning(Exception):
    """a set while the last one's cross-fade is still running (the engine's PBSO_ERR_STATE)"""


class Model:
    def __init__(self, n_in, n_out, n_taps, xfade):
        self.n_in, self.n_out, self.K, self.R = n_in, n_out, n_taps, xfade
        self.H = n_taps - 1
        self.tail = np.zeros((n_in, self.H), dtype=np.float32)       # u(t - H) .. u(t - 1)
        self.t = self.t_set = 0
        self.to = self.frm = self.pending = None

    def fade_end(self):
        """the first t at which the running fade is over; t when none runs"""
        return self.t_set + self.R - 1 if self.frm is not None and self.t - self.t_set + 1 < self.R else self.t

    def set(self, taps):
        if self.fade_end() > self.t:
            raise FadeRunning()
        self.pending = np.array(taps, dtype=np.float32).reshape(self.n_out, self.n_in, self.K)

    def process(self, input, add=None, samples=None):
        """input [n_in][n] float32, the next step; add [n_out][n] or None -> out [n_out][len(samples)] at the step's local samples
        (default: all of them)"""
        u = np.asarray(input, dtype=np.float32).reshape(self.n_in, -1)
        n = u.shape[1]
        if self.pending is not None:
            self.frm, self.to, self.pending, self.t_set = self.to, self.pending, None, self.t
        samples = np.arange(n) if samples is None else np.asarray(samples, dtype=np.int64)
        uu = np.concatenate([self.tail, u], axis=1)                  # uu[:, H + j] = u(t + j)
        a = None if add is None else np.asarray(add, dtype=np.float32).reshape(self.n_out, n)[:, samples]
        out = evaluate(uu, self.t - self.H, self.to, self.frm, self.t_set, self.R, self.t + samples, a, (self.n_out, self.n_in, self.K))
        self.tail = np.ascontiguousarray(uu[:, uu.shape[1] - self.H:])
        self.t += n
        return out
