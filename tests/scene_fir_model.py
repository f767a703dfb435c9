"""The reference of the scene filter mix's tests: tests/cpp/scene_fir_ref.c (the stated chain of fmaf in about 30 lines of C)
compiled with the host compiler into a temporary directory, and a model around it that keeps from / to / t_set and a tail of
past samples as the engine does, and evaluates any list of output samples of a step."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_tmp = None


def ref_lib():
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="scene_fir_ref_")
        so = os.path.join(_tmp.name, "libscene_fir_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-march=native", "-shared", "-fPIC",
                        os.path.join(_HERE, "cpp", "scene_fir_ref.c"), "-o", so, "-lm"], check=True)
        _lib = C.CDLL(so)
        fp, ip, lp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_long)
        _lib.scene_fir_ref.argtypes = [fp, C.c_int, C.c_long, C.c_long, fp, ip, fp, ip, C.c_int, C.c_int, C.c_long, C.c_int, lp, C.c_int, fp]
        _lib.scene_fir_ref.restype = None
    return _lib


def evaluate(x, base, h_to, d_to, h_from, d_from, t_set, R, ts):
    """out [C][len(ts)] float32 at the absolute samples ts; x [N][L] float32 holds samples base .. base + L - 1; h_* [C][N][K]"""
    fp, ip, lp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_long)
    x = np.ascontiguousarray(x, dtype=np.float32)
    h_to = np.ascontiguousarray(h_to, dtype=np.float32)
    d_to = np.ascontiguousarray(d_to, dtype=np.int32)
    n_ch, n_obj, K = h_to.shape
    assert x.shape[0] == n_obj and d_to.shape == (n_obj,)
    if h_from is not None:
        h_from = np.ascontiguousarray(h_from, dtype=np.float32)
        d_from = np.ascontiguousarray(d_from, dtype=np.int32)
        assert h_from.shape == h_to.shape and d_from.shape == d_to.shape
    ts = np.ascontiguousarray(ts, dtype=np.int64).astype(C.c_long)
    out = np.empty((n_ch, ts.size), dtype=np.float32)
    ref_lib().scene_fir_ref(x.ctypes.data_as(fp), n_obj, x.shape[1], int(base), h_to.ctypes.data_as(fp), d_to.ctypes.data_as(ip),
                            None if h_from is None else h_from.ctypes.data_as(fp), None if h_from is None else d_from.ctypes.data_as(ip),
                            n_ch, K, int(t_set), int(R), ts.ctypes.data_as(lp), ts.size, out.ctypes.data_as(fp))
    return out


class FadeRunning(Exception):
    """a set while the last one's cross-fade is still running (the engine's PBSO_ERR_STATE)"""


class Model:
    def __init__(self, n_channels, n_obj, n_taps, max_onset, xfade):
        self.C, self.N, self.K, self.R = n_channels, n_obj, n_taps, xfade
        self.H = max_onset + n_taps - 1
        self.tail = np.zeros((n_obj, self.H), dtype=np.float32)      # x(t - H) .. x(t - 1)
        self.t = self.t_set = 0
        self.to = self.frm = self.pending = None                     # (taps, onsets)

    def fade_end(self):
        """the first t at which the running fade is over; t when none runs"""
        return self.t_set + self.R - 1 if self.frm is not None and self.t - self.t_set + 1 < self.R else self.t

    def set(self, taps, onset=None):
        if self.fade_end() > self.t:
            raise FadeRunning()
        h = np.array(taps, dtype=np.float32).reshape(self.C, self.N, self.K)
        if onset is None:
            last = self.pending or self.to
            d = np.zeros(self.N, dtype=np.int32) if last is None else last[1]
        else:
            d = np.array(onset, dtype=np.int32).reshape(self.N)
        self.pending = (h, d)

    def mix(self, rows, samples=None):
        """rows [N][n] float32, the next step -> out [C][len(samples)] at the step's local samples (default: all of them)"""
        rows = np.asarray(rows, dtype=np.float32)
        n = rows.shape[1]
        if self.pending is not None:
            self.frm, self.to, self.pending, self.t_set = self.to, self.pending, None, self.t
        samples = np.arange(n) if samples is None else np.asarray(samples, dtype=np.int64)
        xx = np.concatenate([self.tail, rows], axis=1)               # xx[:, H + j] = x(t + j)
        if self.to is None:
            out = np.zeros((self.C, samples.size), dtype=np.float32)
        else:
            frm = self.frm or (None, None)
            out = evaluate(xx, self.t - self.H, self.to[0], self.to[1], frm[0], frm[1], self.t_set, self.R, self.t + samples)
        self.tail = np.ascontiguousarray(xx[:, xx.shape[1] - self.H:])
        self.t += n
        return out
