"""The reference of the scene mix's bit-exact tests: tests/cpp/scene_mix_ref.c (the stated order of arithmetic in about 30 lines
of C) compiled with the host compiler into a temporary directory, and a model around it that keeps the (from, to, t_set, slope)
records in fp64 and a tail of past samples as the engine does (scene_mix.cpp), and evaluates any list of output samples of a step."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_tmp = None

PARAM = np.dtype([("from", "<f8"), ("to", "<f8"), ("t_set", "<i8"), ("slope", "<f8")])     # SceneParam of kernels.h


def ref_lib():
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="scene_mix_ref_")
        so = os.path.join(_tmp.name, "libscene_mix_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-march=native", "-shared", "-fPIC",
                        os.path.join(_HERE, "cpp", "scene_mix_ref.c"), "-o", so, "-lm"], check=True)
        _lib = C.CDLL(so)
        fp, llp = C.POINTER(C.c_float), C.POINTER(C.c_longlong)
        _lib.scene_mix_ref.argtypes = [fp, C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.c_int, C.c_int, llp, C.c_int, fp]
        _lib.scene_mix_ref.restype = None
    return _lib


def evaluate(x, base, params, R, ts):
    """out [C][len(ts)] float32 at the absolute samples ts; x [N][L] float32 holds samples base .. base + L - 1;
    params [C][N][2] of PARAM (gain, delay)"""
    fp, llp = C.POINTER(C.c_float), C.POINTER(C.c_longlong)
    x = np.ascontiguousarray(x, dtype=np.float32)
    params = np.ascontiguousarray(params, dtype=PARAM)
    n_ch, n_obj, two = params.shape
    assert two == 2 and x.shape[0] == n_obj and PARAM.itemsize == 32
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    out = np.empty((n_ch, ts.size), dtype=np.float32)
    ref_lib().scene_mix_ref(x.ctypes.data_as(fp), n_obj, x.shape[1], int(base), params.ctypes.data_as(C.c_void_p), n_ch, int(R),
                            ts.ctypes.data_as(llp), ts.size, out.ctypes.data_as(fp))
    return out


def ramp_value(p, t, R):
    """p(t) of every record of p, the engine's expression: two rounded fp64 operations (numpy fuses nothing)"""
    k = t - p["t_set"] + 1
    if R == 0:
        return p["to"].copy()
    return np.where(k >= R, p["to"], p["from"] + p["slope"] * k.astype(np.float64))


class Model:
    def __init__(self, n_channels, n_obj, max_delay, ramp):
        self.C, self.N, self.R = n_channels, n_obj, ramp
        self.H = max_delay + 1
        self.p = np.zeros((n_channels, n_obj, 2), dtype=PARAM)       # (gain, delay): silence until the first set
        self.any_set = False
        self.t = 0
        self.tail = np.zeros((n_obj, self.H), dtype=np.float32)      # x(t - H) .. x(t - 1)

    def set(self, gain, delay=None):
        for kind, v in ((0, gain), (1, delay)):
            if v is None:
                continue
            v = np.asarray(v, dtype=np.float32).astype(np.float64).reshape(self.C, self.N)
            q = self.p[:, :, kind]                                   # (a view)
            frm = ramp_value(q, self.t - 1, self.R) if self.any_set else v
            q["from"], q["to"], q["t_set"] = frm, v, self.t
            q["slope"] = (q["to"] - q["from"]) / float(self.R) if self.R else 0.0
        self.any_set = True

    def reset(self):
        self.p["from"] = self.p["to"]
        self.p["t_set"] = 0
        self.p["slope"] = 0.0
        self.tail[:] = 0
        self.t = 0
        self.any_set = False

    def mix(self, rows, samples=None):
        """rows [N][n] float32, the next step -> out [C][len(samples)] at the step's local samples (default: all of them)"""
        rows = np.asarray(rows, dtype=np.float32)
        n = rows.shape[1]
        samples = np.arange(n) if samples is None else np.asarray(samples, dtype=np.int64)
        xx = np.concatenate([self.tail, rows], axis=1)               # xx[:, H + j] = x(t + j)
        out = evaluate(xx, self.t - self.H, self.p, self.R, self.t + samples)
        self.tail = np.ascontiguousarray(xx[:, xx.shape[1] - self.H:])
        self.t += n
        return out
