"""The reference of the tests of the scene filter mix's delay stage: tests/cpp/scene_fir_delay_ref.c (z of one step, about 20
lines of C) compiled with the host compiler into a temporary directory, and a model around it that keeps the delay records and
both tails as the engine does (scene_fir.cpp): the last max_delay + 1 samples of x here, the last max_onset + K - 1 samples of z
in the filter mix's own model (tests/scene_fir_model.py, imported as it is), which is fed z in place of x."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests.scene_fir_model import Model as FirModel

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
_tmp = None

PARAM = np.dtype([("from", "<f8"), ("to", "<f8"), ("t_set", "<i8"), ("slope", "<f8")])     # SceneParam of scene_ramp.h


def ref_lib():
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="scene_fir_delay_ref_")
        so = os.path.join(_tmp.name, "libscene_fir_delay_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-march=native", "-shared", "-fPIC",
                        os.path.join(_HERE, "cpp", "scene_fir_delay_ref.c"), "-o", so, "-lm"], check=True)
        _lib = C.CDLL(so)
        _lib.scene_fir_delay_ref.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_longlong, C.c_longlong, C.c_void_p, C.c_int,
                                             C.c_longlong, C.POINTER(C.c_float)]
        _lib.scene_fir_delay_ref.restype = None
    return _lib


def delayed(xx, Hx, p, R, t0):
    """z [N][n] float32 of the step that starts at absolute sample t0; xx [N][Hx + n] = the x history ++ the step's rows"""
    fp = C.POINTER(C.c_float)
    xx = np.ascontiguousarray(xx, dtype=np.float32)
    p = np.ascontiguousarray(p, dtype=PARAM)
    n_obj, n = xx.shape[0], xx.shape[1] - Hx
    assert p.shape == (n_obj,) and PARAM.itemsize == 32 and n >= 0
    z = np.empty((n_obj, n), dtype=np.float32)
    ref_lib().scene_fir_delay_ref(xx.ctypes.data_as(fp), n_obj, Hx, n, p.ctypes.data_as(C.c_void_p), int(R), int(t0), z.ctypes.data_as(fp))
    return z


def ramp_value(p, t, R):
    """p(t) of every record of p, the engine's expression: two rounded fp64 operations (numpy fuses nothing)"""
    k = t - p["t_set"] + 1
    if R == 0:
        return p["to"].copy()
    return np.where(k >= R, p["to"], p["from"] + p["slope"] * k.astype(np.float64))


class DelayLine:
    """the delay records and the x tail: rows of a step in, z of that step out"""

    def __init__(self, n_obj, max_delay, ramp):
        self.N, self.max_delay, self.R, self.Hx = n_obj, max_delay, ramp, max_delay + 1
        self.p = np.zeros(n_obj, dtype=PARAM)                        # every delay 0 until the first set
        self.pend = None
        self.any_set = self.ramping = False
        self.t = self.t_set = self.n_sets = 0
        self.tail = np.zeros((n_obj, self.Hx), dtype=np.float32)     # x(t - Hx) .. x(t - 1)

    def set(self, delay):
        v = np.asarray(delay, dtype=np.float32).astype(np.float64).reshape(self.N)
        assert np.isfinite(v).all() and (v >= 0).all() and (v <= self.max_delay).all()
        self.pend = v                                                # (replaces a set that no step has taken up)
        self.n_sets += 1

    def ramp_end(self):
        """the first t at which every ramp is over; t when none runs"""
        return self.t_set + self.R - 1 if self.ramping and self.t - self.t_set + 1 < self.R else self.t

    def reset(self):
        if self.pend is not None:
            self.p["to"], self.pend = self.pend, None
        self.p["from"] = self.p["to"]
        self.p["t_set"] = 0
        self.p["slope"] = 0.0
        self.tail[:] = 0
        self.t = self.t_set = 0
        self.any_set = self.ramping = False

    def step(self, rows):
        rows = np.asarray(rows, dtype=np.float32)
        if self.pend is not None:                                    # takes effect at the first sample of this step
            frm = ramp_value(self.p, self.t - 1, self.R) if self.any_set else self.pend
            self.p["from"], self.p["to"], self.p["t_set"] = frm, self.pend, self.t
            self.p["slope"] = (self.p["to"] - self.p["from"]) / float(self.R) if self.R else 0.0
            self.ramping = self.any_set and self.R > 0
            self.t_set, self.any_set, self.pend = self.t, True, None
        xx = np.concatenate([self.tail, rows], axis=1)               # xx[:, Hx + j] = x(t + j)
        z = delayed(xx, self.Hx, self.p, self.R, self.t)
        self.tail = np.ascontiguousarray(xx[:, xx.shape[1] - self.Hx:])
        self.t += rows.shape[1]
        return z


class Model:
    """the filter mix behind the delay stage: scene_fir_model.Model fed z; its tail is the history of z"""

    def __init__(self, n_channels, n_obj, n_taps, max_onset, xfade, max_delay, ramp):
        self._fir_args = (n_channels, n_obj, n_taps, max_onset, xfade)
        self.fir = FirModel(*self._fir_args)
        self.line = DelayLine(n_obj, max_delay, ramp)

    def set(self, taps, onset=None):
        self.fir.set(taps, onset)

    def set_delay(self, delay):
        self.line.set(delay)

    def reset(self):
        """both histories cleared, the filters gone, the delays kept with their ramps finished"""
        self.fir = FirModel(*self._fir_args)
        self.line.reset()

    def info(self):
        return {"max_delay": self.line.max_delay, "ramp_samples": self.line.R, "ramp_end": self.line.ramp_end(), "sets": self.line.n_sets}

    def mix(self, rows, samples=None):
        return self.fir.mix(self.line.step(rows), samples)
