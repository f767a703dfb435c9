"""The reference of the resampler bus's tests: tests/cpp/resample_ref.c (the stated arithmetic in about 30 lines of C) compiled with
the host compiler into a temporary directory, and a model around it that keeps the tail of the input, t, m and p0 as the engine
does.  The taps are an input of the model, so no bit-exact test depends on a sin; design() is the header's formula in numpy, for
the tests that are about the design.  evaluate64() is an independent fp64 evaluation of the same definition in numpy."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
METER_DTYPE = np.dtype([("out_peak", np.float32), ("n_over", np.int32)])
_lib = None
_tmp = None


def ref_lib():
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="resample_ref_")
        so = os.path.join(_tmp.name, "libresample_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-march=native", "-shared", "-fPIC",
                        os.path.join(_HERE, "cpp", "resample_ref.c"), "-o", so, "-lm"], check=True)
        _lib = C.CDLL(so)
        fp = C.POINTER(C.c_float)
        _lib.resample_ref.argtypes = [fp, C.c_int, C.c_long, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_int, fp, fp]
        _lib.resample_ref.restype = None
    return _lib


def ratio(rate_in, rate_out):
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g                                     # L, M


def ceil_div(a, b):
    return -((-a) // b)


def i0(x):
    """the power series of the header: ((x / 2)^k / k!)^2 in ascending k until a term is below 1e-17 of the sum"""
    q, s = 1.0, 1.0
    for k in range(1, 1000):
        q *= (0.5 * x) / k
        s += q * q
        if q * q < 1e-17 * s:
            break
    return s


def prototype(L, M, T, beta=9.0, cutoff=0.9):
    """g[j], j < N = L T, fp64"""
    N = L * T
    x = np.arange(N, dtype=np.float64) - 0.5 * (N - 1)
    fc = cutoff * 0.5 / max(L, M)
    a = 2.0 * fc * x
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(a == 0.0, 1.0, np.sin(np.pi * a) / (np.pi * a))
    if N > 1:
        r = 2.0 * x / (N - 1)
        arg = beta * np.sqrt(np.maximum(1.0 - r * r, 0.0))
        win = np.array([i0(float(v)) for v in arg]) / i0(beta)
    else:
        win = np.ones(1)
    return L * 2.0 * fc * sinc * win


def design(L, M, T, beta=9.0, cutoff=0.9, dtype=np.float32):
    """the phase table h[phi][k] = g[k L + phi], [L][T]"""
    return np.ascontiguousarray(prototype(L, M, T, beta, cutoff).reshape(T, L).T.astype(dtype))


def evaluate(u, t0, m_lo, n_out, L, M, h):
    """u [C][T - 1 + n] float32: the history in front of the step -> y [C][n_out] for the outputs m_lo .. m_lo + n_out - 1"""
    fp = C.POINTER(C.c_float)
    u = np.ascontiguousarray(u, dtype=np.float32)
    h = np.ascontiguousarray(h, dtype=np.float32)
    T = h.shape[1]
    assert h.shape == (L, T)
    n = u.shape[1] - (T - 1)
    y = np.empty((u.shape[0], n_out), dtype=np.float32)
    if n_out:
        assert t0 <= m_lo * M // L and (m_lo + n_out - 1) * M // L < t0 + n
        ref_lib().resample_ref(u.ctypes.data_as(fp), u.shape[0], n, t0, m_lo, n_out, L, M, T, h.ctypes.data_as(fp), y.ctypes.data_as(fp))
    return y


def evaluate64(u, L, M, h, m_lo=0, n_out=None):
    """u [C][n] from t = 0 (silence before it) -> (y [C][n_out] in fp64 with the taps h as given, bound [C][n_out] = sum_k |h[phi][k]|
    max|u|): the definition once more, gathered in numpy and summed in fp64, independent of the C reference"""
    u = np.asarray(u, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    T = h.shape[1]
    n = u.shape[1]
    if n_out is None:
        n_out = ceil_div(n * L, M) - m_lo
    m = m_lo + np.arange(n_out, dtype=np.int64)
    i, phi = (m * M) // L, (m * M) % L
    up = np.concatenate([np.zeros((u.shape[0], T - 1)), u], axis=1)
    idx = (i + (T - 1))[:, None] - np.arange(T)[None, :]                   # u(i - k) in up
    y = np.einsum("mk,cmk->cm", h[phi], up[:, idx])
    bound = np.abs(h[phi]).sum(axis=1)[None, :] * np.abs(u).max()
    return y, np.broadcast_to(bound, y.shape)


class Model:
    def __init__(self, n_channels, L, M, h):
        self.C, self.L, self.M = n_channels, L, M
        self.h = np.ascontiguousarray(h, dtype=np.float32)
        self.T = self.h.shape[1]
        assert self.h.shape == (L, self.T)
        self.tail = np.zeros((n_channels, self.T - 1), dtype=np.float32)   # u(t - (T - 1)) .. u(t - 1)
        self.t = self.m = self.p0 = 0
        self.meters = None

    def n_out(self, n):
        """of the next call of n input samples: ceil((t + n) L / M) - ceil(t L / M), in exact integers"""
        return ceil_div((self.t + n) * self.L, self.M) - ceil_div(self.t * self.L, self.M)

    def reset(self):
        self.tail[:] = 0
        self.t = self.m = self.p0 = 0

    def process(self, input):
        """input [C][n] float32, the next step -> y [C][n_out]; self.meters [C]"""
        u = np.asarray(input, dtype=np.float32).reshape(self.C, -1)
        n = u.shape[1]
        k = self.n_out(n)
        assert self.m == ceil_div(self.t * self.L, self.M) and self.p0 == self.m * self.M - self.t * self.L
        uu = np.concatenate([self.tail, u], axis=1)
        y = evaluate(uu, self.t, self.m, k, self.L, self.M, self.h)
        self.tail = np.ascontiguousarray(uu[:, uu.shape[1] - (self.T - 1):])
        self.t += n
        self.m += k
        self.p0 = self.m * self.M - self.t * self.L
        assert 0 <= self.p0 < self.M
        m = np.zeros(self.C, dtype=METER_DTYPE)
        if k:
            m["out_peak"] = np.abs(y).max(axis=1)
            m["n_over"] = (np.abs(y) > np.float32(1)).sum(axis=1)
        self.meters = m
        return y


def pcm16(y):
    """interleaved [n][C] int16: (int16_t)lrintf(fminf(fmaxf(y, -1.f), 1.f) * 32767.f)"""
    x = np.clip(np.asarray(y, dtype=np.float32), np.float32(-1), np.float32(1)) * np.float32(32767.0)
    return np.ascontiguousarray(np.rint(x).astype(np.int16).T)
