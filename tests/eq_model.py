"""The reference of the EQ bus's tests: tests/cpp/eq_ref.c (the stated arithmetic in about 40 lines of C with fma(), and the plain
serial fp64 recurrence) compiled with the host compiler into a temporary directory, and a model around it that keeps the clock, the
cross-fade and the histories of every signal of both cascades as the engine does, so that it can be stepped in cuts.  The tables
are an input of the model (set(tables=...)), so that a bit-exact test can feed it the engine's own; tables() builds them from
coefficients with the C reference; design() is the header's cookbook formulas in numpy scalars."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("lowpass", "highpass", "peak", "lowshelf", "highshelf")
_lib = None
_tmp = None


def block_size():
    hdr = open(os.path.join(os.path.dirname(_HERE), "include", "openpbso_amd.h")).read()
    import re
    return int(re.search(r"#define\s+PBSO_EQ_BLOCK\s+(\d+)", hdr).group(1))


P = block_size()
H = P + 2


def ref_lib():
    global _lib, _tmp
    if _lib is None:
        _tmp = tempfile.TemporaryDirectory(prefix="eq_ref_")
        so = os.path.join(_tmp.name, "libeq_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-march=native", "-shared", "-fPIC",
                        os.path.join(_HERE, "cpp", "eq_ref.c"), "-o", so, "-lm"], check=True)
        _lib = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        _lib.eq_ref_serial.argtypes = [dp, C.c_long, dp, dp, dp]
        _lib.eq_ref_tables.argtypes = [dp, C.c_int, dp]
        _lib.eq_ref_block.argtypes = [dp, C.c_int, C.c_long, C.c_long, dp, dp]
        for f in (_lib.eq_ref_serial, _lib.eq_ref_tables, _lib.eq_ref_block):
            f.restype = None
    return _lib


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def identity(n_channels, n_sections):
    sos = np.zeros((n_channels, n_sections, 5))
    sos[..., 0] = 1.0
    return sos


def tables(sos, block=None):
    """sos [...][5] -> [...][5][P] = h r s p q, by the C reference's recurrence"""
    block = P if block is None else block
    sos = np.ascontiguousarray(sos, dtype=np.float64)
    out = np.empty(sos.shape[:-1] + (5, block))
    flat_in, flat_out = sos.reshape(-1, 5), out.reshape(-1, 5 * block)
    for i in range(flat_in.shape[0]):
        ref_lib().eq_ref_tables(_dp(flat_in[i]), block, _dp(flat_out[i]))
    return out


def serial(sos, x):
    """x [n] through the cascade sos [S][5] by the plain fp64 recurrence, from silence"""
    y = np.ascontiguousarray(x, dtype=np.float64)
    for c in np.ascontiguousarray(sos, dtype=np.float64).reshape(-1, 5):
        out, st = np.empty_like(y), np.zeros(4)
        ref_lib().eq_ref_serial(_dp(c), y.size, _dp(y), _dp(st), _dp(out))
        y = out
    return y


def block_section(tab, k0, x, y, block=None):
    """x, y rows of block + 2 + n doubles (history in front); fills y[block + 2:] in place"""
    block = P if block is None else block
    n = x.size - (block + 2)
    assert x.flags.c_contiguous and y.flags.c_contiguous and y.size == x.size and tab.shape == (5, block)
    ref_lib().eq_ref_block(_dp(np.ascontiguousarray(tab)), block, k0, n, _dp(x), _dp(y))


def design(kind, rate, f0, q=math.sqrt(0.5), gain_db=0.0):
    """the header's formulas, line by line, in fp64"""
    f = np.float64
    w0 = f(2.0) * f(math.pi) * f(f0) / f(rate)
    cs, sn = f(math.cos(w0)), f(math.sin(w0))
    alpha = sn / (f(2.0) * f(q))
    A = f(math.pow(10.0, f(gain_db) / f(40.0)))
    g = f(2.0) * f(math.sqrt(A)) * alpha
    one, two = f(1.0), f(2.0)
    if kind == "lowpass":
        b1 = one - cs
        b0 = b2 = b1 / two
        a0, a1, a2 = one + alpha, -two * cs, one - alpha
    elif kind == "highpass":
        b1 = -(one + cs)
        b0 = b2 = (one + cs) / two
        a0, a1, a2 = one + alpha, -two * cs, one - alpha
    elif kind == "peak":
        b0, b1, b2 = one + alpha * A, -two * cs, one - alpha * A
        a0, a1, a2 = one + alpha / A, -two * cs, one - alpha / A
    elif kind == "lowshelf":
        b0, b1, b2 = A * ((A + one) - (A - one) * cs + g), two * A * ((A - one) - (A + one) * cs), A * ((A + one) - (A - one) * cs - g)
        a0, a1, a2 = (A + one) + (A - one) * cs + g, -two * ((A - one) + (A + one) * cs), (A + one) + (A - one) * cs - g
    elif kind == "highshelf":
        b0, b1, b2 = A * ((A + one) + (A - one) * cs + g), -two * A * ((A - one) + (A + one) * cs), A * ((A + one) + (A - one) * cs - g)
        a0, a1, a2 = (A + one) - (A - one) * cs + g, two * ((A - one) - (A + one) * cs), (A + one) - (A - one) * cs - g
    else:
        raise ValueError(kind)
    return np.array([b0 / a0, b1 / a0, b2 / a0, a1 / a0, a2 / a0], dtype=np.float64)


def response(sos, f, rate):
    """|H(e^{j 2 pi f / rate})| of one section b0 b1 b2 a1 a2"""
    z = np.exp(-2j * np.pi * f / rate)
    b0, b1, b2, a1, a2 = sos
    return abs((b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z))


class _Cascade:
    """one coefficient set on its grid: the tables, t_set and the last H samples of its S + 1 signals"""

    def __init__(self, tab, t_set, hist):
        self.tab, self.t_set, self.hist = tab, t_set, hist   # [C][S][5][P], int, [C][S + 1][H]

    def run(self, u, t, block):
        """u [C][n] float32 from sample t on -> signal S [C][n] float64; the histories move on"""
        Cn, S = self.tab.shape[:2]
        n = u.shape[1]
        k0 = (t - self.t_set) % block
        out = np.empty((Cn, n))
        for c in range(Cn):
            x = np.concatenate([self.hist[c, 0], u[c].astype(np.float64)])
            self.hist[c, 0] = x[n:]
            for s in range(S):
                y = np.concatenate([self.hist[c, s + 1], np.zeros(n)])
                block_section(self.tab[c, s], k0, x, y, block)
                self.hist[c, s + 1] = y[n:]
                x = y
            out[c] = x[block + 2:]
        return out


class Model:
    def __init__(self, n_channels, n_sections, xfade=0, block=None):
        self.C, self.S, self.R = n_channels, n_sections, xfade
        self.P = P if block is None else block
        self.reset()

    def reset(self):
        self.t = 0
        self.to = _Cascade(tables(identity(self.C, self.S), self.P), 0, np.zeros((self.C, self.S + 1, self.P + 2)))
        self.frm = None
        self.pending = None

    def fading(self):
        return self.frm is not None and self.t - self.to.t_set + 1 < self.R

    def fade_end(self):
        return self.to.t_set + self.R - 1 if self.fading() else self.t

    def set(self, sos=None, tables_=None):
        """takes effect at the next process(); replaces a set that no process() has taken up"""
        assert not self.fading()
        tab = tables(np.asarray(sos, dtype=np.float64).reshape(self.C, self.S, 5), self.P) if tables_ is None else tables_
        self.pending = np.array(tab, dtype=np.float64).reshape(self.C, self.S, 5, self.P)

    def process(self, input):
        """input [C][n] float32, the next step -> out [C][n] float32"""
        u = np.asarray(input, dtype=np.float32).reshape(self.C, -1)
        n = u.shape[1]
        if self.pending is not None:
            self.frm = self.to
            self.to = _Cascade(self.pending, self.t, self.frm.hist.copy())    # before t_set, To's signals are From's
            self.pending = None
        n_fade = min(n, self.to.t_set + self.R - 1 - self.t) if self.fading() else 0
        out = self.to.run(u, self.t, self.P).astype(np.float32)
        if n_fade:
            yf = self.frm.run(u[:, :n_fade], self.t, self.P).astype(np.float32)
            i = np.arange(n_fade, dtype=np.int64)
            w = ((self.t + i - self.to.t_set + 1).astype(np.float64) / np.float64(self.R)).astype(np.float32)
            yt = out[:, :n_fade]
            out[:, :n_fade] = yf + (w[None, :] * (yt - yf)).astype(np.float32)
        self.t += n
        return out
