"""The reference of the filter bank's tests: tests/cpp/scene_fir_bank_ref.c (the stated chain of fmaf in about 15 lines of C)
compiled with the host compiler into a temporary directory.  taps_from_bank turns a bank set into the taps it stands for; they
then go to the existing models, or to a second engine, as any caller's taps would."""
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
        _tmp = tempfile.TemporaryDirectory(prefix="scene_fir_bank_ref_")
        so = os.path.join(_tmp.name, "libscene_fir_bank_ref.so")
        subprocess.run([os.environ.get("CC", "cc"), "-O2", "-ffp-contract=off", "-march=native", "-shared", "-fPIC",
                        os.path.join(_HERE, "cpp", "scene_fir_bank_ref.c"), "-o", so, "-lm"], check=True)
        _lib = C.CDLL(so)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        _lib.scene_fir_bank_ref.argtypes = [fp, C.c_int, C.c_int, C.c_int, C.c_int, ip, fp, fp]
        _lib.scene_fir_bank_ref.restype = None
    return _lib


def taps_from_bank(bank, index, weight):
    """bank [F][C][K], index / weight [N][J] -> taps [C][N][K] float32"""
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    bank = np.ascontiguousarray(bank, dtype=np.float32)
    index = np.ascontiguousarray(index, dtype=np.int32)
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    F, n_ch, K = bank.shape
    N, J = index.shape
    assert weight.shape == (N, J) and index.min() >= 0 and index.max() < F
    taps = np.empty((n_ch, N, K), dtype=np.float32)
    ref_lib().scene_fir_bank_ref(bank.ctypes.data_as(fp), n_ch, K, N, J, index.ctypes.data_as(ip), weight.ctypes.data_as(fp),
                                 taps.ctypes.data_as(fp))
    return taps
