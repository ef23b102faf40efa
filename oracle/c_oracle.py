"""ctypes loader for ``oracle/libvnd_oracle.so`` (C restatement).  TEST
INFRASTRUCTURE ONLY - see ``oracle/vnd_oracle.c``.  Build with ``make -C oracle``.
"""
from __future__ import annotations

import ctypes
import pathlib
import subprocess

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
_LIB = None


def build() -> pathlib.Path:
    subprocess.run(['make', '-s', '-C', str(_HERE)], check=True)
    return _HERE / 'libvnd_oracle.so'


def lib():
    global _LIB
    if _LIB is None:
        path = _HERE / 'libvnd_oracle.so'
        if not path.exists():
            build()
        _LIB = ctypes.CDLL(str(path))
        _LIB.vnd_oracle_convolve_f32.restype = ctypes.c_int
        _LIB.vnd_oracle_convolve_fma_f32.restype = ctypes.c_int
    return _LIB


def _p(a, ct):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ct))


def convolve(x, tap_off, idx, w, *, seg_off=None, seg_end=None, seg_gain=None,
             chan_flags=None, apply_gain=False, threads=1) -> np.ndarray:
    """x: (n, C) or (batch, n, C) float32.  Tables as in include/vnd_amd.h."""
    return _convolve('vnd_oracle_convolve_f32', x, tap_off, idx, w, seg_off, seg_end, seg_gain,
                     chan_flags, apply_gain, threads)


def convolve_fma(x, tap_off, idx, w, *, seg_off=None, seg_end=None, seg_gain=None,
                 chan_flags=None, apply_gain=False, threads=1) -> np.ndarray:
    """``convolve`` in VND_MODE_FMA arithmetic (``acc = fmaf(x, w, acc)``): the fast form of
    ``vnd_oracle.convolve_taps_fma``, which the CPU tier holds it to bit for bit."""
    return _convolve('vnd_oracle_convolve_fma_f32', x, tap_off, idx, w, seg_off, seg_end, seg_gain,
                     chan_flags, apply_gain, threads)


def _convolve(entry, x, tap_off, idx, w, seg_off, seg_end, seg_gain, chan_flags, apply_gain,
              threads) -> np.ndarray:
    x = np.ascontiguousarray(x, np.float32)
    shape = x.shape
    xb = x.reshape((1,) + shape) if x.ndim == 2 else x
    batch, n, channels = xb.shape
    y = np.zeros_like(xb)
    tap_off = np.ascontiguousarray(tap_off, np.int32)
    idx = np.ascontiguousarray(idx, np.int32)
    w = np.ascontiguousarray(w, np.float32)
    if seg_off is not None:
        seg_off = np.ascontiguousarray(seg_off, np.int32)
        seg_end = np.ascontiguousarray(seg_end, np.int32)
        seg_gain = np.ascontiguousarray(seg_gain, np.float32)
    if chan_flags is not None:
        chan_flags = np.ascontiguousarray(chan_flags, np.uint8)
    rc = getattr(lib(), entry)(
        _p(xb, ctypes.c_float), _p(y, ctypes.c_float), ctypes.c_int64(batch),
        ctypes.c_int64(n), ctypes.c_int32(channels), _p(tap_off, ctypes.c_int32),
        _p(idx, ctypes.c_int32), _p(w, ctypes.c_float), _p(seg_off, ctypes.c_int32),
        _p(seg_end, ctypes.c_int32), _p(seg_gain, ctypes.c_float),
        _p(chan_flags, ctypes.c_uint8), ctypes.c_int(bool(apply_gain)), ctypes.c_int(threads))
    if rc:
        raise RuntimeError(f'{entry} failed rc={rc}')
    return y.reshape(shape)
