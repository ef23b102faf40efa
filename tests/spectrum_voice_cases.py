"""What the CPU and GPU tiers of the spectrum voice pool share (tests/test_spectrum_voice_pool_cpu.py,
tests/test_gpu_spectrum_voice_pool.py).  TEST INFRASTRUCTURE ONLY.

* :func:`scalar_span` - the slot rule of include/vnd_spectrum_voice_stream.h restated on Python integers;
* :func:`layout` - where the parts of the state begin, from the header's text;
* :class:`Fold` - the host mirror of the documented order of the Welch sums: ``total`` and ``partial`` per bin;
* :func:`raw_call`, :func:`refusals` - the C entry with its arguments by name, and every refusal of the header.

Pure NumPy and ctypes: no device.
"""
from __future__ import annotations

import ctypes

import numpy as np

START, END = 1, 2
INVALID, UNSUPPORTED = 1, 4
MAX_POSITION = 1 << 60


def complete(q, W, H):
    return (q - W) // H + 1 if q >= W else 0


def scalar_span(pos, n, flags, W, H, M):
    """``(out_count, segments, new position)`` of one slot on Python integers; segments is -1 where the means are left alone."""
    p = 0 if flags & START else pos
    if n < 0 or n > M or p < 0 or p > MAX_POSITION:
        return -1, -1, pos
    w0, w1 = complete(p, W, H), complete(p + n, W, H)
    idle = n == 0 and not flags & (START | END)
    return w1 - w0, -1 if idle else w1, 0 if flags & END else p + n


def pad16(v):
    return (v + 15) // 16 * 16


def layout(S, C, W, H, nfft, M, itemsize, R):
    """The state of a pool, as the header lays it out: positions, sums, work, ring, each padded to 16 bytes."""
    F, Q = nfft // 2 + 1, 4 if C == 2 else 1
    rc = -(-M // H)
    G = -(-rc // R) + 1
    cap = W - 1 + M
    sums_at = pad16(8 * S)
    work_at = sums_at + S * F * Q * 16
    ring_at = work_at + pad16(S * G * F * Q * 8)
    need = ring_at + pad16(S * cap * C * itemsize)
    return dict(F=F, Q=Q, rc=rc, G=G, cap=cap, sums_at=sums_at, work_at=work_at, ring_at=ring_at, need=need)


class Fold:
    """The documented order: ``partial`` from +0.0 in ascending t within a run of ``run`` segments, folded into ``total``
    (from +0.0, ascending runs) when the run's last segment has been added; the sum is total + partial inside a run."""

    def __init__(self, run, shape, total=None, partial=None, count=0):
        self.run, self.count = run, count
        self.total = np.zeros(shape, np.float64) if total is None else np.array(total, np.float64)
        self.partial = np.zeros(shape, np.float64) if partial is None else np.array(partial, np.float64)

    def push(self, value):
        """One segment's per-bin values (of the sample type)."""
        if self.count % self.run == 0:
            self.partial = np.zeros_like(self.partial)
        if self.count < self.run:
            self.total = np.zeros_like(self.total)           # logically zero: never read before a run completes
        self.partial = self.partial + np.asarray(value, np.float64)
        self.count += 1
        if self.count % self.run == 0:
            self.total = self.total + self.partial

    def mean(self, dtype):
        if self.count == 0:
            return np.zeros(self.total.shape, dtype)
        s = self.total + self.partial if self.count % self.run else self.total
        return (s / float(self.count)).astype(dtype)


ARGS = ('ctx', 'state', 'state_bytes', 'M', 'x', 'ss', 'fs', 'C', 'counts', 'flags', 'win', 'tw', 'W', 'H', 'nfft', 'detrend',
        'scale', 'cols', 'oc', 'pxx', 'pyy', 'pxy', 'segments', 'S', 'stream')
POINTERS = {'ctx', 'state', 'x', 'counts', 'flags', 'win', 'tw', 'cols', 'oc', 'pxx', 'pyy', 'pxy', 'segments', 'stream'}


def raw_call(lib, float64, a):
    """The C entry on a dict of its arguments by the names of ARGS; returns the status."""
    fn = lib.vnd_spectrum_voice_stream_f64_dev if float64 else lib.vnd_spectrum_voice_stream_f32_dev
    def pointer(v):
        return v if isinstance(v, ctypes.c_void_p) else ctypes.c_void_p(v)      # (a context's handle is one already)
    return fn(*[pointer(a[k]) if k in POINTERS else a[k] for k in ARGS])


def refusals(a, itemsize):
    """``[(changes, status), ...]``: every refusal of the header from a good call's arguments `a` (ctx aside)."""
    big = dict(state_bytes=2 ** 60)
    invalid = [dict(state=0), dict(x=0), dict(counts=0), dict(flags=0), dict(win=0), dict(tw=0), dict(oc=0),
               dict(S=0), dict(S=-1), dict(M=0), dict(M=2 ** 31), dict(ss=0), dict(fs=0), dict(C=0), dict(C=3), dict(C=2, fs=1),
               dict(W=1), dict(H=0), dict(H=-3), dict(scale=float('nan')), dict(scale=0.0), dict(scale=-1.0),
               dict(scale=float('inf')), dict(scale=-0.0 if itemsize == 8 else 1e-60),  # (float32: rounds to 0)
               dict(pxx=0), dict(segments=0), dict(pyy=0) if a['C'] == 2 else dict(pxx=0, pyy=0), dict(pxy=0) if a['C'] == 2
               else dict(segments=0, pxy=0),
               dict(state_bytes=a['state_bytes'] - 1), dict(state=a['state'] + 8), dict(ss=2 ** 62),
               dict(cols=a['x']), dict(cols=a['state']), dict(x=a['state']), dict(pxx=a['win']), dict(oc=a['counts']),
               dict(segments=a['flags']), dict(pxx=a['state'] + 16), dict(cols=a['pxx']), dict(oc=a['segments']),
               dict(tw=a['state'])]
    unsupported = [dict(nfft=100), dict(nfft=32), dict(nfft=8192, **big), dict(W=a['nfft'] + 1), dict(H=a['W'] + 1),
                   dict(S=65536, **big),
                   dict(M=2 ** 22, H=1, **big),                              # RC 2^22: above 65535 runs per slot
                   dict(M=2 ** 20, H=1, S=300, **big),                       # 32769 runs x 300 slots > 2^23 workgroups
                   # float32: R = 32, G = 4096, 2^23 workgroups exactly, and 2048 x 131040 x 2 x 2049 values > 2^40 (the one
                   # shape family that meets this limit below the workgroup limit); float64: R = 19, the workgroups
                   dict(M=131040 * 64, H=64, W=4096, nfft=4096, S=2048, C=2, fs=2, **big)]
    # INVALID is reported before UNSUPPORTED
    invalid += [dict(nfft=100, x=0), dict(S=65536, fs=0), dict(nfft=100, scale=0.0)]
    return [(kw, INVALID) for kw in invalid] + [(kw, UNSUPPORTED) for kw in unsupported]
