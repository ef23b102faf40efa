"""The shapes, inputs and float64 references the CPU and GPU tiers of the short-time spectra share
(tests/test_spectrum_cpu.py, tests/test_gpu_spectrum.py).  TEST INFRASTRUCTURE ONLY.

* :data:`GRID` - every (nfft, nperseg) of the device grid: the first six and :data:`NEW_SHAPES`, which add the transform
  sizes 512, 1024 and 2048 and an odd ``nperseg`` at every pass width;
* :func:`spectrum_run` - the run length, transcribed from the rule in DESIGN.md 3.23 (bytes that fit 156 KiB of LDS);
* :func:`noise`, :func:`inputs`, :func:`parity_case`, :func:`coherent_pair` - the inputs of the parity tests;
* :func:`columns64`, :func:`detrend_budget`, :func:`contract_model` - the float64 column of a segment from a given mean, the
  half-ulp budget of the detrend contract, and a model of the contract itself;
* :func:`replay_mean` - the Welch sum in the documented order, on the host.

Pure NumPy (SciPy for a named window): no device, no native library.
"""
from __future__ import annotations

import functools

import numpy as np

OLD_GRID = [(64, 64), (64, 2), (128, 128), (256, 256), (256, 200), (4096, 4096)]
# 512: pure radix 4, 8 slots a pass, 32 threads a segment in the detrend tree; 1024: a radix-2 stage, 4 slots, one wave a
# segment; 2048: pure radix 4 up to Ns = 256, 2 slots, a tree across two waves; and an odd nperseg at 64, 8, 4, 2, 1 slots
NEW_SHAPES = [(512, 512), (512, 401), (1024, 1024), (1024, 513), (2048, 2048), (2048, 1999), (64, 63), (128, 99), (4096, 4095)]
GRID = OLD_GRID + NEW_SHAPES
IDS = ['%d-%d' % p for p in GRID]
NEW_IDS = ['%d-%d' % p for p in NEW_SHAPES]

# (nfft, nperseg, hop) of the Welch replay; the last four are the shortest runs of a float64 stereo pool: 8, 4, 2, 1
WELCH_SHAPES = [(256, 256, 128), (64, 64, 64), (4096, 4096, 2048), (256, 200, 25),
                (512, 401, 351), (1024, 1024, 896), (2048, 2048, 1792), (4096, 4095, 2048)]
SHORTEST_RUNS = {(512, 401, 351): 8, (1024, 1024, 896): 4, (2048, 2048, 1792): 2, (4096, 4095, 2048): 1,
                 (512, 512, 448): 8, (512, 512, 512): 8, (1024, 1024, 1024): 4, (2048, 2048, 2048): 2}
# (nfft, nperseg) of the Welch parity with SciPy: hop nperseg // 2, 25 segments
WELCH_PARITY = [(128, 128), (512, 512), (1024, 1024), (2048, 2048), (4096, 4096), (1024, 513)]
# (nfft, nperseg, hop) whose staged frames of a channel, (R - 1) * hop + nperseg, are odd for every R: an even hop
ODD_ROOM = [(64, 63, 32), (1024, 513, 256), (4096, 4095, 2048)]

LDS_ELEMENTS = 156 * 1024        # bytes of a workgroup's dynamic LDS
POINTS = 2048 + 5 * (2048 >> 5)  # the padded points of a pass: 2368
MAX_RUN = 32


def hops(nperseg):
    return sorted({1, nperseg - nperseg // 8, nperseg})


def spectrum_run(nfft, nperseg, hop, sample_bytes, cross_channels):
    """The longest run, up to 32 segments, whose elements fit the LDS beside the points: the staged frames of each channel
    and, for the spectrogram (``cross_channels`` 0), the [bin][run | 1] tile; for the cross spectra the points twice (the
    left spectra of a pass).  A whole number of passes when it is more than one pass."""
    budget = LDS_ELEMENTS // sample_bytes
    bins, slots = nfft // 2 + 1, 2048 // (nfft // 2)
    run = 1
    for r in range(2, MAX_RUN + 1):
        room = (r - 1) * hop + nperseg
        need = 4 * POINTS + 2 * room if cross_channels else 2 * POINTS + room + bins * (r | 1)
        if need > budget:
            break
        run = r
    return run - run % slots if run > slots else run


def noise(shape, seed, dtype=np.float32):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(dtype)


def inputs(shape, seed):
    """Uniform noise, and 0.9 + 1e-3 x noise, which puts the detrend's rounding of the mean far above the transform's."""
    return (('noise', noise(shape, seed)),
            ('offset', (np.float32(0.9) + np.float32(1e-3) * noise(shape, seed + 1)).astype(np.float32)))


def parity_case(nfft, nperseg):
    """``(hop, n, seed)`` of the spectrogram parity test: nine columns an eighth overlapped."""
    hop = nperseg - nperseg // 8
    return hop, nperseg + 8 * hop, 7 * nfft + nperseg


def scipy_columns(x, nfft, nperseg, hop, **kw):
    """``(ref, own)`` of a (B, n, C) float32 pool, both (B, C, F, T): SciPy's spectrogram of the float64 copy, and SciPy's own
    float32 call - one 1-D call a signal and channel, as a user would make it."""
    from scipy.signal import spectrogram
    kw = dict(dict(nperseg=nperseg, noverlap=nperseg - hop, nfft=nfft, fs=48000.0), **kw)
    both = [np.stack([[spectrogram(x[b, :, c].astype(dt), **kw)[2] for c in range(x.shape[2])] for b in range(x.shape[0])])
            for dt in (np.float64, np.float32)]
    assert both[0].dtype == np.float64 and both[1].dtype == np.float32
    return both


@functools.lru_cache(maxsize=None)
def parity_reference(nfft, nperseg):
    """``((name, x, ref, own), ...)`` of the parity test's two inputs at SciPy's defaults, computed once and read-only."""
    hop, n, seed = parity_case(nfft, nperseg)
    out = []
    for name, x in inputs((2, n, 2), seed):
        ref, own = scipy_columns(x, nfft, nperseg, hop)
        for a in (x, ref, own):
            a.setflags(write=False)
        out.append((name, x, ref, own))
    return tuple(out)


def coherent_pair(n, seed, batch=1):
    """A (batch, n, 2) float32 pool with L = a, R = 0.6 a + 0.8 b: coherence 0.36 in expectation, so a mean cross spectrum
    that does not cancel."""
    a, b = noise((batch, n), seed), noise((batch, n), seed + 1)
    return np.stack([a, np.float32(0.6) * a + np.float32(0.8) * b], axis=2)


def asymmetric_windows(nperseg):
    """Two windows no reversal leaves alone: an exponential decay, and the default tukey times a ramp."""
    from scipy.signal import get_window
    i = np.arange(nperseg, dtype=np.float64)
    return (('decay', np.exp(-3.0 * i / nperseg)),
            ('tukey-ramp', get_window(('tukey', 0.25), nperseg) * (0.25 + 0.75 * i / nperseg)))


def column_errors(got, ref):
    """The relative L2 distance of every column ([..., F, T]) from the float64 reference."""
    d = np.linalg.norm(np.asarray(got, np.float64) - ref, axis=-2)
    return d / np.linalg.norm(ref, axis=-2)


def segments_of(x, nperseg, hop):
    """(..., T, nperseg) of a (..., n) signal."""
    return np.lib.stride_tricks.sliding_window_view(x, nperseg, axis=-1)[..., ::hop, :]


def columns64(d, win64, nfft, scale):
    """The 'psd' columns (..., F, T) of already detrended and not yet windowed float64 segments d (..., T, nperseg)."""
    p = np.abs(np.fft.rfft(d * win64, nfft, axis=-1)) ** 2 * scale
    p[..., 1:nfft // 2] *= 2.0
    return np.swapaxes(p, -1, -2)


def density_scale(win64, fs=1.0):
    return 1.0 / (fs * np.sum(win64 * win64))


def detrend_budget(x32, nfft, nperseg, hop, win64, fs=1.0):
    """``(ref, budget)`` of a (..., n) float32 signal under 'constant' detrend: the float64 columns from the float64 mean m
    of every segment, and per column the larger relative L2 change when the mean is m + ulp/2 or m - ulp/2 of float32 at m,
    plus the noise cap 8 log2(nfft) 2^-24.  A mean that is the float64 sum divided and rounded once to float32 is within
    that half ulp."""
    seg = segments_of(x32.astype(np.float64), nperseg, hop)
    m = seg.mean(axis=-1, keepdims=True)
    half = np.spacing(m.astype(np.float32)).astype(np.float64) / 2
    scale = density_scale(win64, fs)
    ref = columns64(seg - m, win64, nfft, scale)
    norm = np.linalg.norm(ref, axis=-2)
    change = [np.linalg.norm(columns64(seg - (m + s * half), win64, nfft, scale) - ref, axis=-2) / norm for s in (1.0, -1.0)]
    return ref, np.maximum(*change) + 8 * np.log2(nfft) * 2.0 ** -24


def contract_model(x32, nfft, nperseg, hop, win64, fs=1.0, mean='contract'):
    """The columns of a model of the device's contract: the mean a float64 sum divided and rounded once to float32
    (``mean='running'``: a float32 running sum, the mean a careless kernel forms), float32 subtract and multiply by the
    float32 window, then an exact transform."""
    seg = segments_of(x32, nperseg, hop)
    if mean == 'contract':
        m = (seg.astype(np.float64).sum(axis=-1, keepdims=True) / nperseg).astype(np.float32)
    else:
        m = (np.cumsum(seg, axis=-1, dtype=np.float32)[..., -1:] / np.float32(nperseg)).astype(np.float32)
    d = ((seg - m) * win64.astype(np.float32)).astype(np.float32)
    return columns64(d.astype(np.float64), np.ones(nperseg), nfft, density_scale(win64, fs))


def replay_mean(cols, run, dtype):
    """The Welch mean of the columns (..., F, T) in the documented order: each run of ``run`` columns added in float64 from
    0.0 in ascending t, the run sums added in ascending order from 0.0, divided by the column count, rounded once."""
    cols = np.asarray(cols, np.float64)
    count = cols.shape[-1]
    total = np.zeros(cols.shape[:-1], np.float64)
    for t0 in range(0, count, run):
        part = np.zeros(cols.shape[:-1], np.float64)
        for t in range(t0, min(t0 + run, count)):
            part = part + cols[..., t]
        total = total + part
    return (total / float(count)).astype(dtype)
