"""Drop-in host layer for the velvet-noise path of ckonst/VNDecorrelate.

Same public names, keyword arguments, defaults and exceptions as the
reference's ``vndecorrelate.decorrelation`` (v1.1.0; ``file:line`` citations
are relative to its checkout), but every tap sum runs on an MI355X through the
C ABI in ``include/vnd_amd.h``:

===========================  ==================================================
reference                    here
===========================  ==================================================
``convolve_velvet_noise``    :func:`convolve_velvet_noise`  -> ``vnd_convolve_f32_host``
``generate_velvet_noise``    :func:`generate_velvet_noise`  (host NumPy, O(K))
``VelvetNoise``              :class:`VelvetNoise` (``convolve`` on the GPU)
``SignalChain``              :class:`SignalChain`
``HaasEffect``               :class:`HaasEffect` (device kernel ``vnd_haas_f64_*`` in a
                             device-resident chain, NumPy otherwise)
``WhiteNoise``               :class:`WhiteNoise` (dense float64 FIR + width + normaliser on the
                             GPU through ``vnd_white_noise_f32_dev`` where covered, see
                             ``set_white_noise_device``; NumPy otherwise)
===========================  ==================================================

There is no CPU implementation of the tap sum in this package: without the
built extension or without a gfx950 device the calls raise ``RuntimeError``.

Operand types (DESIGN.md "Parity"): in the exact mode every dtype combination of
the function path is bit-identical to the reference - float32 and the integer
types NumPy promotes to float32 through the float32 kernels, float64 / int32 /
int64 signals and float64 filters through ``vnd_convolve_promote_host``, which
rounds to float32 at every tap as ``out += x * value`` does.  In the tolerance
modes those operands are rounded to float32 first.

Threading: the functions are re-entrant like the reference's; calls that share a
context are serialised inside the library (one stream and one set of staging
buffers per context).
"""
from __future__ import annotations

import hashlib
import threading
from abc import ABC, abstractmethod
from collections import OrderedDict
from dataclasses import dataclass, field
from functools import partial
from typing import Any, Callable, Iterator, List, Optional, Protocol, Sequence

import numpy as np
from numpy.typing import NDArray

from . import _native, analysis
from .taps import TapArrays, class_path_arrays, class_path_bank_arrays, concat_tap_arrays, function_path_arrays
from .utils.dsp import (
    IDENTITY_ENVELOPE,
    LayoutMode,
    LR_to_MS,
    MS_to_LR,
    apply_log_distribution,
    apply_stereo_width,
    check_equal_length,
    encode_signal_to_side_channel,
    generate_log_distribution,
    mono_to_stereo,
    rms_normalize,
    to_float32,
)

DEFAULT_SEGMENT_ENVELOPE = (0.85, 0.55, 0.35, 0.2)

# Arithmetic used by the host API.  EXACT reproduces the reference bit for bit
# for float32 inputs; FMA is the single-rounding variant (<= 1e-6 of peak).
MODE_EXACT = _native.MODE_EXACT
MODE_FMA = _native.MODE_FMA
MODE_FAST = _native.MODE_FAST
_default_mode = MODE_EXACT


_device_epilogue: Optional[bool] = None


def set_device_epilogue(enabled: Optional[bool]) -> None:
    """Where ``VelvetNoise.decorrelate``'s epilogue (side-channel encode, width, RMS
    normalise) runs.

    ``None`` (default): on the GPU behind the convolution, with the normaliser's sums of
    squares in NumPy's own order (a sequential float32 recurrence for ``(n, C >= 2)`` arrays,
    reproduced bit for bit).  In MODE_EXACT the whole stage is then bit-identical to the
    reference; in the other modes it differs from it only through the convolution
    (~1e-6 of peak).  A single-channel table's sums are NumPy's pairwise ones (8192-sample
    chunks, 128-sample leaves), reproduced the same way; custom normalisers keep the host epilogue.
    ``True``: on the GPU in its fastest form - in MODE_FAST everything fused into the fast
    kernel with float64 sums of float32 partials (include/vnd_amd.h), which puts the normalised output ~1e-4
    relative from the reference's on long signals (NumPy's sequential sum is that far off).
    ``False``: in NumPy on the host, behind the device convolution."""
    global _device_epilogue
    _device_epilogue = None if enabled is None else bool(enabled)


def _use_device_epilogue(num_outs: int, has_normalizer: bool, frames: int = 0, c_contiguous: bool = True) -> bool:
    """The default policy: the device epilogue wherever it repeats what NumPy would do."""
    if _device_epilogue is not None:
        return _device_epilogue
    if not has_normalizer:
        return True                                       # the pointwise steps are always NumPy's
    # NumPy's row-by-row float32 sums are repeated on the device for 2 to 32 channels of a C-contiguous
    # signal, and so are the pairwise sums it forms for a single channel (other memory layouts: host)
    return 1 <= num_outs <= 32 and c_contiguous


def _normalize_flag(has_normalizer: bool) -> int:
    if not has_normalizer:
        return _native.NORMALIZE_OFF
    return _native.NORMALIZE_RMS if _device_epilogue else _native.NORMALIZE_RMS_REFERENCE_ORDER


_white_noise_device: Optional[bool] = None


def set_white_noise_device(enabled: Optional[bool]) -> None:
    """Where ``WhiteNoise.decorrelate`` (and ``decorrelate_batched``) runs.

    ``None`` (default): on the GPU (``vnd_white_noise_f32_dev``: one float64 FMA chain per output, rounded once, then the
    width and NumPy-order normaliser of the velvet-noise stage) when a gfx950 device is present and the call is covered
    (``white_noise_covers``); otherwise the NumPy code.  Per output the device result is within one float32 ulp plus
    2^-40 * sum |h x| of NumPy's (whose float64 summation order is the host BLAS's); where the convolution's float32
    outputs agree, the stage is bit-identical.
    ``True``: the device for every covered call; ``RuntimeError`` when there is no device.
    ``False``: always NumPy, bit-identical to the reference."""
    global _white_noise_device
    if enabled is not None and not isinstance(enabled, (bool, np.bool_)):
        raise TypeError(f'set_white_noise_device takes True, False or None, not {enabled!r}')
    _white_noise_device = None if enabled is None else bool(enabled)


def white_noise_covers(shape: Sequence[int], num_outs: int, width, fir, c_contiguous: bool = True) -> bool:
    """Whether ``WhiteNoise.decorrelate`` of a float32 signal of ``shape`` has a device form: a finite float64 2-D
    filter with at least ``num_outs`` columns and 1 <= M <= n taps; a ``(n, num_outs)`` C-contiguous signal (NumPy's
    sums of squares follow the memory layout), or a ``(n,)`` one with ``num_outs == 2``; width only on two channels;
    at most 32 channels (the device repeats NumPy's sum order up to there).  Everything else keeps the NumPy code and
    its exceptions."""
    if not isinstance(fir, np.ndarray) or fir.dtype != np.float64 or fir.ndim != 2:
        return False
    if not 1 <= num_outs <= 32 or fir.shape[1] < num_outs:
        return False
    if len(shape) == 1:
        if num_outs != 2:
            return False
    elif len(shape) != 2 or shape[1] != num_outs or not c_contiguous:
        return False
    if width is not None and num_outs != 2:
        return False
    m = fir.shape[0]
    if not 1 <= m <= shape[0] or m > 2 ** 31 - 1:
        return False
    return bool(np.isfinite(fir[:, :num_outs]).all())


def set_default_mode(mode: int) -> None:
    """Choose the arithmetic of subsequent host-API calls (MODE_EXACT / MODE_FMA)."""
    global _default_mode
    if mode not in (MODE_EXACT, MODE_FMA, MODE_FAST):
        raise ValueError(f'unknown mode {mode}')
    _default_mode = mode


# ----------------------------------------------------------------------------
# Protocols / abstract bases   (decorrelation.py:31-59)
# ----------------------------------------------------------------------------
class SignalProcessor(Protocol):
    sample_rate_hz: int
    num_outs: int

    def __call__(self, input_signal: NDArray) -> NDArray: ...


class StatelessDecorrelator(Protocol):
    def __call__(self, input_signal: NDArray, **kwargs) -> NDArray: ...


@dataclass(kw_only=True)
class Decorrelator(ABC):
    """Base of the stateful stages: ``stage(x)`` is ``stage.decorrelate(x)``."""

    sample_rate_hz: int
    num_outs: int = 2
    width: Optional[float] = None

    @abstractmethod
    def decorrelate(self, input_signal: NDArray) -> NDArray:
        raise NotImplementedError

    def __call__(self, input_signal: NDArray) -> NDArray:
        return self.decorrelate(input_signal)


# ----------------------------------------------------------------------------
# tap placement shared by both generators   (decorrelation.py:488-523, :573-611)
# ----------------------------------------------------------------------------
def _draw_taps(seed, num_impulses: int, num_filters: int, fir_length: int, sample_rate_hz,
               duration_seconds: float, strength: float):
    """Positions ``int32 (K+1, F)`` and signs ``(K, F)`` in {-1, +1}.

    The order of the two uniform draws (signs, then offsets) and their shapes
    are part of the contract: they fix which PCG64 values land where.
    """
    rng = np.random.default_rng(seed)
    weights = generate_log_distribution(strength, num_impulses)
    marks = np.cumsum(weights)
    if strength == 0.0:
        marks -= 1.0                      # uniform case starts at sample 0
    marks *= fir_length / marks[-1]
    sign_draw = rng.uniform(low=0, high=1, size=(num_impulses, num_filters))
    offset_draw = rng.uniform(low=0, high=1, size=(num_impulses + 1, num_filters))
    signs = (2 * np.round(sign_draw)) - 1
    mean_gap = sample_rate_hz / (num_impulses / duration_seconds)
    positions = np.stack([apply_log_distribution(offset_draw[:, f], weights, marks, mean_gap)
                          for f in range(num_filters)], axis=1)
    return positions, signs


def _segment_index(k: int, num_impulses: int, num_segments: int) -> int:
    return int(k / (num_impulses / num_segments))


def generate_velvet_noise(*, duration_seconds: float, num_impulses: int, num_outs: int = 2,
                          sample_rate_hz: int = 44100,
                          segment_envelope: Sequence[float] = DEFAULT_SEGMENT_ENVELOPE,
                          log_distribution_strength: float = 1.0,
                          seed: Optional[int] = None) -> NDArray:
    """Dense seeded velvet-noise FIR, float32 ``(int(duration*fs), num_outs)``.

    Mirrors ``generate_velvet_noise`` (decorrelation.py:549-627): the length
    truncates, a later impulse on an occupied sample overwrites the earlier one.
    Feed the result to :func:`convolve_velvet_noise`.
    """
    fir_length = int(duration_seconds * sample_rate_hz)
    envelope = tuple(segment_envelope) if len(segment_envelope) else IDENTITY_ENVELOPE
    fir = np.zeros((fir_length, num_outs), dtype=np.float32)
    positions, signs = _draw_taps(seed, num_impulses, num_outs, fir_length, sample_rate_hz,
                                  duration_seconds, log_distribution_strength)
    for c in range(num_outs):
        for k in range(num_impulses):
            fir[positions[k, c], c] = signs[k, c] * envelope[_segment_index(k, num_impulses, len(envelope))]
    return fir


# ----------------------------------------------------------------------------
# device tap-table cache for the stateless path
# ----------------------------------------------------------------------------
class _TableCache:
    """Small LRU of device tables keyed by FIR content, so calling the stateless
    function repeatedly with one FIR uploads its 8*K*C bytes once."""

    def __init__(self, capacity: int = 16):
        self.capacity = capacity
        self._items: 'OrderedDict[tuple, _native.TapTable]' = OrderedDict()
        self._lock = threading.Lock()

    def get(self, key, build: Callable[[], TapArrays]) -> _native.TapTable:
        with self._lock:
            table = self._items.get(key)
            if table is not None:
                self._items.move_to_end(key)
                return table
        arrays = build()
        table = _native.TapTable.create(_native.default_context(), arrays.tap_offsets,
                                        arrays.tap_index, arrays.tap_weight, **arrays.kwargs())
        with self._lock:
            table = self._items.setdefault(key, table)      # another thread may have built it meanwhile
            self._items.move_to_end(key)
            # An evicted table is only dropped, never closed here: a thread still inside a call
            # holds a reference, and the device memory goes when the last one does (TapTable.__del__).
            while len(self._items) > self.capacity:
                self._items.popitem(last=False)
        return table

    def clear(self):
        with self._lock:
            self._items.clear()


_fir_tables = _TableCache()


try:                                   # a 128-bit content hash of the filter per call: xxh3 takes 0.7 us for a 30 ms stereo
    from xxhash import xxh3_128_digest as _digest16          # filter where blake2b takes 16 (of a 190 us call)
except ImportError:                    # pragma: no cover - the hash is an optional dependency
    def _digest16(view):
        return hashlib.blake2b(view.tobytes(), digest_size=16).digest()


def _fir_key(fir: np.ndarray, channels: int):
    view = np.ascontiguousarray(fir[:, :channels])
    return (view.shape, str(view.dtype), _digest16(view), _native.default_context().device)


class _ArraysCache:
    """Function-path tap arrays (and their transport image) of the filters last spread over a device list: the several-device
    call otherwise rebuilds them - a scan of the dense FIR and a serialisation - on every call.  Keyed by the filter's content."""

    def __init__(self, capacity: int = 32):
        self.capacity, self._lock, self._items = capacity, threading.Lock(), OrderedDict()

    def get(self, fir: np.ndarray, channels: int):
        view = np.ascontiguousarray(fir[:, :channels])
        key = (view.shape, str(view.dtype), _digest16(view))
        with self._lock:
            found = self._items.get(key)
            if found is not None:
                self._items.move_to_end(key)
                return found
        arrays = function_path_arrays(fir, channels)
        image = arrays.to_bytes()
        arrays.to_bytes = lambda: image                      # (immutable from here on: the pool keys its device copies by the image)
        with self._lock:
            self._items[key] = arrays
            while len(self._items) > self.capacity:
                self._items.popitem(last=False)
        return arrays


_fir_arrays = _ArraysCache()


def _promoted_convolve(x: NDArray, fir: NDArray, num_channels: int, mode: int) -> Optional[NDArray]:
    """The operand types NumPy multiplies in float64 (a float64 or int32/int64 signal, or any
    signal with a float64 filter such as ``VelvetNoise.FIR``): in the exact mode they take the
    promoting kernel, which rounds to float32 at every tap exactly as ``out += x * value`` does
    (decorrelation.py:656-658).  None when the float32 kernels apply."""
    if mode != MODE_EXACT or np.result_type(x.dtype, fir.dtype) != np.float64 or x.size == 0:
        return None
    offsets = np.zeros(num_channels + 1, np.int32)
    idx, weights = [], []
    for c in range(num_channels):
        nz = np.flatnonzero(fir[:, c] != 0.0)
        idx.append(nz.astype(np.int32))
        weights.append(fir[nz, c].astype(np.float64))
        offsets[c + 1] = offsets[c] + len(nz)
    xin = x if x.dtype in (np.float32, np.float64) else x.astype(np.float64)
    return _native.convolve_promote_host(_native.default_context(), np.ascontiguousarray(xin), offsets,
                                         np.concatenate(idx), np.concatenate(weights))


def convolve_velvet_noise(input_signal: NDArray, velvet_noise_filters: NDArray, *,
                          mode: Optional[int] = None) -> NDArray:
    """Stateless sparse convolution ``y[n,c] = sum_k w[c,k] * x[n + i[c,k], c]``.

    Drop-in for ``convolve_velvet_noise`` (decorrelation.py:630-660): same
    shapes in and out (float32 ``(n, C)`` result), ``ValueError`` when a
    multi-channel signal and the filters disagree on channel count, and the
    reference's ``IndexError`` for a 1-D signal.  ``mode`` picks the arithmetic
    (default: the bit-exact one).  Runs on the GPU; raises ``RuntimeError``
    without one.
    """
    fir = np.asarray(velvet_noise_filters)
    if fir.ndim == 1:
        fir = fir[:, None]
    if input_signal.ndim == 1:
        # The reference indexes the 1-D signal with two subscripts at its first tap.
        if np.any(fir[:, 0] != 0.0):
            raise IndexError('too many indices for array: array is 1-dimensional, but 2 were indexed')
        return np.zeros(input_signal.shape, dtype=np.float32)
    num_channels = input_signal.shape[1]
    if num_channels > 1:
        check_equal_length(input_signal, fir, dim=1)
    mode = _default_mode if mode is None else mode
    if num_channels:
        promoted = _promoted_convolve(np.asarray(input_signal), fir, num_channels, mode)
        if promoted is not None:
            return promoted
    x = np.ascontiguousarray(input_signal, dtype=np.float32)
    if x.shape[0] == 0 or num_channels == 0:
        return np.zeros(x.shape, dtype=np.float32)
    table = _fir_tables.get(_fir_key(fir, num_channels),
                            lambda: function_path_arrays(fir, num_channels))
    return table.convolve_host(x, mode)


def convolve_velvet_noise_batched(input_signals: NDArray, velvet_noise_filters: NDArray, *,
                                  mode: Optional[int] = None, devices=None) -> NDArray:
    """Many independent streams with one shared filter bank: ``(B, n, C)`` in and
    out, one kernel launch.  Equals stacking :func:`convolve_velvet_noise` over B.

    ``devices``: ``None`` - the process's default device; ``'all'`` or a list of device indices - the
    batch is cut into contiguous blocks of streams, one per device, run side by side from this one
    process (``multi.DevicePool``: the table is built once and replicated - over RCCL with more than one
    device -, no collective on the data path); the result is the same array either way."""
    if input_signals.ndim != 3:
        raise ValueError(f'expected (batch, n, C), got shape {input_signals.shape}')
    fir = np.asarray(velvet_noise_filters)
    if fir.ndim == 1:
        fir = fir[:, None]
    num_channels = input_signals.shape[2]
    if num_channels > 1 and fir.shape[1] != num_channels:
        raise ValueError('Input length mismatch: Expected signals of equal length, but got lengths '
                         f'{num_channels} and {fir.shape[1]} for dimension 1.')
    mode = _default_mode if mode is None else mode
    if num_channels:
        promoted = _promoted_convolve(np.asarray(input_signals), fir, num_channels, mode)
        if promoted is not None:
            return promoted
    x = np.ascontiguousarray(input_signals, dtype=np.float32)
    if x.size == 0:
        return np.zeros(x.shape, dtype=np.float32)
    if devices is not None:
        from . import multi
        arrays = _fir_arrays.get(fir, num_channels)
        out = _native.pinned_pool.empty(x.shape[:-1] + (arrays.num_channels,), np.float32)
        return multi.pool_for(devices).map_streams(arrays, x, out, 'convolve', mode)
    table = _fir_tables.get(_fir_key(fir, num_channels),
                            lambda: function_path_arrays(fir, num_channels))
    return table.convolve_host(x, mode)


def convolve_velvet_noise_bank(input_signal: NDArray, filter_bank: Sequence[NDArray], *,
                               mode: Optional[int] = None) -> NDArray:
    """One ``(n, C)`` signal through F filters ``(L_f, C)`` in a single launch; returns
    ``(F, n, C)`` float32 (a transposed view of the device result) with
    ``out[f] == convolve_velvet_noise(input_signal, filter_bank[f])``, bit for bit in the
    exact mode.  This is the candidate scan of the reference's optimiser
    (optimization.py:107-117 runs the F convolutions one after the other): the signal is
    uploaded once and every tile is staged per filter from L2, not from the host."""
    if input_signal.ndim != 2:
        raise ValueError(f'expected a (n, C) signal, got shape {input_signal.shape}')
    firs = [np.asarray(f) if np.asarray(f).ndim == 2 else np.asarray(f)[:, None] for f in filter_bank]
    if not firs:
        raise ValueError('empty filter bank')
    num_channels = input_signal.shape[1]
    for fir in firs:
        if num_channels > 1:
            check_equal_length(input_signal, fir, dim=1)
    x = np.ascontiguousarray(input_signal, dtype=np.float32)
    if x.shape[0] == 0 or num_channels == 0:
        return np.zeros((len(firs),) + x.shape, dtype=np.float32)
    key = ('bank', num_channels) + tuple(_fir_key(fir, num_channels) for fir in firs)
    table = _fir_tables.get(key, lambda: concat_tap_arrays([function_path_arrays(fir, num_channels)
                                                             for fir in firs]))
    y = table.convolve_host(x, _default_mode if mode is None else mode)       # (n, F*C)
    return y.reshape(x.shape[0], len(firs), num_channels).transpose(1, 0, 2)


# ----------------------------------------------------------------------------
# Velvet-noise impulse containers   (decorrelation.py:240-323)
# ----------------------------------------------------------------------------
@dataclass
class VelvetNoiseSegment:
    """Impulse positions of one envelope segment, split by sign."""

    negative_impulse_indexes: List[int] = field(default_factory=list)
    positive_impulse_indexes: List[int] = field(default_factory=list)

    def __iter__(self) -> Iterator:
        yield self.negative_impulse_indexes, '__isub__'
        yield self.positive_impulse_indexes, '__iadd__'

    def __getitem__(self, key: int) -> List[int]:
        if key == 0:
            return self.negative_impulse_indexes
        if key == 1:
            return self.positive_impulse_indexes
        raise ValueError('Invalid key')

    def __setitem__(self, key: int, value) -> None:
        if key == 0:
            self.negative_impulse_indexes = value
        elif key == 1:
            self.positive_impulse_indexes = value
        else:
            raise ValueError('Invalid key')


@dataclass
class VelvetNoiseSequence:
    """The segments of one output channel."""

    segments: List[VelvetNoiseSegment] = field(default_factory=list)

    @classmethod
    def create(cls, *, num_segments: int) -> 'VelvetNoiseSequence':
        return cls(segments=[VelvetNoiseSegment() for _ in range(num_segments)])

    def __iter__(self):
        return iter(self.segments)

    def __len__(self):
        return len(self.segments)

    def __getitem__(self, key: int) -> VelvetNoiseSegment:
        return self.segments[key]

    def __setitem__(self, key: int, value) -> None:
        self.segments[key] = value


@dataclass
class ParallelVelvetNoise:
    """One sequence per output channel; an unfiltered channel is an empty list."""

    fir_length_samples: int
    output_channels: list = field(default_factory=list)

    @property
    def num_outs(self) -> int:
        return len(self.output_channels)

    @property
    def num_impluses(self) -> int:      # (sic) - the reference's spelling, counted on channel 0
        return sum(len(seg.negative_impulse_indexes) + len(seg.positive_impulse_indexes)
                   for channel in self.output_channels[0:1] for seg in channel)

    num_impulses = num_impluses

    def __iter__(self):
        return iter(self.output_channels)

    def __getitem__(self, key: int):
        return self.output_channels[key]

    def __setitem__(self, key: int, value) -> None:
        self.output_channels[key] = value


_VelvetNoiseSegment = VelvetNoiseSegment
_VelvetNoiseSequence = VelvetNoiseSequence
_ParallelVelvetNoise = ParallelVelvetNoise


# ----------------------------------------------------------------------------
# VelvetNoise   (decorrelation.py:326-546)
# ----------------------------------------------------------------------------
@dataclass(kw_only=True)
class VelvetNoise(Decorrelator):
    """Velvet-noise decorrelator with the reference's fields and defaults.

    The impulse table is drawn once at construction and again only when
    ``num_outs``, ``num_impulses`` or ``fir_length_samples`` change
    (decorrelation.py:368-379); ``segment_envelope`` is read at convolve time.
    ``convolve`` uploads the table to the GPU once and reuses it.
    """

    duration_seconds: float = 0.03
    num_impulses: int = 30
    segment_envelope: Sequence[float] = DEFAULT_SEGMENT_ENVELOPE
    log_distribution_strength: float = 1.0
    normalizer: Optional[Callable[[NDArray, NDArray], None]] = rms_normalize
    filtered_channels: Sequence[int] = (0, 1)
    mode: LayoutMode = LayoutMode.MS
    seed: Optional[int] = None

    _velvet_noise: Any = field(default=None, repr=False, compare=False)
    _device: Any = field(default=None, repr=False, compare=False)   # (impulse table, envelope key, device, TapTable)

    def __post_init__(self) -> None:
        if self.num_impulses >= self.fir_length_samples * 0.2:
            raise ValueError(
                f'Velvet Noise Filter of length {self.fir_length_samples} with {self.num_impulses} '
                f'impulses is not sparse. (density={self.density:.2f})\n'
                '\tnum_impulses must be less than 20% the FIR length in samples.')
        if not self.segment_envelope:
            self.segment_envelope = IDENTITY_ENVELOPE
        self._velvet_noise = self._generate()

    # ---- derived quantities --------------------------------------------------
    @property
    def density(self) -> float:
        """Impulses per second."""
        return self.num_impulses / self.duration_seconds

    @property
    def fir_length_samples(self) -> int:
        return int(round(self.sample_rate_hz * self.duration_seconds))

    @property
    def unfiltered_channels(self):
        return filter(lambda c: c not in self.filtered_channels, range(self.num_outs))

    @property
    def velvet_noise(self) -> ParallelVelvetNoise:
        vn = self._velvet_noise
        if (self.num_outs != vn.num_outs or self.num_impulses != vn.num_impluses
                or self.fir_length_samples != vn.fir_length_samples):
            self._velvet_noise = self._generate()
        return self._velvet_noise

    @property
    def FIR(self) -> NDArray:
        """Dense float64 ``(fir_length_samples, len(filtered_channels))`` view of
        the impulse table; a later impulse on an occupied sample wins."""
        filtered = [seq for seq in self.velvet_noise if len(seq)]
        fir = np.zeros((self.fir_length_samples, len(self.filtered_channels)))
        for f, sequence in enumerate(filtered):
            for s, segment in enumerate(sequence):
                for i in segment.negative_impulse_indexes:
                    fir[i, f] = self.segment_envelope[s] * -1
                for i in segment.positive_impulse_indexes:
                    fir[i, f] = self.segment_envelope[s] * 1
        return fir

    # ---- generation ----------------------------------------------------------
    def _generate(self) -> ParallelVelvetNoise:
        num_segments = len(self.segment_envelope)
        table = ParallelVelvetNoise(fir_length_samples=self.fir_length_samples)
        positions, signs = _draw_taps(self.seed, self.num_impulses, len(self.filtered_channels),
                                      self.fir_length_samples, self.sample_rate_hz,
                                      self.duration_seconds, self.log_distribution_strength)
        for channel in range(self.num_outs):
            if channel not in self.filtered_channels:
                table.output_channels.append([])
                continue
            # random columns are addressed by OUTPUT channel number, as upstream (:531)
            column, column_signs = positions[:, channel], signs[:, channel]
            sequence = VelvetNoiseSequence.create(num_segments=num_segments)
            for k in range(self.num_impulses):
                segment = sequence[_segment_index(k, self.num_impulses, num_segments)]
                segment[int((column_signs[k] + 1) / 2)].append(column[k])
            table.output_channels.append(sequence)
        return table

    # ---- the hot path --------------------------------------------------------
    def _tap_member(self):
        """``(channels, envelope, apply_gain)`` as ``taps.class_path_arrays`` / ``class_path_bank_arrays`` take them."""
        apply_gain = self.segment_envelope != IDENTITY_ENVELOPE
        channels = []
        for sequence in self.velvet_noise:
            if not len(sequence):
                channels.append(None)
            else:
                channels.append([(seg.negative_impulse_indexes, seg.positive_impulse_indexes)
                                 for seg in sequence])
        return channels, self.segment_envelope, apply_gain

    def _tap_arrays(self) -> TapArrays:
        return class_path_arrays(*self._tap_member())

    def _device_table(self) -> _native.TapTable:
        """Device image of the current impulse table + envelope, uploaded once.  The
        cache holds the impulse-table OBJECT (compared with ``is``), not its id: a
        regenerated table may be allocated at a freed table's address."""
        vn = self.velvet_noise
        env = self.segment_envelope
        env_key = (type(env).__name__, tuple(env))
        device = _native.default_context().device
        cached = self._device
        if cached is None or cached[0] is not vn or cached[1] != env_key or cached[2] != device:
            arrays = self._tap_arrays()
            if cached is not None:
                cached[3].close()
            table = _native.TapTable.create(_native.default_context(), arrays.tap_offsets, arrays.tap_index,
                                            arrays.tap_weight, **arrays.kwargs())
            self._device = cached = (vn, env_key, device, table)
        return cached[3]

    def convolve(self, input_signal: NDArray) -> NDArray:
        """Velvet-noise filter every ``filtered_channel`` of a ``(n, >= num_outs)``
        signal on the GPU; other output channels are copied through.  float32
        ``(n, num_outs)``, bit-identical to ``VelvetNoise.convolve``
        (decorrelation.py:393-415) for float32 input."""
        if input_signal.ndim != 2:
            raise IndexError('too many indices for array: convolve expects a (n, channels) signal')
        x = np.ascontiguousarray(input_signal[:, :self.num_outs], dtype=np.float32)
        if x.shape[1] != self.num_outs:
            raise IndexError(f'index {self.num_outs - 1} is out of bounds for axis 1 '
                             f'with size {input_signal.shape[1]}')
        table = self._device_table()
        if x.shape[0] == 0:
            return np.zeros((0, self.num_outs), dtype=np.float32)
        return table.convolve_host(x, _default_mode)

    def decorrelate(self, input_signal: NDArray) -> NDArray:
        """Full stage (decorrelation.py:417-442): float32 cast, mono->stereo, GPU convolution,
        then the epilogue - side-channel encode (MS mode), width, normaliser - on the device
        where that is faithful to the reference (see ``set_device_epilogue``), else in NumPy."""
        input_signal = to_float32(input_signal)
        if input_signal.ndim == 1 and self.num_outs == 2 and input_signal.shape[0] > 0:
            # a mono signal (mono_to_stereo, decorrelation.py:428-431): the device reads the one channel for both outputs (fan-out);
            # the (n, 2) copy the reference makes is materialised only where the host epilogue needs it - it costs more than the
            # whole device stage of a 10 s signal
            mono = np.ascontiguousarray(input_signal, dtype=np.float32)[:, None]
            if _use_device_epilogue(2, self.normalizer is not None, mono.shape[0], True) and \
                    (self.normalizer is None or self.normalizer is rms_normalize):
                return self._decorrelate_on_device(mono)
            output_signal = self._device_table().convolve_host(mono, _default_mode)
            return self._host_epilogue(mono_to_stereo(input_signal), output_signal)
        if input_signal.ndim == 1:
            input_signal = mono_to_stereo(input_signal)
        # NumPy's sum order follows the memory layout (a Fortran-ordered signal is summed pairwise,
        # column by column): the device repeats the C-contiguous order only, so by default other
        # layouts keep the host epilogue, which sees the caller's array as the reference does
        if _use_device_epilogue(self.num_outs, self.normalizer is not None, input_signal.shape[0],
                                input_signal.flags.c_contiguous) and self._device_epilogue_applies(input_signal):
            return self._decorrelate_on_device(input_signal)
        output_signal = self.convolve(input_signal)
        return self._host_epilogue(input_signal, output_signal)

    def stream(self, *, num_streams: int = 1, in_channels: Optional[int] = None, mode: int = MODE_EXACT,
               max_frames_per_call: int = 4800):
        """A chunked stream of ``decorrelate`` (``streaming.Stream``): a pool of ``num_streams`` signals fed block by block,
        each block's final outputs returned at once, ``H = latency_frames`` frames behind the input.  The concatenation
        equals ``decorrelate`` of the whole signal - bit for bit in ``MODE_EXACT`` - with the mid/side encode (MS mode) and
        the width on the device.  ``in_channels``: ``num_outs`` (default), or 1 for a mono signal of a stereo stage
        (``mono_to_stereo``, read by both output channels).  Chunks of any real dtype are cast to float32 first, as
        ``decorrelate`` casts its input.  The impulse table and envelope are taken as they are now.

        The RMS normaliser scales by the RMS of the whole input and output, which a stream has not seen: a stage with a
        normaliser raises ``ValueError`` - build it with ``normalizer=None`` (and, if wanted, normalise afterwards)."""
        from . import streaming
        if self.normalizer is not None:
            raise ValueError('VelvetNoise.stream needs normalizer=None: the RMS normaliser scales by the RMS of the whole '
                             'input and output signals, which a stream only has once it has ended')
        channels = self.num_outs if in_channels is None else in_channels
        if channels != self.num_outs and not (channels == 1 and self.num_outs == 2):
            raise ValueError(f'in_channels={channels}: a stage of {self.num_outs} outputs streams {self.num_outs} '
                             'input channels' + (', or 1 (mono to stereo)' if self.num_outs == 2 else ''))
        if (self.mode == LayoutMode.MS or self.width is not None) and self.num_outs != 2:
            raise ValueError('Input shape invalid: Expected shape (num samples, 2), '
                             f'but got shape (num samples, {self.num_outs}).')
        return streaming.Stream(self._tap_arrays(), num_streams=num_streams, in_channels=channels, mode=mode,
                                max_frames_per_call=max_frames_per_call, ms_encode=self.mode == LayoutMode.MS,
                                width=self.width, any_dtype=True, one_shot='VelvetNoise.decorrelate')

    def _host_epilogue(self, input_signal: NDArray, output_signal: NDArray) -> NDArray:
        """decorrelation.py:433-440, in place on ``output_signal`` (NumPy: bit-identical)."""
        if self.mode == LayoutMode.MS:
            encode_signal_to_side_channel(input_signal, output_signal)
        if self.width is not None:
            apply_stereo_width(output_signal, self.width)
        if self.normalizer:
            self.normalizer(input_signal, output_signal)
        return output_signal


    # ---- device epilogue ------------------------------------------
    def _device_epilogue_applies(self, x: NDArray) -> bool:
        """The fused path covers the default normaliser (or none) on signals whose
        channel count equals ``num_outs``; anything else keeps the host epilogue."""
        return (x.ndim in (2, 3) and x.shape[-1] == self.num_outs and x.shape[-2] > 0
                and (self.normalizer is None or self.normalizer is rms_normalize))

    def _decorrelate_on_device(self, x: NDArray, devices=None) -> NDArray:
        stereo_steps = self.mode == LayoutMode.MS or self.width is not None
        if stereo_steps and self.num_outs != 2:
            raise ValueError('Input shape invalid: Expected shape (num samples, 2), '
                             f'but got shape {x.shape[:-1] + (self.num_outs,)}.')
        x = np.ascontiguousarray(x, dtype=np.float32)
        stage = dict(ms_encode=self.mode == LayoutMode.MS, width=self.width,
                     normalize=_normalize_flag(self.normalizer is not None))
        if devices is not None and x.ndim == 3:
            from . import multi
            out = _native.pinned_pool.empty(x.shape[:-1] + (self.num_outs,), np.float32)
            return multi.pool_for(devices).map_streams(self._tap_arrays(), x, out, 'decorrelate', _default_mode, **stage)
        return self._device_table().decorrelate_host(x, _default_mode, **stage)

    def decorrelate_batched(self, input_signals: NDArray, *, devices=None) -> NDArray:
        """``(B, n, num_outs)`` independent signals through the whole stage in one
        device pass (convolution + epilogue on the GPU); float32 result, same shape.
        ``devices='all'`` or a list of device indices: contiguous blocks of the batch on several GPUs
        from this one process (see :func:`convolve_velvet_noise_batched`); the stage's reductions are per
        stream, so nothing crosses devices."""
        x = to_float32(np.asarray(input_signals))
        if x.ndim != 3:
            raise ValueError(f'expected (batch, n, channels), got shape {x.shape}')
        if devices is not None:
            from . import multi
            multi.resolve_devices(devices)              # a bad list is an error whatever path the batch takes
        if _device_epilogue is None and not _use_device_epilogue(self.num_outs, self.normalizer is not None,
                                                                  x.shape[1], True):
            return np.stack([self.decorrelate(sig[:, 0] if x.shape[-1] == 1 else sig) for sig in x]) \
                if len(x) else np.zeros(x.shape[:-1] + (self.num_outs,), np.float32)
        if x.shape[-1] == 1 and self.num_outs == 2 and x.shape[1] > 0 and \
                (self.normalizer is None or self.normalizer is rms_normalize):
            return self._decorrelate_on_device(x, devices if len(x) else None)      # mono signals, fanned out on the device
        if not self._device_epilogue_applies(x):
            return np.stack([self.decorrelate(sig) for sig in x]) if len(x) else np.zeros(x.shape, np.float32)
        return self._decorrelate_on_device(x, devices if len(x) else None)


def decorrelate_bank(input_signal: NDArray, decorrelators: Sequence[VelvetNoise]) -> List[NDArray]:
    """``[d.decorrelate(input_signal) for d in decorrelators]`` with the F convolutions in ONE
    device launch (the tables concatenated channel-wise, the signal fanned out to them) and
    each decorrelator's own epilogue on the host afterwards - the shape of the reference
    optimiser's candidate scan (optimization.py:71, :107-117).  Bit-identical to the loop
    in the exact mode."""
    decorrelators = list(decorrelators)
    if not decorrelators:
        return []
    num_outs = decorrelators[0].num_outs
    if any(d.num_outs != num_outs for d in decorrelators):
        raise ValueError('all decorrelators of a bank must have the same num_outs')
    input_signal = to_float32(input_signal)
    if input_signal.ndim == 1:
        input_signal = mono_to_stereo(input_signal)
    if input_signal.ndim != 2:
        raise IndexError('too many indices for array: decorrelate expects a (n,) or (n, channels) signal')
    x = np.ascontiguousarray(input_signal[:, :num_outs], dtype=np.float32)
    if x.shape[1] != num_outs:
        raise IndexError(f'index {num_outs - 1} is out of bounds for axis 1 with size {input_signal.shape[1]}')
    if x.shape[0] == 0:
        return [d.decorrelate(input_signal) for d in decorrelators]
    arrays = concat_tap_arrays([d._tap_arrays() for d in decorrelators])
    table = _native.TapTable.create(_native.default_context(), arrays.tap_offsets, arrays.tap_index,
                                    arrays.tap_weight, **arrays.kwargs())
    try:
        y = table.convolve_host(x, _default_mode)                           # (n, F * num_outs)
    finally:
        table.close()
    return [d._host_epilogue(input_signal, np.ascontiguousarray(y[:, f * num_outs:(f + 1) * num_outs]))
            for f, d in enumerate(decorrelators)]


# ----------------------------------------------------------------------------
# The chain stages either side of the path: HaasEffect, WhiteNoise
# ----------------------------------------------------------------------------
@dataclass(kw_only=True)
class HaasEffect(Decorrelator):
    """Delay one channel by ``round(delay_time_seconds * fs)`` samples
    (decorrelation.py:163-230).  Returns float64 ``(n + delay, 2)``."""

    delayed_channel: int = 0
    delay_time_seconds: float = 0.02
    mode: LayoutMode = LayoutMode.LR

    def decorrelate(self, input_signal: NDArray) -> NDArray:
        output_signal = self.haas_delay(to_float32(input_signal))
        if self.width is not None:
            apply_stereo_width(output_signal, self.width)
        return output_signal

    def stream(self, *, num_streams: int = 1, in_channels: int = 2, max_frames_per_call: int = 4800):
        """A chunked stream of ``decorrelate`` (``streaming.HaasStream``): a pool of ``num_streams`` signals fed block by
        block.  The delay is causal, so each call returns the frames it was given, at no latency; ``flush()`` returns the
        ``d = tail_frames`` tail frames, and the concatenation equals ``decorrelate`` of the whole signal bit for bit,
        float64 ``(n + d, 2)``.  ``in_channels``: 2, or 1 for a mono ``(n,)`` signal.  Chunks of any real dtype are cast to
        float32 first, as ``decorrelate`` casts its input.  The stage's settings are taken as they are now.

        Covered: what ``optimization.haas_scan_covers`` accepts - a plain ``HaasEffect`` in LR or MS layout, delayed
        channel 0 or 1, a delay in [0, 2**31) frames and a finite Python / float64 width or None; anything else raises
        ``ValueError`` before any device call."""
        from . import optimization, streaming
        if not optimization.haas_scan_covers(np.zeros(1), self):
            raise ValueError('HaasEffect.stream covers a plain HaasEffect in LR or MS layout with delayed channel 0 or 1, '
                             'an integer delay in [0, 2**31) and a finite Python / float64 width or None')
        delayed_channel, ms_mode, width = optimization._haas_key(self)
        return streaming.HaasStream(num_streams=num_streams, in_channels=in_channels,
                                    max_frames_per_call=max_frames_per_call, delay=optimization._haas_delay(self),
                                    delayed_channel=delayed_channel, ms_mode=ms_mode, width=width)

    def haas_delay(self, input_signal: NDArray) -> NDArray:
        delay = round(self.delay_time_seconds * self.sample_rate_hz)
        n = len(input_signal)
        mono = input_signal.ndim == 1
        if mono:
            input_signal = mono_to_stereo(input_signal)
        out = np.zeros((n + delay, 2))
        out[:n, :] = input_signal
        mid_side = self.mode == LayoutMode.MS
        if mid_side and not mono:
            LR_to_MS(out)
        out[:, self.delayed_channel] = np.roll(out[:, self.delayed_channel], delay, axis=0)
        if mid_side:
            MS_to_LR(out)
            if mono:
                out *= 0.5          # the duplicated mono channel counted twice
        return out


@dataclass(kw_only=True)
class WhiteNoise(Decorrelator):
    """Dense Gaussian FIR per channel via ``np.convolve(mode='same')``, then width and
    ``rms_normalize`` (decorrelation.py:670-716) - the comparison baseline of the reference's plots.
    On the GPU where covered (``set_white_noise_device``), in NumPy otherwise."""

    duration_seconds: float = 0.03
    seed: Optional[int] = None
    white_noise_filter: Any = field(default=None, repr=False)

    def __post_init__(self) -> None:
        rng = np.random.default_rng(self.seed)
        self.white_noise_filter = rng.normal(loc=0, scale=1,
                                             size=(self.fir_length_samples, self.num_outs))
        self._device_fir = None           # (key, device tensor) of the filter's used columns

    @property
    def fir_length_samples(self) -> int:
        return int(round(self.sample_rate_hz * self.duration_seconds))

    @property
    def FIR(self) -> NDArray:
        return self.white_noise_filter

    def decorrelate(self, input_signal: NDArray) -> NDArray:
        input_signal = to_float32(input_signal)
        if self._on_device(input_signal.shape, input_signal.ndim != 2 or input_signal.flags.c_contiguous):
            x = np.ascontiguousarray(input_signal)
            return self._decorrelate_on_device(x.reshape((1,) + x.shape[:1] + (x.shape[1] if x.ndim == 2 else 1,)))[0]
        if input_signal.ndim == 1:
            input_signal = mono_to_stereo(input_signal)
        out = np.zeros((len(input_signal), self.num_outs), dtype=np.float32)
        for c in range(self.num_outs):
            out[:, c] = np.convolve(input_signal[:, c], self.white_noise_filter[:, c], mode='same')
        if self.width is not None:
            apply_stereo_width(out, self.width)
        rms_normalize(input_signal, out)
        return out

    def decorrelate_batched(self, input_signals: NDArray) -> NDArray:
        """``(B, n, C)`` or mono ``(B, n)`` independent signals through the whole stage; float32 ``(B, n, num_outs)``,
        equal bit for bit to stacking ``decorrelate`` over the streams.  Covered shapes take one device pass per
        VND_MAX_STREAMS streams; others the per-stream loop."""
        x = to_float32(np.asarray(input_signals))
        if x.ndim not in (2, 3):
            raise ValueError(f'expected (batch, n) or (batch, n, channels), got shape {x.shape}')
        if len(x) and self._on_device(x.shape[1:], x.flags.c_contiguous):
            x = np.ascontiguousarray(x)
            return self._decorrelate_on_device(x if x.ndim == 3 else x[:, :, None])
        if not len(x):
            return np.zeros((0, x.shape[1], self.num_outs), np.float32)
        return np.stack([self.decorrelate(sig) for sig in x])

    def _on_device(self, shape, c_contiguous: bool) -> bool:
        return analysis.device_route(
            _white_noise_device, white_noise_covers(shape, self.num_outs, self.width, self.white_noise_filter, c_contiguous),
            'set_white_noise_device(True): no gfx950 device (or no built extension) to run WhiteNoise on')

    def _device_filter(self, torch, device):
        """The filter's ``num_outs`` columns as a float64 device tensor, uploaded again only when their bytes change."""
        view = np.ascontiguousarray(self.white_noise_filter[:, :self.num_outs], dtype=np.float64)
        key = (view.shape, _digest16(view), str(device))
        cached = getattr(self, '_device_fir', None)
        if cached is None or cached[0] != key:
            cached = self._device_fir = (key, torch.from_numpy(view.copy()).to(device))
        return cached[1]

    def _decorrelate_on_device(self, x: NDArray) -> NDArray:
        """x: C-contiguous float32 ``(B, n, Cx)``, Cx = num_outs or 1 (fanned out to 2)."""
        torch = _native.torch_module()
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        batch, n, cx = x.shape
        h = self._device_filter(torch, device)
        out = _native.pinned_pool.empty((batch, n, self.num_outs), np.float32)
        step = _native.MAX_STREAMS_PER_CALL
        for first in range(0, batch, step):
            part = x[first:first + step]
            xd = torch.from_numpy(part if part.flags.writeable else part.copy()).to(device)
            yd = torch.empty((len(part), n, self.num_outs), dtype=torch.float32, device=device)
            ws_bytes = _native.decorrelate_workspace_bytes(len(part), n, self.num_outs)
            work = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
            _native.white_noise_device(ctx, xd.data_ptr(), h.data_ptr(), yd.data_ptr(), len(part), n, cx, self.num_outs,
                                       h.shape[0], width=self.width, normalize=_native.NORMALIZE_RMS_REFERENCE_ORDER,
                                       workspace_ptr=work.data_ptr(), workspace_bytes=ws_bytes,
                                       stream=torch.cuda.current_stream(device).cuda_stream)
            torch.from_numpy(out[first:first + len(part)]).copy_(yd)
        return out


# ----------------------------------------------------------------------------
# decorrelate_each: a pool through one decorrelator PER SIGNAL (include/vnd_each.h) - the application side of
# optimize_velvet_noise_batched / optimize_haas_delay_batched, which return one kappa or one delay per signal
# ----------------------------------------------------------------------------
# the padded float64 block of the Haas route, (B, n + max delay, 2): above this many bytes the call takes the host loop
_EACH_HAAS_BYTES = 4 << 30

_each_device: Optional[bool] = None


def set_each_device(enabled: Optional[bool]) -> None:
    """Where :func:`decorrelate_each` runs.

    ``None`` (default): on the GPU when a gfx950 device is present and the call is covered (:func:`each_covers`),
    otherwise the loop ``[d.decorrelate(x_b) ...]``.  ``True``: the device for every covered call; ``RuntimeError`` when
    there is none.  ``False``: always the loop."""
    global _each_device
    if enabled is not None and not isinstance(enabled, (bool, np.bool_)):
        raise TypeError(f'set_each_device takes True, False or None, not {enabled!r}')
    _each_device = None if enabled is None else bool(enabled)


@dataclass
class EachStats:
    """The work of one :func:`decorrelate_each` call (tools, tests), after ``optimization.VelvetSearchStats``."""
    route: str                                            # 'device', 'host' (the loop) or 'none' (an empty pool)
    kind: str = ''                                        # 'velvet' or 'haas' on the device route
    signals: int = 0
    tables: int = 0                                       # velvet: distinct tap tables among the signals'
    launches: int = 0                                     # calls into the library
    launch_signals: List[int] = field(default_factory=list)
    launch_tables: List[int] = field(default_factory=list)   # velvet: candidates in each call's bank
    launch_pool: List[int] = field(default_factory=list)  # a tensor pool: the device address each call read its signals at
    pool_uploads: int = 0                                 # a NumPy pool: the calls that took it up from host memory
    result_downloads: int = 0                             # ... and brought their result back


last_each: Optional[EachStats] = None


def _each_pool(input_signals):
    """``(pool, is_torch)``: the pool as it came, after the shape and dtype checks."""
    is_torch = _native.is_torch(input_signals)
    x = input_signals if is_torch else np.asarray(input_signals)
    shape = tuple(x.shape)
    if not (len(shape) == 2 or (len(shape) == 3 and shape[2] in (1, 2))):
        raise ValueError(f'expected a stereo pool (B, n, 2) or a mono pool (B, n, 1) or (B, n), got shape {shape}')
    if is_torch:
        import torch
        if x.is_complex() or x.dtype == torch.bool:
            raise TypeError(f'signals must be real numbers, got {x.dtype}')
    elif x.dtype.kind not in 'biuf':
        raise TypeError(f'signals must be real numbers, got {x.dtype}')
    return x, is_torch


def _each_signal(x, b: int):
    """Signal b of a pool as ``decorrelate`` takes it: ``(n, 2)``, or ``(n,)`` of a mono pool."""
    return x[b, :, 0] if x.ndim == 3 and x.shape[2] == 1 else x[b]


def _each_velvet_key(d):
    """``(MS?, width, normaliser?)`` of a VelvetNoise whose stage the device form covers, else None."""
    if type(d) is not VelvetNoise or d.num_outs != 2 or d.mode not in (LayoutMode.LR, LayoutMode.MS):
        return None
    if d.normalizer is not None and d.normalizer is not rms_normalize:
        return None
    w = d.width
    if w is not None and (type(w) not in (int, float, np.float64) or not np.isfinite(w)):
        return None
    return d.mode == LayoutMode.MS, None if w is None else float(w), d.normalizer is not None


def _member_key(member):
    channels, envelope, apply_gain = member
    return (tuple(None if segs is None else tuple((tuple(neg), tuple(pos)) for neg, pos in segs) for segs in channels),
            tuple(envelope), bool(apply_gain))


def _member_in_window(member) -> bool:
    """Whether a table's largest index is within the kernel's staged window and its weights (+-1 times the gains) are
    finite as float32."""
    channels, envelope, apply_gain = member
    for segs in channels:
        if segs is None:
            continue
        for s, (neg, pos) in enumerate(segs):
            if (neg and not 0 <= min(neg) <= max(neg) <= _native.VELVET_PAIRS_MAX_TAP_INDEX) or \
                    (pos and not 0 <= min(pos) <= max(pos) <= _native.VELVET_PAIRS_MAX_TAP_INDEX):
                return False
            with np.errstate(over='ignore'):
                if apply_gain and not np.isfinite(np.float32(envelope[s])):
                    return False
    return True


def each_velvet_members(decorrelators: Sequence[VelvetNoise]):
    """``(members, tables)``: the distinct ``d._tap_member()`` triples of the list in order of first appearance -
    deduplicated by content: equal tap arrays, envelope and gain flag share a member - and the int32 index of every
    decorrelator's member.  ``class_path_bank_arrays(members)`` is the bank of a call over all of them."""
    members, index, tables = [], {}, []
    for d in decorrelators:
        member = d._tap_member()
        tables.append(index.setdefault(_member_key(member), len(members)))
        if tables[-1] == len(members):
            members.append(member)
    return members, np.asarray(tables, np.int32)


def _each_plan(shape: Sequence[int], decorrelators: Sequence):
    """The device form of one call, or None: ``('velvet', (MS?, width, normaliser?), members, tables)`` or
    ``('haas', (delayed channel, MS?, width), delays)``."""
    shape = tuple(shape)
    if not (len(shape) == 2 or (len(shape) == 3 and shape[2] in (1, 2))) or shape[0] != len(decorrelators) \
            or shape[0] == 0 or shape[1] == 0:
        return None
    if all(type(d) is VelvetNoise for d in decorrelators):
        if _default_mode != MODE_EXACT:
            return None
        keys = {_each_velvet_key(d) for d in decorrelators}
        if len(keys) != 1 or None in keys:
            return None
        try:
            members, tables = each_velvet_members(decorrelators)
            if not all(_member_in_window(m) for m in members):
                return None
        except (IndexError, TypeError, ValueError):       # e.g. an envelope shorter than the segment list: the loop's error
            return None
        return 'velvet', keys.pop(), members, tables
    if all(type(d) is HaasEffect for d in decorrelators):
        from . import optimization
        keys = {optimization._haas_key(d) for d in decorrelators}
        delays = [optimization._haas_delay(d) for d in decorrelators]
        if len(keys) != 1 or None in keys or None in delays:
            return None
        if shape[0] * (shape[1] + max(delays)) * 16 > _EACH_HAAS_BYTES:
            return None
        return 'haas', keys.pop(), np.asarray(delays, np.int32)
    return None


def each_covers(input_signals, decorrelators: Sequence) -> bool:
    """Whether :func:`decorrelate_each` has a device form for this pool and list: a pool ``(B, n, 2)``, ``(B, n, 1)``
    or ``(B, n)`` with B = ``len(decorrelators)`` > 0 and n > 0, and

    * all plain ``VelvetNoise`` with ``num_outs == 2``; ``mode`` (LR or MS), ``width`` and ``normalizer`` equal across
      the list, the normaliser None or ``rms_normalize``, the width None or a finite Python / float64 number; the
      default mode ``MODE_EXACT``; every table's largest index at most ``VND_VELVET_PAIRS_MAX_TAP_INDEX`` (4094) and its
      weights finite; or
    * all plain ``HaasEffect`` that ``optimization.haas_scan_covers`` accepts (LR or MS layout, delayed channel 0 or 1,
      a delay in [0, 2^31) frames, a finite Python / float64 width or None), with ``delayed_channel``, ``mode`` and
      ``width`` equal across the list, and a padded result of at most ``_EACH_HAAS_BYTES``.

    Everything else keeps the loop and its exceptions."""
    return _each_plan(np.shape(input_signals) if not _native.is_torch(input_signals) else tuple(input_signals.shape),
                      list(decorrelators)) is not None


def _each_ranges(tables, max_signals: int, max_tables: int):
    """Contiguous signal ranges ``[first, last)`` of at most ``max_signals`` signals and ``max_tables`` distinct tables
    each, greedily: one library call per range (a row depends on no other signal, so the split changes no bit)."""
    ranges, first, seen = [], 0, set()
    for b, t in enumerate(np.asarray(tables).tolist()):
        if b - first == max_signals or (t not in seen and len(seen) == max_tables):
            ranges.append((first, b))
            first, seen = b, set()
        seen.add(t)
    if len(tables) > first:
        ranges.append((first, len(tables)))
    return ranges


class _EachBanks:
    """The last few banks built, by content and device: a repeated call uploads nothing, and a bank a kernel may still
    be reading is not freed behind an asynchronous call (a dropped table goes with its last reference)."""

    def __init__(self, capacity: int = 4):
        self.capacity, self._lock, self._items = capacity, threading.Lock(), OrderedDict()

    def get(self, ctx, arrays: TapArrays) -> _native.TapTable:
        key = (ctx.device, hashlib.blake2b(arrays.to_bytes(), digest_size=16).digest())
        with self._lock:
            table = self._items.get(key)
            if table is not None:
                self._items.move_to_end(key)
                return table
        table = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())
        with self._lock:
            table = self._items.setdefault(key, table)
            self._items.move_to_end(key)
            while len(self._items) > self.capacity:
                self._items.popitem(last=False)
        return table

    def clear(self):
        with self._lock:
            self._items.clear()


_each_banks = _EachBanks()


class _EachVelvet:
    """The velvet-noise driver of :func:`decorrelate_each` over a float32 ``(B, n, C)`` pool - a C-contiguous NumPy
    array (through ``vnd_decorrelate_each_f32_host``) or a device tensor (read in place by
    ``vnd_decorrelate_each_f32_dev`` on the current stream): per range of :func:`_each_ranges` one bank of the range's
    distinct members and one call."""

    def __init__(self, ctx, pool, is_torch: bool, stage, stats: EachStats):
        self.ctx, self.pool, self.is_torch, self.stats = ctx, pool, is_torch, stats
        ms_encode, width, has_normalizer = stage
        self.stage = dict(ms_encode=ms_encode, width=width, normalize=_normalize_flag(has_normalizer))
        self.batch, self.n, self.channels = (int(v) for v in pool.shape)

    def run(self, members, tables):
        out = self._result()
        self.stats.tables = len(members)
        for first, last in _each_ranges(tables, _native.MAX_STREAMS_PER_CALL, _native.VELVET_BANK_MAX_CANDIDATES):
            distinct, local = np.unique(tables[first:last], return_inverse=True)
            arrays = class_path_bank_arrays([members[t] for t in distinct.tolist()])
            self._call(arrays, local.reshape(-1).astype(np.int32), first, last, out)
            self.stats.launches += 1
            self.stats.launch_signals.append(last - first)
            self.stats.launch_tables.append(int(distinct.size))
        return out

    def _result(self):
        if not self.is_torch:
            return np.empty((self.batch, self.n, 2), np.float32)
        import torch
        return torch.empty((self.batch, self.n, 2), dtype=torch.float32, device=self.pool.device)

    def _call(self, arrays: TapArrays, local, first: int, last: int, out) -> None:
        bank = _each_banks.get(self.ctx, arrays)
        if not self.is_torch:
            out[first:last] = _native.decorrelate_each_host(self.ctx, bank, self.pool[first:last], local, **self.stage)
            self.stats.pool_uploads += 1
            self.stats.result_downloads += 1
            return
        import torch
        dev = self.pool.device
        part, y = self.pool[first:last], out[first:last]
        ws = _native.decorrelate_workspace_bytes(last - first, self.n, 2) if self.stage['normalize'] else 0
        work = torch.empty(max(ws, 1), dtype=torch.uint8, device=dev)
        index = torch.from_numpy(local).to(dev)
        _native.decorrelate_each_device(self.ctx, bank, part.data_ptr(), index.data_ptr(), y.data_ptr(), last - first,
                                        self.n, self.channels, workspace_ptr=work.data_ptr(), workspace_bytes=ws,
                                        stream=torch.cuda.current_stream(dev).cuda_stream, **self.stage)
        self.stats.launch_pool.append(int(part.data_ptr()))


def _each_haas(ctx, pool, is_torch: bool, key, delays, stats: EachStats):
    """The Haas driver of :func:`decorrelate_each`: one padded float64 block ``(B, n + max delay, 2)`` and one call per
    ``VND_MAX_STREAMS`` signals; the result is the list of views ``block[b, :n + d_b]``."""
    delayed_channel, ms_mode, width = key
    batch, n, channels = (int(v) for v in pool.shape)
    max_delay = int(delays.max())
    settings = dict(max_delay=max_delay, delayed_channel=delayed_channel, ms_mode=ms_mode, width=width)
    step = _native.MAX_STREAMS_PER_CALL
    if is_torch:
        import torch
        dev = pool.device
        block = torch.empty((batch, n + max_delay, 2), dtype=torch.float64, device=dev)
        frames = torch.from_numpy(delays).to(dev)
        for first in range(0, batch, step):
            part, count = pool[first:first + step], min(step, batch - first)
            _native.haas_each_device(ctx, part.data_ptr(), block[first:first + step].data_ptr(), count, n, channels,
                                     frames[first:first + step].data_ptr(),
                                     stream=torch.cuda.current_stream(dev).cuda_stream, **settings)
            stats.launches += 1
            stats.launch_signals.append(count)
            stats.launch_pool.append(int(part.data_ptr()))
    else:
        block = np.empty((batch, n + max_delay, 2), np.float64)
        for first in range(0, batch, step):
            block[first:first + step] = _native.haas_each_host(ctx, pool[first:first + step], delays[first:first + step],
                                                               **settings)
            stats.launches += 1
            stats.launch_signals.append(min(step, batch - first))
            stats.pool_uploads += 1
            stats.result_downloads += 1
    return [block[b, :n + int(d)] for b, d in enumerate(delays.tolist())]


def decorrelate_each(input_signals, decorrelators: Sequence[Decorrelator]):
    """Signal b of a pool through ``decorrelators[b]``: ``[d.decorrelate(x_b) for x_b, d in zip(pool, decorrelators)]``
    as one launch chain for the whole pool - what applies the per-signal results of
    ``optimization.optimize_velvet_noise_batched`` / ``optimize_haas_delay_batched``.

    ``input_signals`` is a pool ``(B, n, 2)``, ``(B, n, 1)`` or ``(B, n)`` (mono signals, fanned out to both outputs):
    a NumPy array of any real dtype (cast as ``to_float32`` casts it) or a CUDA torch tensor, which is read in place -
    the result is then a device tensor (tensors), enqueued on the current stream without synchronising.
    ``len(decorrelators)`` must be B (``ValueError``); the list is of one type (``TypeError`` for a mix).

    All ``VelvetNoise``: ``(B, n, 2)`` float32, equal to ``np.stack`` of the loop bit for bit.  The signals' tap tables
    (``d._tap_member()``) are deduplicated by content and go up as one class-path bank (several past 32767 distinct
    tables or ``VND_MAX_STREAMS`` signals); signal b runs through its own candidate (``vnd_decorrelate_each_f32_*``,
    always ``VND_MODE_EXACT``).
    All ``HaasEffect``: a list of B float64 ``(n + d_b, 2)`` arrays (tensors), views of one padded block, each equal to
    ``d.decorrelate(x_b)`` bit for bit (``vnd_haas_each_f64_*``).

    Device route (:func:`set_each_device`: ``None`` with a gfx950 device, or ``True``) for the calls
    :func:`each_covers` accepts; everything else - other decorrelator types, per-signal stage settings, a custom
    normaliser, a tolerance mode, filters past 4094 frames - is the loop, with the loop's own exceptions.
    ``last_each`` records the call's work (:class:`EachStats`)."""
    global last_each
    decorrelators = list(decorrelators)
    x, is_torch = _each_pool(input_signals)
    batch = int(x.shape[0])
    if len(decorrelators) != batch:
        raise ValueError(f'{len(decorrelators)} decorrelators for a pool of {batch} signals')
    if len({type(d) for d in decorrelators}) > 1:
        raise TypeError('decorrelate_each takes decorrelators of one type, got '
                        + ', '.join(sorted({type(d).__name__ for d in decorrelators})))
    if batch == 0:
        last_each = EachStats(route='none')
        if is_torch:
            import torch
            return torch.zeros((0, int(x.shape[1]), 2), dtype=torch.float32, device=x.device)
        return np.zeros((0, x.shape[1], 2), np.float32)
    plan = _each_plan(tuple(x.shape), decorrelators)
    if not analysis.device_route(_each_device, plan is not None,
                                 'set_each_device(True): no gfx950 device (or no built extension) to run on'):
        last_each = EachStats(route='host', signals=batch)
        pool = x.detach().cpu().numpy() if is_torch else x
        rows = [d.decorrelate(_each_signal(pool, b)) for b, d in enumerate(decorrelators)]
        if type(decorrelators[0]) is VelvetNoise:
            rows = np.stack(rows)
        if not is_torch:
            return rows
        import torch
        return torch.from_numpy(rows).to(x.device) if isinstance(rows, np.ndarray) \
            else [torch.from_numpy(np.ascontiguousarray(r)).to(x.device) for r in rows]
    stats = last_each = EachStats(route='device', kind=plan[0], signals=batch)
    if is_torch:
        import torch
        if not x.is_cuda:
            raise ValueError('a torch pool must be a device tensor (NumPy arrays are uploaded)')
        ctx = _native.context_for(x.device.index if x.device.index is not None else torch.cuda.current_device())
        pool = x.reshape(batch, x.shape[1], -1)
        pool = (pool if pool.dtype == torch.float32 else pool.to(torch.float32)).contiguous()
    else:
        ctx = _native.default_context()
        pool = np.ascontiguousarray(to_float32(x.reshape(batch, x.shape[1], -1)))
    if plan[0] == 'velvet':
        return _EachVelvet(ctx, pool, is_torch, plan[1], stats).run(plan[2], plan[3])
    return _each_haas(ctx, pool, is_torch, plan[1], plan[2], stats)


def _same_across(decorrelators, fields: Sequence[str], entry: str = 'decorrelate_each_stream', one: str = 'stream') -> None:
    """``ValueError`` naming the first of ``fields`` that differs across the list: the stage settings are scalars of a
    call, the same for every stream (``entry``, ``one``: the words of the message)."""
    for name in fields:
        first = getattr(decorrelators[0], name)
        for b, d in enumerate(decorrelators):
            v = getattr(d, name)
            if not (v is first or (type(v) is type(first) and v == first)):
                raise ValueError(f'{entry}: {name} differs across the list ({first!r}, and {v!r} for {one} '
                                 f'{b}): the stage settings are the same for every {one} of a pool')


def _velvet_stream_bank(decorrelators, entry: str, one: str):
    """What a streamed pool of plain ``VelvetNoise`` checks of its list, and the bank it runs on:
    ``(bank arrays, tables, ms_encode, width)``, ``tables[b]`` the candidate of ``decorrelators[b]`` in the deduplicated
    bank.  Every refusal is a ``ValueError`` that starts with ``entry`` or names the ``one`` (stream, bank entry) at fault."""
    _same_across(decorrelators, ('mode', 'width', 'normalizer'), entry, one)
    if decorrelators[0].normalizer is not None:
        raise ValueError('VelvetNoise.stream needs normalizer=None: the RMS normaliser scales by the RMS of the whole '
                         'input and output signals, which a stream only has once it has ended')
    for b, d in enumerate(decorrelators):
        if d.num_outs != 2:
            raise ValueError(f'{one} {b}: num_outs={d.num_outs}; a bank holds stereo pairs (num_outs == 2)')
    key = _each_velvet_key(decorrelators[0])
    if key is None:
        raise ValueError(f'{entry} covers the LR and MS layouts and a finite Python / float64 width or '
                         f'None, got mode={decorrelators[0].mode!r}, width={decorrelators[0].width!r}')
    try:
        members, tables = each_velvet_members(decorrelators)
        inside = [_member_in_window(m) for m in members]
    except (IndexError, TypeError) as exc:
        raise ValueError(f'{entry}: a tap table cannot be built ({exc})') from exc
    if not all(inside):
        b = int(np.flatnonzero(tables == inside.index(False))[0])
        raise ValueError(f'{one} {b}: its table reaches past {_native.VELVET_PAIRS_MAX_TAP_INDEX} frames or has a gain '
                         'that is not finite as float32; stream that decorrelator with its own .stream()')
    if len(members) > _native.VELVET_BANK_MAX_CANDIDATES:
        raise ValueError(f'{len(members)} distinct tap tables, above {_native.VELVET_BANK_MAX_CANDIDATES} per bank: '
                         'split the pool')
    ms_encode, width, _ = key
    return class_path_bank_arrays(members), tables, ms_encode, width


def decorrelate_each_stream(decorrelators: Sequence[Decorrelator], *, in_channels: int = 2, max_frames_per_call: int = 4800):
    """A block stream in which stream b of a pool runs through ``decorrelators[b]`` - the streaming form of
    :func:`decorrelate_each`, and what runs the per-signal results of ``optimization.optimize_velvet_noise_batched`` /
    ``optimize_haas_delay_batched`` live: one kernel launch per call for the whole pool, the state in a per-stream ring on
    the device.  ``num_streams = len(decorrelators)``; ``in_channels``: 2, or 1 for mono signals (fanned out to both
    outputs); blocks are ``(num_streams, B, in_channels)`` with ``0 <= B <= max_frames_per_call``, NumPy arrays of any real
    dtype (cast to float32 first, as ``decorrelate`` casts its input) or CUDA tensors, answered in kind.

    All ``VelvetNoise`` (``normalizer=None``): a ``streaming.EachStream``.  The tap tables (``d._tap_member()``) are
    deduplicated by content and go up as one class-path bank; the pool advances at one latency, ``latency_frames`` = the
    bank's largest tap index.  For every stream the concatenation of everything returned equals
    ``decorrelators[b].decorrelate(x_b)`` bit for bit.
    All ``HaasEffect``: a ``streaming.HaasEachStream``, ``latency_frames`` 0 and ``tail_frames`` the largest delay; stream
    b's own signal is the first ``n + tail_frames_each[b]`` frames of its concatenation, the rest is zeros.

    A stream has no host loop to fall back to: everything not covered raises here, before any device call - ``TypeError``
    for a mixed or unsupported decorrelator type; ``ValueError`` for an empty list, a normaliser, stage settings that
    differ across the list, ``num_outs != 2``, a table past 4094 frames or a non-finite gain (stream those with the
    decorrelator's own ``.stream()``), more than ``VND_MAX_STREAMS`` streams or 32767 distinct tables, or ``in_channels``
    not in {1, 2}."""
    from . import optimization, streaming
    decorrelators = list(decorrelators)
    if not decorrelators:
        raise ValueError('decorrelate_each_stream needs at least one decorrelator: the pool has one stream per decorrelator')
    kinds = {type(d) for d in decorrelators}
    if len(kinds) > 1:
        raise TypeError('decorrelate_each_stream takes decorrelators of one type, got '
                        + ', '.join(sorted(k.__name__ for k in kinds)))
    kind = kinds.pop()
    if kind is not VelvetNoise and kind is not HaasEffect:
        raise TypeError(f'decorrelate_each_stream streams plain VelvetNoise or HaasEffect decorrelators, not {kind.__name__}')
    if isinstance(in_channels, (bool, np.bool_)) or in_channels not in (1, 2):
        raise ValueError(f'in_channels must be 1 (mono, fanned out) or 2 (stereo), got {in_channels!r}')
    if len(decorrelators) > _native.MAX_STREAMS_PER_CALL:
        raise ValueError(f'{len(decorrelators)} streams, above {_native.MAX_STREAMS_PER_CALL} per pool: split the pool')
    if kind is VelvetNoise:
        arrays, tables, ms_encode, width = _velvet_stream_bank(decorrelators, 'decorrelate_each_stream', 'stream')
        return streaming.EachStream(arrays, tables, in_channels=in_channels,
                                    max_frames_per_call=max_frames_per_call, ms_encode=ms_encode, width=width)
    _same_across(decorrelators, ('delayed_channel', 'mode', 'width'))
    key = optimization._haas_key(decorrelators[0])
    delays = [optimization._haas_delay(d) for d in decorrelators]
    if key is None or None in delays:
        raise ValueError('decorrelate_each_stream covers a plain HaasEffect in LR or MS layout with delayed channel 0 or 1, '
                         'an integer delay in [0, 2**31) and a finite Python / float64 width or None')
    delayed_channel, ms_mode, width = key
    return streaming.HaasEachStream(delays, in_channels=in_channels, max_frames_per_call=max_frames_per_call,
                                    delayed_channel=delayed_channel, ms_mode=ms_mode, width=width)


def _haas_pool_settings(decorrelators, entry: str, one: str):
    """What a streamed pool of ``HaasEffect`` checks of its list: ``(delayed_channel, ms_mode, width, delays)``, the
    stage settings the same for every ``one`` (stream, bank entry) and a delay each; ``ValueError`` otherwise."""
    from . import optimization
    _same_across(decorrelators, ('delayed_channel', 'mode', 'width'), entry, one)
    key = optimization._haas_key(decorrelators[0])
    delays = [optimization._haas_delay(d) for d in decorrelators]
    if key is None or None in delays:
        raise ValueError(f'{entry} covers a plain HaasEffect in LR or MS layout with delayed channel 0 or 1, '
                         'an integer delay in [0, 2**31) and a finite Python / float64 width or None')
    return (*key, delays)


def _chain_pool_stages(bank):
    """The ``(VelvetNoise, HaasEffect)`` stages of a bank of chains, each exactly those two in that order; ``ValueError`` /
    ``TypeError`` naming the bank entry otherwise."""
    velvets, haases = [], []
    for b, chain in enumerate(bank):
        chain._init_decorrelators()
        stages = list(chain._decorrelators)
        if len(stages) != 2:
            raise ValueError(f'bank entry {b}: a chain of {len(stages)} stages; a voice pool runs exactly one VelvetNoise '
                             'stage and then one HaasEffect stage')
        if type(stages[0]) is not VelvetNoise or type(stages[1]) is not HaasEffect:
            raise TypeError(f'bank entry {b}: a chain of {type(stages[0]).__name__} then {type(stages[1]).__name__}; a voice '
                            'pool runs exactly one VelvetNoise stage and then one HaasEffect stage')
        velvets.append(stages[0])
        haases.append(stages[1])
    return velvets, haases


def decorrelate_voice_pool(bank: Sequence, *, slots: int, in_channels: int = 2, max_frames_per_call: int = 4800,
                           fade_frames: Optional[int] = None, fade='linear'):
    """A voice pool: ``slots`` slots over a ``bank``, each slot a voice with a life of its own - it starts on any call
    with any entry of the bank, brings blocks of any size up to ``max_frames_per_call`` or none, ends on any call, and the
    slot goes to the next voice.  Where :func:`decorrelate_each_stream` advances a pool in lockstep from a position the
    host holds, the voice pool keeps one position per slot in the device state, so a call is a pure function of device
    memory and ``process_dev`` can be replayed from a captured graph.  Three kinds of bank:

    * all plain ``VelvetNoise`` (``normalizer=None``): a ``streaming.VoicePool`` (``vnd_voice_stream_f32_*``), float32
      out, ``latency_frames`` the bank's largest tap index.  The bank is deduplicated by content
      (``pool.bank_tables[bank_index]`` is the candidate ``process_dev`` names).
    * all ``HaasEffect``: a ``streaming.HaasVoicePool`` (``vnd_haas_voice_stream_f64_*``), float64 out, no latency, and a
      voice's end returns its own delay's tail, ``pool.bank_delays[bank_index]`` frames.
    * all ``SignalChain``, each exactly one ``VelvetNoise(normalizer=None)`` stage and then one ``HaasEffect`` stage (the
      chains are instantiated now): a ``streaming.ChainVoicePool``, both stages on the device, float64 out.

    ``pool.process({slot: block}, start={slot: bank_index}, end=[slot])`` takes float32 NumPy blocks and returns
    ``{slot: (n_out, 2)}``; ``pool.process_dev(...)`` takes device tensors of fixed shape and only enqueues.  For every
    voice the concatenation of its outputs equals ``bank[i].decorrelate(x_voice)`` - ``bank[i](x_voice)`` for a chain - bit
    for bit.  The velvet stages are checked as :func:`decorrelate_each_stream` checks its ``VelvetNoise`` list and the Haas
    stages as it checks its ``HaasEffect`` list, with the same exceptions before any device call; a mixed bank is a
    ``TypeError`` listing the types.  There is no host fallback: a stream has no host loop to fall back to.

    ``fade_frames`` (an int, with a bank of plain ``VelvetNoise`` only; ``ValueError`` for a Haas or chain bank) returns a
    ``streaming.FadeVoicePool`` (``vnd_voice_fade_stream_f32_dev``): ``pool.process(..., switch={slot: bank_index})`` moves a
    live voice to another bank entry, crossfaded over ``fade_frames`` frames from the first frame the slot has not yet
    returned.  ``fade`` names the gains (``streaming.fade_gains``): ``'linear'``, ``'equal_power'``, or a pair
    ``(fade_out, fade_in)`` of finite float32 arrays of length ``fade_frames``.  ``None`` returns the pools above.
    :func:`decorrelate_fade_voice_pool` is the entry for switchable pools of all three bank kinds."""
    from . import streaming
    bank = list(bank)
    if not bank:
        raise ValueError('decorrelate_voice_pool needs at least one decorrelator: a voice starts with a filter of the bank')
    kinds = {type(d) for d in bank}
    if kinds not in ({VelvetNoise}, {HaasEffect}, {SignalChain}):
        raise TypeError('decorrelate_voice_pool takes a bank of plain VelvetNoise decorrelators, of HaasEffect decorrelators '
                        'or of VelvetNoise -> HaasEffect SignalChains, got ' + ', '.join(sorted(k.__name__ for k in kinds)))
    if isinstance(in_channels, (bool, np.bool_)) or in_channels not in (1, 2):
        raise ValueError(f'in_channels must be 1 (mono, fanned out) or 2 (stereo), got {in_channels!r}')
    if fade_frames is not None and kinds != {VelvetNoise}:
        raise ValueError('decorrelate_voice_pool: fade_frames is taken with a bank of plain VelvetNoise decorrelators; Haas '
                         'and chain voices do not switch')
    if kinds == {VelvetNoise}:
        arrays, tables, ms_encode, width = _velvet_stream_bank(bank, 'decorrelate_voice_pool', 'bank entry')
        if fade_frames is not None:
            gains = streaming.fade_gains(fade_frames, fade)
            return streaming.FadeVoicePool(arrays, tables, slots=slots, in_channels=in_channels,
                                           max_frames_per_call=max_frames_per_call, fade_frames=fade_frames, fade_gains=gains,
                                           ms_encode=ms_encode, width=width)
        return streaming.VoicePool(arrays, tables, slots=slots, in_channels=in_channels,
                                   max_frames_per_call=max_frames_per_call, ms_encode=ms_encode, width=width)
    if kinds == {HaasEffect}:
        delayed_channel, ms_mode, width, delays = _haas_pool_settings(bank, 'decorrelate_voice_pool', 'bank entry')
        return streaming.HaasVoicePool(delays, slots=slots, in_channels=in_channels, max_frames_per_call=max_frames_per_call,
                                       delayed_channel=delayed_channel, ms_mode=ms_mode, width=width)
    velvets, haases = _chain_pool_stages(bank)
    arrays, tables, ms_encode, velvet_width = _velvet_stream_bank(velvets, 'decorrelate_voice_pool', 'bank entry')
    delayed_channel, ms_mode, haas_width, delays = _haas_pool_settings(haases, 'decorrelate_voice_pool', 'bank entry')
    return streaming.ChainVoicePool(arrays, tables, delays, slots=slots, in_channels=in_channels,
                                    max_frames_per_call=max_frames_per_call, ms_encode=ms_encode, velvet_width=velvet_width,
                                    delayed_channel=delayed_channel, ms_mode=ms_mode, haas_width=haas_width)


def decorrelate_fade_voice_pool(bank: Sequence, *, slots: int, in_channels: int = 2, max_frames_per_call: int = 4800,
                                fade_frames: int, fade='linear'):
    """A voice pool whose live voices can move to another entry of the ``bank`` without a click:
    ``pool.process(..., switch={slot: bank_index})`` crossfades a live voice over ``fade_frames`` frames from the first frame
    the slot has not yet returned, and ``process_dev`` takes ``streaming.VOICE_SWITCH`` in its flags.  The banks, their
    checks and their exceptions are :func:`decorrelate_voice_pool`'s; ``fade`` names the gains as there
    (``streaming.fade_gains``).

    * all plain ``VelvetNoise``: what ``decorrelate_voice_pool(..., fade_frames=fade_frames, fade=fade)`` returns, a
      ``streaming.FadeVoicePool``.
    * all ``HaasEffect``: a ``streaming.HaasFadeVoicePool`` (``vnd_haas_voice_fade_stream_f64_dev``): the delayed column
      fades from the old delay to the new one in float64 - what applies the result of
      ``optimization.optimize_haas_delay_batched`` to a voice that is running.
    * all ``VelvetNoise`` -> ``HaasEffect`` ``SignalChain``: a ``streaming.ChainFadeVoicePool``, both stages fading on the
      same gains from the same output frame.

    A voice that never switches returns the bytes of the pool :func:`decorrelate_voice_pool` builds on the same bank."""
    from . import streaming
    bank = list(bank)
    kinds = {type(d) for d in bank}
    if fade_frames is None:
        raise ValueError('decorrelate_fade_voice_pool: fade_frames must be an integer; decorrelate_voice_pool builds the '
                         'pools whose voices do not switch')
    if kinds not in ({HaasEffect}, {SignalChain}):            # a velvet bank, and every refusal of an empty or mixed one
        return decorrelate_voice_pool(bank, slots=slots, in_channels=in_channels, max_frames_per_call=max_frames_per_call,
                                      fade_frames=fade_frames, fade=fade)
    if isinstance(in_channels, (bool, np.bool_)) or in_channels not in (1, 2):
        raise ValueError(f'in_channels must be 1 (mono, fanned out) or 2 (stereo), got {in_channels!r}')
    gains = streaming.fade_gains(fade_frames, fade)
    if kinds == {HaasEffect}:
        delayed_channel, ms_mode, width, delays = _haas_pool_settings(bank, 'decorrelate_fade_voice_pool', 'bank entry')
        return streaming.HaasFadeVoicePool(delays, slots=slots, in_channels=in_channels,
                                           max_frames_per_call=max_frames_per_call, delayed_channel=delayed_channel,
                                           ms_mode=ms_mode, fade_frames=fade_frames, fade_gains=gains, width=width)
    velvets, haases = _chain_pool_stages(bank)
    arrays, tables, ms_encode, velvet_width = _velvet_stream_bank(velvets, 'decorrelate_fade_voice_pool', 'bank entry')
    delayed_channel, ms_mode, haas_width, delays = _haas_pool_settings(haases, 'decorrelate_fade_voice_pool', 'bank entry')
    return streaming.ChainFadeVoicePool(arrays, tables, delays, slots=slots, in_channels=in_channels,
                                        max_frames_per_call=max_frames_per_call, fade_frames=fade_frames, fade_gains=gains,
                                        ms_encode=ms_encode, velvet_width=velvet_width, delayed_channel=delayed_channel,
                                        ms_mode=ms_mode, haas_width=haas_width)


# ----------------------------------------------------------------------------
# SignalChain   (decorrelation.py:71-153)
# ----------------------------------------------------------------------------
class SignalChain:
    """Fluent, lazily-instantiated cascade of stages; ``chain(x)`` feeds each
    stage the previous stage's output.  ``device_resident=True`` (an extension) keeps the
    signal in HBM between stages that have a device form (``resident.py``)."""

    def __init__(self, *, sample_rate_hz: int, num_outs: int = 2, lazy: bool = True,
                 device_resident: bool = False, _hot: bool = False, _decorrelators=None):
        if _decorrelators is not None:
            raise TypeError(
                'Cannot supply decorrelators directly, use ``SignalChain.velvet_noise``,'
                ' ``SignalChain.haas_effect``, ``SignalChain.white_noise``, or ``SignalChain.stateless``.')
        self.sample_rate_hz = sample_rate_hz
        self.num_outs = num_outs
        self.lazy = lazy
        self.device_resident = bool(device_resident)
        self._resident_pool = None            # device buffers of a resident chain, reused from call to call
        self._hot = bool(_hot) or not lazy
        self._decorrelators: list = []

    def __repr__(self) -> str:
        return (f'SignalChain(sample_rate_hz={self.sample_rate_hz}, num_outs={self.num_outs}, '
                f'lazy={self.lazy}, stages={len(self._decorrelators)})')

    # ---- builders ------------------------------------------------------------
    def velvet_noise(self, **kwargs) -> 'SignalChain':
        return self._add(VelvetNoise, kwargs)

    def haas_effect(self, **kwargs) -> 'SignalChain':
        return self._add(HaasEffect, kwargs)

    def white_noise(self, **kwargs) -> 'SignalChain':
        return self._add(WhiteNoise, kwargs)

    def stateless(self, function: StatelessDecorrelator, *args, **kwargs) -> 'SignalChain':
        """``function`` is later called as ``function(*args, signal, **kwargs)`` -
        ``functools.partial`` semantics, positional extras BEFORE the signal,
        exactly as upstream (decorrelation.py:104-110)."""
        bound = partial(function, *args, **kwargs)
        self._decorrelators.append(bound if self._hot else (lambda: bound))
        return self

    def _add(self, cls, kwargs: dict) -> 'SignalChain':
        rate = kwargs.pop('sample_rate_hz', None)
        if rate is not None and rate != self.sample_rate_hz:
            raise TypeError(f'sample_rate_hz={rate} was supplied to {cls} but differs from the sample '
                            f'rate of the enclosing ``SignalChain`` ({self.sample_rate_hz})')
        params = dict(kwargs)
        params.setdefault('num_outs', self.num_outs)

        def make():
            return cls(sample_rate_hz=self.sample_rate_hz, **params)

        self._decorrelators.append(make() if self._hot else make)
        return self

    # ---- execution -----------------------------------------------------------
    def _init_decorrelators(self) -> None:
        if self._hot:
            return
        self._decorrelators = [factory() for factory in self._decorrelators]
        self._hot = True

    def stream(self, *, num_streams: int = 1, in_channels: int = 2, mode: int = MODE_EXACT,
               max_frames_per_call: int = 4800):
        """A chunked stream of the whole chain (``streaming.ChainStream``): a pool of ``num_streams`` signals of
        ``in_channels`` channels (1: a mono ``(n,)`` signal) fed block by block, every stage on the device.  The
        concatenation of every call's outputs equals ``chain(x)`` of the whole signal.  The stages are instantiated now and
        taken as they are; a stage without a stream form (a normaliser, ``WhiteNoise``, other callables) raises
        ``ValueError`` / ``TypeError`` naming it."""
        from . import streaming
        self._init_decorrelators()
        return streaming.ChainStream(list(self._decorrelators), num_streams=num_streams, in_channels=in_channels,
                                     mode=mode, max_frames_per_call=max_frames_per_call)

    def __call__(self, input_signal: NDArray) -> NDArray:
        self._init_decorrelators()
        if self.device_resident:
            from . import resident
            if self._resident_pool is None:
                self._resident_pool = resident.BufferPool()
            return resident.run(self._decorrelators, input_signal, self._resident_pool)
        signal = input_signal
        for stage in self._decorrelators:
            signal = stage(signal)
        return signal
