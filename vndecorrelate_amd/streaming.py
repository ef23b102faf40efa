"""Chunked streaming of the velvet-noise stage (``include/vnd_stream.h``).

The tap sum is anti-causal, ``y[n] = sum_k w_k * x[n + i_k]`` (decorrelation.py:656-658), so output frame ``n`` is
final once input frame ``n + H`` has arrived, ``H`` being the table's largest tap index.  A stream therefore has a
fixed latency of ``H`` frames: :meth:`Stream.process` takes the next block of every stream of a pool and returns the
output frames that became final, :meth:`Stream.flush` returns the rest, and the concatenation of everything returned
equals the one-shot call on the whole signal - bit for bit in ``MODE_EXACT`` and ``MODE_FMA``, within the fast mode's
tolerance in ``MODE_FAST``.

Two ways in:

* :func:`convolve_velvet_noise_stream` - ``convolve_velvet_noise`` on a float32 filter (the function path);
* ``VelvetNoise(..., normalizer=None).stream(...)`` - ``VelvetNoise.decorrelate`` (the class path): a mono input fanned
  out to stereo, the side-channel encode of MS mode and the width ride in the kernel's store phase.

NumPy chunks in give NumPy arrays out, synchronously (``vnd_stream_f32_host``).  torch device tensors in give device
tensors out, enqueued on the current stream (``vnd_stream_f32_dev``), with no host copy.  The per-stream state is a
ring of the last input frames in device memory (torch).  Every argument and shape check runs here, before any device
call.  The calls are not graph-capturable: the stream position is a kernel argument.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _native
from .taps import TapArrays, function_path_arrays

MODES = (_native.MODE_EXACT, _native.MODE_FMA, _native.MODE_FAST)


def output_span(position: int, n_in: int, latency: int, final: bool) -> Tuple[int, int]:
    """``(E, E')``: the output frames ``[E, E')`` of a call that pushes ``n_in`` frames at ``position``
    (frames pushed before it) into a stream of latency ``latency`` (``include/vnd_stream.h``)."""
    first = max(0, position - latency)
    end = position + n_in if final else max(0, position + n_in - latency)
    return first, end


def _is_torch(x) -> bool:
    return type(x).__module__.split('.')[0] == 'torch'


class Stream:
    """A pool of ``num_streams`` streams through one tap table, advancing in lockstep.

    ``process(x)``: ``x`` is ``(B, in_channels)`` (a pool of one stream; ``(B,)`` as well when ``in_channels == 1``) or
    ``(num_streams, B, in_channels)``, with ``0 <= B <= max_frames_per_call`` free to change from call to call; returns
    ``(n_out, C)`` or ``(num_streams, n_out, C)``.  ``flush()``: the remaining frames; ``process`` raises ``RuntimeError``
    after it until ``reset()``.  ``latency_frames``: ``H``.  Nothing touches the device until frames need computing."""

    def __init__(self, arrays: TapArrays, *, num_streams: int, in_channels: int, mode: int, max_frames_per_call: int,
                 ms_encode: bool = False, width: Optional[float] = None, any_dtype: bool = False,
                 one_shot: str = 'convolve_velvet_noise'):
        for name, v in (('num_streams', num_streams), ('in_channels', in_channels),
                        ('max_frames_per_call', max_frames_per_call)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f'{name} must be a positive integer, got {v!r}')
        if num_streams > _native.MAX_STREAMS_PER_CALL:
            raise ValueError(f'num_streams {num_streams} above {_native.MAX_STREAMS_PER_CALL}: split the pool')
        if mode not in MODES:
            raise ValueError(f'unknown mode {mode!r}')
        channels = arrays.num_channels
        if channels < 1 or channels % in_channels:
            raise ValueError(f'{in_channels} input channels do not divide the table\'s {channels} channels')
        if (ms_encode or width is not None) and channels != 2:
            raise ValueError('the side-channel encode and the width need 2 output channels, '
                             f'the table has {channels}')
        self.arrays = arrays
        self.num_streams, self.in_channels, self.num_channels = int(num_streams), int(in_channels), channels
        self.mode, self.max_frames_per_call = int(mode), int(max_frames_per_call)
        self.ms_encode, self.width = bool(ms_encode), width
        self.latency_frames = int(arrays.tap_index.max()) if len(arrays.tap_index) else 0
        self._any_dtype, self._one_shot = any_dtype, one_shot
        self._table = None
        self._state = None            # (torch uint8 tensor, bytes)
        self._pending = None          # torch stream of the last device call (a host call waits for it)
        self._torch_out = False       # the last process() took a torch tensor: flush() answers in kind
        self.position = 0
        self.flushed = False

    # ---- public ------------------------------------------------------------------------
    def process(self, x):
        """Push the next block of every stream; returns the outputs that became final."""
        if self.flushed:
            raise RuntimeError('process() after flush(): call reset() to start a new signal')
        x3, squeeze, is_torch = self._chunk(x)
        self._torch_out = is_torch
        return self._call(x3, is_torch, squeeze, final=False)

    def flush(self):
        """The outputs still held back (the last ``latency_frames`` of every stream, or fewer); ends the signal."""
        if self.flushed:
            raise RuntimeError('flush() after flush(): call reset() to start a new signal')
        return self._call(None, self._torch_out, self.num_streams == 1 and self._squeeze_last, final=True)

    def reset(self):
        """Start a new signal at position 0 (the state needs no clearing: it is never read before it is written)."""
        self.position = 0
        self.flushed = False

    _squeeze_last = True

    # ---- checks --------------------------------------------------------------------------
    def _chunk(self, x):
        is_torch = _is_torch(x)
        if is_torch:
            import torch
            if not x.is_cuda:
                raise ValueError('a torch chunk must be a device tensor (NumPy arrays take the host path)')
            if x.dtype != torch.float32:
                if x.dtype in (torch.float64, torch.int32, torch.int64) and not self._any_dtype:
                    raise TypeError(f'a {x.dtype} signal is multiplied in float64 by the one-shot {self._one_shot}; '
                                    'streaming takes float32 (or int16) chunks: use the one-shot call for it')
                if x.dtype.is_complex:
                    raise TypeError(f'complex chunks are not signals: {x.dtype}')
                x = x.to(torch.float32)
        else:
            x = np.asarray(x)
            if x.dtype != np.float32:
                if x.dtype.kind not in 'biuf':
                    raise TypeError(f'chunks must be real numbers, got {x.dtype}')
                if not self._any_dtype and np.result_type(x.dtype, np.float32) != np.float32:
                    raise TypeError(f'a {x.dtype} signal is multiplied in float64 by the one-shot {self._one_shot} '
                                    '(vnd_convolve_promote_host); streaming takes float32 (or int16) chunks: '
                                    'use the one-shot call for it')
                x = x.astype(np.float32)
        shape = tuple(x.shape)
        S, cx = self.num_streams, self.in_channels
        if len(shape) == 1 and S == 1 and cx == 1:
            x3, squeeze = x.reshape(1, shape[0], 1), True
        elif len(shape) == 2 and S == 1:
            x3, squeeze = x.reshape(1, shape[0], shape[1]), True
        elif len(shape) == 3:
            x3, squeeze = x, False
        else:
            raise ValueError(f'chunk of shape {shape}: expected (num_streams={S}, frames, {cx})'
                             + (f' or (frames, {cx})' if S == 1 else ''))
        if x3.shape[0] != S or x3.shape[2] != cx:
            raise ValueError(f'chunk of shape {shape} does not match the pool: {S} streams of {cx} channels')
        if x3.shape[1] > self.max_frames_per_call:
            raise ValueError(f'{x3.shape[1]} frames in one call, above max_frames_per_call={self.max_frames_per_call}')
        self._squeeze_last = squeeze
        return x3, squeeze, is_torch

    # ---- the device -------------------------------------------------------------------------
    def _ensure(self, torch, device_index: int):
        if self._table is None:
            a = self.arrays
            self._table = _native.TapTable.create(_native.default_context(), a.tap_offsets, a.tap_index, a.tap_weight,
                                                  **a.kwargs())
        if self._state is None:
            need = ctypes.c_int64()
            _native._check(self._table._lib.vnd_stream_state_bytes(self._table.handle, self.num_streams, self.in_channels,
                                                                   self.max_frames_per_call, ctypes.byref(need)),
                           'vnd_stream_state_bytes')
            buf = torch.empty((max(need.value, 1),), dtype=torch.uint8, device=torch.device('cuda', device_index))
            self._state = (buf, need.value)
        return self._table, self._state

    def _call(self, x3, is_torch: bool, squeeze: bool, final: bool):
        n_in = 0 if x3 is None else int(x3.shape[1])
        first, end = output_span(self.position, n_in, self.latency_frames, final)
        n_out = end - first
        S, C = self.num_streams, self.num_channels
        if n_in == 0 and n_out == 0:                      # nothing to compute or to keep: no device call
            out = self._empty(is_torch, x3)
        elif is_torch:
            out = self._call_device(x3, n_in, n_out, final)
        else:
            out = self._call_host(x3, n_in, n_out, final)
        self.position += n_in
        if final:
            self.flushed = True
        return out[0] if squeeze else out

    def _empty(self, is_torch: bool, x3):
        shape = (self.num_streams, 0, self.num_channels)
        if is_torch:
            import torch
            device = x3.device if x3 is not None else torch.device('cuda', _native.default_context().device)
            return torch.empty(shape, dtype=torch.float32, device=device)
        return np.zeros(shape, np.float32)

    def _tail(self, n_in: int, final: bool):
        return (self.num_streams, self.position, n_in, self.in_channels, int(final), self.mode, int(self.ms_encode),
                int(self.width is not None), float(self.width or 0.0))

    def _call_host(self, x3, n_in: int, n_out: int, final: bool):
        from .resident import _torch
        torch = _torch()
        ctx = _native.default_context()
        table, (state, state_bytes) = self._ensure(torch, ctx.device)
        if self._pending is not None:                     # a device call of this stream may still run on its stream
            self._pending.synchronize()
            self._pending = None
        x = np.ascontiguousarray(x3, np.float32) if x3 is not None else np.zeros((self.num_streams, 0, self.in_channels),
                                                                                 np.float32)
        y = np.empty((self.num_streams, n_out, self.num_channels), np.float32)
        got = ctypes.c_int64()
        _native._check(table._lib.vnd_stream_f32_host(
            ctx.handle, table.handle, ctypes.c_void_p(state.data_ptr()), state_bytes, self.max_frames_per_call,
            ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(y.ctypes.data), *self._tail(n_in, final), ctypes.byref(got)),
            'vnd_stream_f32_host')
        assert got.value == n_out, (got.value, n_out)
        return y

    def _call_device(self, x3, n_in: int, n_out: int, final: bool):
        from .resident import _torch
        torch = _torch()
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        if x3 is not None and x3.device != device:
            raise ValueError(f'chunk on {x3.device}, the stream runs on {device}')
        table, (state, state_bytes) = self._ensure(torch, ctx.device)
        stream = torch.cuda.current_stream(device)
        x = x3.contiguous() if x3 is not None else torch.empty((self.num_streams, 0, self.in_channels),
                                                               dtype=torch.float32, device=device)
        y = torch.empty((self.num_streams, n_out, self.num_channels), dtype=torch.float32, device=device)
        got = ctypes.c_int64()
        _native._check(table._lib.vnd_stream_f32_dev(
            ctx.handle, table.handle, ctypes.c_void_p(state.data_ptr()), state_bytes, self.max_frames_per_call,
            ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), *self._tail(n_in, final), ctypes.byref(got),
            ctypes.c_void_p(stream.cuda_stream)), 'vnd_stream_f32_dev')
        assert got.value == n_out, (got.value, n_out)
        if x.numel():
            x.record_stream(stream)
        state.record_stream(stream)
        self._pending = stream
        return y


def convolve_velvet_noise_stream(velvet_noise_filters, *, num_streams: int = 1, in_channels: Optional[int] = None,
                                 mode: int = _native.MODE_EXACT, max_frames_per_call: int = 4800) -> Stream:
    """A :class:`Stream` of ``convolve_velvet_noise(x, velvet_noise_filters)``: the concatenated outputs of every stream
    equal the one-shot call on its whole signal.  ``velvet_noise_filters``: a float32 ``(L, C)`` (or ``(L,)``) FIR, as
    ``generate_velvet_noise`` makes it.  ``in_channels`` (default C): as in ``convolve_velvet_noise``, a one-channel
    signal goes through the filter's first column only, a wider one must match the filter's columns.

    A float64 filter raises ``TypeError``, and so do float64 and int32 / int64 chunks: NumPy multiplies those in float64,
    which the one-shot call repeats through its promoting kernel and the stream does not."""
    if _is_torch(velvet_noise_filters):
        raise TypeError('the filter is a host array (NumPy), as for convolve_velvet_noise')
    fir = np.asarray(velvet_noise_filters)
    if fir.dtype != np.float32:
        raise TypeError(f'a {fir.dtype} filter is multiplied in float64 by the one-shot convolve_velvet_noise '
                        '(vnd_convolve_promote_host); streaming takes a float32 filter: use the one-shot call for it')
    if fir.ndim == 1:
        fir = fir[:, None]
    if fir.ndim != 2 or fir.shape[1] < 1:
        raise ValueError(f'expected a (L, C) filter, got shape {fir.shape}')
    channels = fir.shape[1] if in_channels is None else in_channels
    if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or channels < 1:
        raise ValueError(f'in_channels must be a positive integer, got {in_channels!r}')
    if channels > 1 and channels != fir.shape[1]:
        raise ValueError('Input length mismatch: Expected signals of equal length, but got lengths '
                         f'{channels} and {fir.shape[1]} for dimension 1.')
    return Stream(function_path_arrays(fir, channels), num_streams=num_streams, in_channels=channels, mode=mode,
                  max_frames_per_call=max_frames_per_call)
