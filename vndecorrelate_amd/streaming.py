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

Two more stream forms build on it: :class:`HaasStream` (``HaasEffect(...).stream(...)``, ``include/vnd_haas_stream.h``),
the causal Haas delay with no latency and a tail of ``d`` frames, and :class:`ChainStream` (``SignalChain(...).stream(...)``),
every stage of a chain on the device, block by block.  :class:`EachStream` and :class:`HaasEachStream`
(``decorrelate_each_stream``, ``include/vnd_each_stream.h``) run every stream of a pool through its own filter of a bank
or its own delay, one launch per call for the whole pool.  :class:`VoicePool` (``decorrelate_voice_pool``,
``include/vnd_voice_stream.h``) is that pool with the position of every slot in the device state: voices start, end and
bring their own block sizes call by call, and ``process_dev`` can be captured in a graph.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Optional, Tuple

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


def _check_counts(**counts):
    """Each of ``counts`` (in order) a positive integer, else ``ValueError`` naming it."""
    for name, v in counts.items():
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f'{name} must be a positive integer, got {v!r}')


class BlockStream:
    """What every block stream shares: a pool of ``num_streams`` streams advancing in lockstep, ``0 <= B <=
    max_frames_per_call`` frames per call; ``process`` returns the outputs that became final, ``flush()`` the rest and
    ends the signal (``process`` raises ``RuntimeError`` after it until ``reset()``), answering in kind - a device tensor
    after a device block, unbatched after an unbatched one.  The state lives in device memory (torch), allocated on first
    use.  Every device call of a stream is ordered after its previous one, whatever torch stream each runs on; a host
    call waits for a pending device call.

    A subclass gives its block rules (``_chunk``: ``(block, squeeze, is_torch)``), its
    output span (``_span``), dtype (``_out_dtype``) and width (``_out_width``), its state size (``_state_bytes``), its
    native device call (``_launch``) and its host path (``_call_host``)."""

    _out_dtype = np.float32
    _noun = 'chunk'                   # what the error messages call one call's input
    _squeeze_last = True

    def __init__(self, **counts):
        """``counts``: ``num_streams``, ``max_frames_per_call`` and the stream's other sizes, each a positive integer."""
        _check_counts(**counts)
        for name, v in counts.items():
            setattr(self, name, int(v))
        if self.num_streams > _native.MAX_STREAMS_PER_CALL:
            raise ValueError(f'num_streams {self.num_streams} above {_native.MAX_STREAMS_PER_CALL}: split the pool')
        self._state = None            # (torch uint8 tensor, bytes)
        self._last_stream = None      # torch stream of the last device call: the next call is ordered after it
        self._torch_out = False       # the last process() took a device tensor: flush() answers in kind
        self.position = 0
        self.flushed = False

    # ---- public ------------------------------------------------------------------------
    def flush(self):
        """The outputs still held back; ends the signal."""
        if self.flushed:
            raise RuntimeError('flush() after flush(): call reset() to start a new signal')
        return self._push(None, self._torch_out, self.num_streams == 1 and self._squeeze_last, final=True)

    def reset(self):
        """Start a new signal at position 0 (the state needs no clearing: it is never read before it is written)."""
        self.position = 0
        self.flushed = False

    # ---- the lifecycle -----------------------------------------------------------------------
    def _process(self, args, final: bool):
        if self.flushed:
            raise RuntimeError('process() after flush(): call reset() to start a new signal')
        block, squeeze, is_torch = self._chunk(*args)
        self._squeeze_last, self._torch_out = squeeze, is_torch
        return self._push(block, is_torch, squeeze, final)

    def _push(self, block, on_device: bool, squeeze: bool, final: bool):
        """One checked block (None: no frames) through the stream, on the device or the host."""
        lead = None if block is None else self._lead(block)
        n_in = 0 if lead is None else int(lead.shape[1])
        first, end = self._span(n_in, final)
        if n_in == 0 and end == first:                    # nothing to compute or to keep: no device call
            out = self._empty(on_device, lead)
        elif on_device:
            out = self._call_device(block, n_in, end - first, final)
        else:
            out = self._call_host(block, n_in, end - first, final)
        self.position += n_in
        if final:
            self.flushed = True
        return out[0] if squeeze else out

    def _lead(self, block):
        """The array of a block that carries its frame count and device."""
        return block

    def _empty(self, on_device: bool, lead):
        shape = (self.num_streams, 0, self._out_width)
        if on_device:
            torch = _native.torch_module()
            device = lead.device if lead is not None else torch.device('cuda', _native.default_context().device)
            return torch.empty(shape, dtype=getattr(torch, self._out_dtype.__name__), device=device)
        return np.zeros(shape, self._out_dtype)

    # ---- the device -------------------------------------------------------------------------
    def _ensure_state(self, torch, ctx):
        if self._state is None:
            need = self._state_bytes(ctx)
            buf = torch.empty((max(need, 1),), dtype=torch.uint8, device=torch.device('cuda', ctx.device))
            self._state = (buf, need)
        return self._state

    def _wait_for_last(self):
        """A host call: wait for this stream's pending device call."""
        if self._last_stream is not None:
            self._last_stream.synchronize()
            self._last_stream = None

    def _call_device(self, block, n_in: int, n_out: int, final: bool):
        torch = _native.torch_module()
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        lead = None if block is None else self._lead(block)
        if lead is not None and lead.device != device:
            raise ValueError(f'{self._noun} on {lead.device}, the stream runs on {device}')
        state, state_bytes = self._ensure_state(torch, ctx)
        stream = torch.cuda.current_stream(device)
        last = self._last_stream
        if last is not None and last.cuda_stream != stream.cuda_stream:
            stream.wait_stream(last)                      # the state is read and written in call order
        out = torch.empty((self.num_streams, n_out, self._out_width), dtype=getattr(torch, self._out_dtype.__name__),
                          device=device)
        got, read = self._launch(torch, ctx, state, state_bytes, block, out, n_in, final, stream)
        assert got == n_out, (got, n_out)
        for t in read:
            if t.numel():
                t.record_stream(stream)
        state.record_stream(stream)
        self._last_stream = stream
        return out


class Stream(BlockStream):
    """A pool of ``num_streams`` streams through one tap table, advancing in lockstep.

    ``process(x)``: ``x`` is ``(B, in_channels)`` (a pool of one stream; ``(B,)`` as well when ``in_channels == 1``) or
    ``(num_streams, B, in_channels)``, with ``0 <= B <= max_frames_per_call`` free to change from call to call; returns
    ``(n_out, C)`` or ``(num_streams, n_out, C)``.  ``flush()``: the remaining frames; ``process`` raises ``RuntimeError``
    after it until ``reset()``.  ``latency_frames``: ``H``.  Nothing touches the device until frames need computing.
    Every device call is ordered after the stream's previous call, whatever torch stream each one runs on."""

    _host_entry, _dev_entry = 'vnd_stream_f32_host', 'vnd_stream_f32_dev'

    def __init__(self, arrays: TapArrays, *, num_streams: int, in_channels: int, mode: int, max_frames_per_call: int,
                 ms_encode: bool = False, width: Optional[float] = None, any_dtype: bool = False,
                 one_shot: str = 'convolve_velvet_noise'):
        super().__init__(num_streams=num_streams, in_channels=in_channels, max_frames_per_call=max_frames_per_call)
        if mode not in MODES:
            raise ValueError(f'unknown mode {mode!r}')
        channels = arrays.num_channels
        if channels < 1 or channels % in_channels:
            raise ValueError(f'{in_channels} input channels do not divide the table\'s {channels} channels')
        if (ms_encode or width is not None) and channels != 2:
            raise ValueError('the side-channel encode and the width need 2 output channels, '
                             f'the table has {channels}')
        self.arrays, self.num_channels, self.mode = arrays, channels, int(mode)
        self.ms_encode, self.width = bool(ms_encode), width
        self.latency_frames = int(arrays.tap_index.max()) if len(arrays.tap_index) else 0
        self._any_dtype, self._one_shot = any_dtype, one_shot
        self._table = None

    @property
    def _out_width(self) -> int:
        return self.num_channels

    def process(self, x, *, final: bool = False):
        """Push the next block of every stream; returns the outputs that became final.  ``final=True``: ``x`` is the last
        block, and the outputs ``flush()`` would return come with it, in one device call; the signal ends."""
        return self._process((x,), bool(final))

    # ---- checks --------------------------------------------------------------------------
    def _chunk(self, x):
        is_torch = _native.is_torch(x)
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
        return x3, squeeze, is_torch

    # ---- the native entries ------------------------------------------------------------------
    def _span(self, n_in: int, final: bool) -> Tuple[int, int]:
        return output_span(self.position, n_in, self.latency_frames, final)

    def _head(self, ctx):
        """The native entries' arguments before the state (the table is made with the state)."""
        return ctx.handle, self._table.handle

    def _tail(self, n_in: int, final: bool):
        """The native entries' arguments after the output pointer."""
        return (self.num_streams, self.position, n_in, self.in_channels, int(final), self.mode, int(self.ms_encode),
                int(self.width is not None), float(self.width or 0.0))

    def _state_bytes(self, ctx) -> int:
        a = self.arrays
        self._table = _native.TapTable.create(ctx, a.tap_offsets, a.tap_index, a.tap_weight, **a.kwargs())
        need = ctypes.c_int64()
        _native._check(ctx._lib.vnd_stream_state_bytes(self._table.handle, self.num_streams, self.in_channels,
                                                       self.max_frames_per_call, ctypes.byref(need)),
                       'vnd_stream_state_bytes')
        return need.value

    def _entry(self, ctx, name: str, state, state_bytes: int, x_ptr: int, y_ptr: int, n_in: int, final: bool, *stream):
        got = ctypes.c_int64()
        _native._check(getattr(ctx._lib, name)(
            *self._head(ctx), ctypes.c_void_p(state.data_ptr()), state_bytes, self.max_frames_per_call,
            ctypes.c_void_p(x_ptr), ctypes.c_void_p(y_ptr), *self._tail(n_in, final), ctypes.byref(got), *stream), name)
        return got.value

    def _call_host(self, x3, n_in: int, n_out: int, final: bool):
        ctx = _native.default_context()
        state, state_bytes = self._ensure_state(_native.torch_module(), ctx)
        self._wait_for_last()
        x = np.ascontiguousarray(x3, np.float32) if x3 is not None else np.zeros((self.num_streams, 0, self.in_channels),
                                                                                 np.float32)
        y = np.empty((self.num_streams, n_out, self.num_channels), self._out_dtype)
        got = self._entry(ctx, self._host_entry, state, state_bytes, x.ctypes.data, y.ctypes.data, n_in, final)
        assert got == n_out, (got, n_out)
        return y

    def _launch(self, torch, ctx, state, state_bytes: int, x3, y, n_in: int, final: bool, stream):
        x = x3.contiguous() if x3 is not None else torch.empty((self.num_streams, 0, self.in_channels),
                                                               dtype=torch.float32, device=y.device)
        got = self._entry(ctx, self._dev_entry, state, state_bytes, x.data_ptr(), y.data_ptr(), n_in, final,
                          ctypes.c_void_p(stream.cuda_stream))
        return got, (x,)


def convolve_velvet_noise_stream(velvet_noise_filters, *, num_streams: int = 1, in_channels: Optional[int] = None,
                                 mode: int = _native.MODE_EXACT, max_frames_per_call: int = 4800) -> Stream:
    """A :class:`Stream` of ``convolve_velvet_noise(x, velvet_noise_filters)``: the concatenated outputs of every stream
    equal the one-shot call on its whole signal.  ``velvet_noise_filters``: a float32 ``(L, C)`` (or ``(L,)``) FIR, as
    ``generate_velvet_noise`` makes it.  ``in_channels`` (default C): as in ``convolve_velvet_noise``, a one-channel
    signal goes through the filter's first column only, a wider one must match the filter's columns.

    A float64 filter raises ``TypeError``, and so do float64 and int32 / int64 chunks: NumPy multiplies those in float64,
    which the one-shot call repeats through its promoting kernel and the stream does not."""
    if _native.is_torch(velvet_noise_filters):
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


def haas_output_span(position: int, n_in: int, delay: int, final: bool) -> Tuple[int, int]:
    """``(E, E')`` of a call of a Haas stream (``include/vnd_haas_stream.h``): the delay is causal, so a call returns the
    frames it pushed, and the final call the ``delay`` tail frames as well."""
    return position, position + n_in + (delay if final else 0)


class HaasStream(Stream):
    """A pool of ``num_streams`` streams through one ``HaasEffect``, advancing in lockstep (``HaasEffect.stream``).

    The same interface as :class:`Stream`; ``latency_frames`` is 0 (the delay is causal) and ``tail_frames`` is the delay
    ``d``: the final call returns ``d`` frames more than it was given, so the concatenation is ``n + d`` frames, float64
    ``(..., 2)``, bit-identical to ``HaasEffect.decorrelate`` of the whole signal.  ``in_channels``: 2, or 1 for a mono
    ``(n,)`` signal.  Chunks of any real dtype are cast to float32 first, as ``decorrelate`` casts its input."""

    _out_dtype = np.float64
    _host_entry, _dev_entry = 'vnd_haas_stream_f64_host', 'vnd_haas_stream_f64_dev'
    _any_dtype, _one_shot = True, 'HaasEffect.decorrelate'
    num_channels = 2

    def __init__(self, *, num_streams: int, in_channels: int, max_frames_per_call: int, delay: int,
                 delayed_channel: int, ms_mode: bool, width: Optional[float]):
        BlockStream.__init__(self, num_streams=num_streams, in_channels=in_channels,
                             max_frames_per_call=max_frames_per_call)
        if in_channels not in (1, 2):
            raise ValueError(f'HaasEffect streams a mono (1) or stereo (2) signal, got in_channels={in_channels}')
        self.delay, self.delayed_channel, self.ms_mode, self.width = int(delay), int(delayed_channel), bool(ms_mode), width
        self.latency_frames, self.tail_frames = 0, self.delay

    def _span(self, n_in: int, final: bool) -> Tuple[int, int]:
        return haas_output_span(self.position, n_in, self.delay, final)

    def _head(self, ctx):
        return (ctx.handle,)

    def _tail(self, n_in: int, final: bool):
        return (self.num_streams, self.position, n_in, self.in_channels, int(final), self.delay, self.delayed_channel,
                int(self.ms_mode), int(self.width is not None), float(self.width or 0.0))

    def _state_bytes(self, ctx) -> int:
        need = ctypes.c_int64()
        _native._check(ctx._lib.vnd_haas_stream_state_bytes(self.num_streams, self.in_channels, self.delay,
                                                            self.max_frames_per_call, ctypes.byref(need)),
                       'vnd_haas_stream_state_bytes')
        return need.value


class _PerStream:
    """What the two per-stream forms share: one int32 value per stream (a table index, a delay) that the device entry
    reads from device memory and the host entry from host memory.  The device copy goes up once, with the state, and
    lives as long as the stream."""

    def _set_each(self, values):
        self._each_host = np.ascontiguousarray(values, np.int32)
        self._each_dev = None
        self._each_ptr = None

    def _upload_each(self, ctx):
        torch = _native.torch_module()
        self._each_dev = torch.from_numpy(self._each_host).to(torch.device('cuda', ctx.device))

    def _entry(self, ctx, name: str, *args):
        self._each_ptr = self._each_host.ctypes.data if name == self._host_entry else self._each_dev.data_ptr()
        return super()._entry(ctx, name, *args)


class EachStream(_PerStream, Stream):
    """A pool whose stream ``b`` runs through its own velvet-noise filter of a bank (``decorrelate_each_stream``).

    The same interface as :class:`Stream`.  The pool advances in lockstep at one latency, ``latency_frames`` = the bank's
    largest tap index: a stream whose own filter is shorter waits with the others.  For every stream the concatenation of
    everything returned equals ``decorrelators[b].decorrelate(x_b)`` on the whole signal bit for bit, float32
    ``(num_streams, n, 2)``.  ``tables`` is the int32 index of every stream's candidate in ``arrays``, a
    ``class_path_bank_arrays`` bank.  Always ``MODE_EXACT``.  One kernel launch per call (``vnd_each_stream_f32_*``)."""

    _host_entry, _dev_entry = 'vnd_each_stream_f32_host', 'vnd_each_stream_f32_dev'
    num_channels = 2

    def __init__(self, arrays: TapArrays, tables, *, in_channels: int, max_frames_per_call: int, ms_encode: bool = False,
                 width: Optional[float] = None):
        BlockStream.__init__(self, num_streams=len(tables), in_channels=in_channels,
                             max_frames_per_call=max_frames_per_call)
        if in_channels not in (1, 2):
            raise ValueError(f'a pool of mono (1) or stereo (2) streams is taken, got in_channels={in_channels}')
        if arrays.num_channels < 2 or arrays.num_channels % 2:
            raise ValueError(f'a bank holds stereo pairs: this one has {arrays.num_channels} channels')
        self._set_each(tables)
        if self._each_host.min() < 0 or self._each_host.max() >= arrays.num_channels // 2:
            raise ValueError(f'table indices outside [0, {arrays.num_channels // 2})')
        self.arrays, self.tables, self.mode = arrays, self._each_host, _native.MODE_EXACT
        self.ms_encode, self.width = bool(ms_encode), width
        self.latency_frames = int(arrays.tap_index.max()) if len(arrays.tap_index) else 0
        self._any_dtype, self._one_shot = True, 'VelvetNoise.decorrelate'
        self._table = None

    def _head(self, ctx):
        return ctx.handle, self._table.handle, ctypes.c_void_p(self._each_ptr)

    def _state_bytes(self, ctx) -> int:
        from . import decorrelation
        self._table = decorrelation._each_banks.get(ctx, self.arrays)
        self._upload_each(ctx)
        return _native.each_stream_state_bytes(self._table, self.num_streams, self.in_channels, self.max_frames_per_call)


class HaasEachStream(_PerStream, HaasStream):
    """A pool whose stream ``b`` is delayed by its own ``delays[b]`` frames (``decorrelate_each_stream``).

    The same interface as :class:`HaasStream`; ``latency_frames`` is 0 and ``tail_frames`` the largest delay: the final
    call returns that many frames more than it was given.  ``tail_frames_each`` is the int array of the streams' own
    delays: stream ``b``'s signal is the first ``n + tail_frames_each[b]`` frames of its concatenation - bit-identical to
    ``decorrelators[b].decorrelate(x_b)`` - and the rest is zeros.  One kernel launch per call
    (``vnd_haas_each_stream_f64_*``)."""

    _host_entry, _dev_entry = 'vnd_haas_each_stream_f64_host', 'vnd_haas_each_stream_f64_dev'

    def __init__(self, delays, *, in_channels: int, max_frames_per_call: int, delayed_channel: int, ms_mode: bool,
                 width: Optional[float]):
        self._set_each(delays)
        if self._each_host.ndim != 1 or not self._each_host.size or self._each_host.min() < 0:
            raise ValueError('delays: one delay >= 0 per stream')
        HaasStream.__init__(self, num_streams=len(self._each_host), in_channels=in_channels,
                            max_frames_per_call=max_frames_per_call, delay=int(self._each_host.max()),
                            delayed_channel=delayed_channel, ms_mode=ms_mode, width=width)
        self.tail_frames_each = self._each_host.astype(np.int64)

    def _tail(self, n_in: int, final: bool):
        return (self.num_streams, self.position, n_in, self.in_channels, int(final), ctypes.c_void_p(self._each_ptr),
                self.delay, self.delayed_channel, int(self.ms_mode), int(self.width is not None), float(self.width or 0.0))

    def _state_bytes(self, ctx) -> int:
        self._upload_each(ctx)
        return _native.haas_each_stream_state_bytes(self.num_streams, self.in_channels, self.delay, self.max_frames_per_call)


class StagePlan(NamedTuple):
    """How :class:`ChainStream` runs one stage: ``kind`` ('velvet', 'haas' or 'convolve'), the channels it is fed, the dtype
    it is handed (None: the caller's chunk, cast as that stage casts it; 'float64': a Haas output, cast to float32 on the
    device), the most frames one of its calls takes, and its latency and tail in frames."""
    kind: str
    in_channels: int
    in_dtype: Optional[str]
    max_frames_per_call: int
    latency_frames: int
    tail_frames: int


class ChainStream:
    """A pool of ``num_streams`` streams through every stage of a ``SignalChain`` (``SignalChain.stream``).

    ``process(x)`` takes the next block, as :meth:`Stream.process` does, and runs every stage on the device, in order, on
    the current stream; ``flush()`` hands each stage's remaining frames to the next one as that stage's final block.  The
    concatenation of everything returned equals ``chain(x)`` on the whole signal (bit for bit in ``MODE_EXACT`` and
    ``MODE_FMA``): ``n + tail_frames`` frames, ``latency_frames`` behind the input.  A NumPy block makes one upload and one
    download (``transfers`` counts those of the last call); a torch device block makes none and does not synchronise.

    Stages: ``VelvetNoise`` with ``normalizer=None``, a covered ``HaasEffect`` (``optimization.haas_scan_covers``),
    ``stateless(convolve_velvet_noise, velvet_noise_filters=<float32 FIR>)`` fed float32 or int16.  Anything else -
    normalisers, ``WhiteNoise``, other callables, channel counts or dtypes the one-shot chain treats otherwise - raises
    ``ValueError`` / ``TypeError`` naming the stage, here, before any device call."""

    def __init__(self, stages, *, num_streams: int = 1, in_channels: int = 2, mode: int = _native.MODE_EXACT,
                 max_frames_per_call: int = 4800):
        _check_counts(num_streams=num_streams, in_channels=in_channels, max_frames_per_call=max_frames_per_call)
        if mode not in MODES:
            raise ValueError(f'unknown mode {mode!r}')
        if not stages:
            raise ValueError('a chain stream needs at least one stage')
        self.num_streams, self.in_channels, self.mode = int(num_streams), int(in_channels), int(mode)
        self.max_frames_per_call = int(max_frames_per_call)
        self.streams, self.plan = [], []
        channels, one_d, dtype, final_frames = self.in_channels, self.in_channels == 1, None, 0
        for index, stage in enumerate(stages):
            frames = max(self.max_frames_per_call, final_frames)    # a final call takes the previous stage's tail
            try:
                kind, stream = self._stage_stream(stage, channels, one_d, dtype, frames)
            except (ValueError, TypeError) as exc:
                raise type(exc)(f'stage {index} ({type(stage).__name__}): {exc}') from exc
            tail = stream.tail_frames if kind == 'haas' else 0
            self.plan.append(StagePlan(kind, channels, dtype, frames, stream.latency_frames, tail))
            self.streams.append(stream)
            final_frames += stream.latency_frames + tail        # a final call returns n_in + H (or n_in + d) frames
            channels, one_d, dtype = stream.num_channels, False, ('float64' if kind == 'haas' else 'float32')
        self.num_channels = channels
        self.latency_frames = sum(p.latency_frames for p in self.plan)
        self.tail_frames = sum(p.tail_frames for p in self.plan)
        self.transfers = {'to_device': 0, 'to_host': 0}
        self._torch_out = False
        self._squeeze = self.num_streams == 1
        self.position = 0
        self.flushed = False

    def _stage_stream(self, stage, channels: int, one_d: bool, dtype: Optional[str], frames: int):
        from functools import partial
        from . import decorrelation as dec
        from . import optimization
        S = self.num_streams
        if isinstance(stage, dec.VelvetNoise):
            if not one_d and channels != stage.num_outs:
                raise ValueError(f'a stage of {stage.num_outs} outputs is fed {channels} channels: the one-shot chain '
                                 f'convolves its first {stage.num_outs} columns, which a stream does not')
            return 'velvet', stage.stream(num_streams=S, in_channels=channels, mode=self.mode, max_frames_per_call=frames)
        if isinstance(stage, dec.HaasEffect):
            if not optimization.haas_scan_covers(np.zeros(1), stage):
                raise ValueError('only a plain HaasEffect in LR or MS layout, delayed channel 0 or 1, an integer delay '
                                 'in [0, 2**31) and a finite Python / float64 width or None streams')
            if not one_d and channels != 2:
                raise ValueError(f'HaasEffect streams a mono (n,) or a stereo (n, 2) signal, it is fed {channels} channels')
            return 'haas', stage.stream(num_streams=S, in_channels=channels, max_frames_per_call=frames)
        if isinstance(stage, dec.WhiteNoise):
            raise ValueError('WhiteNoise does not stream: its RMS normaliser scales by the RMS of the whole signal')
        if isinstance(stage, partial) and stage.func is dec.convolve_velvet_noise and not stage.args \
                and set(stage.keywords) == {'velvet_noise_filters'}:
            if dtype == 'float64':
                raise TypeError('a stateless convolve fed a float64 Haas output is multiplied in float64 by the one-shot '
                                'convolve_velvet_noise (it promotes); a stream runs float32 only')
            if one_d:
                raise ValueError('a stateless convolve takes a (n, C) signal: the one-shot convolve_velvet_noise raises '
                                 'IndexError for a mono (n,) one')
            return 'convolve', convolve_velvet_noise_stream(stage.keywords['velvet_noise_filters'], num_streams=S,
                                                            in_channels=channels, mode=self.mode,
                                                            max_frames_per_call=frames)
        raise TypeError(f'{stage!r} has no stream form: stateless stages stream as '
                        'stateless(convolve_velvet_noise, velvet_noise_filters=<float32 FIR>) only')

    # ---- public ------------------------------------------------------------------------
    def process(self, x):
        """Push the next block of every stream through every stage; returns the outputs that became final."""
        if self.flushed:
            raise RuntimeError('process() after flush(): call reset() to start a new signal')
        first = self.streams[0]
        x3, squeeze, is_torch = first._chunk(x)          # the first stage's shape and dtype rules, on the host or device
        self.transfers = {'to_device': 0, 'to_host': 0}
        self._torch_out, self._squeeze = is_torch, squeeze
        if not is_torch:
            torch = _native.torch_module()
            x3 = torch.from_numpy(np.ascontiguousarray(x3)).to(torch.device('cuda', _native.default_context().device))
            self.transfers['to_device'] += 1
        self.position += int(x3.shape[1])
        return self._run(x3, final=False)

    def flush(self):
        """Every stage's remaining outputs, each handed to the next stage as its final block; ends the signal."""
        if self.flushed:
            raise RuntimeError('flush() after flush(): call reset() to start a new signal')
        self.transfers = {'to_device': 0, 'to_host': 0}
        out = self._run(None, final=True)
        self.flushed = True
        return out

    def reset(self):
        """Start a new signal at position 0 in every stage."""
        for stream in self.streams:
            stream.reset()
        self.position = 0
        self.flushed = False

    def _run(self, buf, final: bool):
        for stream in self.streams:                      # device tensors from stage to stage, on the current stream
            if buf is not None:
                buf, _, _ = stream._chunk(buf)           # a float64 Haas output is cast to float32 here, on the device
            buf = stream._push(buf, True, False, final)
        if not self._torch_out:
            buf = buf.cpu().numpy()
            self.transfers['to_host'] += 1
        return buf[0] if self._squeeze else buf


# ----------------------------------------------------------------------------
# A voice pool   (include/vnd_voice_stream.h)
# ----------------------------------------------------------------------------
VOICE_START, VOICE_END = _native.VOICE_START, _native.VOICE_END
VOICE_MAX_POSITION = 1 << 60            # the largest position a call goes on from


def _voice_head(positions, counts, flags, max_frames_per_call: Optional[int]):
    """What every span function starts from: ``(pos, n, start, end, p, bad)`` as int64 / bool arrays of one shape, with
    ``p = START ? 0 : pos`` and ``bad`` the slots whose count or ``p`` the device refuses."""
    pos = np.asarray(positions, np.int64)
    n = np.asarray(counts, np.int64)
    f = np.asarray(flags, np.int64)
    if not (pos.shape == n.shape == f.shape):
        raise ValueError(f'positions, counts and flags of one shape, got {pos.shape}, {n.shape}, {f.shape}')
    start, end = (f & VOICE_START) != 0, (f & VOICE_END) != 0
    p = np.where(start, 0, pos)
    bad = (n < 0) | (p < 0) | (p > VOICE_MAX_POSITION)
    if max_frames_per_call is not None:
        bad |= n > int(max_frames_per_call)
    return pos, n, start, end, p, bad


def voice_spans(positions, counts, flags, latency: int, max_frames_per_call: Optional[int] = None):
    """``(out_counts, new_positions)`` of one call of a voice pool (``include/vnd_voice_stream.h``), per slot, from the
    positions before the call, the frames pushed and the ``VOICE_START`` / ``VOICE_END`` flags alone - what the device
    computes from its own state::

        p  = START ? 0 : position            E  = max(0, p - H)
        E' = END ? p + n : max(0, p + n - H)  out_count = E' - E        new position = END ? 0 : p + n

    A count below 0 (or above ``max_frames_per_call``, when given), or without START a position outside ``[0, 2^60]``,
    answers -1 and leaves the position as it was."""
    pos, n, start, end, p, bad = _voice_head(positions, counts, flags, max_frames_per_call)
    H = int(latency)
    first = np.maximum(0, p - H)
    last = np.where(end, p + n, np.maximum(0, p + n - H))
    out = np.where(bad, -1, last - first).astype(np.int64)
    new = np.where(bad, pos, np.where(end, 0, p + n)).astype(np.int64)
    return out, new


def _valid_voice_spans(positions, counts, flags, max_frames_per_call: Optional[int] = None):
    """``(valid, new_positions)`` of one call of a pool that answers ``valid`` (``analysis.polar_voice_spans``,
    ``vectorscope.scope_voice_spans``), per slot, from the positions before the call, the frames pushed and the
    ``VOICE_START`` / ``VOICE_END`` flags alone - what the device computes from its own state::

        p = START ? 0 : position      valid = 1, or 0 for n = 0 without a flag      new position = END ? 0 : p + n

    A count below 0 (or above ``max_frames_per_call``, when given), or without START a position outside ``[0, 2^60]``,
    answers -1 and leaves the position as it was."""
    pos, n, start, end, p, bad = _voice_head(positions, counts, flags, max_frames_per_call)
    idle = ~bad & (n == 0) & ~start & ~end
    p, n = np.where(bad, 0, p), np.where(bad, 0, n)          # (no arithmetic on a bad value)
    valid = np.where(bad, -1, np.where(idle, 0, 1)).astype(np.int64)
    new = np.where(bad | idle, pos, np.where(end, 0, p + n)).astype(np.int64)
    return valid, new


def _check_slots(slots: int):
    if slots > _native.MAX_STREAMS_PER_CALL:
        raise ValueError(f'slots {slots} above {_native.MAX_STREAMS_PER_CALL}: split the pool')


def _slot_ints(slots: int, *names):
    """The spec of a pool's int32 ``(slots,)`` input tensors."""
    return tuple((name, (slots,), 'int32', None) for name in names)


def _check_device_tensors(tensors, specs):
    """``process_dev``'s look at its tensors, each against its ``(name, shape, dtype, fill)`` of the pool's spec: an
    output (``fill`` set) may be None; no device memory is read."""
    for t, (name, shape, dtype, fill) in zip(tensors, specs):
        if t is None and fill:
            continue
        if not _native.is_torch(t) or not t.is_cuda:
            raise ValueError(f'{name} must be a device tensor')
        if tuple(t.shape) != shape or str(t.dtype) != 'torch.' + dtype or not t.is_contiguous():
            raise ValueError(f'{name} must be a contiguous {dtype} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}')


class _SlotPool:
    """What the voice pools share (:class:`VoicePool`, :class:`HaasVoicePool`, :class:`ChainVoicePool` and, through
    :class:`_MeterPool`, the five meters of ``analysis.py``, ``spectral.py`` and ``vectorscope.py``): the host's mirror of
    the slots, ``reset()``, the dict form ``process`` with every refusal before the device, the state and the device form.
    A pool sets ``slots``, ``in_channels``, ``max_frames_per_call``, ``_state = None`` and the spec of its device tensors
    - ``_inputs`` and its two ``_outputs``, ``(name, shape, dtype, fill)`` each, ``fill`` None for an input and
    ``'empty'`` or ``'zeros'``, how an absent one is allocated, for an output - calls ``_mirror()``, and supplies the hooks below and ``_call_host``."""

    def _mirror(self):
        """The host's copy of what the device state says, for the dict form: all slots idle at position 0."""
        self.positions = np.zeros(self.slots, np.int64)
        self.live = np.zeros(self.slots, bool)
        self.tables = np.zeros(self.slots, np.int32)
        self._form = None

    def _require_form(self, form: str):
        """A pool runs through one form until ``reset()``: refuse a call of ``form`` after one of the other."""
        if form == 'dict' and self._form == 'dev':
            raise RuntimeError('this pool runs through process_dev(): the host does not know its positions; reset() first')
        if form == 'dev' and self._form == 'dict':
            raise RuntimeError('this pool runs through process(): mixing in process_dev() would leave the host mirror '
                               'of the positions stale; reset() first')

    # ---- public ------------------------------------------------------------------------
    def reset(self):
        """End every voice, unflushed: every position back to 0 (enqueued on the current torch stream; the ring is not
        cleared, it is never read before it is written), and either form may follow.  Allocates the state on first use."""
        torch = _native.torch_module()
        ctx = _native.default_context()
        if self._state is None:
            self._allocate(torch, ctx)
        else:
            self._reset_device(torch, ctx)
        self._mirror()

    def process(self, blocks=None, *, start=None, end=(), discard: bool = False):
        """One call of the dict form.  ``blocks``: ``{slot: float32 (n, in_channels) array}`` (``(n,)`` as well for mono),
        ``0 <= n <= max_frames_per_call``; ``start``: ``{slot: bank_index}``, the voices that begin with this call;
        ``end``: the slots whose voice ends with it (its tail comes with this call).  Returns ``{slot: (n_out, 2)}`` for
        every slot that got a block or ended.  Raises before any device call: ``ValueError`` for a slot outside the pool,
        a block or an end for a slot that was never started, a start on a live slot (``discard=True`` allows it: what
        the slot held is dropped, unflushed), a bank index outside the bank, a block above ``max_frames_per_call`` or of
        another channel count; ``TypeError`` for a block that is not float32."""
        self._require_form('dict')
        return self._run_schedule(*self._schedule(blocks, start, end, discard))

    def _run_schedule(self, counts, flags, tables, live, x, answered):
        """The call that ``_schedule`` drew up: the device call, its counts against the spans, the mirror moved on."""
        if not counts.any() and not flags.any():              # nothing pushed, started or ended: no device call
            return {slot: np.zeros((0, self._out_width), self._out_dtype) for slot in answered}
        want, positions = self._spans(counts, flags, tables)
        y, got = self._call_host(x, counts, flags, *self._per_slot(tables))
        if not np.array_equal(np.asarray(got, np.int64), want):
            raise _native.NativeError(f'the voice pool returned the counts {list(got)}, the spans are {list(want)}')
        self._commit(positions)
        self.tables, self._form = tables, 'dict'
        live[(flags & VOICE_END) != 0] = False
        self.live = live
        return {slot: np.array(y[slot, :int(want[slot])]) for slot in answered}

    # ---- what a pool supplies ------------------------------------------------------------------
    _out_dtype = np.float32
    _out_width = 2                            # the last axis of what a slot returns
    _block_dtype = np.float32                 # what a voice pushes
    _own = None                               # (buffer, first, second): the outputs of a pool that keeps them, once allocated

    def _spans(self, counts, flags, tables):
        """``(out_counts, new positions)`` of the call, from the host mirror."""
        raise NotImplementedError

    def _per_slot(self, tables):
        """The per-slot int32 arrays that go up beside counts and flags, from what ``_schedule`` keeps per slot."""
        return (tables,)

    def _bank_len(self) -> int:
        """Entries in the bank a voice starts with."""
        raise NotImplementedError

    def _slot_value(self, index: int):
        """What ``_schedule`` keeps in ``tables`` for a slot that starts with bank entry ``index``."""
        raise NotImplementedError

    def _commit(self, positions):
        self.positions = positions

    def _state_bytes(self, ctx) -> int:
        """The bytes of the pool's device state."""
        raise NotImplementedError

    def _reset_entry(self, ctx, state_ptr: int, state_bytes: int, stream: int):
        """The pool's native reset."""
        raise NotImplementedError

    def _launch(self, ctx, state_ptr: int, state_bytes: int, inputs, first, second, stream: int):
        """The pool's native device call on its tuple of input tensors and its two output tensors."""
        raise NotImplementedError

    # ---- checks --------------------------------------------------------------------------
    def _slot(self, slot, what: str) -> int:
        if isinstance(slot, (bool, np.bool_)) or not isinstance(slot, (int, np.integer)) or not 0 <= slot < self.slots:
            raise ValueError(f'{what}: slot {slot!r} is outside the pool of {self.slots} slots')
        return int(slot)

    def _schedule(self, blocks, start, end, discard: bool):
        """The call's arrays from the dicts, every refusal included; nothing of the pool is changed."""
        S, M, cx = self.slots, self.max_frames_per_call, self.in_channels
        counts, flags = np.zeros(S, np.int32), np.zeros(S, np.int32)
        tables, live = self.tables.copy(), self.live.copy()
        for slot, index in dict(start or {}).items():
            slot = self._slot(slot, 'start')
            if isinstance(index, (bool, np.bool_)) or not isinstance(index, (int, np.integer)) \
                    or not 0 <= index < self._bank_len():
                raise ValueError(f'start: bank index {index!r} of slot {slot} is outside the bank of {self._bank_len()}')
            if live[slot] and not discard:
                raise ValueError(f'start: slot {slot} holds a live voice: end it first, or pass discard=True to drop it '
                                 'unflushed')
            flags[slot] |= VOICE_START
            tables[slot] = self._slot_value(int(index))
            live[slot] = True
        x = np.zeros((S, M, cx), self._block_dtype)
        answered = set()
        for slot, block in dict(blocks or {}).items():
            slot = self._slot(slot, 'block')
            if not live[slot]:
                raise ValueError(f'block for slot {slot}, which was never started: name it in start=')
            a = np.asarray(block)
            if a.dtype != self._block_dtype:
                raise TypeError(f'block of slot {slot}: voices push {np.dtype(self._block_dtype).name} frames, got {a.dtype}')
            if a.ndim == 1 and cx == 1:
                a = a[:, None]
            if a.ndim != 2 or a.shape[1] != cx:
                raise ValueError(f'block of slot {slot} has shape {tuple(np.shape(block))}: expected (frames, {cx})')
            if a.shape[0] > M:
                raise ValueError(f'block of slot {slot}: {a.shape[0]} frames in one call, above max_frames_per_call={M}')
            counts[slot] = a.shape[0]
            x[slot, :a.shape[0]] = a
            answered.add(slot)
        for slot in list(end):
            slot = self._slot(slot, 'end')
            if not live[slot]:
                raise ValueError(f'end of slot {slot}, which was never started')
            if flags[slot] & VOICE_END:
                raise ValueError(f'end: slot {slot} is named twice')
            flags[slot] |= VOICE_END
            answered.add(slot)
        return counts, flags, tables, live, x, sorted(answered)

    def _start_slots(self, start) -> dict:
        """``start`` as ``_schedule`` takes it, for a pool whose voices start with nothing of their own: a list of slots."""
        starts = {}
        for slot in list(start or ()):
            slot = self._slot(slot, 'start')
            if slot in starts:
                raise ValueError(f'start: slot {slot} is named twice')
            starts[slot] = 0
        return starts

    # ---- the device -------------------------------------------------------------------------
    def _ensure_state(self, torch, ctx):
        if self._state is None:
            self._allocate(torch, ctx)
        return self._state

    def _allocate(self, torch, ctx):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('the state of a voice pool is allocated and zeroed on first use: call reset() before the capture')
        need = self._state_bytes(ctx)
        buf = torch.empty((max(need, 16),), dtype=torch.uint8, device=torch.device('cuda', ctx.device))
        self._state = (buf, need)
        self._reset_device(torch, ctx)

    def _reset_device(self, torch, ctx):
        state, state_bytes = self._state
        self._reset_entry(ctx, state.data_ptr(), state_bytes, torch.cuda.current_stream(state.device).cuda_stream)

    def _process_dev(self, inputs, out=None, *, valid=None):
        """``process_dev``: the form guard and the look at the tensors (no device memory is read), then the call.  ``out``:
        the caller's two outputs; ``valid``: the caller's second output alone, for a pool that keeps the first."""
        if self._form == 'dict':
            self._require_form('dev')
        _check_device_tensors(inputs, self._inputs)
        first, second = (None, valid) if out is None else out
        _check_device_tensors((first, second), self._outputs)
        return self._call_device(_native.torch_module(), inputs, first, second)

    def _call_device(self, torch, inputs, first, second):
        """One device call on the current stream: the tuple of input tensors and the two outputs, each a tensor or None
        (None: the pool's own if it keeps its outputs, else allocated here).  Returns the outputs."""
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        for t in inputs:
            if t.device != device:
                raise ValueError(f'tensor on {t.device}, the pool runs on {device}')
        state, state_bytes = self._ensure_state(torch, ctx)
        if self._own is not None:
            first, second = self._own[1], self._own[2] if second is None else second
        if first is None:
            first = self._new_output(torch, device, *self._outputs[0])
        if second is None:
            second = self._new_output(torch, device, *self._outputs[1])
        self._form = 'dev'
        self._launch(ctx, state.data_ptr(), state_bytes, inputs, first, second, torch.cuda.current_stream(device).cuda_stream)
        return first, second

    @staticmethod
    def _new_output(torch, device, name, shape, dtype, fill):
        return getattr(torch, fill)(shape, dtype=getattr(torch, dtype), device=device)

    def _packed_outputs(self, torch, device, allocate):
        """``(buffer, first, second)``: both outputs in one uint8 buffer from ``allocate``, the first, then the second
        (int32 after a multiple of 4 bytes) - one copy brings both down."""
        (_, shape0, dtype0, _), (_, shape1, dtype1, _) = self._outputs
        bytes0 = int(np.prod(shape0)) * np.dtype(dtype0).itemsize
        bytes1 = int(np.prod(shape1)) * np.dtype(dtype1).itemsize
        down = allocate((bytes0 + bytes1,), dtype=torch.uint8, device=device)
        return (down, down[:bytes0].view(getattr(torch, dtype0)).view(shape0),
                down[bytes0:].view(getattr(torch, dtype1)).view(shape1))

    def _call_host_packed(self, x, ints, first: bool = True):
        """A ``_call_host`` on the device form: one upload (the blocks and the int32 arrays ``ints`` in one buffer), the
        call, one download (the pool's outputs in one buffer - its own at its fixed address if it keeps them, else a fresh
        one; without ``first`` the second output alone, and None for the first); ``transfers`` counts them.  ``_form``
        stays as it was."""
        torch = _native.torch_module()
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        self._ensure_state(torch, ctx)
        ints = np.stack(ints).astype(np.int32)
        up = torch.from_numpy(np.concatenate([x.reshape(-1).view(np.uint8), ints.reshape(-1).view(np.uint8)])).to(device)
        self.transfers = {'to_device': 1, 'to_host': 0}
        x_dev = up[:x.nbytes].view(getattr(torch, x.dtype.name)).view(x.shape)
        int_rows = up[x.nbytes:].view(torch.int32).view(len(ints), self.slots)
        # the download buffer: zeroed as a whole if the pool wants either output zero-filled
        (_, shape0, dtype0, fill0), (_, shape1, dtype1, fill1) = self._outputs
        down, out0, out1 = self._own or self._packed_outputs(torch, device,
                                                             torch.zeros if 'zeros' in (fill0, fill1) else torch.empty)
        form = self._form
        try:
            self._call_device(torch, (x_dev, *int_rows), out0, out1)
        finally:
            self._form = form
        host = (down if first else out1).cpu().numpy()
        self.transfers['to_host'] = 1
        if not first:
            return None, host
        cut = host.nbytes - out1.numel() * out1.element_size()
        return host[:cut].view(dtype0).reshape(shape0), host[cut:].view(dtype1).reshape(shape1)


_INT32_MAX = 2 ** 31 - 1


def _sample_dtype(dtype) -> np.dtype:
    """A meter's ``dtype`` argument as a NumPy dtype: float32 or float64, else ``ValueError``."""
    try:
        parsed = None if dtype is None else np.dtype(dtype)                       # (np.dtype(None) is float64)
    except TypeError:
        parsed = None
    if parsed is None or parsed.name not in ('float32', 'float64'):
        raise ValueError(f"dtype must be 'float32' or 'float64', got {dtype!r}")
    return parsed


class _MeterPool(_SlotPool):
    """What the meters share (``analysis.CorrelogramVoicePool`` and ``PolarVoicePool``, ``spectral.SpectrumVoicePool``,
    ``vectorscope.ScopeVoicePool`` and ``LevelVoicePool``): a meter is a pool whose voices start with nothing of their own.
    It takes ``start`` as a list of slots, pushes stereo frames of its ``dtype`` (float32 or float64) with int32 counts,
    and unless it says otherwise answers ``valid`` in {-1, 0, 1} by :func:`_valid_voice_spans`."""

    in_channels = 2

    def __init__(self, slots: int, max_frames_per_call: int, dtype):
        _check_counts(slots=slots, max_frames_per_call=max_frames_per_call)
        _check_slots(slots)
        if max_frames_per_call > _INT32_MAX:
            raise ValueError(f'max_frames_per_call {max_frames_per_call} above 2**31 - 1: counts are int32')
        self.dtype = _sample_dtype(dtype)
        self.slots, self.max_frames_per_call = int(slots), int(max_frames_per_call)
        self._block_dtype = self.dtype            # what _schedule holds every block to
        self.transfers = {'to_device': 0, 'to_host': 0}
        self._state = None                    # (torch uint8 tensor, bytes)

    def _process_valid(self, blocks, start, end, discard: bool, row, *host_args):
        """The dict form of a meter that answers ``valid``: every slot that got a block, started or ended and answered 1
        (an empty block alone is idle) with ``row(its row of the first output)``, or None without ``row``.
        ``host_args`` go to ``_call_host`` behind x, counts and flags."""
        self._require_form('dict')
        starts = self._start_slots(start)
        counts, flags, tables, live, x, answered = self._schedule(blocks, starts, end, discard)
        answered = sorted(set(answered) | set(starts))
        if not counts.any() and not flags.any():              # nothing pushed, started or ended: no device call
            return {}
        want, positions = self._spans(counts, flags, tables)
        rows, got = self._call_host(x, counts, flags, *host_args)
        if not np.array_equal(np.asarray(got, np.int64), want):
            raise _native.NativeError(f'the voice pool answered {list(got)}, the spans are {list(want)}')
        self._commit(positions)
        self.tables, self._form = tables, 'dict'
        live[(flags & VOICE_END) != 0] = False
        self.live = live
        return {slot: row(rows[slot]) if row else None for slot in answered if want[slot] == 1}

    def _spans(self, counts, flags, tables):
        return _valid_voice_spans(self.positions, counts, flags, self.max_frames_per_call)

    def _per_slot(self, tables):
        return ()

    def _bank_len(self) -> int:
        return 1                                  # a voice starts with nothing of its own: the pool has one setting

    def _slot_value(self, index: int):
        return 0

    def _call_host(self, x, counts, flags):
        """One upload (the blocks and the two int32 arrays in one buffer), the call, one download (both outputs)."""
        return self._call_host_packed(x, (counts, flags))


class VoicePool(_SlotPool):
    """``slots`` slots over a bank of velvet-noise filters, each slot a voice with a life of its own
    (``decorrelation.decorrelate_voice_pool``, ``vnd_voice_stream_f32_*``): voices start and end on any call, bring blocks
    of any size up to ``max_frames_per_call`` or none, and a slot is handed to a new voice with another filter of the bank
    without ending the pool.  The stream position lives in the device state, one per slot, so a call is a pure function
    of device memory.  ``latency_frames`` is the bank's largest tap index, the one latency of the pool.  For every voice
    the concatenation of what its calls return, from its start up to and including its end, equals
    ``bank[t].decorrelate(x_voice)`` on the whole signal bit for bit.

    Two forms; a pool is used through one of them (mixing them raises ``RuntimeError`` until ``reset()``: the host mirror
    of the positions would be stale):

    * ``process({slot: block}, start={slot: bank_index}, end=[slot, ...])`` - float32 NumPy blocks ``(n, in_channels)``
      in, ``{slot: (n_out, 2) array}`` out for every slot that got a block or ended, synchronously.  Everything is checked
      before any device call.
    * ``process_dev(x, counts, flags, tables)`` - the caller's device tensors of fixed shape on the current stream; only
      enqueues, and can be captured with ``torch.cuda.graph`` (call ``reset()`` before the capture: it allocates the
      state).  ``tables`` holds candidates of the deduplicated bank: ``bank_tables[bank_index]``."""

    def __init__(self, arrays: TapArrays, bank_tables, *, slots: int, in_channels: int, max_frames_per_call: int,
                 ms_encode: bool = False, width: Optional[float] = None):
        _check_counts(slots=slots, in_channels=in_channels, max_frames_per_call=max_frames_per_call)
        if in_channels not in (1, 2):
            raise ValueError(f'a pool of mono (1) or stereo (2) voices is taken, got in_channels={in_channels}')
        _check_slots(slots)
        if max_frames_per_call > 1 << 24:
            raise ValueError(f'max_frames_per_call {max_frames_per_call} above 2**24')
        if arrays.num_channels < 2 or arrays.num_channels % 2:
            raise ValueError(f'a bank holds stereo pairs: this one has {arrays.num_channels} channels')
        self.slots, self.in_channels, self.max_frames_per_call = int(slots), int(in_channels), int(max_frames_per_call)
        self.arrays, self.num_tables = arrays, arrays.num_channels // 2
        self.bank_tables = np.ascontiguousarray(bank_tables, np.int32)
        if self.bank_tables.ndim != 1 or not self.bank_tables.size or self.bank_tables.min() < 0 \
                or self.bank_tables.max() >= self.num_tables:
            raise ValueError(f'table indices outside [0, {self.num_tables})')
        self.ms_encode, self.width, self.mode = bool(ms_encode), width, _native.MODE_EXACT
        self.latency_frames = int(arrays.tap_index.max()) if len(arrays.tap_index) else 0
        self.num_channels = 2
        self._table = None
        self._state = None                    # (torch uint8 tensor, bytes)
        S, M = self.slots, self.max_frames_per_call
        self._inputs = (('x', (S, M, self.in_channels), 'float32', None),) + _slot_ints(S, 'counts', 'flags', 'tables')
        self._outputs = (('y', (S, M + self.latency_frames, 2), 'float32', 'empty'), ('out_counts', (S,), 'int32', 'empty'))
        self._mirror()

    @property
    def row_frames(self) -> int:
        """Frames per row of the result: ``max_frames_per_call + latency_frames``."""
        return self.max_frames_per_call + self.latency_frames

    def process_dev(self, x, counts, flags, tables, *, out=None):
        """One call on device tensors, enqueued on the current stream: ``x`` float32 ``(slots, M, in_channels)``,
        ``counts`` / ``flags`` / ``tables`` int32 ``(slots,)``.  Returns ``(y, out_counts)``: float32
        ``(slots, M + H, 2)`` - the first ``out_counts[b]`` frames of row b are written, nothing at or past them - and
        int32 ``(slots,)``; ``out=(y, out_counts)`` takes the caller's.  No check reads device memory; bad per-slot
        values answer as ``include/vnd_voice_stream.h`` says (-1, NaN rows)."""
        return self._process_dev((x, counts, flags, tables), out)

    def _spans(self, counts, flags, tables):
        return voice_spans(self.positions, counts, flags, self.latency_frames, self.max_frames_per_call)

    def _bank_len(self) -> int:
        return len(self.bank_tables)

    def _slot_value(self, index: int):
        return self.bank_tables[index]

    # ---- the device -------------------------------------------------------------------------
    def _state_bytes(self, ctx) -> int:
        from . import decorrelation
        self._table = decorrelation._each_banks.get(ctx, self.arrays)
        return _native.voice_stream_state_bytes(self._table, self.slots, self.in_channels, self.max_frames_per_call)

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        _native.voice_stream_reset_device(ctx, self._table, state_ptr, state_bytes, self.slots, self.in_channels,
                                          self.max_frames_per_call, stream=stream)

    def _call_host(self, x, counts, flags, tables):
        torch = _native.torch_module()
        ctx = _native.default_context()
        state, state_bytes = self._ensure_state(torch, ctx)
        torch.cuda.current_stream(state.device).synchronize()          # (the reset, or a reset() on this stream)
        y = np.empty((self.slots, self.row_frames, 2), np.float32)
        got = _native.voice_stream_host(ctx, self._table, state.data_ptr(), state_bytes, self.max_frames_per_call, x, counts,
                                        flags, tables, y, ms_encode=self.ms_encode, width=self.width)
        return y, got

    def _launch(self, ctx, state_ptr, state_bytes, inputs, y, out_counts, stream):
        x, counts, flags, tables = inputs
        _native.voice_stream_device(ctx, self._table, state_ptr, state_bytes, self.max_frames_per_call, x.data_ptr(),
                                    counts.data_ptr(), flags.data_ptr(), tables.data_ptr(), y.data_ptr(),
                                    out_counts.data_ptr(), self.slots, self.in_channels, ms_encode=self.ms_encode,
                                    width=self.width, stream=stream)


# ----------------------------------------------------------------------------
# A voice pool whose live voices change their filter, crossfaded   (include/vnd_voice_fade_stream.h)
# ----------------------------------------------------------------------------
VOICE_SWITCH = _native.VOICE_SWITCH
VOICE_FADE_MAX_FRAMES = _native.VOICE_FADE_MAX_FRAMES


def voice_fade_spans(positions, records, counts, flags, tables, latency: int, fade_frames: int,
                     max_frames_per_call: Optional[int] = None):
    """``(out_counts, new_positions, new_records, fade_left)`` of one call of a crossfading voice pool
    (``include/vnd_voice_fade_stream.h``), per slot, from the positions and records before the call - ``records`` is int64
    ``(slots, 3)``: ``s``, ``old``, ``cur`` - the frames pushed, the ``VOICE_START`` / ``VOICE_END`` / ``VOICE_SWITCH``
    flags and the tables of the call alone - what the device computes from its own state::

        fresh = START or position == 0          p, E, E', out_count, new position: voice_spans'
        (old, cur, s) = (table, table, -F) if fresh else the record
        accept = SWITCH and not fresh and E >= s + F:    (old, cur, s) = (cur, table, E)
        fade_left = 0 if END else min(F, max(0, s + F - E'))

    A bad slot (``voice_spans``' rule) answers -1 twice and keeps its position and its record."""
    pos, n, start, end, p, bad = _voice_head(positions, counts, flags, max_frames_per_call)
    rec = np.asarray(records, np.int64)
    t = np.asarray(tables, np.int64)
    if rec.shape != pos.shape + (3,) or t.shape != pos.shape:
        raise ValueError(f'records of shape {pos.shape + (3,)} and tables of shape {pos.shape}, got {rec.shape}, {t.shape}')
    H, F = int(latency), int(fade_frames)
    p, n = np.where(bad, 0, p), np.where(bad, 0, n)          # (no arithmetic on a bad value)
    first = np.maximum(0, p - H)
    last = np.where(end, p + n, np.maximum(0, p + n - H))
    s, old, cur = rec[..., 0], rec[..., 1], rec[..., 2]
    fresh = ~bad & (start | (pos == 0))
    switch = (np.asarray(flags, np.int64) & VOICE_SWITCH) != 0
    accept = ~bad & ~fresh & switch & (first - F >= s)         # E >= s + F, without a sum a planted s could wrap
    new_s = np.where(fresh, -F, np.where(accept, first, s))
    new_old = np.where(fresh, t, np.where(accept, cur, old))
    new_cur = np.where(fresh | accept, t, cur)
    left = np.where(new_s >= last, F, np.where(new_s < last - F, 0, new_s + F - last))
    out = np.where(bad, -1, last - first).astype(np.int64)
    new = np.where(bad, pos, np.where(end, 0, p + n)).astype(np.int64)
    fade_left = np.where(bad, -1, np.where(end, 0, left)).astype(np.int64)
    return out, new, np.stack([new_s, new_old, new_cur], axis=-1).astype(np.int64), fade_left


def fade_gains(fade_frames: int, fade='linear') -> np.ndarray:
    """The float32 ``(2, fade_frames)`` gains of a crossfade, row 0 fade-out and row 1 fade-in, frame ``j`` of the fade
    scaled by column ``j``.  ``fade``: ``'linear'`` - ``in[j] = float32((j + 1) / (F + 1))``, ``out = float32(1) - in``;
    ``'equal_power'`` - ``in, out = sin, cos`` of ``pi/2 * (j + 1) / (F + 1)`` in float64, then rounded to float32; or a
    pair ``(fade_out, fade_in)`` of finite float32 arrays of length ``fade_frames``.  ``ValueError`` otherwise."""
    if isinstance(fade_frames, (bool, np.bool_)) or not isinstance(fade_frames, (int, np.integer)) \
            or not 0 <= fade_frames <= VOICE_FADE_MAX_FRAMES:
        raise ValueError(f'fade_frames must be an integer in [0, {VOICE_FADE_MAX_FRAMES}], got {fade_frames!r}')
    F = int(fade_frames)
    if isinstance(fade, str):
        ramp = (np.arange(F, dtype=np.float64) + 1.0) / (F + 1.0)
        if fade == 'linear':
            rise = ramp.astype(np.float32)
            return np.stack([np.float32(1) - rise, rise])
        if fade == 'equal_power':
            return np.stack([np.cos(np.pi / 2 * ramp), np.sin(np.pi / 2 * ramp)]).astype(np.float32)
        raise ValueError(f"fade must be 'linear', 'equal_power' or a pair of float32 arrays, got {fade!r}")
    try:
        fall, rise = fade
    except (TypeError, ValueError):
        raise ValueError("fade must be 'linear', 'equal_power' or a pair (fade_out, fade_in) of float32 arrays") from None
    for name, g in (('fade_out', fall), ('fade_in', rise)):
        if not isinstance(g, np.ndarray) or g.dtype != np.float32 or g.shape != (F,):
            raise ValueError(f'{name} must be a float32 array of shape ({F},), got {getattr(g, "dtype", type(g).__name__)} '
                             f'{getattr(g, "shape", "")}')
        if not np.isfinite(g).all():
            raise ValueError(f'{name} holds a gain that is not finite')
    return np.ascontiguousarray(np.stack([fall, rise]))


def _fade_settings(fade_frames, fade_gains):
    """``(fade_frames, fade_gains)`` as a crossfading pool keeps them: an int in ``[0, VOICE_FADE_MAX_FRAMES]`` and a finite
    contiguous float32 ``(2, fade_frames)`` array; ``ValueError`` otherwise."""
    gains = np.ascontiguousarray(fade_gains)
    if isinstance(fade_frames, (bool, np.bool_)) or not isinstance(fade_frames, (int, np.integer)) \
            or not 0 <= fade_frames <= VOICE_FADE_MAX_FRAMES:
        raise ValueError(f'fade_frames must be an integer in [0, {VOICE_FADE_MAX_FRAMES}], got {fade_frames!r}')
    if gains.dtype != np.float32 or gains.shape != (2, fade_frames) or not np.isfinite(gains).all():
        raise ValueError(f'fade_gains must be a finite float32 array of shape (2, {fade_frames})')
    return int(fade_frames), gains


class FadeVoicePool(VoicePool):
    """A :class:`VoicePool` whose live voices change their filter (``decorrelation.decorrelate_voice_pool`` with
    ``fade_frames``, ``vnd_voice_fade_stream_f32_dev``): a voice that switches keeps its position, its history and its
    latency, and from the first frame it has not yet returned its output fades over ``fade_frames`` frames from the bank
    entry it had to the new one - ``old * fade_gains[0][j] + new * fade_gains[1][j]`` on the convolved frames, float32, before
    the stage's pointwise steps.  One fade per voice is in flight: ``fade_left[slot]`` is the number of frames of it the
    slot has yet to return, and a switch is taken only at 0.  A voice that never switches returns :class:`VoicePool`'s
    bytes.

    * ``process({slot: block}, start=..., end=..., switch={slot: bank_index})`` - the dict form.  Besides
      :class:`VoicePool`'s refusals, ``ValueError`` before any device call for a switch on a slot with no live voice,
      together with a start of that slot, to an index outside the bank, or while ``fade_left[slot] > 0``.
    * ``process_dev(x, counts, flags, tables)`` - flags may carry ``VOICE_SWITCH``, and ``tables[b]`` is read when a
      voice begins and when its switch is accepted; a switch that comes while ``fade_left_dev[b] > 0`` is ignored.
      ``(y, out_counts)`` are :class:`VoicePool`'s, so every meter attaches unchanged; ``fade_left_dev`` is the pool's
      own int32 ``(slots,)`` tensor at a fixed address, written by every call."""

    def __init__(self, arrays: TapArrays, bank_tables, *, slots: int, in_channels: int, max_frames_per_call: int,
                 fade_frames: int, fade_gains: np.ndarray, ms_encode: bool = False, width: Optional[float] = None):
        self.fade_frames, self.fade_gains = _fade_settings(fade_frames, fade_gains)
        self.transfers = {'to_device': 0, 'to_host': 0}
        self._fade = None                     # (gains on the device or None, fade_left_dev)
        VoicePool.__init__(self, arrays, bank_tables, slots=slots, in_channels=in_channels,
                           max_frames_per_call=max_frames_per_call, ms_encode=ms_encode, width=width)

    def _mirror(self):
        VoicePool._mirror(self)
        self.records = np.zeros((self.slots, 3), np.int64)        # (s, old, cur); a slot at position 0 takes its own from the call
        self.fade_left = np.zeros(self.slots, np.int64)

    @property
    def fade_left_dev(self):
        """The int32 ``(slots,)`` device tensor every call writes ``fade_left`` to; allocated by ``reset()``."""
        if self._fade is None:
            raise RuntimeError('fade_left_dev is allocated with the state: call reset() first')
        return self._fade[1]

    def process(self, blocks=None, *, start=None, end=(), switch=None, discard: bool = False):
        """:meth:`VoicePool.process` with ``switch``: ``{slot: bank_index}``, the live voices that change to another bank
        entry with this call.  The fade begins at the first frame the slot returns in this call."""
        self._require_form('dict')
        counts, flags, tables, live, x, answered = self._schedule(blocks, start, end, discard)
        for slot, index in dict(switch or {}).items():
            slot = self._slot(slot, 'switch')
            if isinstance(index, (bool, np.bool_)) or not isinstance(index, (int, np.integer)) \
                    or not 0 <= index < self._bank_len():
                raise ValueError(f'switch: bank index {index!r} of slot {slot} is outside the bank of {self._bank_len()}')
            if flags[slot] & VOICE_START:
                raise ValueError(f'switch: slot {slot} starts with this call: a voice begins with the entry in start=')
            if not live[slot]:
                raise ValueError(f'switch: slot {slot} holds no live voice')
            if self.fade_left[slot] > 0:
                raise ValueError(f'switch: slot {slot} has {int(self.fade_left[slot])} frames of its fade left to return')
            flags[slot] |= VOICE_SWITCH
            tables[slot] = self._slot_value(int(index))
        return self._run_schedule(counts, flags, tables, live, x, answered)

    def _spans(self, counts, flags, tables):
        out, positions, records, fade_left = voice_fade_spans(self.positions, self.records, counts, flags, tables,
                                                              self.latency_frames, self.fade_frames, self.max_frames_per_call)
        return out, (positions, records, fade_left)

    def _commit(self, state):
        self.positions, self.records, self.fade_left = state

    # ---- the device -------------------------------------------------------------------------
    def _state_bytes(self, ctx) -> int:
        from . import _native_fade, decorrelation
        self._table = decorrelation._each_banks.get(ctx, self.arrays)
        return _native_fade.voice_fade_stream_state_bytes(self._table, self.slots, self.in_channels, self.max_frames_per_call,
                                                          self.fade_frames)

    def _allocate(self, torch, ctx):
        VoicePool._allocate(self, torch, ctx)
        device = torch.device('cuda', ctx.device)
        gains = torch.from_numpy(self.fade_gains).to(device) if self.fade_frames else None     # uploaded once
        self._fade = (gains, torch.zeros((self.slots,), dtype=torch.int32, device=device))

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        from . import _native_fade
        _native_fade.voice_fade_stream_reset_device(ctx, self._table, state_ptr, state_bytes, self.slots, self.in_channels,
                                                    self.max_frames_per_call, self.fade_frames, stream=stream)

    def _call_host(self, x, counts, flags, tables):
        """One upload (the blocks and the three int32 arrays in one buffer), the call, one download (y and out_counts)."""
        return self._call_host_packed(x, (counts, flags, tables))

    def _launch(self, ctx, state_ptr, state_bytes, inputs, y, out_counts, stream):
        from . import _native_fade
        x, counts, flags, tables = inputs
        gains, fade_left = self._fade
        _native_fade.voice_fade_stream_device(ctx, self._table, state_ptr, state_bytes, self.max_frames_per_call,
                                              self.fade_frames, None if gains is None else gains.data_ptr(), x.data_ptr(),
                                              counts.data_ptr(), flags.data_ptr(), tables.data_ptr(), y.data_ptr(),
                                              out_counts.data_ptr(), fade_left.data_ptr(), self.slots, self.in_channels,
                                              ms_encode=self.ms_encode, width=self.width, stream=stream)


# ----------------------------------------------------------------------------
# A voice pool of Haas delays, and of velvet-then-Haas chains   (include/vnd_haas_voice_stream.h)
# ----------------------------------------------------------------------------
HAAS_VOICE_MAX_ROW_FRAMES = 65535 * 256       # VND_HAAS_VOICE_MAX_ROW_FRAMES: the workgroups of a row are one grid dimension


def haas_voice_spans(positions, counts, flags, delays, max_delay: int, max_frames_per_call: Optional[int] = None):
    """``(out_counts, new_positions)`` of one call of a Haas voice pool (``include/vnd_haas_voice_stream.h``), per slot,
    from the positions before the call, the frames pushed, the ``VOICE_START`` / ``VOICE_END`` flags and the delays
    alone - what the device computes from its own state::

        p = START ? 0 : position      out_count = n + (END ? d : 0)      new position = END ? 0 : p + n

    A count below 0 (or above ``max_frames_per_call``, when given), without START a position outside ``[0, 2^60]``, or -
    on a slot with frames or a flag - a delay outside ``[0, max_delay]`` answers -1 and leaves the position as it was."""
    d = np.asarray(delays, np.int64)
    out, new = voice_spans(positions, counts, flags, 0, max_frames_per_call)
    if d.shape != out.shape:
        raise ValueError(f'delays of the shape of positions, counts and flags, got {d.shape} and {out.shape}')
    pos, n, f = np.asarray(positions, np.int64), np.asarray(counts, np.int64), np.asarray(flags, np.int64)
    work = (n != 0) | ((f & (VOICE_START | VOICE_END)) != 0)
    bad = (out < 0) | (work & ((d < 0) | (d > int(max_delay))))
    end = (f & VOICE_END) != 0
    out = np.where(bad, -1, out + np.where(end & work, d, 0)).astype(np.int64)
    return out, np.where(bad, pos, new).astype(np.int64)


class HaasVoicePool(_SlotPool):
    """``slots`` slots over a bank of ``HaasEffect`` delays, each slot a voice with a life of its own
    (``decorrelation.decorrelate_voice_pool``, ``vnd_haas_voice_stream_f64_*``): :class:`VoicePool` for the Haas delay.
    ``latency_frames`` is 0 - the delay is causal, a call returns the frames it was given - and a voice's end returns its
    own delay's tail as well; ``tail_frames`` is the bank's largest delay, ``bank_delays[bank_index]`` the delay a voice
    started with ``bank_index`` gets, ``row_frames = max_frames_per_call + tail_frames``.  For every voice the
    concatenation of what its calls return equals ``bank[i].decorrelate(x_voice)`` bit for bit: float64, ``n + d`` frames.

    The two forms of :class:`VoicePool`, with the same refusals and the same rule against mixing them:
    ``process({slot: float32 block}, start={slot: bank_index}, end=[slot], discard=False)`` returns
    ``{slot: float64 (n_out, 2)}``; ``process_dev(x, counts, flags, delays)`` takes device tensors of fixed shape, only
    enqueues, and can be captured after ``reset()``."""

    _out_dtype = np.float64

    def __init__(self, bank_delays, *, slots: int, in_channels: int, max_frames_per_call: int, delayed_channel: int,
                 ms_mode: bool, width: Optional[float] = None):
        _check_counts(slots=slots, in_channels=in_channels, max_frames_per_call=max_frames_per_call)
        if in_channels not in (1, 2):
            raise ValueError(f'a pool of mono (1) or stereo (2) voices is taken, got in_channels={in_channels}')
        _check_slots(slots)
        self.bank_delays = np.ascontiguousarray(bank_delays, np.int32)
        if self.bank_delays.ndim != 1 or not self.bank_delays.size or self.bank_delays.min() < 0:
            raise ValueError('bank_delays: one delay >= 0 per bank entry')
        if delayed_channel not in (0, 1):
            raise ValueError(f'delayed_channel must be 0 or 1, got {delayed_channel!r}')
        self.max_delay = int(self.bank_delays.max())
        if max_frames_per_call + self.max_delay > HAAS_VOICE_MAX_ROW_FRAMES:
            raise ValueError(f'max_frames_per_call {max_frames_per_call} and the largest delay {self.max_delay} make a row '
                             f'above {HAAS_VOICE_MAX_ROW_FRAMES} frames')
        self.slots, self.in_channels, self.max_frames_per_call = int(slots), int(in_channels), int(max_frames_per_call)
        self.delayed_channel, self.ms_mode, self.width = int(delayed_channel), bool(ms_mode), width
        self.latency_frames, self.tail_frames = 0, self.max_delay
        self.num_channels = 2
        self._state = None
        S, M = self.slots, self.max_frames_per_call
        self._inputs = (('x', (S, M, self.in_channels), 'float32', None),) + _slot_ints(S, 'counts', 'flags', 'delays')
        self._outputs = (('y', (S, self.row_frames, 2), 'float64', 'empty'), ('out_counts', (S,), 'int32', 'empty'))
        self._mirror()

    @property
    def row_frames(self) -> int:
        """Frames per row of the result: ``max_frames_per_call + tail_frames``."""
        return self.max_frames_per_call + self.max_delay

    def process_dev(self, x, counts, flags, delays, *, out=None):
        """One call on device tensors, enqueued on the current stream: ``x`` float32 ``(slots, M, in_channels)``,
        ``counts`` / ``flags`` / ``delays`` int32 ``(slots,)``.  Returns ``(y, out_counts)``: float64
        ``(slots, M + max delay, 2)`` - the first ``out_counts[b]`` frames of row b are written, nothing at or past
        them - and int32 ``(slots,)``; ``out=(y, out_counts)`` takes the caller's.  No check reads device memory; bad
        per-slot values answer -1 (``include/vnd_haas_voice_stream.h``)."""
        return self._process_dev((x, counts, flags, delays), out)

    def _spans(self, counts, flags, delays):
        return haas_voice_spans(self.positions, counts, flags, delays, self.max_delay, self.max_frames_per_call)

    def _bank_len(self) -> int:
        return len(self.bank_delays)

    def _slot_value(self, index: int):
        return self.bank_delays[index]                           # ``tables`` holds the slots' delays

    # ---- the device -------------------------------------------------------------------------
    def _state_bytes(self, ctx) -> int:
        return _native.haas_voice_stream_state_bytes(self.slots, self.in_channels, self.max_delay, self.max_frames_per_call)

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        _native.haas_voice_stream_reset_device(ctx, state_ptr, state_bytes, self.slots, self.in_channels, self.max_delay,
                                               self.max_frames_per_call, stream=stream)

    def _call_host(self, x, counts, flags, delays):
        torch = _native.torch_module()
        ctx = _native.default_context()
        state, state_bytes = self._ensure_state(torch, ctx)
        torch.cuda.current_stream(state.device).synchronize()          # (the reset, or a reset() on this stream)
        y = np.empty((self.slots, self.row_frames, 2), np.float64)
        got = _native.haas_voice_stream_host(ctx, state.data_ptr(), state_bytes, self.max_frames_per_call, x, counts, flags,
                                             delays, y, max_delay=self.max_delay, delayed_channel=self.delayed_channel,
                                             ms_mode=self.ms_mode, width=self.width)
        return y, got

    def _launch(self, ctx, state_ptr, state_bytes, inputs, y, out_counts, stream):
        x, counts, flags, delays = inputs
        _native.haas_voice_stream_device(ctx, state_ptr, state_bytes, self.max_frames_per_call, x.data_ptr(),
                                         counts.data_ptr(), flags.data_ptr(), delays.data_ptr(), y.data_ptr(),
                                         out_counts.data_ptr(), self.slots, self.in_channels, max_delay=self.max_delay,
                                         delayed_channel=self.delayed_channel, ms_mode=self.ms_mode, width=self.width,
                                         stream=stream)


class ChainVoicePool(VoicePool):
    """``slots`` slots over a bank of chains ``VelvetNoise`` -> ``HaasEffect``, each slot a voice with a life of its own
    (``decorrelation.decorrelate_voice_pool`` on a bank of ``SignalChain``): a voice goes through its velvet-noise filter
    and then its Haas delay entirely on the device.  Two calls of the C ABI on one stream: ``vnd_voice_stream_f32_dev``
    writes a float32 ``(slots, M + H, 2)`` buffer and an int32 ``out_counts`` that the pool owns (allocated in
    ``reset()``, so nothing is allocated during a capture), and ``vnd_haas_voice_stream_f64_dev`` - with
    ``max_frames_per_call = M + H``, stereo in - reads that ``out_counts`` as its ``counts`` from device memory and gets the
    caller's own ``flags`` and ``delays``; a -1 of stage 1 is a bad count of stage 2 and answers -1.  A call stays a pure
    function of device memory.

    ``latency_frames`` is H, the velvet bank's largest tap index; ``tail_frames`` the bank's largest delay, a voice's own
    tail is ``bank_delays[bank_index]``; ``bank_tables[bank_index]`` is its candidate of the deduplicated velvet bank;
    ``row_frames = M + H + tail_frames``.  For every voice the concatenation of what its calls return equals
    ``bank[i](x_voice)`` - ``chain(x)`` - bit for bit, float64.

    ``process({slot: block}, start={slot: bank_index}, end=[slot], discard=False)`` makes one upload, runs both stages on
    the device and makes one download (``transfers`` counts those of the last call);
    ``process_dev(x, counts, flags, tables, delays)`` only enqueues and can be captured after ``reset()``.  Refusals and
    the rule against mixing the forms are :class:`VoicePool`'s."""

    _out_dtype = np.float64

    def __init__(self, arrays: TapArrays, bank_tables, bank_delays, *, slots: int, in_channels: int, max_frames_per_call: int,
                 ms_encode: bool, velvet_width: Optional[float], delayed_channel: int, ms_mode: bool,
                 haas_width: Optional[float]):
        VoicePool.__init__(self, arrays, bank_tables, slots=slots, in_channels=in_channels,
                           max_frames_per_call=max_frames_per_call, ms_encode=ms_encode, width=velvet_width)
        self.bank_delays = np.ascontiguousarray(bank_delays, np.int32)
        if self.bank_delays.shape != self.bank_tables.shape or self.bank_delays.min() < 0:
            raise ValueError('bank_delays: one delay >= 0 per bank entry')
        self.haas = HaasVoicePool(self.bank_delays, slots=slots, in_channels=2,
                                  max_frames_per_call=self.max_frames_per_call + self.latency_frames,
                                  delayed_channel=delayed_channel, ms_mode=ms_mode, width=haas_width)
        self.max_delay = self.tail_frames = self.haas.max_delay
        self.transfers = {'to_device': 0, 'to_host': 0}
        self._mid = None                      # (float32 (slots, M + H, 2), int32 (slots,)): stage 1's result, on the device
        self._inputs += _slot_ints(self.slots, 'delays')
        # stage 2's: what process_dev checks and the host call carves.  Stage 1 runs through the inherited _call_device
        # with _mid always passed, so these shapes are never what its outputs are allocated from.
        self._outputs = self.haas._outputs

    def _mirror(self):
        VoicePool._mirror(self)
        self.haas_positions = np.zeros(self.slots, np.int64)      # stage 2's: the frames stage 1 has returned

    @property
    def row_frames(self) -> int:
        """Frames per row of the result: ``max_frames_per_call + latency_frames + tail_frames``."""
        return self.haas.row_frames

    def reset(self):
        """End every voice in both stages, unflushed; allocates both states and the intermediate buffers on first use."""
        VoicePool.reset(self)
        self.haas.reset()

    def process_dev(self, x, counts, flags, tables, delays, *, out=None):
        """One call on device tensors, enqueued on the current stream: ``x`` float32 ``(slots, M, in_channels)``,
        ``counts`` / ``flags`` / ``tables`` / ``delays`` int32 ``(slots,)``.  Returns ``(y, out_counts)``: float64
        ``(slots, M + H + max delay, 2)`` and int32 ``(slots,)``; ``out=(y, out_counts)`` takes the caller's.  A bad
        count answers -1 from both stages and leaves the slot alone.  A bad ``delays[b]`` on a slot with work is seen by
        stage 2 only: it answers -1 and stands still, but stage 1 has taken the block and moved on, so the two stages of
        that voice are out of step and its frames of this call are lost - restart the voice (START) before it goes on.
        The dict form cannot send one: its delays come from the bank."""
        return self._process_dev((x, counts, flags, tables, delays), out)

    def _spans(self, counts, flags, entries):
        mid, first = voice_spans(self.positions, counts, flags, self.latency_frames, self.max_frames_per_call)
        out, second = haas_voice_spans(self.haas_positions, mid, flags, self.bank_delays[entries], self.max_delay,
                                       self.haas.max_frames_per_call)
        return out, (first, second)

    def _per_slot(self, entries):
        return self.bank_tables[entries], self.bank_delays[entries]

    def _slot_value(self, index: int):
        return index                          # the bank entry: its table and its delay go up together

    def _commit(self, positions):
        self.positions, self.haas_positions = positions

    # ---- the device -------------------------------------------------------------------------
    def _allocate(self, torch, ctx):
        VoicePool._allocate(self, torch, ctx)
        device = torch.device('cuda', ctx.device)
        self._mid = (torch.empty((self.slots, self.haas.max_frames_per_call, 2), dtype=torch.float32, device=device),
                     torch.empty((self.slots,), dtype=torch.int32, device=device))

    def _call_host(self, x, counts, flags, tables, delays):
        """One upload (the blocks and the four int32 arrays in one buffer), both stages, one download (y and out_counts)."""
        form = self._form
        try:
            return self._call_host_packed(x, (counts, flags, tables, delays))
        finally:
            self.haas._form = form

    def _call_device(self, torch, inputs, y, out_counts):
        x, counts, flags, tables, delays = inputs
        ctx = _native.default_context()
        self._ensure_state(torch, ctx)
        self.haas._ensure_state(torch, ctx)
        mid, mid_counts = self._mid
        VoicePool._call_device(self, torch, (x, counts, flags, tables), mid, mid_counts)
        return self.haas._call_device(torch, (mid, mid_counts, flags, delays), y, out_counts)


# ----------------------------------------------------------------------------
# Haas and chain voice pools whose live voices change their delay, crossfaded   (include/vnd_haas_voice_fade_stream.h)
# ----------------------------------------------------------------------------
def haas_voice_fade_spans(positions, records, counts, flags, delays, max_delay: int, fade_frames: int,
                          max_frames_per_call: Optional[int] = None):
    """``(out_counts, new_positions, new_records, fade_left)`` of one call of a crossfading Haas voice pool
    (``include/vnd_haas_voice_fade_stream.h``), per slot, from the positions and records before the call - ``records`` is
    int64 ``(slots, 3)``: ``s``, ``old``, ``cur``, the delays in frames - the frames pushed, the ``VOICE_START`` /
    ``VOICE_END`` / ``VOICE_SWITCH`` flags and the delays of the call alone - what the device computes from its own state::

        work  = n > 0 or START or END or SWITCH       fresh = START or position == 0
        p = 0 if fresh else position                  e = p + n
        (old, cur, s) = (delay, delay, -F) if fresh else the record
        accept = SWITCH and not fresh and p >= s + F:    (old, cur, s) = (cur, delay, p)
        out_count = n + (max(cur, min(old, max(0, s + F - e))) if END else 0)
        new position = 0 if END else e                fade_left = 0 if END else min(F, max(0, s + F - e))

    An idle slot (no work) answers 0 and keeps its position and its record.  A bad slot answers -1 twice and keeps both:
    ``haas_voice_spans``' bad count or position; a delay outside ``[0, max_delay]`` on a call that takes it (fresh with
    work, or an accepted switch); a stored ``old`` or ``cur`` outside ``[0, max_delay]`` on a slot that goes on with work."""
    pos, n, start, end, p, bad = _voice_head(positions, counts, flags, max_frames_per_call)
    rec = np.asarray(records, np.int64)
    d = np.asarray(delays, np.int64)
    if rec.shape != pos.shape + (3,) or d.shape != pos.shape:
        raise ValueError(f'records of shape {pos.shape + (3,)} and delays of shape {pos.shape}, got {rec.shape}, {d.shape}')
    D, F = int(max_delay), int(fade_frames)
    p, n = np.where(bad, 0, p), np.where(bad, 0, n)          # (no arithmetic on a bad value)
    switch = (np.asarray(flags, np.int64) & VOICE_SWITCH) != 0
    work = (n > 0) | start | end | switch
    fresh = start | (pos == 0)
    s, old, cur = rec[..., 0], rec[..., 1], rec[..., 2]
    kept = (old >= 0) & (old <= D) & (cur >= 0) & (cur <= D)
    accept = ~bad & ~fresh & kept & switch & (p - F >= s)     # p >= s + F, without a sum a planted s could wrap
    bad = bad | (((fresh & work) | accept) & ((d < 0) | (d > D))) | (~fresh & work & ~kept)
    new_s = np.where(fresh, -F, np.where(accept, p, s))
    new_old = np.where(fresh, d, np.where(accept, cur, old))
    new_cur = np.where(fresh | accept, d, cur)
    e = p + n
    left = np.where(new_s >= e, F, np.where(new_s < e - F, 0, new_s + F - e))
    ahead = new_s - e                                         # (read only where s >= e: a fade that begins past e)
    reach = np.where(new_s >= e, np.where(ahead >= new_old, new_old, np.minimum(new_old, ahead + F)),
                     np.minimum(new_old, left))
    still = bad | ~work
    out = np.where(bad, -1, n + np.where(end, np.maximum(new_cur, reach), 0)).astype(np.int64)
    new = np.where(still, pos, np.where(end, 0, e)).astype(np.int64)
    records = np.where(still[..., None], rec, np.stack([new_s, new_old, new_cur], axis=-1)).astype(np.int64)
    fade_left = np.where(bad, -1, np.where(end, 0, left)).astype(np.int64)
    return out, new, records, fade_left


class HaasFadeVoicePool(HaasVoicePool):
    """A :class:`HaasVoicePool` whose live voices change their delay (``decorrelation.decorrelate_fade_voice_pool`` on a
    bank of ``HaasEffect``, ``vnd_haas_voice_fade_stream_f64_dev``): a voice that switches keeps its position and its
    history, and from the first frame it has not yet returned - the delay is causal: its position - its delayed column
    fades over ``fade_frames`` frames from the delay it had to the new one, ``old * fade_gains[0][j] + new * fade_gains[1][j]``
    in float64, before the MS decode and the width.  The fade goes on through the tail of an END, which is as long as
    either delay still contributes.  One fade per voice is in flight: ``fade_left[slot]`` is the number of frames of it the
    slot has yet to return, and a switch is taken only at 0.  ``records[slot]`` is ``(s, old, cur)``: the first frame of the
    slot's latest fade and the delays before and after it.  A voice that never switches returns :class:`HaasVoicePool`'s
    bytes.

    * ``process({slot: block}, start=..., end=..., switch={slot: bank_index})`` - the dict form, with
      :class:`FadeVoicePool`'s refusals before any device call: a switch on a slot with no live voice, together with a
      start of that slot, to an index outside the bank, or while ``fade_left[slot] > 0``.  One upload and one download.
    * ``process_dev(x, counts, flags, delays)`` - flags may carry ``VOICE_SWITCH``, and ``delays[b]`` is read when a voice
      begins and when its switch is accepted; a switch that comes while ``fade_left_dev[b] > 0`` is ignored.
      ``(y, out_counts)`` are :class:`HaasVoicePool`'s, so every meter attaches unchanged; ``fade_left_dev`` is the pool's
      own int32 ``(slots,)`` tensor at a fixed address, written by every call."""

    def __init__(self, bank_delays, *, slots: int, in_channels: int, max_frames_per_call: int, delayed_channel: int,
                 ms_mode: bool, fade_frames: int, fade_gains: np.ndarray, width: Optional[float] = None):
        self.fade_frames, self.fade_gains = _fade_settings(fade_frames, fade_gains)
        self.transfers = {'to_device': 0, 'to_host': 0}
        self._fade = None                     # (gains on the device or None, fade_left_dev)
        HaasVoicePool.__init__(self, bank_delays, slots=slots, in_channels=in_channels,
                               max_frames_per_call=max_frames_per_call, delayed_channel=delayed_channel, ms_mode=ms_mode,
                               width=width)

    def _mirror(self):
        HaasVoicePool._mirror(self)
        self.records = np.zeros((self.slots, 3), np.int64)        # (s, old, cur); a slot at position 0 takes its own from the call
        self.fade_left = np.zeros(self.slots, np.int64)

    fade_left_dev = FadeVoicePool.fade_left_dev

    def process(self, blocks=None, *, start=None, end=(), switch=None, discard: bool = False):
        """:meth:`HaasVoicePool.process` with ``switch``: ``{slot: bank_index}``, the live voices that change to another
        bank entry's delay with this call.  The fade begins at the first frame the slot returns in this call."""
        return FadeVoicePool.process(self, blocks, start=start, end=end, switch=switch, discard=discard)

    def _spans(self, counts, flags, delays):
        out, positions, records, fade_left = haas_voice_fade_spans(self.positions, self.records, counts, flags, delays,
                                                                   self.max_delay, self.fade_frames, self.max_frames_per_call)
        return out, (positions, records, fade_left)

    _commit = FadeVoicePool._commit

    # ---- the device -------------------------------------------------------------------------
    def _state_bytes(self, ctx) -> int:
        from . import _native_haas_fade
        return _native_haas_fade.haas_voice_fade_stream_state_bytes(self.slots, self.in_channels, self.max_delay,
                                                                    self.max_frames_per_call, self.fade_frames)

    def _allocate(self, torch, ctx):
        HaasVoicePool._allocate(self, torch, ctx)
        device = torch.device('cuda', ctx.device)
        gains = torch.from_numpy(self.fade_gains).to(device) if self.fade_frames else None     # uploaded once
        self._fade = (gains, torch.zeros((self.slots,), dtype=torch.int32, device=device))

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        from . import _native_haas_fade
        _native_haas_fade.haas_voice_fade_stream_reset_device(ctx, state_ptr, state_bytes, self.slots, self.in_channels,
                                                              self.max_delay, self.max_frames_per_call, self.fade_frames,
                                                              stream=stream)

    def _call_host(self, x, counts, flags, delays):
        """One upload (the blocks and the three int32 arrays in one buffer), the call, one download (y and out_counts)."""
        return self._call_host_packed(x, (counts, flags, delays))

    def _launch(self, ctx, state_ptr, state_bytes, inputs, y, out_counts, stream):
        from . import _native_haas_fade
        x, counts, flags, delays = inputs
        gains, fade_left = self._fade
        _native_haas_fade.haas_voice_fade_stream_device(
            ctx, state_ptr, state_bytes, self.max_frames_per_call, self.fade_frames,
            None if gains is None else gains.data_ptr(), x.data_ptr(), counts.data_ptr(), flags.data_ptr(), delays.data_ptr(),
            y.data_ptr(), out_counts.data_ptr(), fade_left.data_ptr(), self.slots, self.in_channels, max_delay=self.max_delay,
            delayed_channel=self.delayed_channel, ms_mode=self.ms_mode, width=self.width, stream=stream)


class ChainFadeVoicePool(FadeVoicePool):
    """A :class:`ChainVoicePool` whose live voices change their bank entry - filter and delay together
    (``decorrelation.decorrelate_fade_voice_pool`` on a bank of ``SignalChain``): :class:`FadeVoicePool`
    (``vnd_voice_fade_stream_f32_dev``) and then :class:`HaasFadeVoicePool` (``vnd_haas_voice_fade_stream_f64_dev``),
    composed as :class:`ChainVoicePool` composes its stages: stage 2 has ``max_frames_per_call = M + H``, reads stage 1's
    ``out_counts`` from device memory as its counts, and gets the caller's ``flags`` - ``VOICE_SWITCH`` included - and
    ``delays``, with the same ``fade_frames`` and gains.  The contract is composition: for every schedule the result is
    :class:`HaasFadeVoicePool`'s rule applied to what :class:`FadeVoicePool` returned.  Stage 2's position is the number of
    frames stage 1 has returned, so a switch both stages accept starts both fades at the same output frame.

    One corner: while a voice is inside its first H frames stage 1 has returned nothing, so stage 2 stands at position 0
    and is *fresh*: a switch there gives stage 2 the new delay without a fade, where stage 1 fades its filter.

    ``fade_left`` and ``fade_left_dev`` are the elementwise maximum of the two stages'; on the device the maximum is
    written into the pool's own tensor by every call.  ``records`` are stage 1's and ``haas_records`` stage 2's.
    ``process(..., switch={slot: bank_index})`` refuses a switch while ``fade_left[slot] > 0``, so in the dict form both
    stages take a switch or - at the corner above - stage 2 takes it fresh; ``process_dev(x, counts, flags, tables,
    delays)`` lets each stage apply its own rule.  ``(y, out_counts)`` are :class:`ChainVoicePool`'s."""

    _out_dtype = np.float64

    def __init__(self, arrays: TapArrays, bank_tables, bank_delays, *, slots: int, in_channels: int, max_frames_per_call: int,
                 fade_frames: int, fade_gains: np.ndarray, ms_encode: bool, velvet_width: Optional[float],
                 delayed_channel: int, ms_mode: bool, haas_width: Optional[float]):
        FadeVoicePool.__init__(self, arrays, bank_tables, slots=slots, in_channels=in_channels,
                               max_frames_per_call=max_frames_per_call, fade_frames=fade_frames, fade_gains=fade_gains,
                               ms_encode=ms_encode, width=velvet_width)
        self.bank_delays = np.ascontiguousarray(bank_delays, np.int32)
        if self.bank_delays.shape != self.bank_tables.shape or self.bank_delays.min() < 0:
            raise ValueError('bank_delays: one delay >= 0 per bank entry')
        self.haas = HaasFadeVoicePool(self.bank_delays, slots=slots, in_channels=2,
                                      max_frames_per_call=self.max_frames_per_call + self.latency_frames,
                                      delayed_channel=delayed_channel, ms_mode=ms_mode, fade_frames=self.fade_frames,
                                      fade_gains=self.fade_gains, width=haas_width)
        self.max_delay = self.tail_frames = self.haas.max_delay
        self._mid = None                      # (float32 (slots, M + H, 2), int32 (slots,)): stage 1's result, on the device
        self._left = None                     # int32 (slots,): the maximum of the stages' fade_left, on the device
        self._inputs += _slot_ints(self.slots, 'delays')
        self._outputs = self.haas._outputs    # stage 2's, as ChainVoicePool: stage 1 always gets _mid

    def _mirror(self):
        FadeVoicePool._mirror(self)
        self.haas_positions = np.zeros(self.slots, np.int64)      # stage 2's: the frames stage 1 has returned
        self.haas_records = np.zeros((self.slots, 3), np.int64)

    row_frames = ChainVoicePool.row_frames
    reset = ChainVoicePool.reset

    @property
    def fade_left_dev(self):
        """The int32 ``(slots,)`` device tensor every call writes the maximum of the two stages' ``fade_left`` to;
        allocated by ``reset()``."""
        if self._left is None:
            raise RuntimeError('fade_left_dev is allocated with the state: call reset() first')
        return self._left

    def process_dev(self, x, counts, flags, tables, delays, *, out=None):
        """:meth:`ChainVoicePool.process_dev`, where flags may carry ``VOICE_SWITCH``: stage 1 reads ``tables[b]`` and stage
        2 ``delays[b]`` when a voice begins and when that stage accepts the switch."""
        return self._process_dev((x, counts, flags, tables, delays), out)

    def _spans(self, counts, flags, entries):
        mid, first, records, left = voice_fade_spans(self.positions, self.records, counts, flags, self.bank_tables[entries],
                                                     self.latency_frames, self.fade_frames, self.max_frames_per_call)
        out, second, haas_records, haas_left = haas_voice_fade_spans(
            self.haas_positions, self.haas_records, mid, flags, self.bank_delays[entries], self.max_delay, self.fade_frames,
            self.haas.max_frames_per_call)
        return out, (first, records, second, haas_records, np.maximum(left, haas_left))

    _per_slot = ChainVoicePool._per_slot
    _slot_value = ChainVoicePool._slot_value

    def _commit(self, state):
        self.positions, self.records, self.haas_positions, self.haas_records, self.fade_left = state

    # ---- the device -------------------------------------------------------------------------
    def _allocate(self, torch, ctx):
        FadeVoicePool._allocate(self, torch, ctx)
        device = torch.device('cuda', ctx.device)
        self._mid = (torch.empty((self.slots, self.haas.max_frames_per_call, 2), dtype=torch.float32, device=device),
                     torch.empty((self.slots,), dtype=torch.int32, device=device))
        self._left = torch.zeros((self.slots,), dtype=torch.int32, device=device)

    _call_host = ChainVoicePool._call_host

    def _call_device(self, torch, inputs, y, out_counts):
        x, counts, flags, tables, delays = inputs
        ctx = _native.default_context()
        self._ensure_state(torch, ctx)
        self.haas._ensure_state(torch, ctx)
        mid, mid_counts = self._mid
        VoicePool._call_device(self, torch, (x, counts, flags, tables), mid, mid_counts)
        out = self.haas._call_device(torch, (mid, mid_counts, flags, delays), y, out_counts)
        torch.maximum(self._fade[1], self.haas._fade[1], out=self._left)       # (no allocation: capturable)
        return out
