"""Cross-correlograms on the GPU (``vnd_correlogram_f32_dev``, include/vnd_analysis.h).

The reference measures decorrelation with ``utils/dsp.py:313`` ``cross_correlogram``: per window of W samples,
``np.correlate(x_w, y_w, 'full')`` over ``sqrt(x_w.x_w * y_w.y_w) + eps`` - W^2 multiply-adds a window.  Here:

* ``utils.dsp.cross_correlogram`` - the reference's signature; on the device where covered, NumPy otherwise;
* :func:`cross_correlogram_batched` - ``(B, n)`` pairs, or channel 0 against channel 1 of a ``(B, n, 2)`` signal in
  place; NumPy in, NumPy out (pinned); a float32 torch tensor on the device in, a device tensor out;
* :func:`set_correlogram_device` and the pure routing rule :func:`correlogram_covers`; :func:`device_route`, the
  rule of every ``set_*_device`` switch of the package;
* :func:`cross_correlogram_stream` - the same rows, block by block, for a pool of live streams
  (``include/vnd_correlogram_stream.h``): a :class:`CorrelogramStream`;
* :func:`cross_correlogram_voice_pool` - the same rows for a pool of voices that start, end and push blocks of their own
  sizes (``include/vnd_correlogram_voice_stream.h``): a :class:`CorrelogramVoicePool`, which meters a
  ``decorrelate_voice_pool`` on the device; :func:`correlogram_voice_spans` is the device's mirror;
* :func:`stereo_image_voice_pool` - the eight polar moments behind ``symmetry_aware_objective`` for such a pool of voices
  (``include/vnd_polar_voice_stream.h``): a :class:`PolarVoicePool`; :func:`polar_voice_spans` is the device's mirror and
  :func:`polar_moments_ordered` a NumPy restatement of its summation order.

Numerics: each correlation output is one float64 FMA chain over exact products, rounded once; the
energies are float64 sums rounded once; the normaliser is NumPy 2's float32 arithmetic.  The result is within one
float32 ulp of the same formula with exact sums and within ``(2W + 4) 2^-24`` of the reference's float32 result.
Without a device every call is the NumPy code.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from .streaming import (_INT32_MAX, BlockStream, _MeterPool, _sample_dtype, _slot_ints, _SlotPool,  # noqa: F401
                        _valid_voice_spans, _voice_head)
from .utils.dsp import EPSILON, correlogram_sizes, to_float32

MAX_WINDOW = _native.CORRELOGRAM_MAX_WINDOW
_torch = _native.torch_module          # the name this module's device paths look torch up by

_correlogram_device: Optional[bool] = None


def set_correlogram_device(enabled: Optional[bool]) -> None:
    """Where ``cross_correlogram`` (and :func:`cross_correlogram_batched`) runs.

    ``None`` (default): on the GPU when a gfx950 device is present and the call is covered (:func:`correlogram_covers`),
    otherwise the NumPy code.  ``True``: the device for every covered call; such a call raises ``RuntimeError`` when
    there is no device.  ``False``: always NumPy, bit-identical to the reference."""
    global _correlogram_device
    if enabled is not None and not isinstance(enabled, (bool, np.bool_)):
        raise TypeError(f'set_correlogram_device takes True, False or None, not {enabled!r}')
    _correlogram_device = None if enabled is None else bool(enabled)


def correlogram_covers(n_frames: int, window: int, hop: int, num_lags: int, epsilon) -> bool:
    """Whether a correlogram of these sample counts has a device form: 1 <= window <= MAX_WINDOW, hop >= 1,
    1 <= num_lags < 2^31, and ``epsilon`` a Python float (or an int below 2^24) whose float32 value is finite - NumPy 2
    then adds it in float32, as the kernel does; a NumPy scalar would change the promotion.  Everything else keeps the
    NumPy code and its exceptions (hop 0: ZeroDivisionError, window 0: ValueError, ...)."""
    for v in (n_frames, window, hop, num_lags):
        if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)):
            return False
    if n_frames < 0 or not 1 <= window <= MAX_WINDOW or not 1 <= hop <= _INT32_MAX or not 1 <= num_lags <= _INT32_MAX:
        return False
    if type(epsilon) is int:
        return abs(epsilon) < 2 ** 24
    if type(epsilon) is not float:
        return False
    with np.errstate(over='ignore'):
        return bool(np.isfinite(np.float32(epsilon)))


def _gpu_present() -> bool:
    """The package's one probe for a device: every ``set_*_device`` route (:func:`device_route`) reads it here."""
    try:
        _native.default_context()
        return True
    except RuntimeError:                                  # no built extension, no device, not a gfx950
        return False


def device_route(setting: Optional[bool], covered: bool, refusal: str) -> bool:
    """The rule of every ``set_*_device`` switch (this module's, ``set_haas_scan_device``, ``set_velvet_search_device``,
    ``set_white_noise_device``) for one call: ``False``, or a call without a device form (``covered`` False), runs on the host; ``True`` on the
    device, raising ``RuntimeError(refusal)`` when there is none; ``None`` on the device when one is present."""
    if setting is False or not covered:
        return False
    present = _gpu_present()
    if setting is True and not present:
        raise RuntimeError(refusal)
    return present


def use_device(n_frames: int, window: int, hop: int, num_lags: int, epsilon) -> bool:
    """The routing decision of one call: :func:`correlogram_covers` and :func:`set_correlogram_device`."""
    return device_route(_correlogram_device, correlogram_covers(n_frames, window, hop, num_lags, epsilon),
                        'set_correlogram_device(True): no gfx950 device (or no built extension) to run on')


def _windows(n_frames: int, window: int, hop: int) -> int:
    return (n_frames - window) // hop + 1 if n_frames >= window else 0


def _launch(torch, ctx, x_ptr: int, y_ptr: int, batch: int, n: int, stream_stride: int, frame_stride: int, window: int,
            hop: int, num_lags: int, epsilon, device):
    out = torch.empty((batch, _windows(n, window, hop), num_lags), dtype=torch.float32, device=device)
    if batch and out.numel():
        _native.correlogram_device(ctx, x_ptr, y_ptr, out.data_ptr(), batch, n, max(1, stream_stride), frame_stride,
                                   window=window, hop=hop, num_lags=num_lags, eps=float(epsilon),
                                   stream=torch.cuda.current_stream(device).cuda_stream)
    return out


def correlogram_numpy_batch(x: np.ndarray, y: Optional[np.ndarray], window: int, hop: int, num_lags: int,
                            epsilon) -> np.ndarray:
    """Device correlograms of float32 host signals: ``x``, ``y`` ``(B, n)``, or ``x`` ``(B, n, 2)`` with ``y`` None
    (channel 0 against channel 1, uploaded as it is).  Float32 ``(B, windows, num_lags)`` in pinned memory."""
    torch = _torch()
    ctx = _native.default_context()
    device = torch.device('cuda', ctx.device)
    batch, n = x.shape[:2]
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(device)
    if y is None:
        out_d = _launch(torch, ctx, xd.data_ptr(), xd.data_ptr() + 4, batch, n, n * 2, 2, window, hop, num_lags, epsilon,
                        device)
    else:
        yd = torch.from_numpy(np.ascontiguousarray(y)).to(device)
        out_d = _launch(torch, ctx, xd.data_ptr(), yd.data_ptr(), batch, n, n, 1, window, hop, num_lags, epsilon, device)
    out = _native.pinned_pool.empty(tuple(out_d.shape), np.float32)
    torch.from_numpy(out).copy_(out_d)
    return out


def _tensor_pair(torch, x, y, device):
    """Device pointers and strides of a (x, y) pair of float32 tensors on ``device``: ``(x_ptr, y_ptr, stream_stride,
    frame_stride, keep)`` (``keep``: tensors that must outlive the launch)."""
    if y is None:
        if x.stride(2) != 1 or x.stride(1) < 1:
            x = x.contiguous()
        return x.data_ptr(), x.data_ptr() + 4, x.stride(0), x.stride(1), (x,)
    if x.stride() != y.stride() or x.stride(1) < 1:
        x, y = x.contiguous(), y.contiguous()
    return x.data_ptr(), y.data_ptr(), x.stride(0), x.stride(1), (x, y)


def _check_batch(x, y):
    if y is None:
        if len(x.shape) != 3 or x.shape[2] != 2:
            raise ValueError(f'with y=None, x must be (batch, n, 2): got shape {tuple(x.shape)}')
    else:
        if len(x.shape) != 2 or tuple(x.shape) != tuple(y.shape):
            raise ValueError(f'x and y must both be (batch, n): got shapes {tuple(x.shape)} and {tuple(y.shape)}')


def cross_correlogram_batched(x, y=None, *, sample_rate_hz: int = 44100, max_lag_seconds: float = 0.02,
                              window_size_seconds: float = 0.02, stride_seconds: float = 0.01, epsilon: float = EPSILON):
    """``cross_correlogram`` of B stream pairs: float32 ``(B, windows, 2 max_lag + 1)``, equal bit for bit to stacking
    ``cross_correlogram(x[b], y[b])`` (``(x[b, :, 0], x[b, :, 1])`` for a ``(B, n, 2)`` ``x`` with ``y`` None - the
    shape ``decorrelate_batched`` returns, correlated in place).  NumPy in, NumPy out.  A float32 torch tensor on the
    device in, a device tensor out, with no host transfer.  Calls the device does not cover take the per-stream loop."""
    window, hop, max_lag = correlogram_sizes(sample_rate_hz, max_lag_seconds, window_size_seconds, stride_seconds)
    num_lags = 2 * max_lag + 1
    kw = dict(sample_rate_hz=sample_rate_hz, max_lag_seconds=max_lag_seconds, window_size_seconds=window_size_seconds,
              stride_seconds=stride_seconds, epsilon=epsilon)
    is_tensor = _native.is_torch(x)
    if is_tensor:
        torch = _torch()
        _check_batch(x, y)
        if y is not None and (not _native.is_torch(y) or y.device != x.device):
            raise ValueError('x and y must be tensors on the same device')
        ctx_device = None
        try:
            ctx_device = torch.device('cuda', _native.default_context().device)
        except RuntimeError:
            pass
        on_device = (x.dtype == torch.float32 and (y is None or y.dtype == torch.float32) and x.device == ctx_device
                     and use_device(x.shape[1], window, hop, num_lags, epsilon))
        if on_device:
            ctx = _native.default_context()
            xp, yp, ss, fs, keep = _tensor_pair(torch, x, y, x.device)
            out = _launch(torch, ctx, xp, yp, x.shape[0], x.shape[1], ss, fs, window, hop, num_lags, epsilon, x.device)
            del keep
            return out
        host = cross_correlogram_batched(x.detach().cpu().numpy(), None if y is None else y.detach().cpu().numpy(), **kw)
        return torch.from_numpy(np.ascontiguousarray(host)).to(x.device)

    x = np.asarray(x)
    y = None if y is None else np.asarray(y)
    _check_batch(x, y)
    xs = to_float32(x)
    ys = None if y is None else to_float32(y)
    if len(xs) and use_device(xs.shape[1], window, hop, num_lags, epsilon):
        return correlogram_numpy_batch(xs, ys, window, hop, num_lags, epsilon)
    from .utils.dsp import cross_correlogram
    pairs = [(xs[b, :, 0], xs[b, :, 1]) if ys is None else (xs[b], ys[b]) for b in range(len(xs))]
    if not pairs:
        return np.zeros((0, _windows(xs.shape[1], window, hop), num_lags), np.float32)
    return np.stack([cross_correlogram(a, b, **kw) for a, b in pairs])


def stream_rows(position: int, n_in: int, window: int, hop: int):
    """``(first, end)``: the rows ``[first, end)`` - windows, counted from 0 - that a call pushing ``n_in`` frames at
    ``position`` (frames pushed before it) completes (``include/vnd_correlogram_stream.h``)."""
    return _windows(position, window, hop), _windows(position + n_in, window, hop)


class CorrelogramStream(BlockStream):
    """``cross_correlogram`` of a pool of ``num_streams`` stream pairs, block by block (``cross_correlogram_stream``).

    ``process(x, y=None)`` pushes the next block of every stream: ``x`` ``(S, B, 2)`` (channel 0 against channel 1, read in
    place) or ``(B, 2)`` when ``S == 1``; or ``x``, ``y`` ``(S, B)``, or ``(B,)`` when ``S == 1``.  ``0 <= B <=
    max_frames_per_call``, free to change from call to call.  It returns the rows of the windows that became final, float32
    ``(S, rows, num_lags)`` (``(rows, num_lags)`` for the unbatched forms); their concatenation equals
    :func:`cross_correlogram_batched` of the whole signal bit for bit.  NumPy in, NumPy out (the block goes through the
    device and back, synchronously).  A float32 device tensor in, a device tensor out, enqueued on the current stream with
    no host copy or synchronisation.  Float64 NumPy blocks are cast to float32 as ``cross_correlogram`` casts them, float64
    device tensors by torch on the device (round to nearest even, as ``astype``).

    ``flush()`` returns the zero rows left - windows that never complete are dropped, as in the reference - and ends the
    signal: ``process`` raises ``RuntimeError`` after it until ``reset()``.  ``window``, ``hop``, ``num_lags``: the sizes
    in samples; ``position``: the frames pushed per stream.  Every argument and shape check runs before any device call;
    the state (a ring of the last ``window - 1`` frames per stream) is allocated on first use.  The stream always runs
    on the device: ``set_correlogram_device`` is not consulted, and without a device the first call that needs one
    raises ``RuntimeError``."""

    _noun = 'block'

    def __init__(self, num_streams: int, *, window: int, hop: int, num_lags: int, epsilon, max_frames_per_call: int):
        super().__init__(num_streams=num_streams, max_frames_per_call=max_frames_per_call)
        if not correlogram_covers(0, window, hop, num_lags, epsilon):
            raise ValueError(f'window {window}, hop {hop}, {num_lags} lags and epsilon {epsilon!r} have no device form '
                             f'(correlogram_covers is False) and the stream has no NumPy one: use cross_correlogram')
        self.window, self.hop, self.num_lags, self.epsilon = int(window), int(hop), int(num_lags), epsilon

    @property
    def _out_width(self) -> int:
        return self.num_lags

    def process(self, x, y=None):
        """Push the next block of every stream; returns the rows that became final."""
        return self._process((x, y), False)

    # ---- checks --------------------------------------------------------------------------
    def _cast(self, v, is_torch: bool):
        if is_torch:
            torch = _torch()
            if not v.is_cuda:
                raise ValueError('a torch block must be a device tensor (NumPy arrays take the host path)')
            if v.dtype == torch.float64:
                return v.to(torch.float32)
            if v.dtype != torch.float32:
                raise TypeError(f'device blocks must be float32 or float64, got {v.dtype}')
            return v
        v = np.asarray(v)
        if v.dtype.kind not in 'biuf':
            raise TypeError(f'blocks must be real numbers, got {v.dtype}')
        return to_float32(v)

    def _chunk(self, x, y):
        """``((xs, ys), squeeze, is_torch)``: the block as ``(S, B, 2)`` and None, or two ``(S, B)``."""
        is_torch = _native.is_torch(x)
        if y is not None and _native.is_torch(y) != is_torch:
            raise ValueError('x and y must both be NumPy arrays or both device tensors')
        xs = self._cast(x, is_torch)
        ys = None if y is None else self._cast(y, is_torch)
        S = self.num_streams
        shape = tuple(xs.shape)
        if ys is None:
            if len(shape) == 2 and S == 1:
                xs, squeeze = xs.reshape(1, *shape), True
            elif len(shape) == 3:
                squeeze = False
            else:
                raise ValueError(f'with y=None, x must be (num_streams={S}, frames, 2)'
                                 + (' or (frames, 2)' if S == 1 else '') + f': got shape {shape}')
            if xs.shape[0] != S or xs.shape[2] != 2:
                raise ValueError(f'block of shape {shape} does not match the pool: {S} streams, 2 channels')
        else:
            if tuple(ys.shape) != shape:
                raise ValueError(f'x and y must have one shape: got {shape} and {tuple(ys.shape)}')
            if is_torch and ys.device != xs.device:
                raise ValueError('x and y must be tensors on the same device')
            if len(shape) == 1 and S == 1:
                xs, ys, squeeze = xs.reshape(1, -1), ys.reshape(1, -1), True
            elif len(shape) == 2:
                squeeze = False
            else:
                raise ValueError(f'x and y must be (num_streams={S}, frames)' + (' or (frames,)' if S == 1 else '')
                                 + f': got shape {shape}')
            if xs.shape[0] != S:
                raise ValueError(f'block of shape {shape} does not match the pool of {S} streams')
        if xs.shape[1] > self.max_frames_per_call:
            raise ValueError(f'{xs.shape[1]} frames in one call, above max_frames_per_call={self.max_frames_per_call}')
        return (xs, ys), squeeze, is_torch

    def _lead(self, block):
        return block[0]

    # ---- the device -------------------------------------------------------------------------
    def _span(self, n_in: int, final: bool):
        return stream_rows(self.position, n_in, self.window, self.hop)

    def _state_bytes(self, ctx) -> int:
        return _native.correlogram_stream_state_bytes(self.num_streams, self.window, self.max_frames_per_call)

    def _launch(self, torch, ctx, state, state_bytes: int, block, out, n_in: int, final: bool, stream):
        xs, ys = block
        if ys is None:
            if xs.stride(2) != 1 or not 1 <= xs.stride(1) <= _INT32_MAX or (self.num_streams > 1 and xs.stride(0) < 1):
                xs = xs.contiguous()
            read, xp, yp = (xs,), xs.data_ptr(), xs.data_ptr() + 4
        else:
            if (xs.stride() != ys.stride() or not 1 <= xs.stride(1) <= _INT32_MAX
                    or (self.num_streams > 1 and xs.stride(0) < 1)):
                xs, ys = xs.contiguous(), ys.contiguous()
            read, xp, yp = (xs, ys), xs.data_ptr(), ys.data_ptr()
        got = _native.correlogram_stream_device(
            ctx, state.data_ptr(), state_bytes, self.max_frames_per_call, xp, yp, max(1, xs.stride(0)), xs.stride(1),
            out.data_ptr(), self.num_streams, self.position, n_in, window=self.window, hop=self.hop,
            num_lags=self.num_lags, eps=float(self.epsilon), stream=stream.cuda_stream)
        return got, read

    def _call_host(self, block, n_in: int, rows: int, final: bool):
        """The block goes up, through :meth:`_call_device`, and its rows come back."""
        torch = _torch()
        device = torch.device('cuda', _native.default_context().device)
        up = tuple(None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(device) for v in block)
        out_d = self._call_device(up, n_in, rows, final)
        out = _native.pinned_pool.empty(tuple(out_d.shape), np.float32)
        if out.size:
            torch.from_numpy(out).copy_(out_d)
        return out


def cross_correlogram_stream(num_streams: int = 1, *, sample_rate_hz: int = 44100, max_lag_seconds: float = 0.02,
                             window_size_seconds: float = 0.02, stride_seconds: float = 0.01, epsilon: float = EPSILON,
                             max_frames_per_call: int = 4800) -> CorrelogramStream:
    """A :class:`CorrelogramStream`: ``cross_correlogram`` with these arguments, computed block by block for a pool of
    ``num_streams`` stream pairs as their frames arrive.  The sizes come from ``correlogram_sizes`` as for the one-shot
    call.  Sizes the device does not cover (:func:`correlogram_covers`) and pools above ``MAX_STREAMS_PER_CALL`` raise
    ``ValueError`` here: there is no NumPy stream.  ``set_correlogram_device`` is not consulted."""
    window, hop, max_lag = correlogram_sizes(sample_rate_hz, max_lag_seconds, window_size_seconds, stride_seconds)
    return CorrelogramStream(num_streams, window=window, hop=hop, num_lags=2 * max_lag + 1, epsilon=epsilon,
                             max_frames_per_call=max_frames_per_call)


# ----------------------------------------------------------------------------
# The correlogram of a voice pool   (include/vnd_correlogram_voice_stream.h)
# ----------------------------------------------------------------------------
def correlogram_voice_spans(positions, counts, flags, window: int, hop: int, max_frames_per_call: Optional[int] = None):
    """``(out_counts, new_positions)`` of one call of a correlogram voice pool
    (``include/vnd_correlogram_voice_stream.h``), per slot, from the positions before the call, the frames pushed and the
    ``VOICE_START`` / ``VOICE_END`` flags alone - what the device computes from its own state::

        p = START ? 0 : position        wc(q) = (q - W) // H + 1 if q >= W else 0
        out_count = wc(p + n) - wc(p)   new position = END ? 0 : p + n

    A count below 0 (or above ``max_frames_per_call``, when given), or without START a position outside ``[0, 2^60]``,
    answers -1 and leaves the position as it was."""
    pos, n, start, end, p, bad = _voice_head(positions, counts, flags, max_frames_per_call)
    W, H = int(window), int(hop)
    if W < 1 or H < 1:
        raise ValueError(f'window and hop must be >= 1, got {window} and {hop}')
    p, n = np.where(bad, 0, p), np.where(bad, 0, n)          # (no arithmetic on a bad value)

    def complete(q):
        return np.where(q >= W, (q - W) // H + 1, 0)
    out = np.where(bad, -1, complete(p + n) - complete(p)).astype(np.int64)
    new = np.where(bad, pos, np.where(end, 0, p + n)).astype(np.int64)
    return out, new


class CorrelogramVoicePool(_MeterPool):
    """``cross_correlogram`` of ``slots`` voices, each with a life of its own (:func:`cross_correlogram_voice_pool`,
    ``vnd_correlogram_voice_stream_*_dev``): voices start and end on any call and push blocks of any size up to
    ``max_frames_per_call`` or none.  The position lives in the device state, one per slot, so a call is a pure function
    of device memory.  A call returns, per slot, the rows of the windows that became final - at most ``rows_per_call`` -
    and for every voice the concatenation of its rows, from its start up to and including its end, equals
    :func:`cross_correlogram_batched` of its whole signal bit for bit.  Windows that never complete are dropped, as in the
    reference: an end has no tail.

    Two forms; a pool is used through one of them (mixing them raises ``RuntimeError`` until ``reset()``):

    * ``process({slot: block}, start=[slot, ...], end=[slot, ...], discard=False)`` - float32 or float64 NumPy blocks
      ``(n, 2)`` in (channel 0 against channel 1; float64 is cast as ``cross_correlogram`` casts it),
      ``{slot: float32 (rows, num_lags)}`` out for every slot that got a block or ended.  One upload and one download
      (``transfers`` counts those of the last call); every refusal comes before any device call.
    * ``process_dev(x, counts, flags, *, out=None)`` - ``x`` ``(slots, max_frames_per_call, 2)`` of the pool's ``dtype``
      and int32 ``(slots,)`` ``counts`` and ``flags`` on the device; returns ``(rows, out_counts)``.  It only enqueues on
      the current stream and can be captured with ``torch.cuda.graph`` after a ``reset()``.  To meter a decorrelating
      pool, build the meter with ``max_frames_per_call=pool.row_frames`` (and ``dtype='float64'`` for a Haas or chain
      pool) and hand it that pool's ``y`` and ``out_counts`` and the caller's ``flags``: a -1 of the pool is a bad count
      here and answers -1.  A float64 sample is cast to float32 inside the kernel, round to nearest even."""

    _out_dtype = np.float32

    def __init__(self, slots: int, *, window: int, hop: int, num_lags: int, epsilon, max_frames_per_call: int,
                 dtype='float32'):
        _MeterPool.__init__(self, slots, max_frames_per_call, dtype)
        self._block_dtype = np.float32            # the dict form casts float64 blocks, as cross_correlogram does
        if not correlogram_covers(0, window, hop, num_lags, epsilon):
            raise ValueError(f'window {window}, hop {hop}, {num_lags} lags and epsilon {epsilon!r} have no device form '
                             f'(correlogram_covers is False) and the pool has no NumPy one: use cross_correlogram')
        self.window, self.hop, self.num_lags, self.epsilon = int(window), int(hop), int(num_lags), epsilon
        # the fixed grid of the pool (include/vnd_correlogram_voice_stream.h): window groups of 4 rows x column tiles of
        # 1024 lags per slot, one grid dimension; 2^23 workgroups a launch
        groups, tiles = -(-self.rows_per_call // 4), -(-self.num_lags // 1024)
        if groups * tiles > 65535 or self.slots * groups * tiles > 1 << 23 \
                or self.slots * self.rows_per_call * self.num_lags > 1 << 40:
            raise ValueError(f'{self.slots} slots of {self.rows_per_call} rows of {self.num_lags} lags per call are more than '
                             f'one launch takes: raise the stride or lower max_frames_per_call')
        S = self.slots
        self._inputs = (('x', (S, self.max_frames_per_call, 2), self.dtype.name, None),) + _slot_ints(S, 'counts', 'flags')
        self._outputs = (('rows', (S, self.rows_per_call, self.num_lags), 'float32', 'empty'),
                         ('out_counts', (S,), 'int32', 'empty'))
        self._mirror()

    @property
    def rows_per_call(self) -> int:
        """RC: the most rows a call returns per slot, ``ceil(max_frames_per_call / hop)``."""
        return -(-self.max_frames_per_call // self.hop)

    @property
    def _out_width(self) -> int:
        return self.num_lags

    def process(self, blocks=None, *, start=(), end=(), discard: bool = False):
        """One call of the dict form.  ``blocks``: ``{slot: (n, 2) float32 or float64 array}``,
        ``0 <= n <= max_frames_per_call``; ``start``: the slots whose voice begins with this call; ``end``: the slots whose
        voice ends with it.  Returns ``{slot: float32 (rows, num_lags)}`` for every slot that got a block or ended.  Raises
        before any device call, as the other voice pools do: ``ValueError`` for a slot outside the pool or named twice, a
        block or an end for a slot that was never started, a start on a live slot (``discard=True`` allows it: the voice
        it held is dropped), a block above ``max_frames_per_call`` or not ``(n, 2)``; ``TypeError`` for a block that is
        neither float32 nor float64."""
        self._require_form('dict')
        starts = self._start_slots(start)
        cast = {}
        for slot, block in dict(blocks or {}).items():
            a = np.asarray(block)
            cast[slot] = to_float32(a) if a.dtype == np.float64 else a
        return _SlotPool.process(self, cast, start=starts, end=end, discard=discard)

    def process_dev(self, x, counts, flags, *, out=None):
        """One call on device tensors, enqueued on the current stream: ``x`` ``(slots, M, 2)`` of the pool's dtype,
        ``counts`` / ``flags`` int32 ``(slots,)``.  Returns ``(rows, out_counts)``: float32
        ``(slots, rows_per_call, num_lags)`` - the first ``out_counts[b]`` rows of row-block b are written, nothing at or
        past them - and int32 ``(slots,)``; ``out=(rows, out_counts)`` takes the caller's.  No check reads device memory;
        bad per-slot values answer -1 (``include/vnd_correlogram_voice_stream.h``)."""
        return self._process_dev((x, counts, flags), out)

    # ---- what _SlotPool asks for ---------------------------------------------------------------
    def _spans(self, counts, flags, tables):
        return correlogram_voice_spans(self.positions, counts, flags, self.window, self.hop, self.max_frames_per_call)

    # ---- the device -------------------------------------------------------------------------
    def _state_bytes(self, ctx) -> int:
        return _native.correlogram_voice_stream_state_bytes(self.slots, self.window, self.max_frames_per_call)

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        _native.correlogram_voice_stream_reset_device(ctx, state_ptr, state_bytes, self.slots, self.window,
                                                      self.max_frames_per_call, stream=stream)

    def _launch(self, ctx, state_ptr, state_bytes, inputs, rows, out_counts, stream):
        x, counts, flags = inputs                           # x is the host path's float32 cast or the pool's dtype
        _native.correlogram_voice_stream_device(
            ctx, state_ptr, state_bytes, self.max_frames_per_call, x.data_ptr(), x.data_ptr() + x.element_size(),
            2 * self.max_frames_per_call, 2, counts.data_ptr(), flags.data_ptr(), rows.data_ptr(), out_counts.data_ptr(),
            self.slots, window=self.window, hop=self.hop, num_lags=self.num_lags, eps=float(self.epsilon),
            float64=x.element_size() == 8, stream=stream)


def cross_correlogram_voice_pool(slots: int, *, sample_rate_hz: int = 44100, max_lag_seconds: float = 0.02,
                                 window_size_seconds: float = 0.02, stride_seconds: float = 0.01, epsilon: float = EPSILON,
                                 max_frames_per_call: int = 4800, dtype='float32') -> CorrelogramVoicePool:
    """A :class:`CorrelogramVoicePool`: ``cross_correlogram`` with these arguments for ``slots`` voices that start, end
    and push blocks on their own, the positions in device memory.  The sizes come from ``correlogram_sizes`` as for the
    one-shot call.  Sizes the device does not cover (:func:`correlogram_covers`), pools above ``MAX_STREAMS_PER_CALL`` and
    a ``dtype`` other than ``'float32'`` / ``'float64'`` raise ``ValueError`` here: there is no NumPy pool.
    ``set_correlogram_device`` is not consulted."""
    window, hop, max_lag = correlogram_sizes(sample_rate_hz, max_lag_seconds, window_size_seconds, stride_seconds)
    return CorrelogramVoicePool(slots, window=window, hop=hop, num_lags=2 * max_lag + 1, epsilon=epsilon,
                                max_frames_per_call=max_frames_per_call, dtype=dtype)


# ----------------------------------------------------------------------------
# The polar moments of a voice pool   (include/vnd_polar_voice_stream.h)
# ----------------------------------------------------------------------------
POLAR_CHUNK_FRAMES = 512              # frames per chunk of the moments reducer (kMomFrames)
POLAR_REDUCE_LANES = 256              # its reduce lanes (kMomThreads)
_TMAX = 4                             # the moment that is a maximum, not a sum


def polar_voice_spans(positions, counts, flags, max_frames_per_call: Optional[int] = None):
    """``(valid, new_positions)`` of one call of a polar-moments voice pool (``include/vnd_polar_voice_stream.h``), per
    slot, from the positions before the call, the frames pushed and the ``VOICE_START`` / ``VOICE_END`` flags alone -
    what the device computes from its own state::

        p = START ? 0 : position      valid = 1, or 0 for n = 0 without a flag      new position = END ? 0 : p + n

    A count below 0 (or above ``max_frames_per_call``, when given), or without START a position outside ``[0, 2^60]``,
    answers -1 and leaves the position as it was."""
    return _valid_voice_spans(positions, counts, flags, max_frames_per_call)


def _polar_fold(acc, more):
    """``acc (+) more`` per moment: a float64 add, ``fmax`` for max |theta|."""
    out = acc + more
    out[..., _TMAX] = np.maximum(acc[..., _TMAX], more[..., _TMAX])
    return out


def _polar_tree(v):
    """The workgroup tree of the moments kernels over ``(..., 256, 8)`` lane values: ``shfl_xor`` 32..1 in each wave of
    64, then the four waves in order."""
    w = v.reshape(v.shape[:-2] + (POLAR_REDUCE_LANES // 64, 64, 8))
    lane = np.arange(64)
    for sh in (32, 16, 8, 4, 2, 1):
        w = _polar_fold(w, w[..., lane ^ sh, :])
    out = w[..., 0, 0, :]
    for k in range(1, POLAR_REDUCE_LANES // 64):
        out = _polar_fold(out, w[..., k, 0, :])
    return out


def _polar_chunk_partials(terms):
    """The partials of the chunks of ``(m, 8)`` per-frame terms that begin on a chunk boundary, ``(ceil(m / 512), 8)``:
    lane t adds frames 512 c + t and 512 c + 256 + t from +0.0 (a frame that does not exist adds nothing; +0.0 is the
    same), then the tree."""
    m = len(terms)
    chunks = -(-m // POLAR_CHUNK_FRAMES)
    a = np.zeros((chunks * POLAR_CHUNK_FRAMES, 8), np.float64)
    a[:m] = terms
    a = a.reshape(chunks, 2, POLAR_REDUCE_LANES, 8)
    return _polar_tree(_polar_fold(_polar_fold(np.zeros_like(a[:, 0]), a[:, 0]), a[:, 1]))


class PolarMomentsState:
    """What the streamed form of :func:`polar_moments_ordered` carries between blocks - the device state of one slot
    (``include/vnd_polar_voice_stream.h``): ``position`` (a Python integer), ``lanes`` float64 ``(256, 8)``, reduce lane
    t's sums over the completed chunks c = t (mod 256), and ``pending`` ``(position % 512, 8)``, the terms of the chunk
    still incomplete."""

    def __init__(self, position: int = 0, lanes=None, pending=None):
        self.position = int(position)
        self.lanes = np.zeros((POLAR_REDUCE_LANES, 8), np.float64) if lanes is None else np.array(lanes, np.float64)
        self.pending = np.zeros((0, 8), np.float64) if pending is None else np.array(pending, np.float64)
        if self.position < 0 or self.lanes.shape != (POLAR_REDUCE_LANES, 8) \
                or self.pending.shape != (self.position % POLAR_CHUNK_FRAMES, 8):
            raise ValueError(f'a state at position {position} holds (256, 8) lane sums and '
                             f'({self.position % POLAR_CHUNK_FRAMES}, 8) pending terms, got {self.lanes.shape} and '
                             f'{self.pending.shape}')

    def push(self, terms) -> None:
        """Append ``(n, 8)`` per-frame terms: chunks that become complete are folded into their lanes in ascending c."""
        terms = np.asarray(terms, np.float64).reshape(-1, 8)
        have = np.concatenate([self.pending, terms]) if len(self.pending) else terms
        c0 = self.position // POLAR_CHUNK_FRAMES
        self.position += len(terms)
        done = self.position // POLAR_CHUNK_FRAMES - c0
        if done:
            partials = _polar_chunk_partials(have[:done * POLAR_CHUNK_FRAMES])
            for first in range(0, done, POLAR_REDUCE_LANES):          # 256 consecutive chunks: 256 different lanes
                part = partials[first:first + POLAR_REDUCE_LANES]
                lanes = (c0 + first + np.arange(len(part))) % POLAR_REDUCE_LANES
                self.lanes[lanes] = _polar_fold(self.lanes[lanes], part)
        self.pending = np.array(have[done * POLAR_CHUNK_FRAMES:])

    def moments(self):
        """The eight moments of everything pushed so far."""
        lanes = self.lanes.copy()
        c0 = self.position // POLAR_CHUNK_FRAMES
        lanes[min(c0, POLAR_REDUCE_LANES):] = 0.0                    # a lane without a completed chunk starts from +0.0
        if len(self.pending) or self.position == 0:                  # (no frame at all: the one chunk of zeros)
            t = c0 % POLAR_REDUCE_LANES
            lanes[t] = _polar_fold(lanes[t], _polar_chunk_partials(self.pending if len(self.pending)
                                                                   else np.zeros((1, 8)))[0])
        return _polar_tree(lanes)


def polar_moments_ordered(terms, state: Optional[PolarMomentsState] = None):
    """The eight polar moments from ``(n, 8)`` float64 per-frame terms ``{r, r t, r t^2, r t^3, |t|, L R, L^2, R^2}`` in
    the summation order of ``vnd_polar_moments_f32_dev`` with one pair (``csrc/vnd_moments.hpp``), restated in NumPy
    float64: chunk c is frames ``[512 c, 512 c + 512)``; lane t of 256 adds frames ``512 c + t`` and ``512 c + 256 + t``;
    a ``shfl_xor`` tree 32..1 per wave; the four waves in order; reduce lane t adds the chunk partials c = t (mod 256) in
    ascending c from +0.0; the same tree; ``max |t|`` takes the same path through ``fmax``.

    Without ``state``: the one-shot form, all frames at once.  With a :class:`PolarMomentsState`: the streamed form - the
    terms are pushed onto the state, which carries the lane sums and the pending chunk as the device does, and the result
    is the moments of everything the state has seen.  The two agree bit for bit for every split into blocks."""
    terms = np.asarray(terms, np.float64).reshape(-1, 8)
    if state is not None:
        state.push(terms)
        return state.moments()
    partials = _polar_chunk_partials(terms) if len(terms) else np.zeros((1, 8), np.float64)
    lanes = np.zeros((POLAR_REDUCE_LANES, 8), np.float64)
    for first in range(0, len(partials), POLAR_REDUCE_LANES):
        part = partials[first:first + POLAR_REDUCE_LANES]
        lanes[:len(part)] = _polar_fold(lanes[:len(part)], part)
    return _polar_tree(lanes)


class PolarVoicePool(_MeterPool):
    """The stereo image of ``slots`` voices, each with a life of its own (:func:`stereo_image_voice_pool`,
    ``vnd_polar_voice_stream_*_dev``): voices start and end on any call and push blocks of any size up to
    ``max_frames_per_call`` or none.  The position lives in the device state, one per slot, so a call is a pure function
    of device memory.  After every call a slot's row holds the eight polar moments
    ``{sum r, sum r t, sum r t^2, sum r t^3, max |t|, sum L R, sum L^2, sum R^2}`` of that voice's whole signal so far -
    what ``symmetry_aware_objective`` is made of (:meth:`scores`).  With ``dtype='float32'`` they equal
    ``vnd_polar_moments_f32_dev`` on the concatenation of the voice's frames bit for bit, whatever the schedule; with
    ``dtype='float64'`` theta, r and the products are float64, as NumPy computes them on float64 arrays, and the moments
    do not depend on the schedule either.

    Two forms; a pool is used through one of them (mixing them raises ``RuntimeError`` until ``reset()``):

    * ``process({slot: block}, start=[slot, ...], end=[slot, ...], discard=False)`` - ``(n, 2)`` NumPy blocks of the
      pool's ``dtype`` in, ``{slot: float64 (8,)}`` out for every slot that got a block, started or ended.  One upload and
      one download (``transfers`` counts those of the last call); every refusal comes before any device call.
    * ``process_dev(y, counts, flags, *, out=None)`` - ``y`` ``(slots, max_frames_per_call, 2)`` of the pool's ``dtype``
      and int32 ``(slots,)`` ``counts`` and ``flags`` on the device; returns ``(moments, valid)``.  It only enqueues on
      the current stream and can be captured with ``torch.cuda.graph`` after a ``reset()``.  To meter a decorrelating
      pool, build the meter with ``max_frames_per_call=pool.row_frames`` (and ``dtype='float64'`` for a Haas or chain
      pool) and hand it that pool's ``y`` and ``out_counts`` and the caller's ``flags``: a -1 of the pool is a bad count
      here and answers -1."""

    _out_dtype = np.float64
    _out_width = 8

    def __init__(self, slots: int, *, max_frames_per_call: int, dtype='float32'):
        _MeterPool.__init__(self, slots, max_frames_per_call, dtype)
        # the fixed grid of the pool (include/vnd_polar_voice_stream.h): one workgroup per chunk of 512 frames a call can
        # touch, one grid dimension per slot; 2^23 workgroups a launch
        if self.chunks_per_call > 65535 or self.slots * self.chunks_per_call > 1 << 23:
            raise ValueError(f'{self.slots} slots of {self.chunks_per_call} chunks per call are more than one launch takes: '
                             f'lower max_frames_per_call or split the pool')
        S = self.slots
        self._inputs = (('y', (S, self.max_frames_per_call, 2), self.dtype.name, None),) + _slot_ints(S, 'counts', 'flags')
        self._outputs = (('moments', (S, 8), 'float64', 'zeros'), ('valid', (S,), 'int32', 'empty'))
        self._mirror()

    @property
    def chunks_per_call(self) -> int:
        """G: the chunks of 512 frames a call can touch per slot, ``ceil(max_frames_per_call / 512) + 1``."""
        return -(-self.max_frames_per_call // POLAR_CHUNK_FRAMES) + 1

    def process(self, blocks=None, *, start=(), end=(), discard: bool = False):
        """One call of the dict form.  ``blocks``: ``{slot: (n, 2) array of the pool's dtype}``,
        ``0 <= n <= max_frames_per_call``; ``start``: the slots whose voice begins with this call; ``end``: the slots whose
        voice ends with it.  Returns ``{slot: float64 (8,)}``, the moments of the voice so far, for every slot that got a
        block, started or ended.  Raises before any device call, as the other voice pools do: ``ValueError`` for a slot
        outside the pool or named twice, a block or an end for a slot that was never started, a start on a live slot
        (``discard=True`` allows it: the voice it held is dropped), a block above ``max_frames_per_call`` or not
        ``(n, 2)``; ``TypeError`` for a block of another dtype than the pool's."""
        return self._process_valid(blocks, start, end, discard, np.array)

    def process_dev(self, y, counts, flags, *, out=None):
        """One call on device tensors, enqueued on the current stream: ``y`` ``(slots, M, 2)`` of the pool's dtype,
        ``counts`` / ``flags`` int32 ``(slots,)``.  Returns ``(moments, valid)``: float64 ``(slots, 8)`` - the row of a
        slot that answered 1 is written, no other - and int32 ``(slots,)``; ``out=(moments, valid)`` takes the caller's.
        No check reads device memory; bad per-slot values answer -1 (``include/vnd_polar_voice_stream.h``)."""
        return self._process_dev((y, counts, flags), out)

    def scores(self, moments, *, angle_limit: float, lambda_mean: float, lambda_skew: float, lambda_correlation: float,
               lambda_penalty: float):
        """``symmetry_aware_objective`` of each voice's output so far, from ``(k, 8)`` rows of moments (or one ``(8,)`` row,
        or a device tensor): ``optimization.scores_from_moments``; lower is better."""
        from . import optimization
        if _native.is_torch(moments):
            moments = moments.cpu().numpy()
        m = np.asarray(moments, np.float64)
        if m.shape[-1:] != (8,) or m.ndim not in (1, 2):
            raise ValueError(f'moments of shape (8,) or (k, 8), got {m.shape}')
        s = optimization.scores_from_moments(m.reshape(-1, 8), angle_limit=angle_limit, lambda_mean=lambda_mean,
                                             lambda_skew=lambda_skew, lambda_correlation=lambda_correlation,
                                             lambda_penalty=lambda_penalty)
        return float(s[0]) if m.ndim == 1 else s

    # ---- the device -------------------------------------------------------------------------
    def _state_bytes(self, ctx) -> int:
        return _native.polar_voice_stream_state_bytes(self.slots, self.max_frames_per_call, self.dtype.itemsize)

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        _native.polar_voice_stream_reset_device(ctx, state_ptr, state_bytes, self.slots, self.max_frames_per_call,
                                                self.dtype.itemsize, stream=stream)

    def _launch(self, ctx, state_ptr, state_bytes, inputs, moments, valid, stream):
        y, counts, flags = inputs
        _native.polar_voice_stream_device(
            ctx, state_ptr, state_bytes, self.max_frames_per_call, y.data_ptr(), y.data_ptr() + y.element_size(),
            2 * self.max_frames_per_call, 2, counts.data_ptr(), flags.data_ptr(), moments.data_ptr(), valid.data_ptr(),
            self.slots, float64=self.dtype == np.float64, stream=stream)


def stereo_image_voice_pool(slots: int, *, max_frames_per_call: int = 4800, dtype='float32') -> PolarVoicePool:
    """A :class:`PolarVoicePool`: the eight polar moments of ``symmetry_aware_objective`` for ``slots`` voices that start,
    end and push blocks on their own, the positions in device memory.  Pools above ``MAX_STREAMS_PER_CALL``, a
    ``max_frames_per_call`` whose grid one launch does not take and a ``dtype`` other than ``'float32'`` / ``'float64'``
    raise ``ValueError`` here: a stream has no host loop to fall back to."""
    return PolarVoicePool(slots, max_frames_per_call=max_frames_per_call, dtype=dtype)


# the vectorscope's data (include/vnd_scope.h): the third way the reference looks at a decorrelated signal
from .vectorscope import (LevelVoicePool, ScopeVoicePool, lissajous_histogram_batched,  # noqa: E402
                          lissajous_histogram_voice_pool, polar_coordinates_batched, polar_histogram_batched,
                          polar_histogram_voice_pool, polar_level_batched, polar_level_voice_pool, scope_covers,
                          scope_voice_spans, scope_voice_window, set_scope_device)

__all__ = ['cross_correlogram_batched', 'cross_correlogram_stream', 'CorrelogramStream', 'correlogram_covers',
           'set_correlogram_device', 'MAX_WINDOW', 'cross_correlogram_voice_pool', 'CorrelogramVoicePool',
           'correlogram_voice_spans', 'stereo_image_voice_pool', 'PolarVoicePool', 'polar_voice_spans',
           'polar_moments_ordered', 'PolarMomentsState', 'polar_coordinates_batched', 'polar_histogram_batched',
           'lissajous_histogram_batched', 'polar_level_batched', 'set_scope_device', 'scope_covers', 'ScopeVoicePool',
           'polar_histogram_voice_pool', 'lissajous_histogram_voice_pool', 'scope_voice_spans', 'scope_voice_window',
           'LevelVoicePool', 'polar_level_voice_pool']
