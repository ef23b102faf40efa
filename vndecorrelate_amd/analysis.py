"""Cross-correlograms on the GPU (``vnd_correlogram_f32_dev``, include/vnd_analysis.h).

The reference measures decorrelation with ``utils/dsp.py:313`` ``cross_correlogram``: per window of W samples,
``np.correlate(x_w, y_w, 'full')`` over ``sqrt(x_w.x_w * y_w.y_w) + eps`` - W^2 multiply-adds a window.  Here:

* ``utils.dsp.cross_correlogram`` - the reference's signature; on the device where covered, NumPy otherwise;
* :func:`cross_correlogram_batched` - ``(B, n)`` pairs, or channel 0 against channel 1 of a ``(B, n, 2)`` signal in
  place; NumPy in, NumPy out (pinned); a float32 torch tensor on the device in, a device tensor out;
* :func:`set_correlogram_device` and the pure routing rule :func:`correlogram_covers`.

Numerics: each correlation output is one float64 FMA chain over exact products, rounded once; the
energies are float64 sums rounded once; the normaliser is NumPy 2's float32 arithmetic.  The result is within one
float32 ulp of the same formula with exact sums and within ``(2W + 4) 2^-24`` of the reference's float32 result.
Without a device every call is the NumPy code.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from .utils.dsp import EPSILON, correlogram_sizes, to_float32

MAX_WINDOW = _native.CORRELOGRAM_MAX_WINDOW
_INT32_MAX = 2 ** 31 - 1

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
    try:
        _native.default_context()
        return True
    except RuntimeError:                                  # no built extension, no device, not a gfx950
        return False


def use_device(n_frames: int, window: int, hop: int, num_lags: int, epsilon) -> bool:
    """The routing decision of one call: :func:`correlogram_covers` and :func:`set_correlogram_device`."""
    if _correlogram_device is False or not correlogram_covers(n_frames, window, hop, num_lags, epsilon):
        return False
    if _correlogram_device is True:
        if not _gpu_present():
            raise RuntimeError('set_correlogram_device(True): no gfx950 device (or no built extension) to run on')
        return True
    return _gpu_present()


def _windows(n_frames: int, window: int, hop: int) -> int:
    return (n_frames - window) // hop + 1 if n_frames >= window else 0


def _torch():
    from .resident import _torch as get
    return get()


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
    is_tensor = type(x).__module__.startswith('torch')
    if is_tensor:
        torch = _torch()
        _check_batch(x, y)
        if y is not None and (not type(y).__module__.startswith('torch') or y.device != x.device):
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


__all__ = ['cross_correlogram_batched', 'correlogram_covers', 'set_correlogram_device', 'MAX_WINDOW']
