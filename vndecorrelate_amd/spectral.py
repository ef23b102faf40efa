"""Short-time spectra of a pool on the GPU (include/vnd_spectrum.h): what ``utils/plot.py`` ``plot_spectrogram`` draws from,
and the frequency-domain measures a decorrelator is judged by.

The reference's own test feeds ``plot_spectrogram`` ``scipy.signal.spectrogram(sweep, fs=fs)[-1]``, and L-R coherence per
frequency is how velvet noise is compared with white noise.  Here both are computed for a whole pool that lives in device
memory, by a batched real-input FFT in LDS, with SciPy's defaults and meanings:

* :func:`spectrogram_batched` - ``scipy.signal.spectrogram`` (mode ``'psd'``, one-sided) of every signal and channel;
* :func:`welch_batched`, :func:`csd_batched`, :func:`coherence_batched` - ``scipy.signal.welch``, ``csd`` and ``coherence``
  with ``average='mean'``; the sums over segments are float64, in ascending segment order, on every route of the device;
* :func:`set_spectrum_device` and the pure routing rule :func:`spectrum_covers`;
* :func:`spectrum_voice_pool` - the same columns and means for a pool of voices that start, end and push blocks of their own
  sizes (``include/vnd_spectrum_voice_stream.h``): a :class:`SpectrumVoicePool`, which meters the coherence of a
  ``decorrelate_voice_pool`` on the device; :func:`spectrum_voice_spans` is the device's mirror.

A column of a spectrogram is a function of its own segment of its own channel only: channels and segments are never
packed into one transform, so a quiet side channel keeps its own rounding floor.  Without a device, or for
a call the device does not cover, every function is a loop of the SciPy calls, one signal at a time.  Drawing and the
display scalings (``10 * log10(S + 1e-10)``) are not here.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from .streaming import _INT32_MAX, _MeterPool, _slot_ints, _SlotPool, _voice_head

MIN_NFFT = _native.SPECTRUM_MIN_NFFT
MAX_NFFT = _native.SPECTRUM_MAX_NFFT
RUN = _native.SPECTRUM_RUN                              # the most consecutive segments a workgroup owns
_MAX_BATCH = 65535                                      # VND_MAX_STREAMS
_MAX_GROUPS = 2 ** 23
_MAX_ELEMENTS = 2 ** 59
_torch = _native.torch_module

_spectrum_device: Optional[bool] = None
_table_cache: dict = {}


def set_spectrum_device(enabled: Optional[bool]) -> None:
    """Where the functions of this module run.

    ``None`` (default): on the GPU when a gfx950 device is present and the call is covered (:func:`spectrum_covers`),
    otherwise the SciPy loop.  ``True``: the device for every covered call; such a call raises ``RuntimeError`` when
    there is no device.  ``False``: always SciPy."""
    global _spectrum_device
    if enabled is not None and not isinstance(enabled, (bool, np.bool_)):
        raise TypeError(f'set_spectrum_device takes True, False or None, not {enabled!r}')
    _spectrum_device = None if enabled is None else bool(enabled)


def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _window_values(window, nperseg: int) -> np.ndarray:
    """The float64 window of ``nperseg`` values: ``scipy.signal.get_window`` of a name or tuple, or the array itself."""
    if isinstance(window, (str, tuple)):
        from scipy.signal import get_window
        return np.asarray(get_window(window, nperseg), np.float64)
    win = np.asarray(window)
    if win.ndim != 1:
        raise ValueError('window must be 1-D')
    if win.shape[0] != nperseg:
        raise ValueError('value specified for nperseg is different from length of window')
    return win.astype(np.float64)


def _segment_size(window, nperseg) -> int:
    if nperseg is None:
        return 256 if isinstance(window, (str, tuple)) else int(np.asarray(window).shape[0])
    return int(nperseg)


def spectrum_covers(dtype, batch: int, n_frames: int, channels: int = 1, nperseg: int = 256, noverlap: Optional[int] = None,
                    nfft: Optional[int] = None, detrend='constant', scaling: str = 'density', window='hann') -> bool:
    """Whether a call of this shape has a device form: float32 or float64 frames, 1 <= batch <= 65535, 1 or 2 channels,
    ``nfft`` (default ``nperseg``) a power of two in [64, 4096], 2 <= nperseg <= nfft, 0 <= noverlap < nperseg (default
    ``nperseg // 2``), ``detrend`` ``'constant'`` or ``False``, ``scaling`` ``'density'`` or ``'spectrum'``, a window
    ``scipy.signal.get_window`` accepts or an array of ``nperseg`` real values, nperseg <= n_frames < 2^31, and at most
    2^23 workgroups in a launch.  Everything else - ``'linear'`` detrend, another ``nfft``, complex frames, more channels, a
    signal shorter than a segment - keeps the SciPy loop."""
    try:
        if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
            return False
    except TypeError:
        return False
    if nfft is None:
        nfft = nperseg
    if noverlap is None:
        noverlap = nperseg // 2 if _is_int(nperseg) else None
    for v in (batch, n_frames, channels, nperseg, noverlap, nfft):
        if not _is_int(v):
            return False
    if not 1 <= batch <= _MAX_BATCH or channels not in (1, 2):
        return False
    if not MIN_NFFT <= nfft <= MAX_NFFT or nfft & (nfft - 1):
        return False
    if not 2 <= nperseg <= nfft or not 0 <= noverlap < nperseg or not nperseg <= n_frames <= _INT32_MAX:
        return False
    if not (detrend is False or (isinstance(detrend, str) and detrend == 'constant')):
        return False
    if not (isinstance(scaling, str) and scaling in ('density', 'spectrum')):
        return False
    if not isinstance(window, (str, tuple)):
        win = np.asarray(window)
        if win.ndim != 1 or win.shape[0] != nperseg or win.dtype.kind not in 'fiu':
            return False
    segments = (n_frames - nperseg) // (nperseg - noverlap) + 1
    if batch * channels * segments > _MAX_GROUPS:                  # (a run is at least one segment)
        return False
    return batch * channels * (nfft // 2 + 1) * segments <= _MAX_ELEMENTS


def twiddle_table(nfft: int, dtype) -> np.ndarray:
    """The device's twiddles: ``(nfft, 2)`` of ``dtype``, row i ``(cos, -sin)`` of ``2 pi i / nfft``, formed in float64 and
    rounded once; the values that are exactly 0 are 0."""
    ang = 2.0 * np.pi * np.arange(nfft, dtype=np.float64) / float(nfft)
    table = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    table[np.abs(table) < 1e-15] = 0.0
    return np.ascontiguousarray(table.astype(dtype))


def spectrum_scale(win: np.ndarray, fs: float, scaling: str) -> float:
    """SciPy's scale in float64, from the float64 window: ``1 / (fs * sum(w^2))`` for ``'density'``, ``1 / sum(w)^2`` for
    ``'spectrum'``.  The device rounds it to the sample type once."""
    with np.errstate(divide='ignore', invalid='ignore'):
        if scaling == 'density':
            return float(1.0 / (float(fs) * np.sum(win * win)))
        if scaling == 'spectrum':
            return float(1.0 / np.sum(win) ** 2)
    raise ValueError(f'Unknown scaling: {scaling!r}')


def segment_times(n_frames: int, nperseg: int, noverlap: int, fs: float) -> np.ndarray:
    """SciPy's segment times, its expression."""
    return np.arange(nperseg / 2, n_frames - nperseg / 2 + 1, nperseg - noverlap) / float(fs)


def bin_frequencies(nfft: int, fs: float) -> np.ndarray:
    """SciPy's one-sided bin frequencies, its call."""
    from scipy import fft as sp_fft
    return sp_fft.rfftfreq(nfft, 1 / fs)


def run_length(nfft: int, nperseg: int, hop: int, dtype=np.float32, cross_channels: int = 0) -> int:
    """The consecutive segments of one signal a workgroup owns (``vnd_spectrum_run_length``): ``cross_channels`` 0 for
    :func:`spectrogram_batched`, the pool's channels for the Welch functions."""
    return _native.spectrum_run_length(nfft, nperseg, hop, np.dtype(dtype) == np.float64, cross_channels)


# ---- shapes and routes ---------------------------------------------------------------------------------------------------
def _pool_shape(pool, stereo_only: bool):
    shape = tuple(pool.shape)
    if stereo_only:
        if len(shape) != 3 or shape[2] != 2:
            raise ValueError(f'pool must be (batch, n, 2): got shape {shape}')
        return False, shape
    if len(shape) == 2:
        return True, shape + (1,)
    if len(shape) == 3 and shape[2] >= 1:
        return False, shape
    raise ValueError(f'pool must be (batch, n) or (batch, n, channels): got shape {shape}')


def _dtype_of(pool) -> np.dtype:
    if not _native.is_torch(pool):
        return np.asarray(pool).dtype
    try:
        return np.dtype(str(pool.dtype).replace('torch.', ''))
    except TypeError:
        return np.dtype(object)


def _to_host(pool) -> np.ndarray:
    return pool.detach().cpu().numpy() if _native.is_torch(pool) else np.asarray(pool)


def _device_of(pool):
    try:
        torch = _torch()
        device = torch.device('cuda', _native.default_context().device)
    except RuntimeError:
        return None
    return device if pool.device == device else None


def _host_counts(counts, batch: int, n: int):
    if counts is None:
        return [n] * batch
    if _native.is_torch(counts):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts).astype(np.int64).reshape(-1)
    if len(c) != batch:
        raise ValueError(f'counts must have one entry per signal: got {len(c)} for {batch}')
    return [int(v) if 0 <= v <= n else 0 for v in c]


def _device_counts(torch, counts, batch: int, device):
    if counts is None:
        return None
    if not _native.is_torch(counts):
        counts = torch.from_numpy(np.ascontiguousarray(counts, np.int32))
    if counts.dtype != torch.int32 or tuple(counts.shape) != (batch,):
        raise ValueError(f'counts must be int32 of shape ({batch},): got {counts.dtype} {tuple(counts.shape)}')
    return counts.to(device).contiguous()


def _device_tables(torch, device, win64: np.ndarray, nfft: int, dtype: np.dtype):
    """The window and the twiddles of the sample type on the device, uploaded once per distinct pair: a later call - or a
    graph capture - copies nothing from the host."""
    win = np.ascontiguousarray(win64.astype(dtype))                # as SciPy casts it: win.astype(outdtype)
    key = (str(device), dtype.str, nfft, win.tobytes())
    got = _table_cache.get(key)
    if got is None:
        if len(_table_cache) >= 64:
            _table_cache.clear()
        got = (torch.from_numpy(win).to(device), torch.from_numpy(twiddle_table(nfft, dtype)).to(device))
        _table_cache[key] = got
    return got


def _device_pool(torch, pool, is_tensor: bool, device, shape):
    """``(tensor, stream_stride, frame_stride)`` of a (B, n, C) pool on the device, its strides taken as they are when the
    channels of a frame are adjacent."""
    pd = pool if is_tensor else torch.from_numpy(np.ascontiguousarray(pool)).to(device)
    pd = pd.reshape(shape) if pd.dim() == 3 else pd.unsqueeze(2)
    batch, n, channels = shape
    ok = (channels == 1 or pd.stride(2) == 1) and (n == 1 or channels <= pd.stride(1) < 2 ** 31) \
        and (batch == 1 or pd.stride(0) >= 1)
    if not ok:
        pd = pd.contiguous()
    return pd, max(1, pd.stride(0)), max(channels, pd.stride(1)) if n > 1 else channels


class _Plan:
    """The parameters of one call, SciPy's defaults and errors applied."""

    def __init__(self, pool, fs, window, nperseg, noverlap, nfft, detrend, scaling, default_overlap, stereo_only):
        self.single, (self.batch, self.n, self.channels) = _pool_shape(pool, stereo_only)
        self.fs, self.window, self.detrend, self.scaling = fs, window, detrend, scaling
        self.nperseg = _segment_size(window, nperseg)
        if self.nperseg < 1:
            raise ValueError('nperseg must be a positive integer')
        self.nfft = self.nperseg if nfft is None else int(nfft)
        if self.nfft < self.nperseg:
            raise ValueError('nfft must be greater than or equal to nperseg.')
        self.noverlap = default_overlap(self.nperseg) if noverlap is None else int(noverlap)
        if self.noverlap >= self.nperseg:
            raise ValueError('noverlap must be less than nperseg.')
        if scaling not in ('density', 'spectrum'):
            raise ValueError(f'Unknown scaling: {scaling!r}')
        self.hop = self.nperseg - self.noverlap
        self.is_tensor = _native.is_torch(pool)
        self.dtype = _dtype_of(pool)
        self.kwargs = dict(fs=fs, window=window, nperseg=nperseg if nperseg is None else self.nperseg, noverlap=self.noverlap,
                           nfft=nfft, detrend=detrend, scaling=scaling)

    def on_device(self, pool) -> bool:
        from .analysis import device_route
        covered = spectrum_covers(self.dtype, self.batch, self.n, self.channels, self.nperseg, self.noverlap, self.nfft,
                                  self.detrend, self.scaling, self.window)
        scale = None
        if covered:
            self.win = _window_values(self.window, self.nperseg)
            scale = spectrum_scale(self.win, self.fs, self.scaling)
            covered = bool(np.isfinite(scale) and scale > 0 and np.isfinite(self.dtype.type(scale)) and self.dtype.type(scale) > 0)
        self.scale = scale
        on = device_route(_spectrum_device, covered,
                          'set_spectrum_device(True): no gfx950 device (or no built extension) to run on')
        return on and (not self.is_tensor or _device_of(pool) is not None)

    @property
    def bins(self) -> int:
        return self.nfft // 2 + 1

    @property
    def segments(self) -> int:
        return (self.n - self.nperseg) // self.hop + 1

    def launch(self, pool):
        """What every device call shares: ``(torch, ctx, device, pool tensor, leading arguments, keywords)``; the caller
        keeps the pool tensor until its call is enqueued."""
        torch = _torch()
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        pd, ss, fst = _device_pool(torch, pool, self.is_tensor, device, (self.batch, self.n, self.channels))
        win, tw = _device_tables(torch, device, self.win, self.nfft, self.dtype)
        args = (ctx, pd.data_ptr(), self.batch, self.n, ss, fst, self.channels, win.data_ptr(), tw.data_ptr(), self.nperseg,
                self.hop, self.nfft)
        kw = dict(detrend=self.detrend is not False, scale=self.scale, float64=self.dtype == np.float64,
                  stream=torch.cuda.current_stream(device).cuda_stream)
        return torch, ctx, device, pd, args, kw


def _device_axis(torch, device, axis: np.ndarray):
    """An axis on the device, uploaded once per distinct axis and handed out as a copy made on the device: a later call - or
    a graph capture - copies nothing from the host."""
    key = (str(device), 'axis', axis.tobytes())
    got = _table_cache.get(key)
    if got is None:
        if len(_table_cache) >= 64:
            _table_cache.clear()
        got = torch.from_numpy(axis.copy()).to(device)
        _table_cache[key] = got
    return got.clone()


def _return_axes(plan: _Plan, pool, f: np.ndarray, t: Optional[np.ndarray], on_tensor_device):
    if not plan.is_tensor:
        return (f, t)
    torch = _torch()
    if on_tensor_device is None:
        return (torch.from_numpy(f.copy()).to(pool.device), None if t is None else torch.from_numpy(t.copy()).to(pool.device))
    return (_device_axis(torch, on_tensor_device, f), None if t is None else _device_axis(torch, on_tensor_device, t))


# ---- the spectrogram -----------------------------------------------------------------------------------------------------
def spectrogram_batched(pool, fs=1.0, window=('tukey', 0.25), nperseg=256, noverlap=None, nfft=None, detrend='constant',
                        scaling='density', *, counts=None, out=None):
    """``scipy.signal.spectrogram(pool[b, :, c], fs, window, nperseg, noverlap, nfft, detrend, scaling=scaling)`` for every
    signal and channel of a ``(B, n, C)`` pool, C 1 or 2 on the device (``(B, n)``: one channel): ``(f, t, Sxx)`` with ``Sxx``
    ``(B, C, F, T)`` (``(B, F, T)`` for a 2-D pool) of the pool's dtype, mode ``'psd'``, one-sided, ``F = nfft // 2 + 1``,
    ``T = (n - nperseg) // hop + 1``, ``noverlap`` defaulting to ``nperseg // 8``.  ``f`` and ``t`` are SciPy's, bit for bit.

    ``counts``: optional int32 ``(B,)``, signal b is its first ``counts[b]`` frames (a value outside ``[0, n]``: none) - the
    ``out_counts`` of a voice pool, read on the device.  The columns at or past a signal's own segment count are zero, and a
    signal with no whole segment is all zero: unlike SciPy, ``nperseg`` is never shortened for a short signal under
    ``counts``.

    A float32 or float64 tensor on the device in gives tensors out on the current stream with nothing synchronised (``out``,
    when given, is the contiguous ``Sxx`` tensor to fill); the window and twiddle tables and the axes are uploaded on the
    first call with their parameters, so warm a call up before capturing one in a graph.  NumPy in gives NumPy out.  On the device a column is a
    function of its own segment of its own channel alone, whatever else the pool holds; what the device
    does not cover (:func:`spectrum_covers`) is the SciPy loop."""
    plan = _Plan(pool, fs, window, nperseg, noverlap, nfft, detrend, scaling, lambda m: m // 8, False)
    batch, n, channels = plan.batch, plan.n, plan.channels
    if plan.on_device(pool):
        torch, ctx, device, pd, args, kw = plan.launch(pool)
        shape = (batch, channels, plan.bins, plan.segments)
        each = _device_counts(torch, counts, batch, device)
        if plan.is_tensor and out is not None:
            want = shape if not plan.single else (batch, plan.bins, plan.segments)
            if not _native.is_torch(out) or out.dtype != pd.dtype or tuple(out.shape) != want or out.device != device \
                    or not out.is_contiguous():
                raise ValueError(f'out must be a contiguous {pd.dtype} tensor of shape {want} on {device}')
            sxx = out.reshape(shape)
        else:
            sxx = torch.empty(shape, dtype=pd.dtype, device=device)
        _native.spectrogram_device(*args, sxx.data_ptr(), n_each_ptr=each.data_ptr() if each is not None else 0, **kw)
        del pd
        if plan.single:
            sxx = sxx[:, 0]
        f, t = bin_frequencies(plan.nfft, fs), segment_times(n, plan.nperseg, plan.noverlap, fs)
        if plan.is_tensor:
            return _return_axes(plan, pool, f, t, device) + (out if out is not None else sxx,)
        got = sxx.cpu().numpy()
        if out is not None:
            out[...] = got
            got = out
        return f, t, got

    from scipy.signal import spectrogram
    host = _to_host(pool).reshape(batch, n, channels)
    each_host = _host_counts(counts, batch, n)
    kwargs = dict(plan.kwargs, mode='psd')
    f, t, first = spectrogram(host[0, :, 0], **kwargs)
    if counts is not None and n < plan.nperseg:
        raise ValueError(f'counts need whole segments: the pool has {n} frames, nperseg is {plan.nperseg}')
    sxx = np.zeros((batch, channels) + first.shape, first.dtype)
    for b, m in enumerate(each_host):
        for c in range(channels):
            if counts is None:
                sxx[b, c] = first if (b, c) == (0, 0) else spectrogram(host[b, :, c], **kwargs)[2]
            elif m >= plan.nperseg:
                part = spectrogram(host[b, :m, c], **kwargs)[2]
                sxx[b, c, :, :part.shape[1]] = part
    if plan.single:
        sxx = sxx[:, 0]
    if out is not None and not plan.is_tensor:
        out[...] = sxx
        sxx = out
    if plan.is_tensor:
        torch = _torch()
        as_tensor = torch.from_numpy(sxx).to(pool.device)
        if out is not None:
            out.copy_(as_tensor)
            as_tensor = out
        return _return_axes(plan, pool, f, t, None) + (as_tensor,)
    return f, t, sxx


# ---- Welch, CSD, coherence -----------------------------------------------------------------------------------------------
def _cross_device(plan: _Plan, pool, counts):
    """``(torch, device, pxx, pyy, pxy)``: the three Welch means on the device; ``pyy`` and ``pxy`` None for one channel."""
    torch, ctx, device, pd, args, kw = plan.launch(pool)
    batch, bins, stereo = plan.batch, plan.bins, plan.channels == 2
    each = _device_counts(torch, counts, batch, device)
    pxx = torch.empty((batch, bins), dtype=pd.dtype, device=device)
    pyy = torch.empty((batch, bins), dtype=pd.dtype, device=device) if stereo else None
    pxy = torch.empty((batch, bins, 2), dtype=pd.dtype, device=device) if stereo else None
    work_bytes = _native.cross_spectra_work_bytes(batch, plan.n, plan.channels, plan.nperseg, plan.hop, plan.nfft,
                                                  plan.dtype == np.float64)
    work = torch.empty((max(1, work_bytes // 8),), dtype=torch.int64, device=device)
    _native.cross_spectra_device(*args, pxx.data_ptr(), pyy.data_ptr() if stereo else 0, pxy.data_ptr() if stereo else 0,
                                 work_ptr=work.data_ptr(), work_bytes=work_bytes,
                                 n_each_ptr=each.data_ptr() if each is not None else 0, **kw)
    del pd
    return torch, device, pxx, pyy, pxy


def _host_average(fn, plan: _Plan, host, each_host, counts, pairs: bool):
    """The SciPy loop of ``welch`` (per channel) or ``csd`` (L against R), zero for a signal with no whole segment."""
    if counts is not None and plan.n < plan.nperseg:
        raise ValueError(f'counts need whole segments: the pool has {plan.n} frames, nperseg is {plan.nperseg}')
    rows, f = [], None
    for b, m in enumerate(each_host):
        row = []
        for c in ([0] if pairs else range(plan.channels)):
            short = counts is not None and m < plan.nperseg
            x = host[b, :plan.n if short else m, c]
            f, p = fn(x, host[b, :len(x), 1], **plan.kwargs) if pairs else fn(x, **plan.kwargs)
            row.append(np.zeros_like(p) if short else p)
        rows.append(row[0] if pairs else np.stack(row))
    return f, np.stack(rows)


def welch_batched(pool, fs=1.0, window='hann', nperseg=256, noverlap=None, nfft=None, detrend='constant',
                  scaling='density', *, counts=None):
    """``scipy.signal.welch(pool[b, :, c], fs, window, nperseg, noverlap, nfft, detrend, scaling=scaling)`` for every signal
    and channel of a ``(B, n, C)`` pool (``(B, n)``: one channel): ``(f, Pxx)`` with ``Pxx`` ``(B, C, F)`` (``(B, F)``) of the
    pool's dtype - the mean over the segments (``average='mean'`` only), ``noverlap`` defaulting to ``nperseg // 2``.  On the
    device the per-segment powers are sample-type values, as SciPy's, and their sum is float64 in ascending segment order,
    rounded once: a signal's result does not depend on the pool around it or on the run.  ``counts`` and the tensor / NumPy
    forms as in :func:`spectrogram_batched`; a signal with no whole segment gives zeros where SciPy would shorten
    ``nperseg``."""
    plan = _Plan(pool, fs, window, nperseg, noverlap, nfft, detrend, scaling, lambda m: m // 2, False)
    batch, n, channels = plan.batch, plan.n, plan.channels
    if plan.on_device(pool):
        if channels == 1:
            torch, device, pxx, _, _ = _cross_device(plan, pool, counts)
            pxx = pxx if plan.single else pxx[:, None]
        else:
            torch, device, pxx, pyy, _ = _cross_device(plan, pool, counts)
            pxx = torch.stack([pxx, pyy], dim=1)
        f = bin_frequencies(plan.nfft, fs)
        if plan.is_tensor:
            return _return_axes(plan, pool, f, None, device)[0], pxx
        return f, pxx.cpu().numpy()
    from scipy.signal import welch
    host = _to_host(pool).reshape(batch, n, channels)
    f, pxx = _host_average(welch, plan, host, _host_counts(counts, batch, n), counts, False)
    if plan.single:
        pxx = pxx[:, 0]
    if plan.is_tensor:
        return _return_axes(plan, pool, f, None, None)[0], _torch().from_numpy(pxx).to(pool.device)
    return f, pxx


def _cross_host(plan: _Plan, pool, counts):
    from scipy.signal import csd, welch
    host = _to_host(pool).reshape(plan.batch, plan.n, 2)
    each_host = _host_counts(counts, plan.batch, plan.n)
    f, pxx = _host_average(welch, plan, host, each_host, counts, False)
    _, pxy = _host_average(csd, plan, host, each_host, counts, True)
    return f, pxx[:, 0], pxx[:, 1], pxy


def csd_batched(pool, fs=1.0, window='hann', nperseg=256, noverlap=None, nfft=None, detrend='constant',
                scaling='density', *, counts=None):
    """``scipy.signal.csd(pool[b, :, 0], pool[b, :, 1], fs, window, nperseg, noverlap, nfft, detrend, scaling=scaling)`` for
    every signal of a ``(B, n, 2)`` pool: ``(f, Pxy)`` with ``Pxy`` complex ``(B, F)``, SciPy's convention ``conj(X_L) *
    X_R``, ``average='mean'``.  Sums, ``counts`` and the tensor / NumPy forms as in :func:`welch_batched`."""
    plan = _Plan(pool, fs, window, nperseg, noverlap, nfft, detrend, scaling, lambda m: m // 2, True)
    if plan.on_device(pool):
        torch, device, _, _, pxy = _cross_device(plan, pool, counts)
        pxy = torch.view_as_complex(pxy)
        f = bin_frequencies(plan.nfft, fs)
        if plan.is_tensor:
            return _return_axes(plan, pool, f, None, device)[0], pxy
        return f, pxy.cpu().numpy()
    f, _, _, pxy = _cross_host(plan, pool, counts)
    if plan.is_tensor:
        return _return_axes(plan, pool, f, None, None)[0], _torch().from_numpy(pxy).to(pool.device)
    return f, pxy


def coherence_batched(pool, fs=1.0, window='hann', nperseg=256, noverlap=None, nfft=None, detrend='constant', *,
                      counts=None):
    """``scipy.signal.coherence(pool[b, :, 0], pool[b, :, 1], fs, window, nperseg, noverlap, nfft, detrend)`` for every signal
    of a ``(B, n, 2)`` pool: ``(f, Cxy)`` with ``Cxy = |Pxy|^2 / Pxx / Pyy``, ``(B, F)`` of the pool's dtype.  The three means
    come from one device call; the ratio is SciPy's expression on them - NumPy for arrays, the same torch operations for
    tensors, with nothing synchronised.  A signal with no whole segment under ``counts`` is 0 / 0: NaN.  ``counts`` and the
    tensor / NumPy forms as in :func:`welch_batched`."""
    plan = _Plan(pool, fs, window, nperseg, noverlap, nfft, detrend, 'density', lambda m: m // 2, True)
    if plan.on_device(pool):
        torch, device, pxx, pyy, pxy = _cross_device(plan, pool, counts)
        f = bin_frequencies(plan.nfft, fs)
        if plan.is_tensor:
            cxy = torch.abs(torch.view_as_complex(pxy)) ** 2 / pxx / pyy
            return _return_axes(plan, pool, f, None, device)[0], cxy
        pxx, pyy, pxy = pxx.cpu().numpy(), pyy.cpu().numpy(), torch.view_as_complex(pxy).cpu().numpy()
    else:
        f, pxx, pyy, pxy = _cross_host(plan, pool, counts)
    with np.errstate(divide='ignore', invalid='ignore'):
        cxy = np.abs(pxy) ** 2 / pxx / pyy
    if plan.is_tensor:
        return _return_axes(plan, pool, f, None, None)[0], _torch().from_numpy(cxy).to(pool.device)
    return f, cxy


# ----------------------------------------------------------------------------
# The spectra of a voice pool   (include/vnd_spectrum_voice_stream.h)
# ----------------------------------------------------------------------------
def spectrum_voice_spans(positions, counts, flags, nperseg: int, hop: int, max_frames_per_call: Optional[int] = None):
    """``(out_counts, segments, new_positions)`` of one call of a spectrum voice pool
    (``include/vnd_spectrum_voice_stream.h``), per slot, from the positions before the call, the frames pushed and the
    ``VOICE_START`` / ``VOICE_END`` flags alone - what the device computes from its own state::

        p = START ? 0 : position        sc(q) = (q - W) // H + 1 if q >= W else 0
        out_count = sc(p + n) - sc(p)   segments = sc(p + n)        new position = END ? 0 : p + n

    ``segments`` is what the call leaves in ``segments[b]``, the count the means are taken over; it is -1 where the call
    leaves the slot's means alone: a bad slot, and an idle one (no frame and no flag).  A count below 0 (or above
    ``max_frames_per_call``, when given), or without START a position outside ``[0, 2^60]``, answers -1 and leaves the
    position as it was."""
    pos, n, start, end, p, bad = _voice_head(positions, counts, flags, max_frames_per_call)
    W, H = int(nperseg), int(hop)
    if W < 1 or H < 1:
        raise ValueError(f'nperseg and hop must be >= 1, got {nperseg} and {hop}')
    p, n = np.where(bad, 0, p), np.where(bad, 0, n)          # (no arithmetic on a bad value)

    def complete(q):
        return np.where(q >= W, (q - W) // H + 1, 0)
    idle = ~bad & (n == 0) & ~start & ~end
    out = np.where(bad, -1, complete(p + n) - complete(p)).astype(np.int64)
    segments = np.where(bad | idle, -1, complete(p + n)).astype(np.int64)
    new = np.where(bad, pos, np.where(end, 0, p + n)).astype(np.int64)
    return out, segments, new


class SpectrumVoicePool(_MeterPool):
    """``scipy.signal.spectrogram`` columns and the Welch means ``Pxx``, ``Pyy``, ``Pxy`` of ``slots`` voices, each with a
    life of its own (:func:`spectrum_voice_pool`, ``vnd_spectrum_voice_stream_*_dev``): voices start and end on any call and
    push blocks of any size up to ``max_frames_per_call`` or none.  The position lives in the device state, one per slot,
    so a call is a pure function of device memory.  A call returns, per slot, the ``'psd'`` columns of the segments that
    became complete - at most ``rows_per_call``, time-major ``(rows, channels, F)`` - and leaves in ``pxx``, ``pyy``, ``pxy``
    and ``segments``, tensors the pool owns at fixed addresses, the Welch means over every segment of the voice so far.
    For every voice the concatenation of its columns equals :func:`spectrogram_batched` of its whole signal and the means
    equal :func:`welch_batched` / :func:`csd_batched` of the frames pushed so far, bit for bit.  Segments that never
    complete are dropped: an end has no tail.

    Two forms; a pool is used through one of them (mixing them raises ``RuntimeError`` until ``reset()``):

    * ``process({slot: block}, start=[slot, ...], end=[slot, ...], discard=False)`` - NumPy blocks ``(n, channels)`` of
      the pool's dtype in, ``{slot: (T_new, channels, F)}`` out for every slot that got a block or ended; :meth:`welch`
      reads a slot's means.  One upload and one download (``transfers`` counts those of the last call); every refusal
      comes before any device call.
    * ``process_dev(y, counts, flags, *, out=None)`` - ``y`` ``(slots, max_frames_per_call, channels)`` of the pool's
      dtype and int32 ``(slots,)`` ``counts`` and ``flags`` on the device; returns ``(columns, out_counts)``.  It only
      enqueues on the current stream and can be captured with ``torch.cuda.graph`` after a ``reset()``.  To meter a
      decorrelating pool, build the meter with ``max_frames_per_call=pool.row_frames`` and the pool's dtype and hand it
      that pool's ``y`` and ``out_counts`` and the caller's ``flags``: a -1 of the pool is a bad count here and answers -1.
    """

    def __init__(self, slots: int, max_frames_per_call: int, *, fs=1.0, window='hann', nperseg=256, noverlap=None, nfft=None,
                 detrend='constant', scaling='density', channels: int = 2, dtype='float32', columns: bool = True):
        _MeterPool.__init__(self, slots, max_frames_per_call, dtype)
        parsed = self.dtype
        if isinstance(channels, (bool, np.bool_)) or channels not in (1, 2):
            raise ValueError(f'channels must be 1 or 2, got {channels!r}')
        if not isinstance(columns, (bool, np.bool_)):
            raise ValueError(f'columns must be True or False, got {columns!r}')
        nperseg = _segment_size(window, nperseg) if nperseg is None or _is_int(nperseg) else nperseg
        if nfft is None:
            nfft = nperseg
        if noverlap is None and _is_int(nperseg):
            noverlap = nperseg // 2
        if not spectrum_covers(parsed, int(slots), nperseg, int(channels), nperseg, noverlap, nfft, detrend, scaling, window):
            raise ValueError(f'nperseg {nperseg!r}, noverlap {noverlap!r}, nfft {nfft!r}, detrend {detrend!r}, scaling '
                             f'{scaling!r} and this window have no device form (spectrum_covers is False) and the pool has '
                             f'no SciPy one: use spectrogram_batched / coherence_batched')
        self.in_channels = int(channels)
        self.fs, self.window, self.detrend, self.scaling = fs, window, detrend, scaling
        self.nperseg, self.noverlap, self.nfft = int(nperseg), int(noverlap), int(nfft)
        self.hop = self.nperseg - self.noverlap
        self.columns = bool(columns)
        self._win64 = _window_values(window, self.nperseg)
        self.scale = spectrum_scale(self._win64, fs, scaling)
        if not (np.isfinite(self.scale) and self.scale > 0 and np.isfinite(parsed.type(self.scale)) and parsed.type(self.scale) > 0):
            raise ValueError(f'the scale {self.scale!r} of this window, fs and scaling is not positive and finite in {parsed.name}')
        # the fixed grid of the pool (include/vnd_spectrum_voice_stream.h): G = ceil(RC / R) + 1 run workgroups per slot, one
        # grid dimension; 2^23 workgroups a launch; cols of at most 2^40 values
        self.run = run_length(self.nfft, self.nperseg, self.hop, parsed, self.in_channels)
        groups = -(-self.rows_per_call // self.run) + 1
        if groups > 65535 or self.slots * groups > _MAX_GROUPS \
                or self.slots * self.rows_per_call * self.in_channels * self.bins > 1 << 40:
            raise ValueError(f'{self.slots} slots of {self.rows_per_call} segments of {self.bins} bins per call are more than '
                             f'one launch takes: raise the hop or lower max_frames_per_call')
        self.pxx = self.pyy = self.pxy = self.segments = None
        S, C = self.slots, self.in_channels
        self._out_dtype = parsed.type
        self._inputs = (('y', (S, self.max_frames_per_call, C), parsed.name, None),) + _slot_ints(S, 'counts', 'flags')
        self._outputs = (('columns', (S, self.rows_per_call if self.columns else 0, C, self.bins), parsed.name, 'empty'),
                         ('out_counts', (S,), 'int32', 'empty'))
        self._mirror()

    @property
    def rows_per_call(self) -> int:
        """RC: the most columns a call returns per slot, ``ceil(max_frames_per_call / hop)``."""
        return -(-self.max_frames_per_call // self.hop)

    @property
    def bins(self) -> int:
        return self.nfft // 2 + 1

    @property
    def f(self) -> np.ndarray:
        """SciPy's one-sided bin frequencies."""
        return bin_frequencies(self.nfft, self.fs)

    @property
    def _out_width(self) -> int:
        return self.bins

    def process(self, blocks=None, *, start=(), end=(), discard: bool = False):
        """One call of the dict form.  ``blocks``: ``{slot: (n, channels) array of the pool's dtype}`` (``(n,)`` as well for
        one channel), ``0 <= n <= max_frames_per_call``; ``start``: the slots whose voice begins with this call; ``end``:
        the slots whose voice ends with it.  Returns ``{slot: (T_new, channels, F)}`` for every slot that got a block or
        ended (without ``columns``: ``T_new`` is 0).  Raises before any device call, as the other voice pools do."""
        self._require_form('dict')
        out = _SlotPool.process(self, blocks, start=self._start_slots(start), end=end, discard=discard)
        none = np.zeros((0, self.in_channels, self.bins), self.dtype)
        return {slot: rows if rows.ndim == 3 else none.copy() for slot, rows in out.items()}

    def process_dev(self, y, counts, flags, *, out=None):
        """One call on device tensors, enqueued on the current stream: ``y`` ``(slots, M, channels)`` of the pool's dtype,
        ``counts`` / ``flags`` int32 ``(slots,)``.  Returns ``(columns, out_counts)``: ``(slots, rows_per_call, channels,
        F)`` of the pool's dtype - the first ``out_counts[b]`` rows of row-block b are written, nothing at or past them;
        without ``columns`` it has no rows - and int32 ``(slots,)``; ``out=(columns, out_counts)`` takes the caller's.  The
        means are in ``pxx``, ``pyy``, ``pxy`` and ``segments`` when the call has run.  No check reads device memory; bad
        per-slot values answer -1 (``include/vnd_spectrum_voice_stream.h``)."""
        return self._process_dev((y, counts, flags), out)

    def coherence(self):
        """SciPy's ``abs(Pxy)**2 / Pxx / Pyy`` of every slot, ``(slots, F)``, in torch operations on the means: enqueued on
        the current stream, nothing synchronised.  A slot with no whole segment is 0 / 0: NaN."""
        if self.in_channels != 2:
            raise ValueError('coherence needs two channels')
        if self.pxx is None:
            raise RuntimeError('the pool has no means yet: call reset() or process first')
        torch = _torch()
        return torch.abs(torch.view_as_complex(self.pxy)) ** 2 / self.pxx / self.pyy

    def welch(self, slot: int):
        """``(segments, Pxx, Pyy, Pxy)`` of one slot as NumPy values, read from the device (it waits for the stream):
        the segment count the means are taken over, ``(F,)`` arrays of the pool's dtype and the complex ``Pxy``; ``Pyy``
        and ``Pxy`` are None with one channel."""
        slot = self._slot(slot, 'welch')
        if self.pxx is None:
            raise RuntimeError('the pool has no means yet: call reset() or process first')
        torch = _torch()
        segments = int(self.segments[slot].cpu())
        pxx = self.pxx[slot].cpu().numpy()
        if self.in_channels == 1:
            return segments, pxx, None, None
        return segments, pxx, self.pyy[slot].cpu().numpy(), torch.view_as_complex(self.pxy[slot]).cpu().numpy()

    # ---- what _SlotPool asks for ---------------------------------------------------------------
    def _spans(self, counts, flags, tables):
        out, _, new = spectrum_voice_spans(self.positions, counts, flags, self.nperseg, self.hop, self.max_frames_per_call)
        return out, new

    # ---- the device -------------------------------------------------------------------------
    def _allocate(self, torch, ctx):
        """The means at their fixed addresses and the tables of the transform, then the state."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('the state of a voice pool is allocated and zeroed on first use: call reset() before the capture')
        device = torch.device('cuda', ctx.device)
        tdt = getattr(torch, self.dtype.name)
        S, F = self.slots, self.bins
        self._win, self._tw = _device_tables(torch, device, self._win64, self.nfft, self.dtype)
        self.pxx = torch.zeros((S, F), dtype=tdt, device=device)
        self.pyy = torch.zeros((S, F), dtype=tdt, device=device) if self.in_channels == 2 else None
        self.pxy = torch.zeros((S, F, 2), dtype=tdt, device=device) if self.in_channels == 2 else None
        self.segments = torch.zeros((S,), dtype=torch.int64, device=device)
        _SlotPool._allocate(self, torch, ctx)

    def _state_bytes(self, ctx) -> int:
        return _native.spectrum_voice_stream_state_bytes(self.slots, self.in_channels, self.nperseg, self.hop, self.nfft,
                                                         self.max_frames_per_call, self.dtype == np.float64)

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        _native.spectrum_voice_stream_reset_device(ctx, state_ptr, state_bytes, self.slots, self.in_channels, self.nperseg,
                                                   self.hop, self.nfft, self.max_frames_per_call, self.dtype == np.float64,
                                                   stream=stream)

    def _launch(self, ctx, state_ptr, state_bytes, inputs, cols, out_counts, stream):
        y, counts, flags = inputs
        C, M = self.in_channels, self.max_frames_per_call
        stereo = C == 2
        _native.spectrum_voice_stream_device(
            ctx, state_ptr, state_bytes, M, y.data_ptr(), C * M, C, C, counts.data_ptr(), flags.data_ptr(),
            self._win.data_ptr(), self._tw.data_ptr(), self.nperseg, self.hop, self.nfft,
            cols.data_ptr() if self.columns else 0, out_counts.data_ptr(), self.pxx.data_ptr(),
            self.pyy.data_ptr() if stereo else 0, self.pxy.data_ptr() if stereo else 0, self.segments.data_ptr(), self.slots,
            detrend=self.detrend is not False, scale=self.scale, float64=self.dtype == np.float64, stream=stream)


def spectrum_voice_pool(slots: int, max_frames_per_call: int, fs=1.0, window='hann', nperseg=256, noverlap=None, nfft=None,
                        detrend='constant', scaling='density', channels: int = 2, dtype='float32',
                        columns: bool = True) -> SpectrumVoicePool:
    """A :class:`SpectrumVoicePool`: ``scipy.signal.spectrogram`` columns and ``welch`` / ``csd`` / ``coherence`` means with
    these arguments - ``welch``'s defaults, ``noverlap = nperseg // 2`` - for ``slots`` voices that start, end and push
    blocks on their own, the positions in device memory.  What :func:`spectrum_covers` rejects, what one launch does not
    take, pools above 65535 slots and a ``dtype`` other than ``'float32'`` / ``'float64'`` raise ``ValueError`` here: a
    stream has no SciPy loop to fall back to.  ``columns=False`` keeps the means only.  ``set_spectrum_device`` is not
    consulted."""
    return SpectrumVoicePool(slots, max_frames_per_call, fs=fs, window=window, nperseg=nperseg, noverlap=noverlap, nfft=nfft,
                             detrend=detrend, scaling=scaling, channels=channels, dtype=dtype, columns=columns)


__all__ = ['spectrogram_batched', 'welch_batched', 'csd_batched', 'coherence_batched', 'set_spectrum_device',
           'spectrum_covers', 'twiddle_table', 'spectrum_scale', 'segment_times', 'bin_frequencies', 'run_length', 'MIN_NFFT',
           'MAX_NFFT', 'RUN', 'spectrum_voice_pool', 'SpectrumVoicePool', 'spectrum_voice_spans']
