"""The vectorscope's data on the GPU (include/vnd_scope.h, include/vnd_level.h): what ``utils/plot.py`` reduces a signal to
before it draws.

The reference looks at a decorrelated signal through ``plot_polar_sample``, ``plot_lissajous`` and ``plot_polar_level``; all
are matplotlib around steps that touch every frame - ``polar_coordinates(L, R, compute_weights=False)``, then
``np.histogram2d`` or, for the level envelope, ``np.percentile`` per angular slice.  Here those steps run on the device for a
whole pool, so a pool of voices that lives in device memory never comes down to be looked at:

* :func:`polar_coordinates_batched` - ``(radii, thetas)`` of every frame of a pool (``vnd_polar_coords_*_dev``);
* :func:`polar_histogram_batched` - the count grid of ``plot_polar_sample``'s heatmap, fused: no theta or radius is written
  (``vnd_polar_hist_*_dev``);
* :func:`lissajous_histogram_batched` - the count grid of ``plot_lissajous(color_mode='density')``
  (``vnd_lissajous_hist_*_dev``);
* :func:`polar_level_batched` - the raw envelope of ``plot_polar_level``: ``_build_pseudo_hull``'s per-slice percentiles of
  the radii, an exact radix select (``vnd_polar_level_*_dev``), with :func:`percentile_rule`, NumPy's rule in one place;
* :func:`polar_histogram_voice_pool` / :func:`lissajous_histogram_voice_pool` - the same grids for the voices of a voice
  pool, block by block, of each voice's whole signal or of its last ``window_frames`` frames (:class:`ScopeVoicePool`,
  ``include/vnd_scope_voice_stream.h``);
* :func:`polar_level_voice_pool` - the level envelope of each voice's last ``window_frames`` frames, the same select over
  a ring of staged keys (:class:`LevelVoicePool`, ``include/vnd_polar_level_voice_stream.h``);
* :func:`set_scope_device` and the pure routing rule :func:`scope_covers`, through ``analysis.device_route``.

Counts are integers: a grid equals ``np.histogram2d`` of the same coordinates cell for cell, whatever the route
(``VND_SCOPE_ROUTE``) and the run.  The coordinates are NumPy 2's arithmetic on the sample type except for the
last bits of ``atan2`` (two libm implementations).  Without a device, or for a call the device does not cover, every
function is the NumPy loop: ``utils.dsp.polar_coordinates`` and ``np.histogram2d`` (``np.percentile`` per slice) per signal.
Drawing, the heatmap's smoothing and ``log1p``, the envelope's Gaussian smoothing and convex hull, and
``compute_weights=True`` are not here.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from .streaming import _INT32_MAX, _check_counts, _MeterPool, _slot_ints, _SlotPool, _valid_voice_spans
from .utils.dsp import LayoutMode, polar_coordinates

MAX_BINS = _native.SCOPE_MAX_BINS
SPAN_FRAMES = _native.SCOPE_SPAN_FRAMES               # frames of one signal per workgroup on the LDS-private route
DIRECT_SPAN_FRAMES = _native.SCOPE_DIRECT_SPAN_FRAMES
LDS_BYTES = _native.SCOPE_LDS_BYTES
ROUTE_LDS, ROUTE_DIRECT = _native.SCOPE_ROUTE_LDS, _native.SCOPE_ROUTE_DIRECT
LEVEL_MAX_BINS = _native.LEVEL_MAX_BINS               # slices of the level envelope on the device
LEVEL_MAX_PERCENTILES = _native.LEVEL_MAX_PERCENTILES
LEVEL_SPAN_FRAMES = _native.LEVEL_SPAN_FRAMES         # frames of one signal per workgroup of the level kernels
_MAX_FRAMES = 2 ** 32 - 1                             # counts are uint32
_MAX_BATCH = 65535                                    # VND_MAX_STREAMS
_MAX_GROUPS = 2 ** 23
_COORDS_SPAN = 2048                                   # the smallest span of any kernel: bounds every launch
_torch = _native.torch_module

_scope_device: Optional[bool] = None
_edges_cache: dict = {}


def set_scope_device(enabled: Optional[bool]) -> None:
    """Where the three functions of this module run.

    ``None`` (default): on the GPU when a gfx950 device is present and the call is covered (:func:`scope_covers`),
    otherwise the NumPy code.  ``True``: the device for every covered call; such a call raises ``RuntimeError`` when
    there is no device.  ``False``: always NumPy."""
    global _scope_device
    if enabled is not None and not isinstance(enabled, (bool, np.bool_)):
        raise TypeError(f'set_scope_device takes True, False or None, not {enabled!r}')
    _scope_device = None if enabled is None else bool(enabled)


def scope_covers(dtype, batch: int, n_frames: int, bins0: int = 1, bins1: int = 1) -> bool:
    """Whether a pool of ``batch`` signals of ``n_frames`` frames of ``dtype`` has a device form, for a grid of ``bins0`` x
    ``bins1`` cells: float32 or float64 frames, 1 <= batch <= 65535, 1 <= n_frames < 2^32, bins of 1..MAX_BINS an axis and
    at most 2^23 workgroups in a launch.  Everything else keeps the NumPy code and its exceptions (an empty signal:
    ``ValueError`` from ``max``)."""
    try:
        if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
            return False
    except TypeError:
        return False
    for v in (batch, n_frames, bins0, bins1):
        if not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)):
            return False
    if not 1 <= batch <= _MAX_BATCH or not 1 <= n_frames <= _MAX_FRAMES:
        return False
    if not 1 <= bins0 <= MAX_BINS or not 1 <= bins1 <= MAX_BINS:
        return False
    return batch * (-(-n_frames // _COORDS_SPAN)) <= _MAX_GROUPS


def use_device(dtype, batch: int, n_frames: int, bins0: int = 1, bins1: int = 1) -> bool:
    """The routing decision of one call: :func:`scope_covers` and :func:`set_scope_device`."""
    from .analysis import device_route
    return device_route(_scope_device, scope_covers(dtype, batch, n_frames, bins0, bins1),
                        'set_scope_device(True): no gfx950 device (or no built extension) to run on')


# ---- the binning rule ------------------------------------------------------------------------------------------------
def histogram_bins(values, edges) -> np.ndarray:
    """The device's binning rule in NumPy, which is ``np.histogramdd``'s: the bin of each value on ascending ``edges``
    (``edges[k] <= v < edges[k + 1]``, ``v == edges[-1]`` in the last bin), -1 for a value that is dropped (outside the
    range, NaN, +-inf)."""
    edges = np.asarray(edges, np.float64)
    v = np.asarray(values).astype(np.float64)
    k = np.searchsorted(edges, v, side='right')
    k[v == edges[-1]] -= 1
    k -= 1
    k[(k < 0) | (k >= len(edges) - 1)] = -1
    return k


def histogram_counts(v0, v1, edges0, edges1) -> np.ndarray:
    """The count grid of coordinate pairs under :func:`histogram_bins`: int64 ``(len(edges0) - 1, len(edges1) - 1)``,
    equal to ``np.histogram2d(v0, v1, [edges0, edges1])[0]`` cell for cell."""
    k0, k1 = histogram_bins(v0, edges0), histogram_bins(v1, edges1)
    keep = (k0 >= 0) & (k1 >= 0)
    grid = np.zeros((len(edges0) - 1, len(edges1) - 1), np.int64)
    np.add.at(grid, (k0[keep], k1[keep]), 1)
    return grid


def polar_edges(num_angle_bins: int = 240, num_radius_bins: int = 150):
    """``plot_polar_sample``'s edges: degrees on [-90, 90] and normalised radii on [0, 1]."""
    return np.linspace(-90.0, 90.0, num_angle_bins + 1), np.linspace(0.0, 1.0, num_radius_bins + 1)


def lissajous_edges(bins=512, range=((-1.1, 1.1), (-1.1, 1.1))):      # noqa: A002 - np.histogram2d's name
    """``np.histogram2d(..., bins=bins, range=range)``'s edges: ``np.linspace(lo, hi, bins + 1)`` an axis."""
    bx, by = (bins, bins) if isinstance(bins, (int, np.integer)) else bins
    (x0, x1), (y0, y1) = range
    return np.linspace(float(x0), float(x1), int(bx) + 1), np.linspace(float(y0), float(y1), int(by) + 1)


def lissajous_step(n_frames: int, max_points: Optional[int]) -> int:
    """``plot_lissajous``'s decimation: every ``n // max_points``-th frame when ``n > max_points``."""
    if max_points is None:
        return 1
    if isinstance(max_points, (bool, np.bool_)) or not isinstance(max_points, (int, np.integer)) or max_points < 1:
        raise ValueError(f'max_points must be a positive integer or None, not {max_points!r}')
    return n_frames // int(max_points) if n_frames > max_points else 1


# ---- shapes ----------------------------------------------------------------------------------------------------------
def _pool_shape(pool):
    shape = tuple(pool.shape)
    if len(shape) == 2 and shape[1] == 2:
        return True, (1,) + shape
    if len(shape) == 3 and shape[2] == 2:
        return False, shape
    raise ValueError(f'pool must be (batch, n, 2), or (n, 2) for one signal: got shape {shape}')


def _mode(mode) -> bool:
    if mode == LayoutMode.MS:
        return True
    if mode == LayoutMode.LR:
        return False
    raise ValueError(f"mode must be 'MS' or 'LR', not {mode!r}")


def _bins(n, what: str) -> int:
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f'{what} must be a positive integer, not {n!r}')
    return int(n)


def _scale(radius_scale, accumulate: bool):
    if radius_scale is None:
        if accumulate:
            raise ValueError('accumulate=True needs a fixed radius_scale: the per-signal maximum of a later block would '
                             'rescale the earlier frames')
        return None
    scale = float(radius_scale)
    if not (scale > 0.0 and np.isfinite(scale)):
        raise ValueError(f'radius_scale must be a positive finite number or None, not {radius_scale!r}')
    return scale


def _host_n_each(counts, batch: int, n: int):
    """Frames each signal contributes on the host route: ``counts`` outside ``[0, n]`` contributes none."""
    if counts is None:
        return [n] * batch
    if _native.is_torch(counts):
        counts = counts.detach().cpu().numpy()
    c = np.asarray(counts).astype(np.int64).reshape(-1)
    if len(c) != batch:
        raise ValueError(f'counts must have one entry per signal: got {len(c)} for {batch}')
    return [int(v) if 0 <= v <= n else 0 for v in c]


def _device_of(pool):
    """The context's torch device when ``pool`` is a tensor on it, else None."""
    try:
        torch = _torch()
        device = torch.device('cuda', _native.default_context().device)
    except RuntimeError:
        return None
    return device if pool.device == device else None


def _tensor_channels(pool):
    """Device pointers and strides of the channels of a (B, n, 2) tensor: ``(l_ptr, r_ptr, stream_stride, frame_stride,
    keep)``."""
    if pool.stride(2) != 1 or pool.stride(1) < 1 or (pool.shape[0] > 1 and pool.stride(0) < 1):
        pool = pool.contiguous()
    return (pool.data_ptr(), pool.data_ptr() + pool.element_size(), max(1, pool.stride(0)), pool.stride(1), pool)


def _device_edges(torch, device, e0: np.ndarray, e1: np.ndarray):
    """The two edge arrays on the device, uploaded once per distinct pair: a later call - or a graph capture - copies
    nothing from the host."""
    key = (str(device), e0.tobytes(), e1.tobytes())
    got = _edges_cache.get(key)
    if got is None:
        if len(_edges_cache) >= 64:
            _edges_cache.clear()
        got = (torch.from_numpy(e0.copy()).to(device), torch.from_numpy(e1.copy()).to(device))
        _edges_cache[key] = got
    return got


def _device_counts(torch, counts, batch: int, device):
    if counts is None:
        return None
    if not _native.is_torch(counts):
        counts = torch.from_numpy(np.ascontiguousarray(counts, np.int32))
    if counts.dtype != torch.int32 or tuple(counts.shape) != (batch,):
        raise ValueError(f'counts must be int32 of shape ({batch},): got {counts.dtype} {tuple(counts.shape)}')
    return counts.to(device).contiguous()


def _device_out(torch, out, shape, device, accumulate: bool):
    if out is None:
        if accumulate:
            raise ValueError('accumulate=True needs the grid to add to: pass out=')
        return torch.empty(shape, dtype=torch.int32, device=device)
    if not _native.is_torch(out) or out.dtype != torch.int32 or tuple(out.shape) != tuple(shape) \
            or out.device != device or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous int32 tensor of shape {tuple(shape)} on {device}')
    return out


def _host_out(out, grid: np.ndarray, accumulate: bool) -> np.ndarray:
    if out is None:
        if accumulate:
            raise ValueError('accumulate=True needs the grid to add to: pass out=')
        return grid
    if not isinstance(out, np.ndarray) or out.shape != grid.shape:
        raise ValueError(f'out must be a NumPy array of shape {grid.shape}')
    if accumulate:
        out += grid.astype(out.dtype)
    else:
        out[...] = grid
    return out


def _dtype_of(pool) -> np.dtype:
    if not _native.is_torch(pool):
        return np.asarray(pool).dtype
    try:
        return np.dtype(str(pool.dtype).replace('torch.', ''))
    except TypeError:                                     # a torch dtype NumPy has no name for: not covered
        return np.dtype(object)


def _to_host(pool) -> np.ndarray:
    return pool.detach().cpu().numpy() if _native.is_torch(pool) else np.asarray(pool)


# ---- polar coordinates -----------------------------------------------------------------------------------------------
def polar_coordinates_batched(pool, mode=LayoutMode.MS, semicircular: bool = True, normalize: bool = True):
    """``polar_coordinates(pool[b, :, 0], pool[b, :, 1], mode, semicircular, normalize, compute_weights=False)`` for every
    signal of a ``(B, n, 2)`` pool (``(n, 2)``: one signal): ``(radii, thetas)``, each ``(B, n)`` (``(n,)``) of the pool's
    dtype.  ``normalize`` divides each signal's radii by its own maximum plus ``EPSILON``.  A float32 or float64 tensor on
    the device in gives device tensors out, with nothing synchronised; NumPy in gives NumPy out.  On the device the radii
    are NumPy's bit for bit, and the thetas within the last bits of ``atan2``."""
    ms = _mode(mode)
    single, (batch, n, _) = _pool_shape(pool)
    is_tensor = _native.is_torch(pool)
    dtype = _dtype_of(pool)
    if use_device(dtype, batch, n) and (not is_tensor or _device_of(pool) is not None):
        torch = _torch()
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        pd = (pool if is_tensor else torch.from_numpy(np.ascontiguousarray(pool)).to(device)).reshape(batch, n, 2)
        lp, rp, ss, fs, keep = _tensor_channels(pd)
        radii = torch.empty((batch, n), dtype=pd.dtype, device=device)
        thetas = torch.empty((batch, n), dtype=pd.dtype, device=device)
        work = torch.empty((batch,), dtype=torch.int64, device=device) if normalize else None
        _native.polar_coords_device(ctx, lp, rp, batch, n, ss, fs, radii.data_ptr(), thetas.data_ptr(), ms_mode=ms,
                                    semicircular=semicircular, normalize=normalize,
                                    work_ptr=work.data_ptr() if normalize else 0, work_bytes=batch * 8 if normalize else 0,
                                    float64=dtype == np.float64, stream=torch.cuda.current_stream(device).cuda_stream)
        del keep
        if single:
            radii, thetas = radii[0], thetas[0]
        return (radii, thetas) if is_tensor else (radii.cpu().numpy(), thetas.cpu().numpy())

    host = _to_host(pool).reshape(batch, n, 2)
    pairs = [polar_coordinates(host[b, :, 0], host[b, :, 1], LayoutMode.MS if ms else LayoutMode.LR, semicircular, normalize,
                               compute_weights=False) for b in range(batch)]
    radii = np.stack([p[0] for p in pairs]) if pairs else np.zeros((0, n), host.dtype)
    thetas = np.stack([p[1] for p in pairs]) if pairs else np.zeros((0, n), host.dtype)
    if single:
        radii, thetas = radii[0], thetas[0]
    if is_tensor:
        torch = _torch()
        return torch.from_numpy(radii).to(pool.device), torch.from_numpy(thetas).to(pool.device)
    return radii, thetas


# ---- histograms ------------------------------------------------------------------------------------------------------
def _histogram(pool, e0: np.ndarray, e1: np.ndarray, counts, out, accumulate: bool, *, polar: bool, ms: bool = True,
               semicircular: bool = True, scale: Optional[float] = None, step: int = 1):
    """Both grids, on either route: ``(grid, edges0, edges1)``."""
    single, (batch, n, _) = _pool_shape(pool)
    bins0, bins1 = len(e0) - 1, len(e1) - 1
    shape = (bins0, bins1) if single else (batch, bins0, bins1)
    is_tensor = _native.is_torch(pool)
    dtype = _dtype_of(pool)
    if use_device(dtype, batch, n, bins0, bins1) and (not is_tensor or _device_of(pool) is not None):
        torch = _torch()
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        pd = (pool if is_tensor else torch.from_numpy(np.ascontiguousarray(pool)).to(device)).reshape(batch, n, 2)
        lp, rp, ss, fs, keep = _tensor_channels(pd)
        d0, d1 = _device_edges(torch, device, e0, e1)
        each = _device_counts(torch, counts, batch, device)
        if is_tensor:
            grid = _device_out(torch, out, shape, device, accumulate)
        else:
            if accumulate and out is None:
                raise ValueError('accumulate=True needs the grid to add to: pass out=')
            grid = torch.empty(shape, dtype=torch.int32, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream
        on_device = is_tensor and accumulate
        kw = dict(n_each_ptr=each.data_ptr() if each is not None else 0, accumulate=on_device, float64=dtype == np.float64,
                  stream=stream)
        if polar:
            by_max = scale is None
            work = torch.empty((batch,), dtype=torch.int64, device=device) if by_max else None
            _native.polar_hist_device(ctx, lp, rp, batch, n, ss, fs, d0.data_ptr(), bins0, d1.data_ptr(), bins1, grid.data_ptr(),
                                      ms_mode=ms, semicircular=semicircular, radius_scale=0.0 if by_max else scale,
                                      work_ptr=work.data_ptr() if by_max else 0, work_bytes=batch * 8 if by_max else 0, **kw)
        else:
            _native.lissajous_hist_device(ctx, lp, rp, batch, n, ss, fs, d0.data_ptr(), bins0, d1.data_ptr(), bins1,
                                          grid.data_ptr(), frame_step=step, **kw)
        del keep
        if is_tensor:
            return grid, d0.clone(), d1.clone()
        host_grid = grid.cpu().numpy().view(np.uint32).astype(np.float64)
        return _host_out(out, host_grid, accumulate), e0, e1

    host = _to_host(pool).reshape(batch, n, 2)
    each_host = _host_n_each(counts, batch, n)
    grids = np.zeros((batch, bins0, bins1), np.float64)
    for b, m in enumerate(each_host):
        left, right = host[b, :m, 0], host[b, :m, 1]
        if m == 0:
            continue
        if polar:
            radii, thetas = polar_coordinates(left, right, LayoutMode.MS if ms else LayoutMode.LR, semicircular,
                                              scale is None, compute_weights=False)
            if scale is not None:
                radii = radii / radii.dtype.type(scale)
            grids[b] = np.histogram2d(np.degrees(thetas), radii, bins=[e0, e1])[0]
        else:
            grids[b] = np.histogram2d(left[::step], right[::step], bins=[e0, e1])[0]
    grids = grids.reshape(shape)
    if is_tensor:
        torch = _torch()
        as_tensor = torch.from_numpy(grids.astype(np.int64).astype(np.uint32).view(np.int32)).to(pool.device)
        if out is not None:
            if not _native.is_torch(out) or out.dtype != torch.int32 or tuple(out.shape) != tuple(shape):
                raise ValueError(f'out must be an int32 tensor of shape {tuple(shape)}')
            if accumulate:
                out += as_tensor.to(out.device)
            else:
                out.copy_(as_tensor)
            as_tensor = out
        elif accumulate:
            raise ValueError('accumulate=True needs the grid to add to: pass out=')
        return as_tensor, torch.from_numpy(e0.copy()).to(pool.device), torch.from_numpy(e1.copy()).to(pool.device)
    return _host_out(out, grids, accumulate), e0, e1


def polar_histogram_batched(pool, num_angle_bins: int = 240, num_radius_bins: int = 150, *, radius_scale=None, counts=None,
                            out=None, accumulate: bool = False, mode=LayoutMode.MS, semicircular: bool = True):
    """The count grid of ``plot_polar_sample``'s heatmap for every signal of a ``(B, n, 2)`` pool (``(n, 2)``: one signal):
    ``(grid, angle_edges, radius_edges)`` with ``grid[b] == np.histogram2d(np.degrees(thetas), radii, bins=[angle_edges,
    radius_edges])[0]`` of that signal's polar sample, edges ``np.linspace(-90, 90, num_angle_bins + 1)`` degrees and
    ``np.linspace(0, 1, num_radius_bins + 1)``.

    ``radius_scale`` None: the reference's radii, normalised by each signal's own maximum.  A positive number: ``radii /
    radius_scale`` instead, which does not depend on the rest of the signal - so blocks of a signal can be added up:
    ``accumulate=True`` adds to the grid passed as ``out`` (and needs a ``radius_scale``).  ``counts``: optional int32
    ``(B,)``, signal b is its first ``counts[b]`` frames (a value outside ``[0, n]``: none) - the ``out_counts`` of a voice
    pool or a block stream, read on the device.

    A float32 or float64 tensor on the device in gives device tensors out with nothing synchronised - the grid an int32
    tensor holding the uint32 counts (``out``, when given, is such a tensor); the device edges are uploaded on the first
    call with a grid size, so warm a call up before capturing one in a graph.  NumPy in gives NumPy out, the grid float64 as
    ``np.histogram2d`` returns it."""
    bins0, bins1 = _bins(num_angle_bins, 'num_angle_bins'), _bins(num_radius_bins, 'num_radius_bins')
    scale = _scale(radius_scale, accumulate)
    e0, e1 = polar_edges(bins0, bins1)
    return _histogram(pool, e0, e1, counts, out, accumulate, polar=True, ms=_mode(mode), semicircular=semicircular,
                      scale=scale)


def lissajous_histogram_batched(pool, bins=512, range=((-1.1, 1.1), (-1.1, 1.1)), *, max_points: Optional[int] = None,  # noqa: A002
                                counts=None, out=None, accumulate: bool = False):
    """The count grid of ``plot_lissajous(color_mode='density')`` for every signal of a ``(B, n, 2)`` pool (``(n, 2)``: one
    signal): ``(grid, x_edges, y_edges)`` with ``grid[b] == np.histogram2d(left, right, bins=bins, range=range)[0]``, L on
    the first axis.  ``max_points``: as the reference, every ``n // max_points``-th frame when ``n > max_points``
    (``left[::step]``).  ``counts``, ``out``, ``accumulate`` and the tensor / NumPy forms as in
    :func:`polar_histogram_batched`."""
    e0, e1 = lissajous_edges(bins, range)
    if len(e0) < 2 or len(e1) < 2 or not (np.all(np.diff(e0) > 0) and np.all(np.diff(e1) > 0)
                                          and np.all(np.isfinite(e0)) and np.all(np.isfinite(e1))):
        raise ValueError(f'bins {bins!r} and range {range!r} do not give ascending finite edges')
    _, (_, n, _) = _pool_shape(pool)
    step = lissajous_step(n, max_points)
    return _histogram(pool, e0, e1, counts, out, accumulate, polar=False, step=step)


# ---- the polar level envelope (include/vnd_level.h) ------------------------------------------------------------------
def percentile_rule(m: int, p: float, dtype=np.float32):
    """``np.percentile``'s rule (NumPy 2, ``method='linear'``) for ``m`` values of ``dtype`` and percentile ``p``:
    ``(prev, next, gamma)`` - the two order statistics it reads, as indices into the sorted values, and the weight between
    them, a ``dtype`` scalar.  Every step is one correctly rounded operation in ``dtype``; it is the arithmetic of the
    device's init kernel.  ``p`` outside [0, 100], or NaN, raises NumPy's ``ValueError``."""
    kind = np.dtype(dtype).type
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 1:
        raise ValueError(f'm must be a positive integer, not {m!r}')
    p = float(p)
    if not 0.0 <= p <= 100.0:
        raise ValueError('Percentiles must be in the range [0, 100]')
    q = kind(p) / kind(100)
    top = kind(int(m) - 1)
    v = top * q
    if v >= top:
        return int(m) - 1, int(m) - 1, kind(0)
    prev = int(np.floor(v))
    return prev, prev + 1, v - kind(prev)


def percentile_of_sorted(values: np.ndarray, p: float):
    """``np.percentile(values, p)`` of ascending ``values`` through :func:`percentile_rule`, bit for bit: NumPy's lerp, every
    operation rounded on its own in the values' dtype."""
    kind = values.dtype.type
    prev, nxt, g = percentile_rule(len(values), p, values.dtype)
    a, b = values[prev], values[nxt]
    with np.errstate(invalid='ignore'):
        d = b - a
        return b - d * (kind(1) - g) if g >= kind(0.5) else a + d * g


def level_edges(num_bins: int = 360):
    """``_build_pseudo_hull``'s slices: ``(bin_edges, bin_centers)`` in degrees on [-90, 90]."""
    edges = np.linspace(-90.0, 90.0, num_bins + 1)
    return edges, 0.5 * (edges[:-1] + edges[1:])


def _percentiles(percentiles):
    ps = [float(p) for p in np.atleast_1d(np.asarray(percentiles, np.float64)).reshape(-1)]
    if not ps:
        raise ValueError('percentiles must hold at least one value')
    for p in ps:
        if not 0.0 <= p <= 100.0:
            raise ValueError('Percentiles must be in the range [0, 100]')
    return ps


def level_covers(dtype, batch: int, n_frames: int, num_bins: int, num_percentiles: int) -> bool:
    """Whether ``polar_level_batched`` of this shape has a device form: :func:`scope_covers` and the two limits of
    include/vnd_level.h, at most ``LEVEL_MAX_BINS`` slices and ``LEVEL_MAX_PERCENTILES`` percentiles."""
    return (scope_covers(dtype, batch, n_frames, num_bins, 1) and num_bins <= LEVEL_MAX_BINS
            and 1 <= num_percentiles <= LEVEL_MAX_PERCENTILES)


def _host_levels(left, right, edges, ps, ms: bool, semicircular: bool, scale):
    """One signal on the host: the reference's mask and ``np.percentile`` per slice."""
    radii, thetas = polar_coordinates(left, right, LayoutMode.MS if ms else LayoutMode.LR, semicircular, scale is None,
                                      compute_weights=False)
    if scale is not None:
        radii = radii / radii.dtype.type(scale)
    degrees = np.degrees(thetas)
    bins = len(edges) - 1
    levels, counts = np.zeros((len(ps), bins)), np.zeros(bins, np.int64)
    for k in range(bins):
        mask = (degrees >= edges[k]) & (degrees < edges[k + 1])
        counts[k] = np.count_nonzero(mask)
        if counts[k]:
            inside = radii[mask]
            for i, p in enumerate(ps):
                levels[i, k] = np.percentile(inside, p)
    return levels, counts


def polar_level_batched(pool, num_bins: int = 360, percentiles=(95.0, 50.0), *, radius_scale=None, counts=None,
                        mode=LayoutMode.MS, semicircular: bool = True):
    """The raw envelope of ``plot_polar_level`` for every signal of a ``(B, n, 2)`` pool (``(n, 2)``: one signal):
    ``(levels, bin_counts, bin_edges, bin_centers)`` with ``levels[b, i]`` the ``bin_percentile_radii`` of
    ``_build_pseudo_hull(np.degrees(thetas), radii, num_bins, percentiles[i], smoothing_sigma=0, use_convex_hull=False)`` of
    that signal's polar sample - per slice ``edges[k] <= degrees < edges[k + 1]`` of ``np.linspace(-90, 90, num_bins + 1)``,
    ``np.percentile`` of the radii inside, 0 for an empty slice (a frame at exactly +90 degrees, R = -L with L > 0, is in no
    slice) - and ``bin_counts[b]`` the frames per slice.  The envelope's smoothing and convex hull work on these ``num_bins``
    numbers and stay with the caller.

    ``radius_scale``, ``counts``, ``mode`` and ``semicircular`` as in :func:`polar_histogram_batched`.  There is no
    ``accumulate``: percentiles of blocks do not add up.  ``percentiles`` outside [0, 100] raise NumPy's ``ValueError``.

    A float32 or float64 tensor on the device in gives device tensors out with nothing synchronised: ``levels`` of the
    pool's dtype, ``bin_counts`` int32 holding uint32; on the device a level is ``np.percentile`` of the device's own radii
    bit for bit (an exact radix select).  The edges are uploaded on the first call with a ``num_bins``, so
    warm a call up before capturing one in a graph.  NumPy in gives NumPy out: ``levels`` float64 holding the sample-type
    values, as the reference's ``np.zeros(num_bins)`` array does, ``bin_counts`` int64.  More than ``LEVEL_MAX_BINS`` slices
    or ``LEVEL_MAX_PERCENTILES`` percentiles, another dtype, or no device: the NumPy loop."""
    bins = _bins(num_bins, 'num_bins')
    ps = _percentiles(percentiles)
    scale = _scale(radius_scale, False)
    ms = _mode(mode)
    edges, centers = level_edges(bins)
    single, (batch, n, _) = _pool_shape(pool)
    is_tensor = _native.is_torch(pool)
    dtype = _dtype_of(pool)
    from .analysis import device_route
    on_device = device_route(_scope_device, level_covers(dtype, batch, n, bins, len(ps)),
                             'set_scope_device(True): no gfx950 device (or no built extension) to run on')
    if on_device and (not is_tensor or _device_of(pool) is not None):
        torch = _torch()
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        pd = (pool if is_tensor else torch.from_numpy(np.ascontiguousarray(pool)).to(device)).reshape(batch, n, 2)
        lp, rp, ss, fs, keep = _tensor_channels(pd)
        d_edges, d_centers = _device_edges(torch, device, edges, centers)
        each = _device_counts(torch, counts, batch, device)
        is64 = dtype == np.float64
        levels = torch.empty((batch, len(ps), bins), dtype=pd.dtype, device=device)
        bin_counts = torch.empty((batch, bins), dtype=torch.int32, device=device)
        work_bytes = _native.polar_level_work_bytes(batch, n, bins, len(ps), is64)
        work = torch.empty(((work_bytes + 7) // 8,), dtype=torch.int64, device=device)
        _native.polar_level_device(ctx, lp, rp, batch, n, ss, fs, d_edges.data_ptr(), bins, ps, levels.data_ptr(),
                                   bin_counts.data_ptr(), work_ptr=work.data_ptr(), work_bytes=work_bytes, ms_mode=ms,
                                   semicircular=semicircular, radius_scale=0.0 if scale is None else scale,
                                   n_each_ptr=each.data_ptr() if each is not None else 0, float64=is64,
                                   stream=torch.cuda.current_stream(device).cuda_stream)
        del keep
        if single:
            levels, bin_counts = levels[0], bin_counts[0]
        if is_tensor:
            return levels, bin_counts, d_edges.clone(), d_centers.clone()
        return (levels.cpu().numpy().astype(np.float64), bin_counts.cpu().numpy().view(np.uint32).astype(np.int64), edges,
                centers)

    host = _to_host(pool).reshape(batch, n, 2)
    levels, bin_counts = np.zeros((batch, len(ps), bins)), np.zeros((batch, bins), np.int64)
    for b, m in enumerate(_host_n_each(counts, batch, n)):
        if m:
            levels[b], bin_counts[b] = _host_levels(host[b, :m, 0], host[b, :m, 1], edges, ps, ms, semicircular, scale)
    if single:
        levels, bin_counts = levels[0], bin_counts[0]
    if is_tensor:
        torch = _torch()
        out_dtype = host.dtype if host.dtype in (np.float32, np.float64) else np.float64
        return (torch.from_numpy(levels.astype(out_dtype)).to(pool.device),
                torch.from_numpy(bin_counts.astype(np.uint32).view(np.int32)).to(pool.device),
                torch.from_numpy(edges.copy()).to(pool.device), torch.from_numpy(centers.copy()).to(pool.device))
    return levels, bin_counts, edges, centers


# ---- the vectorscope of a voice pool (include/vnd_scope_voice_stream.h) -----------------------------------------------
VOICE_SPAN_FRAMES = _native.SCOPE_VOICE_SPAN_FRAMES   # frames of one slot per workgroup of the pool's bin kernel
_VOICE_CLEAR_BYTES = 16384                            # bytes of one grid row per workgroup of its clear kernel


def scope_voice_spans(positions, counts, flags, max_frames_per_call: Optional[int] = None):
    """``(valid, new_positions)`` of one call of a count-grid voice pool (``include/vnd_scope_voice_stream.h``), per slot,
    from the positions before the call, the frames pushed and the ``VOICE_START`` / ``VOICE_END`` flags alone - what the
    device computes from its own state::

        p = START ? 0 : position      valid = 1, or 0 for n = 0 without a flag      new position = END ? 0 : p + n

    A slot that answers 1 from ``p = 0`` has its grid row cleared first.  A count below 0 (or above
    ``max_frames_per_call``, when given), or without START a position outside ``[0, 2^60]``, answers -1 and leaves the
    position as it was."""
    return _valid_voice_spans(positions, counts, flags, max_frames_per_call)


def scope_voice_window(position_after: int, window_frames: Optional[int] = None):
    """``(lo, hi)``: the frames of a voice its grid row counts once the voice has pushed ``position_after`` frames (``p + n``
    of the call, before an END sets the position back to 0) - the last ``window_frames`` of them, or all of them for the
    whole-voice form (``None`` or 0)."""
    q = int(position_after)
    if q < 0:
        raise ValueError(f'position_after must be >= 0, not {position_after!r}')
    w = 0 if window_frames is None else int(window_frames)
    if w < 0:
        raise ValueError(f'window_frames must be >= 0 or None, not {window_frames!r}')
    return (max(0, q - w) if w else 0), q


def _window(window_frames, max_frames_per_call: int) -> int:
    """A pool's ``window_frames`` against its (checked) ``max_frames_per_call``, as an int."""
    _check_counts(window_frames=window_frames)
    if window_frames < max_frames_per_call:
        raise ValueError(f'window_frames {window_frames} below max_frames_per_call {max_frames_per_call}: two frames '
                         'of one call would share a ring entry')
    if window_frames > _INT32_MAX:
        raise ValueError(f'window_frames {window_frames} above 2**31 - 1')
    return int(window_frames)


def _fixed_scale(radius_scale, dtype: np.dtype) -> float:
    """A voice pool's ``radius_scale``: given, positive, and neither zero nor infinite in the pool's ``dtype``."""
    if radius_scale is None:
        raise ValueError('a voice pool needs a fixed radius_scale: the per-voice maximum of a later block would '
                         'rescale the earlier frames')
    scale = _scale(radius_scale, True)
    if not 0.0 < float(dtype.type(scale)) < np.inf:
        raise ValueError(f'radius_scale {radius_scale!r} is zero or infinite in {dtype.name}')
    return scale


class ScopeVoicePool(_MeterPool):
    """The vectorscope of ``slots`` voices, each with a life of its own (:func:`polar_histogram_voice_pool`,
    :func:`lissajous_histogram_voice_pool`; ``vnd_polar_hist_voice_stream_*_dev``, ``vnd_lissajous_hist_voice_stream_*_dev``):
    voices start and end on any call and push blocks of any size up to ``max_frames_per_call`` or none.  The position lives
    in the device state, one per slot, so a call is a pure function of device memory.  After every call row b of
    :attr:`grid` is the count grid of voice b - of its whole signal so far, or with ``window_frames=W`` of its last ``W``
    frames - equal to :func:`polar_histogram_batched` (``radius_scale=...``) / :func:`lissajous_histogram_batched` of those
    frames cell for cell, whatever the schedule: counts are integers, and the frame that leaves the window takes its count
    out of the cell it was put in.  A row is cleared when the slot's next voice begins; an END leaves it readable.

    :attr:`grid` is one int32 ``(slots, bins0, bins1)`` device tensor holding the uint32 counts, at a fixed address,
    allocated as zeros with the state: it belongs to the pool - read it, do not write it.

    Two forms; a pool is used through one of them (mixing them raises ``RuntimeError`` until ``reset()``):

    * ``process({slot: block}, start=[slot, ...], end=[slot, ...], discard=False, grids=True)`` - ``(n, 2)`` NumPy blocks of
      the pool's ``dtype`` in, ``{slot: float64 (bins0, bins1)}`` out for every slot that got a block, started or ended -
      the dtype :func:`polar_histogram_batched` gives NumPy callers.  One upload and one download (``transfers`` counts
      those of the last call); ``grids=False`` downloads ``valid`` only and answers ``{slot: None}``.  Every refusal comes
      before any device call.
    * ``process_dev(y, counts, flags)`` - ``y`` ``(slots, max_frames_per_call, 2)`` of the pool's ``dtype`` and int32
      ``(slots,)`` ``counts`` and ``flags`` on the device; returns ``(grid, valid)``.  It only enqueues on the current
      stream and can be captured with ``torch.cuda.graph`` after a ``reset()``.  To meter a decorrelating pool, build the
      meter with ``max_frames_per_call=pool.row_frames`` (and ``dtype='float64'`` for a Haas or chain pool) and hand it that
      pool's ``y`` and ``out_counts`` and the caller's ``flags``: a -1 of the pool is a bad count here and answers -1."""

    _out_dtype = np.float64

    def __init__(self, slots: int, *, max_frames_per_call: int, edges, polar: bool, window_frames: Optional[int] = None,
                 dtype='float32', radius_scale: Optional[float] = None, ms: bool = True, semicircular: bool = True):
        _MeterPool.__init__(self, slots, max_frames_per_call, dtype)
        self.window_frames = 0 if window_frames is None else _window(window_frames, max_frames_per_call)
        self.polar = bool(polar)
        self.radius_scale = _fixed_scale(radius_scale, self.dtype) if self.polar else None
        self.ms, self.semicircular = bool(ms), bool(semicircular)
        e0, e1 = (np.ascontiguousarray(e, np.float64) for e in edges)
        self.edges = (e0, e1)
        self.bins = (len(e0) - 1, len(e1) - 1)
        if not (1 <= self.bins[0] <= MAX_BINS and 1 <= self.bins[1] <= MAX_BINS):
            raise ValueError(f'{self.bins[0]} x {self.bins[1]} bins: 1 to {MAX_BINS} an axis')
        # the fixed grids of the pool's launches (include/vnd_scope_voice_stream.h): 2^23 workgroups each
        cells = self.bins[0] * self.bins[1]
        groups = max(-(-self.max_frames_per_call // VOICE_SPAN_FRAMES), -(-cells * 4 // _VOICE_CLEAR_BYTES))
        if self.slots * groups > _MAX_GROUPS:
            raise ValueError(f'{self.slots} slots of {groups} workgroups are more than one launch takes: split the pool')
        self._edges_dev = None
        S = self.slots
        self._inputs = (('y', (S, self.max_frames_per_call, 2), self.dtype.name, None),) + _slot_ints(S, 'counts', 'flags')
        self._outputs = (('grid', (S,) + self.bins, 'int32', 'zeros'), ('valid', (S,), 'int32', 'empty'))
        self._mirror()

    @property
    def grid(self):
        """The pool's count grids: int32 ``(slots, bins0, bins1)`` on the device, holding uint32; allocated, as zeros, with
        the state on first use."""
        if self._own is None:
            self._ensure_state(_torch(), _native.default_context())
        return self._own[1]

    def process(self, blocks=None, *, start=(), end=(), discard: bool = False, grids: bool = True):
        """One call of the dict form.  ``blocks``: ``{slot: (n, 2) array of the pool's dtype}``,
        ``0 <= n <= max_frames_per_call``; ``start``: the slots whose voice begins with this call; ``end``: the slots whose
        voice ends with it.  Returns ``{slot: float64 (bins0, bins1)}``, the grid of the voice (``grids=False``: ``None``,
        and only ``valid`` comes down), for every slot that got a block, started or ended.  Raises before any device call,
        as the other voice pools do: ``ValueError`` for a slot outside the pool or named twice, a block or an end for a
        slot that was never started, a start on a live slot (``discard=True`` allows it: the voice it held is dropped), a
        block above ``max_frames_per_call`` or not ``(n, 2)``; ``TypeError`` for a block of another dtype than the
        pool's."""
        row = (lambda counts: counts.view(np.uint32).astype(np.float64)) if grids else None
        return self._process_valid(blocks, start, end, discard, row, bool(grids))

    def process_dev(self, y, counts, flags, *, valid=None):
        """One call on device tensors, enqueued on the current stream: ``y`` ``(slots, M, 2)`` of the pool's dtype,
        ``counts`` / ``flags`` int32 ``(slots,)``.  Returns ``(grid, valid)``: the pool's own :attr:`grid` - the row of a
        slot that answered 1 is updated, no other - and int32 ``(slots,)``, the pool's own tensor at a fixed address
        unless ``valid=`` gives the caller's.  No check reads device memory; bad per-slot values answer -1
        (``include/vnd_scope_voice_stream.h``)."""
        return self._process_dev((y, counts, flags), valid=valid)

    # ---- the device -------------------------------------------------------------------------
    def _state_bytes(self, ctx) -> int:
        return _native.scope_voice_stream_state_bytes(self.slots, self.max_frames_per_call, self.window_frames)

    def _allocate(self, torch, ctx):
        _SlotPool._allocate(self, torch, ctx)
        device = torch.device('cuda', ctx.device)
        self._own = self._packed_outputs(torch, device, torch.zeros)      # the grid and valid, kept
        self._edges_dev = _device_edges(torch, device, *self.edges)

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        _native.scope_voice_stream_reset_device(ctx, state_ptr, state_bytes, self.slots, self.max_frames_per_call,
                                                self.window_frames, stream=stream)

    def _call_host(self, x, counts, flags, grids: bool = True):
        """One upload (the blocks and the two int32 arrays in one buffer), the call, one download (the grids and valid, or
        valid alone)."""
        return self._call_host_packed(x, (counts, flags), first=grids)

    def _launch(self, ctx, state_ptr, state_bytes, inputs, grid, valid, stream):
        y, counts, flags = inputs
        e0, e1 = self._edges_dev
        _native.scope_voice_stream_device(
            ctx, state_ptr, state_bytes, self.max_frames_per_call, self.window_frames, y.data_ptr(),
            y.data_ptr() + y.element_size(), 2 * self.max_frames_per_call, 2, counts.data_ptr(), flags.data_ptr(),
            e0.data_ptr(), self.bins[0], e1.data_ptr(), self.bins[1], grid.data_ptr(), valid.data_ptr(), self.slots,
            polar=self.polar, ms_mode=self.ms, semicircular=self.semicircular,
            radius_scale=self.radius_scale if self.polar else 0.0, float64=self.dtype == np.float64, stream=stream)


def polar_histogram_voice_pool(slots: int, *, max_frames_per_call: int, radius_scale, num_angle_bins: int = 240,
                               num_radius_bins: int = 150, window_frames: Optional[int] = None, dtype='float32',
                               mode=LayoutMode.MS, semicircular: bool = True) -> ScopeVoicePool:
    """A :class:`ScopeVoicePool` of polar grids: ``plot_polar_sample``'s heatmap counts for ``slots`` voices that start, end
    and push blocks on their own - of each voice's whole signal, or with ``window_frames`` of its last ``window_frames``
    frames (at least ``max_frames_per_call``).  ``radius_scale``, a positive number, is required: the per-voice maximum
    cannot stream.  Edges, ``mode`` and ``semicircular`` as in :func:`polar_histogram_batched`.  There is no ``frame_step``:
    the reference decimates only above 100 000 points, and a window of a second is below that."""
    bins0, bins1 = _bins(num_angle_bins, 'num_angle_bins'), _bins(num_radius_bins, 'num_radius_bins')
    return ScopeVoicePool(slots, max_frames_per_call=max_frames_per_call, edges=polar_edges(bins0, bins1), polar=True,
                          window_frames=window_frames, dtype=dtype, radius_scale=radius_scale, ms=_mode(mode),
                          semicircular=semicircular)


def lissajous_histogram_voice_pool(slots: int, *, max_frames_per_call: int, bins=512, range=((-1.1, 1.1), (-1.1, 1.1)),  # noqa: A002
                                   window_frames: Optional[int] = None, dtype='float32') -> ScopeVoicePool:
    """A :class:`ScopeVoicePool` of Lissajous grids: ``plot_lissajous(color_mode='density')``'s counts, L on the first
    axis, for ``slots`` voices - whole-voice, or over the last ``window_frames`` frames.  ``bins`` and ``range`` as in
    :func:`lissajous_histogram_batched`; there is no ``max_points``."""
    e0, e1 = lissajous_edges(bins, range)
    if len(e0) < 2 or len(e1) < 2 or not (np.all(np.diff(e0) > 0) and np.all(np.diff(e1) > 0)
                                          and np.all(np.isfinite(e0)) and np.all(np.isfinite(e1))):
        raise ValueError(f'bins {bins!r} and range {range!r} do not give ascending finite edges')
    return ScopeVoicePool(slots, max_frames_per_call=max_frames_per_call, edges=(e0, e1), polar=False,
                          window_frames=window_frames, dtype=dtype)


# ---- the level envelope of a voice pool (include/vnd_polar_level_voice_stream.h) -------------------------------------
class LevelVoicePool(_MeterPool):
    """The level envelope of ``slots`` voices, each with a life of its own (:func:`polar_level_voice_pool`;
    ``vnd_polar_level_voice_stream_*``): voices start and end on any call and push blocks of any size up to
    ``max_frames_per_call`` or none, by the slot rule of :class:`ScopeVoicePool` (:func:`scope_voice_spans`).  Percentiles of
    blocks do not add up, so the device state keeps the window: a ring per slot with the key (the radius's bit pattern) and
    the slice of each of the voice's last ``window_frames`` frames, and the radix select of :func:`polar_level_batched` runs
    over the ring as it lies - an order statistic does not depend on the order of its multiset.  Row b of :attr:`levels` is
    :func:`polar_level_batched` (``radius_scale=...``) of the frames :func:`scope_voice_window` names, bit for bit,
    whatever the schedule.  An END leaves the envelope readable; the slot's next voice drops it.

    :attr:`levels`, ``(slots, len(percentiles), num_bins)`` of the pool's dtype, and :attr:`bin_counts`, int32 ``(slots,
    num_bins)`` holding uint32, are device tensors at fixed addresses, allocated as zeros with the state: they belong to
    the pool - read them, do not write them.  :attr:`bin_edges` and :attr:`bin_centers` are :func:`level_edges`' arrays.

    Pushing and reading are two device entries: blocks arrive a hundred times a second, a display redraws thirty times.
    Two forms; a pool is used through one of them (mixing them raises ``RuntimeError`` until ``reset()``):

    * ``process({slot: block}, start=[slot, ...], end=[slot, ...], discard=False, levels=True)`` - ``(n, 2)`` NumPy blocks
      of the pool's ``dtype`` in, ``{slot: float64 (len(percentiles), num_bins)}`` out for every slot that got a block,
      started or ended - the dtype :func:`polar_level_batched` gives NumPy callers.  One upload and one download;
      ``levels=False`` pushes only, downloads ``valid`` alone and answers ``{slot: None}``.  Every refusal comes before any
      device call.
    * ``process_dev(y, counts, flags, levels=True)`` - ``y`` ``(slots, max_frames_per_call, 2)`` of the pool's ``dtype`` and
      int32 ``(slots,)`` ``counts`` and ``flags`` on the device; returns ``(levels, valid)``.  It only enqueues on the
      current stream and can be captured with ``torch.cuda.graph`` after a ``reset()``; ``levels=False`` pushes only, and
      ``read_dev()`` enqueues the levels entry alone.  To meter a decorrelating pool, build the meter with
      ``max_frames_per_call=pool.row_frames`` (and ``dtype='float64'`` for a Haas or chain pool) and hand it that pool's
      ``y`` and ``out_counts`` and the caller's ``flags``: a -1 of the pool is a bad count here and answers -1."""

    _out_dtype = np.float64

    def __init__(self, slots: int, *, max_frames_per_call: int, window_frames: int, radius_scale, num_bins: int = 360,
                 percentiles=(95.0, 50.0), dtype='float32', ms: bool = True, semicircular: bool = True):
        _MeterPool.__init__(self, slots, max_frames_per_call, dtype)
        self.window_frames = _window(window_frames, max_frames_per_call)
        self.radius_scale = _fixed_scale(radius_scale, self.dtype)
        self.num_bins = _bins(num_bins, 'num_bins')
        if self.num_bins > LEVEL_MAX_BINS:
            raise ValueError(f'num_bins {num_bins}: a level voice pool takes 1 to {LEVEL_MAX_BINS} slices')
        self.percentiles = tuple(_percentiles(percentiles))
        if len(self.percentiles) > LEVEL_MAX_PERCENTILES:
            raise ValueError(f'{len(self.percentiles)} percentiles: a level voice pool takes 1 to {LEVEL_MAX_PERCENTILES}')
        self.ms, self.semicircular = bool(ms), bool(semicircular)
        self.bin_edges, self.bin_centers = level_edges(self.num_bins)
        # the fixed grids of the pool's launches (include/vnd_polar_level_voice_stream.h): 2^23 workgroups each
        groups = max(-(-self.max_frames_per_call // VOICE_SPAN_FRAMES), -(-self.window_frames // LEVEL_SPAN_FRAMES))
        if self.slots * groups > _MAX_GROUPS:
            raise ValueError(f'{self.slots} slots of {groups} workgroups are more than one launch takes: split the pool')
        self._bin_counts = self._work = self._edges_dev = None
        self._with_levels = True
        S = self.slots
        self._inputs = (('y', (S, self.max_frames_per_call, 2), self.dtype.name, None),) + _slot_ints(S, 'counts', 'flags')
        self._outputs = (('levels', (S, len(self.percentiles), self.num_bins), self.dtype.name, 'zeros'),
                         ('valid', (S,), 'int32', 'empty'))
        self._mirror()

    @property
    def levels(self):
        """The pool's envelopes: ``(slots, len(percentiles), num_bins)`` of the pool's dtype on the device; allocated, as
        zeros, with the state on first use."""
        if self._own is None:
            self._ensure_state(_torch(), _native.default_context())
        return self._own[1]

    @property
    def bin_counts(self):
        """The frames per slice of every slot's window, as of the last levels call: int32 ``(slots, num_bins)`` on the
        device, holding uint32."""
        if self._bin_counts is None:
            self._ensure_state(_torch(), _native.default_context())
        return self._bin_counts

    def process(self, blocks=None, *, start=(), end=(), discard: bool = False, levels: bool = True):
        """One call of the dict form.  ``blocks``: ``{slot: (n, 2) array of the pool's dtype}``,
        ``0 <= n <= max_frames_per_call``; ``start``: the slots whose voice begins with this call; ``end``: the slots whose
        voice ends with it.  Returns ``{slot: float64 (len(percentiles), num_bins)}``, the envelope of the voice's window
        (``levels=False``: ``None``; the frames are pushed, nothing is selected and only ``valid`` comes down), for every
        slot that got a block, started or ended.  Raises before any device call, as :meth:`ScopeVoicePool.process`
        does."""
        row = (lambda values: values.astype(np.float64)) if levels else None
        return self._process_valid(blocks, start, end, discard, row, bool(levels))

    def process_dev(self, y, counts, flags, *, levels: bool = True, valid=None):
        """One call on device tensors, enqueued on the current stream: ``y`` ``(slots, M, 2)`` of the pool's dtype,
        ``counts`` / ``flags`` int32 ``(slots,)``.  The frames are pushed into the rings; with ``levels`` the envelopes of
        all slots are computed from the state behind the push.  Returns ``(levels, valid)``: the pool's own
        :attr:`levels` and int32 ``(slots,)``, the pool's own tensor at a fixed address unless ``valid=`` gives the
        caller's.  No check reads device memory; bad per-slot values answer -1
        (``include/vnd_polar_level_voice_stream.h``)."""
        self._with_levels = bool(levels)
        try:
            return self._process_dev((y, counts, flags), valid=valid)
        finally:
            self._with_levels = True

    def read_dev(self):
        """The levels entry alone, enqueued on the current stream: :attr:`levels` and :attr:`bin_counts` of every slot from
        the state as the pushes so far left it.  Returns :attr:`levels`."""
        torch = _torch()
        ctx = _native.default_context()
        state, state_bytes = self._ensure_state(torch, ctx)
        self._read(ctx, state.data_ptr(), state_bytes, self._own[1], torch.cuda.current_stream(state.device).cuda_stream)
        return self._own[1]

    # ---- the device -------------------------------------------------------------------------
    def _is64(self) -> bool:
        return self.dtype == np.float64

    def _state_bytes(self, ctx) -> int:
        return _native.level_voice_stream_state_bytes(self.slots, self.max_frames_per_call, self.window_frames, self._is64())

    def _allocate(self, torch, ctx):
        _SlotPool._allocate(self, torch, ctx)
        device = torch.device('cuda', ctx.device)
        self._own = self._packed_outputs(torch, device, torch.zeros)      # the levels and valid, kept
        self._bin_counts = torch.zeros((self.slots, self.num_bins), dtype=torch.int32, device=device)
        self._work_bytes = _native.level_voice_stream_work_bytes(self.slots, self.window_frames, self.num_bins,
                                                                 len(self.percentiles), self._is64())
        self._work = torch.empty(((self._work_bytes + 7) // 8,), dtype=torch.int64, device=device)
        self._edges_dev = _device_edges(torch, device, self.bin_edges, self.bin_centers)
        # one read of the fresh state: whatever the select sets up on its first launch happens here, not inside a capture
        state, state_bytes = self._state
        self._read(ctx, state.data_ptr(), state_bytes, self._own[1], torch.cuda.current_stream(device).cuda_stream)

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        _native.level_voice_stream_reset_device(ctx, state_ptr, state_bytes, self.slots, self.max_frames_per_call,
                                                self.window_frames, float64=self._is64(), stream=stream)

    def _call_host(self, x, counts, flags, levels: bool = True):
        """One upload (the blocks and the two int32 arrays in one buffer), the call, one download (the levels and valid,
        or valid alone)."""
        self._with_levels = levels
        try:
            return self._call_host_packed(x, (counts, flags), first=levels)
        finally:
            self._with_levels = True

    def _launch(self, ctx, state_ptr, state_bytes, inputs, levels, valid, stream):
        y, counts, flags = inputs
        _native.level_voice_stream_push_device(
            ctx, state_ptr, state_bytes, self.max_frames_per_call, self.window_frames, y.data_ptr(),
            y.data_ptr() + y.element_size(), 2 * self.max_frames_per_call, 2, counts.data_ptr(), flags.data_ptr(),
            self._edges_dev[0].data_ptr(), self.num_bins, valid.data_ptr(), self.slots, radius_scale=self.radius_scale,
            ms_mode=self.ms, semicircular=self.semicircular, float64=self._is64(), stream=stream)
        if self._with_levels:
            self._read(ctx, state_ptr, state_bytes, levels, stream)

    def _read(self, ctx, state_ptr, state_bytes, levels, stream):
        _native.level_voice_stream_levels_device(
            ctx, state_ptr, state_bytes, self.max_frames_per_call, self.window_frames, self.num_bins, self.percentiles,
            levels.data_ptr(), self._bin_counts.data_ptr(), self.slots, work_ptr=self._work.data_ptr(),
            work_bytes=self._work_bytes, float64=self._is64(), stream=stream)


def polar_level_voice_pool(slots: int, *, max_frames_per_call: int, window_frames: int, radius_scale, num_bins: int = 360,
                           percentiles=(95.0, 50.0), dtype='float32', mode=LayoutMode.MS,
                           semicircular: bool = True) -> LevelVoicePool:
    """A :class:`LevelVoicePool`: ``plot_polar_level``'s raw envelope - the ``percentiles`` of the radius in each of
    ``num_bins`` angular slices - over the last ``window_frames`` frames (at least ``max_frames_per_call``) of ``slots``
    voices that start, end and push blocks on their own.  ``radius_scale``, a positive number, is required: the per-voice
    maximum cannot stream.  Slices, ``percentiles``, ``mode`` and ``semicircular`` as in :func:`polar_level_batched`.
    There is no whole-voice form (its ring would be unbounded) and no host loop: another dtype, more than
    ``LEVEL_MAX_BINS`` slices or ``LEVEL_MAX_PERCENTILES`` percentiles raise ``ValueError`` here."""
    return LevelVoicePool(slots, max_frames_per_call=max_frames_per_call, window_frames=window_frames,
                          radius_scale=radius_scale, num_bins=num_bins, percentiles=percentiles, dtype=dtype, ms=_mode(mode),
                          semicircular=semicircular)


__all__ = ['polar_coordinates_batched', 'polar_histogram_batched', 'lissajous_histogram_batched', 'polar_level_batched',
           'ScopeVoicePool', 'polar_histogram_voice_pool', 'lissajous_histogram_voice_pool', 'scope_voice_spans',
           'scope_voice_window', 'VOICE_SPAN_FRAMES', 'LevelVoicePool', 'polar_level_voice_pool',
           'set_scope_device', 'scope_covers', 'level_covers', 'histogram_bins', 'histogram_counts', 'polar_edges',
           'lissajous_edges', 'lissajous_step', 'level_edges', 'percentile_rule', 'percentile_of_sorted', 'SPAN_FRAMES',
           'DIRECT_SPAN_FRAMES', 'MAX_BINS', 'ROUTE_LDS', 'ROUTE_DIRECT', 'LEVEL_MAX_BINS', 'LEVEL_MAX_PERCENTILES',
           'LEVEL_SPAN_FRAMES']
