"""Parameter search of the reference's ``vndecorrelate.optimization``.

Same functions, keyword arguments and return values as
``src/vndecorrelate/optimization.py``: a scalar objective built from the
amplitude-weighted angular moments of a decorrelated signal's polar samples
(:46-105), a grid scan over candidate decorrelators (:107-117), local minima of the
scan (:120-128) refined with SciPy's bounded scalar minimiser (:131-157), and the two
drivers ``optimize_velvet_noise`` (:230-310) and ``optimize_haas_delay`` (:160-227).

What moves to the GPU is the scan.  The reference decorrelates and scores the F
candidates one after the other; here the candidates' tap tables are concatenated into
one bank, the signal is uploaded once, ONE fan-out launch convolves all of them and a
reduction kernel turns the result into eight moments per candidate
(``vnd_scan_bank_f32_host``), so F x 64 bytes come back instead of F signals.  That
covers candidates that are plain velvet-noise convolutions - ``VelvetNoise`` in LR
mode without width or normaliser, which is what ``optimize_velvet_noise`` builds
(:259-271).  ``HaasEffect`` candidates - what ``optimize_haas_delay`` builds (:186-193) -
go to their own kernel (``vnd_haas_scan_f64_host``, :func:`scan_haas_moments`): one
upload, and the float64 moments of every delay from one sweep that never writes a
delayed signal.  Anything else (MS encode, width, normalisers) is scored on the host
from its ``decorrelate`` output exactly as upstream.  A single
``symmetry_aware_objective`` call always takes the host route, so its value is
bit-identical to the reference's given the bit-identical exact-mode convolution;
scanned velvet-noise scores agree to ~1e-7 relative (float64 sums where NumPy adds
float32), scanned Haas scores to ~1e-12 (both float64; sum order and atan2 ulps differ).
``optimize_haas_delay``'s refinement memoises its host objective by the integer delay,
on which alone it depends.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
from numpy.typing import NDArray

from . import _native
from . import decorrelation as _dec
from .decorrelation import Decorrelator, HaasEffect, VelvetNoise
from .taps import class_path_bank_arrays
from .utils.dsp import EPSILON, LayoutMode, polar_coordinates, to_float32

# one bank's device output is n * 2F floats: keep it under this many bytes per launch
_SCAN_BYTES = 2 << 30
# the Haas scan's workspace is ceil((n + max d) / 2048) * F * 64 bytes: keep it under this many bytes per launch
_HAAS_SCAN_BYTES = 1 << 30
_HAAS_SCAN_MAX_DELAYS = 1048560                      # VND_HAAS_SCAN_MAX_DELAYS: delays per launch
_INT32_MAX = 2 ** 31 - 1

_haas_scan_device: Optional[bool] = None


def set_haas_scan_device(enabled: Optional[bool]) -> None:
    """Where :func:`grid_scan` scores ``HaasEffect`` candidates.

    ``None`` (default): on the GPU when a gfx950 device is present and the input is covered
    (:func:`haas_scan_covers`), otherwise one by one on the host.  ``True``: the device for every covered input;
    such a call raises ``RuntimeError`` when there is no device.  ``False``: always the host, bit-identical to the
    reference."""
    global _haas_scan_device
    if enabled is not None and not isinstance(enabled, (bool, np.bool_)):
        raise TypeError(f'set_haas_scan_device takes True, False or None, not {enabled!r}')
    _haas_scan_device = None if enabled is None else bool(enabled)


# ---- the objective's terms (optimization.py:11-44) -----------------------------------
def left_right_correlation(stereo_signal: NDArray) -> float:
    """Dot product of the channels, both scaled by the LEFT channel's norm (as upstream, :14-17)."""
    left_norm = np.linalg.norm(stereo_signal[:, 0]) + EPSILON
    return np.dot(stereo_signal[:, 0] / left_norm, stereo_signal[:, 1] / left_norm)


def angular_variance(thetas: NDArray, weights: NDArray) -> float:
    return float(np.sum(weights * thetas**2))


def centroid(thetas: NDArray, weights: NDArray) -> float:
    return float(np.sum(weights * thetas))


def polar_skewness(thetas: NDArray, weights: NDArray, angular_variance: float) -> float:
    return float(np.sum(weights * thetas**3)) / (max(angular_variance, EPSILON) ** 1.5)


def max_angular_exceedance(thetas: NDArray, angle_limit: float) -> float:
    return max(0.0, float(np.max(np.abs(thetas)) - angle_limit))


def _combine(spread: float, mean_theta: float, skew: float, correlation: float, exceedance: float, *,
             lambda_mean: float, lambda_skew: float, lambda_correlation: float, lambda_penalty: float) -> float:
    """optimization.py:79-105: maximise spread, penalise the rest; minimiser convention."""
    objective = (spread
                 - lambda_mean * mean_theta ** 2
                 - lambda_skew * skew ** 2
                 - lambda_correlation * correlation ** 2
                 - lambda_penalty * exceedance ** 2)
    return -objective


def symmetry_aware_objective(input_signal: NDArray, decorrelator: Decorrelator, *, angle_limit: float,
                             lambda_mean: float, lambda_skew: float, lambda_correlation: float,
                             lambda_penalty: float) -> float:
    """Score of one decorrelator on one signal (optimization.py:46-105); lower is better."""
    output_signal = decorrelator.decorrelate(input_signal)
    _, thetas, weights = polar_coordinates(output_signal[:, 0], output_signal[:, 1], normalize=False)
    spread = angular_variance(thetas, weights)
    return _combine(spread, centroid(thetas, weights), polar_skewness(thetas, weights, spread),
                    left_right_correlation(output_signal), max_angular_exceedance(thetas, angle_limit),
                    lambda_mean=lambda_mean, lambda_skew=lambda_skew, lambda_correlation=lambda_correlation,
                    lambda_penalty=lambda_penalty)


# ---- the scan -------------------------------------------------------------------------
def _scannable(decorrelator) -> bool:
    """A candidate whose ``decorrelate`` is the bare convolution of a stereo pair."""
    return (isinstance(decorrelator, VelvetNoise) and decorrelator.num_outs == 2
            and decorrelator.mode == LayoutMode.LR and decorrelator.width is None
            and not decorrelator.normalizer)


def score_from_moments(moments: NDArray, *, angle_limit: float, lambda_mean: float, lambda_skew: float,
                       lambda_correlation: float, lambda_penalty: float) -> float:
    """The objective from one row of device moments
    ``{sum r, sum r*t, sum r*t^2, sum r*t^3, max|t|, sum L*R, sum L^2, sum R^2}``."""
    s0, s1, s2, s3, tmax, lr, ll, _ = (float(v) for v in moments)
    total = s0 + EPSILON                                 # weights = radii / (radii.sum() + EPSILON)
    spread = s2 / total
    skew = (s3 / total) / (max(spread, EPSILON) ** 1.5)
    correlation = lr / (np.sqrt(ll) + EPSILON) ** 2
    return _combine(spread, s1 / total, skew, correlation, max(0.0, tmax - angle_limit),
                    lambda_mean=lambda_mean, lambda_skew=lambda_skew, lambda_correlation=lambda_correlation,
                    lambda_penalty=lambda_penalty)


def scores_from_moments(moments: NDArray, *, angle_limit: float, lambda_mean: float, lambda_skew: float,
                        lambda_correlation: float, lambda_penalty: float) -> NDArray:
    """:func:`score_from_moments` for all rows of an ``(F, 8)`` moments matrix at once: the same float64
    operations element by element, without F trips through the interpreter (NumPy's array ``**`` and
    Python's float ``**`` may differ in the last bit: 6e-16 relative on the scores)."""
    m = np.asarray(moments, np.float64)
    s0, s1, s2, s3, tmax, lr, ll = (m[:, k] for k in range(7))
    total = s0 + EPSILON
    spread = s2 / total
    skew = (s3 / total) / (np.maximum(spread, EPSILON) ** 1.5)
    correlation = lr / (np.sqrt(ll) + EPSILON) ** 2
    exceedance = np.maximum(0.0, tmax - angle_limit)
    objective = (spread - lambda_mean * (s1 / total) ** 2 - lambda_skew * skew ** 2
                 - lambda_correlation * correlation ** 2 - lambda_penalty * exceedance ** 2)
    return -objective


def scan_moments(input_signal: NDArray, decorrelators: Sequence[VelvetNoise], *,
                 mode: Optional[int] = None) -> NDArray:
    """``(F, 8)`` float64 device moments of ``d.decorrelate(input_signal)`` for scannable
    candidates: one upload, one fan-out convolution per sub-bank, only the moments return."""
    x = to_float32(np.asarray(input_signal))
    if x.ndim == 1:
        x = x[:, None]                                   # the device fans the one channel out (mono_to_stereo)
    elif x.ndim != 2 or x.shape[1] < 2:
        raise ValueError(f'expected a mono (n,) or stereo (n, 2) signal, got shape {x.shape}')
    else:
        x = x[:, :2]
    x = np.ascontiguousarray(x, dtype=np.float32)
    frames = max(x.shape[0], 1)
    per_launch = max(1, _SCAN_BYTES // (frames * 8))
    mode = _dec._default_mode if mode is None else mode
    rows: List[NDArray] = []
    for first in range(0, len(decorrelators), per_launch):
        arrays = class_path_bank_arrays([d._tap_member() for d in decorrelators[first:first + per_launch]])
        table = _native.TapTable.create(_native.default_context(), arrays.tap_offsets, arrays.tap_index,
                                        arrays.tap_weight, **arrays.kwargs())
        try:
            rows.append(table.scan_host(x, mode))
        finally:
            table.close()
    return np.concatenate(rows) if rows else np.zeros((0, _native.MOMENTS))


def haas_scan_covers(input_signal, decorrelator=None) -> bool:
    """Whether the Haas kernel covers this input (and candidate): a mono ``(n,)`` or stereo ``(n, 2)`` array with
    n > 0, and - for a candidate - a plain ``HaasEffect`` in LR or MS layout with delayed channel 0 or 1, a delay
    ``round(delay_time_seconds * sample_rate_hz)`` in [0, 2^31) and a width that is None or a Python / float64
    number (a float32 width would make NumPy's ``1.0 - width`` float32).  Everything else keeps the host path and its
    exceptions, e.g. ``(n, 3)`` input."""
    shape = np.shape(input_signal)
    if not (len(shape) == 1 or (len(shape) == 2 and shape[1] == 2)) or shape[0] == 0:
        return False
    if decorrelator is None:
        return True
    return _haas_key(decorrelator) is not None and _haas_delay(decorrelator) is not None


def _haas_key(d) -> Optional[Tuple[int, bool, Optional[float]]]:
    """``(delayed_channel, MS?, width)`` of a covered HaasEffect candidate, else None."""
    if type(d) is not HaasEffect or type(d.delayed_channel) not in (int, np.int64) or d.delayed_channel not in (0, 1):
        return None
    if d.mode not in (LayoutMode.LR, LayoutMode.MS):
        return None
    w = d.width
    if w is not None and (type(w) not in (int, float, np.float64) or not np.isfinite(w)):
        return None
    return int(d.delayed_channel), d.mode == LayoutMode.MS, None if w is None else float(w)


def _haas_delay(d) -> Optional[int]:
    """The delay in frames, as ``HaasEffect.haas_delay`` computes it (decorrelation.py:201), if covered."""
    try:
        delay = round(d.delay_time_seconds * d.sample_rate_hz)
    except (TypeError, ValueError, OverflowError):
        return None
    if not isinstance(delay, (int, np.integer)) or not 0 <= delay <= _INT32_MAX:
        return None
    return int(delay)


def _haas_route(input_signal) -> bool:
    """The routing decision of one :func:`grid_scan` call's HaasEffect candidates."""
    if _haas_scan_device is False or not haas_scan_covers(input_signal):
        return False
    from .analysis import _gpu_present
    if _haas_scan_device is True:
        if not _gpu_present():
            raise RuntimeError('set_haas_scan_device(True): no gfx950 device (or no built extension) to run on')
        return True
    return _gpu_present()


def _haas_groups(decorrelators: Sequence) -> Dict[Tuple, Tuple[List[int], NDArray, NDArray]]:
    """Covered HaasEffect candidates grouped by configuration: ``key -> (candidate indices, unique delays ascending,
    index of each candidate's delay in the unique ones)``.  Duplicate delays (``linspace`` + ``round`` makes many on
    fine grids) are scanned once."""
    members: Dict[Tuple, Tuple[List[int], List[int]]] = {}
    for i, d in enumerate(decorrelators):
        key = _haas_key(d)
        delay = None if key is None else _haas_delay(d)
        if delay is None:
            continue
        idx, delays = members.setdefault(key, ([], []))
        idx.append(i)
        delays.append(delay)
    groups = {}
    for key, (idx, delays) in members.items():
        unique, inverse = np.unique(np.asarray(delays, np.int64), return_inverse=True)
        groups[key] = (idx, unique, inverse.reshape(-1))
    return groups


def scan_haas_moments(input_signal: NDArray, decorrelators: Sequence[HaasEffect]) -> NDArray:
    """``(F, 8)`` float64 device moments of ``d.decorrelate(input_signal)`` for covered ``HaasEffect`` candidates
    (:func:`haas_scan_covers`), in candidate order: one kernel per configuration over its distinct delays."""
    if not haas_scan_covers(input_signal):
        raise ValueError(f'expected a mono (n,) or stereo (n, 2) signal with n > 0, got shape {np.shape(input_signal)}')
    decorrelators = list(decorrelators)
    groups = _haas_groups(decorrelators)
    if sum(len(idx) for idx, _, _ in groups.values()) != len(decorrelators):
        raise ValueError('scan_haas_moments takes HaasEffect candidates the device covers (see haas_scan_covers)')
    x = to_float32(np.asarray(input_signal))
    x = np.ascontiguousarray(x.reshape(x.shape[0], -1), dtype=np.float32)
    ctx = _native.default_context()
    out = np.empty((len(decorrelators), _native.MOMENTS), np.float64)
    for (channel, ms, width), (idx, unique, inverse) in groups.items():
        rows: List[NDArray] = []
        first = 0
        while first < unique.size:                       # launches bounded by their workspace (delays ascending)
            last = first + 1
            while (last < unique.size and last - first < _HAAS_SCAN_MAX_DELAYS and _native.haas_scan_workspace_bytes(
                    x.shape[0], last + 1 - first, int(unique[last])) <= _HAAS_SCAN_BYTES):
                last += 1
            rows.append(_native.haas_scan_host(ctx, x, unique[first:last], delayed_channel=channel, ms_mode=ms,
                                               width=width))
            first = last
        out[idx] = np.concatenate(rows)[inverse]
    return out


def grid_scan(input_signal: NDArray, decorrelators: Sequence[Decorrelator], **kwargs) -> NDArray:
    """Scores of every candidate (optimization.py:107-117).  Velvet-noise candidates without an
    epilogue and HaasEffect candidates are scored on the device, each kind in one pass; the rest
    one by one on the host."""
    print('Starting Grid Scan')
    decorrelators = list(decorrelators)
    scores = np.empty(len(decorrelators), np.float64)
    on_device = [i for i, d in enumerate(decorrelators) if _scannable(d)]
    if on_device and np.asarray(input_signal).shape[0] > 0:
        moments = scan_moments(input_signal, [decorrelators[i] for i in on_device])
        scores[on_device] = scores_from_moments(moments, **kwargs)
    else:
        on_device = []
    haas = [i for i, d in enumerate(decorrelators) if haas_scan_covers(input_signal, d)]
    if haas and _haas_route(input_signal):
        moments = scan_haas_moments(input_signal, [decorrelators[i] for i in haas])
        scores[haas] = scores_from_moments(moments, **kwargs)
        on_device += haas
    for i in sorted(set(range(len(decorrelators))) - set(on_device)):
        scores[i] = symmetry_aware_objective(input_signal, decorrelators[i], **kwargs)
    return scores


def get_local_minima(scores: NDArray, grid_size: int) -> List[int]:
    """Interior grid points lower than both neighbours, else the global minimum (:120-128)."""
    inner = [i for i in range(1, grid_size - 1) if scores[i - 1] > scores[i] < scores[i + 1]]
    return inner if inner else [int(np.argmin(scores))]


def optimize_local_minima(local_minima: List[int], scalars: NDArray, grid_size: int,
                          scalar_objective: Callable[[float], float]):
    """Bounded scalar minimisation between the neighbours of each local minimum (:131-157)."""
    from scipy.optimize import minimize_scalar
    best_scalar, best_score = 0.0, np.inf
    print('Starting Local Minima optimization')
    for i in local_minima:
        bounds = (scalars[max(0, i - 1)], scalars[min(grid_size - 1, i + 1)])
        result = minimize_scalar(fun=scalar_objective, bounds=bounds, method='bounded', options={'xatol': 1e-4})
        if result.fun < best_score:
            best_score, best_scalar = result.fun, result.x
    return best_scalar


def _search(input_signal: NDArray, scalars: NDArray, make: Callable[[float], Decorrelator], grid_size: int,
            weights: dict, objective: Optional[Callable[[float], float]] = None):
    scores = grid_scan(input_signal, [make(value) for value in scalars], **weights)
    if objective is None:
        def objective(value):
            return symmetry_aware_objective(input_signal, make(value), **weights)
    return optimize_local_minima(get_local_minima(scores, grid_size), scalars, grid_size, objective)


class DelayMemo:
    """A τ objective of a ``HaasEffect`` memoised by the integer delay ``round(τ * fs)``: the candidate's output, and so
    its score, depends on τ through that integer alone (decorrelation.py:201).  The values, and the minimiser's path
    through them, are the un-memoised objective's; only repeated host evaluations are saved (``calls`` vs ``evaluations``)."""

    def __init__(self, objective: Callable[[float], float], sample_rate_hz):
        self.objective = objective
        self.sample_rate_hz = sample_rate_hz
        self.values: Dict[int, float] = {}
        self.calls = 0

    @property
    def evaluations(self) -> int:
        return len(self.values)

    def __call__(self, tau: float) -> float:
        self.calls += 1
        key = round(tau * self.sample_rate_hz)
        if key not in self.values:
            self.values[key] = self.objective(tau)
        return self.values[key]


last_haas_memo: Optional[DelayMemo] = None      # the last optimize_haas_delay call's refinement memo (tools, tests)


def optimize_haas_delay(*, input_signal: NDArray, sample_rate_hz: int, max_delay_seconds: int,
                        grid_size: int = 400, angle_limit: float = np.pi / 4, lambda_mean: float = 5.0,
                        lambda_skew: float = 2.0, lambda_correlation: float = 15.0,
                        lambda_penalty: float = 1e3) -> float:
    """Best ``delay_time_seconds`` in ``[0, max_delay_seconds]`` for an LR ``HaasEffect`` (:160-227).
    The grid is scored on the device where :func:`grid_scan` routes it; the refinement's host objective is
    memoised by the integer delay (:class:`DelayMemo`)."""
    global last_haas_memo
    weights = dict(angle_limit=angle_limit, lambda_mean=lambda_mean, lambda_skew=lambda_skew,
                   lambda_correlation=lambda_correlation, lambda_penalty=lambda_penalty)

    def make(tau: float) -> HaasEffect:
        return HaasEffect(sample_rate_hz=sample_rate_hz, delay_time_seconds=tau, mode='LR')

    memo = DelayMemo(lambda tau: symmetry_aware_objective(input_signal, make(tau), **weights), sample_rate_hz)
    last_haas_memo = memo
    return _search(input_signal, np.linspace(0.0, max_delay_seconds, grid_size), make, grid_size, weights, memo)


def optimize_velvet_noise(*, input_signal: NDArray, sample_rate_hz: int, duration_seconds: float,
                          num_impulses: int, seed: int = 1, grid_size: int = 400,
                          angle_limit: float = np.pi / 4, lambda_mean: float = 5.0, lambda_skew: float = 2.0,
                          lambda_correlation: float = 15.0, lambda_penalty: float = 1e3) -> float:
    """Best ``log_distribution_strength`` in ``[0, 1]`` for a one-sided LR ``VelvetNoise`` (:230-310)."""
    weights = dict(angle_limit=angle_limit, lambda_mean=lambda_mean, lambda_skew=lambda_skew,
                   lambda_correlation=lambda_correlation, lambda_penalty=lambda_penalty)

    def make(kappa: float) -> VelvetNoise:
        return VelvetNoise(sample_rate_hz=sample_rate_hz, duration_seconds=duration_seconds,
                           num_impulses=num_impulses, log_distribution_strength=kappa, normalizer=None,
                           filtered_channels=(0,), mode='LR', seed=seed)

    return _search(input_signal, np.linspace(0.0, 1.0, grid_size), make, grid_size, weights)
