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
on which alone it depends.  ``optimize_haas_delay_batched`` runs the whole search, refinement
included, for a pool of signals on the device: one launch over (signal, delay) pairs for the
grid and one per round of a lockstep bounded minimiser (``bounded.py``) for the refinements.
``optimize_velvet_noise_batched`` does the same for ``optimize_velvet_noise``: one launch over (signal, distinct table)
pairs for the kappa grid and one bank and one launch per refinement round (``vnd_velvet_pairs_f32_dev``).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
from numpy.typing import NDArray

from . import _native, analysis
from . import _native_haas_scan_voice as _scan_native
from . import decorrelation as _dec
from .bounded import minimize_bounded_lockstep, round_half_even
from .decorrelation import Decorrelator, HaasEffect, VelvetNoise
from .streaming import VOICE_START, _check_device_tensors, _MeterPool, _slot_ints, _SlotPool, _valid_voice_spans
from .taps import TapArrays, class_path_bank_arrays
from .utils.dsp import EPSILON, LayoutMode, polar_coordinates, to_float32

# one bank's device output is n * 2F floats: keep it under this many bytes per launch
_SCAN_BYTES = 2 << 30
# the Haas scan's workspace is ceil((n + max d) / 2048) * F * 64 bytes: keep it under this many bytes per launch
_HAAS_SCAN_BYTES = 1 << 30
_HAAS_SCAN_MAX_DELAYS = 1048560                      # VND_HAAS_SCAN_MAX_DELAYS: delays per launch
# optimize_haas_delay_batched keeps at most this many bytes of its float32 pool on the device (else chunks of signals)
_HAAS_POOL_BYTES = 4 << 30
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


def _haas_route(covered: bool = True) -> bool:
    """The routing decision of one :func:`grid_scan` call's HaasEffect candidates (``covered``:
    :func:`haas_scan_covers` of its input), or of one :func:`optimize_haas_delay_batched` call."""
    return analysis.device_route(_haas_scan_device, covered,
                                 'set_haas_scan_device(True): no gfx950 device (or no built extension) to run on')


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
    if haas and _haas_route(haas_scan_covers(input_signal)):
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


# ---- the batched Haas-delay optimiser -------------------------------------------------------------------------------
@dataclass
class HaasSearchStats:
    """The work of one :func:`optimize_haas_delay_batched` call (tools, tests).  ``rounds`` counts the lockstep
    refinement's rounds, the first points of every minimum included; ``pairs_per_round`` the distinct (signal, delay)
    pairs each round scored in one launch; ``grid_pairs`` those of the grid; ``evaluations[b]`` the objective
    evaluations of signal b's refinements (SciPy's ``nfev`` summed over its local minima); ``minimum_signal`` and
    ``minimum_nfev`` the signal and ``nfev`` of each refined minimum in order (device route); ``pool_uploads`` how many
    chunks of the pool went to the device (0 for a device tensor and on the host route)."""
    route: str
    signals: int
    rounds: int = 0
    pairs_per_round: List[int] = field(default_factory=list)
    grid_pairs: int = 0
    evaluations: NDArray = field(default_factory=lambda: np.zeros(0, np.int64))
    minimum_signal: NDArray = field(default_factory=lambda: np.zeros(0, np.int64))
    minimum_nfev: NDArray = field(default_factory=lambda: np.zeros(0, np.int64))
    pool_uploads: int = 0


last_haas_search: Optional[HaasSearchStats] = None   # the last optimize_haas_delay_batched call's work


def haas_delays(taus, sample_rate_hz) -> NDArray[np.int64]:
    """``round(tau * sample_rate_hz)`` of each tau, as ``HaasEffect.haas_delay`` rounds it (ties to even)."""
    return round_half_even(np.asarray(taus, np.float64) * sample_rate_hz)


def haas_search(score_pairs: Callable[[NDArray, NDArray], NDArray], num_signals: int, taus: NDArray,
                sample_rate_hz, grid_size: int, stats: Optional[HaasSearchStats] = None) -> NDArray[np.float64]:
    """``optimize_haas_delay``'s search for ``num_signals`` signals at once, given a scorer.

    ``score_pairs(signals, delays)`` returns the objective of ``HaasEffect(delay).decorrelate(signal)`` for distinct
    (signal, integer delay) pairs sorted by (signal, delay).  The grid is one call over every signal and distinct grid
    delay; each refinement round is one call over the distinct pairs its lanes ask for.  Per signal: the grid's local
    minima (:func:`get_local_minima`), each refined over its neighbours by :func:`minimize_bounded_lockstep` (SciPy's
    bounded method, ``xatol=1e-4``) on ``f(tau) = score of round(tau * fs)``, and :func:`optimize_local_minima`'s
    choice among them."""
    taus = np.asarray(taus, np.float64)
    stats = HaasSearchStats(route='custom', signals=num_signals) if stats is None else stats

    def delays_of(values):
        delays = haas_delays(values, sample_rate_hz)
        if delays.size and (delays.min() < 0 or delays.max() > _INT32_MAX):
            raise ValueError(f'Haas delays must lie in [0, 2^31): got {int(delays.min())}..{int(delays.max())}')
        return delays

    def score(signals, delays):
        return np.asarray(score_pairs(signals, delays), np.float64)

    unique, inverse = np.unique(delays_of(taus), return_inverse=True)
    grid = score(np.repeat(np.arange(num_signals, dtype=np.int64), unique.size), np.tile(unique, num_signals))
    scores = grid.reshape(num_signals, unique.size)[:, inverse.reshape(-1)]
    stats.grid_pairs += num_signals * unique.size
    lane_signal, lower, upper = [], [], []
    for b in range(num_signals):
        for i in get_local_minima(scores[b], grid_size):
            lane_signal.append(b)
            lower.append(taus[max(0, i - 1)])
            upper.append(taus[min(grid_size - 1, i + 1)])
    lane_signal = np.asarray(lane_signal, np.int64)

    def objective(lanes, x):
        key = (lane_signal[lanes] << 32) | delays_of(x)
        pairs, back = np.unique(key, return_inverse=True)
        stats.pairs_per_round.append(int(pairs.size))
        return score(pairs >> 32, pairs & 0xFFFFFFFF)[back.reshape(-1)]

    result = minimize_bounded_lockstep(objective, lower, upper, xatol=1e-4)
    stats.rounds += result.rounds
    best_tau, best_score = np.zeros(num_signals), np.full(num_signals, np.inf)
    evaluations = np.zeros(num_signals, np.int64)
    for lane, b in enumerate(lane_signal):               # minima in order, strict <, from (0.0, inf)
        evaluations[b] += result.nfev[lane]
        if result.fun[lane] < best_score[b]:
            best_score[b], best_tau[b] = result.fun[lane], result.x[lane]
    stats.minimum_signal = np.concatenate([stats.minimum_signal, lane_signal + stats.evaluations.size])
    stats.minimum_nfev = np.concatenate([stats.minimum_nfev, result.nfev])
    stats.evaluations = np.concatenate([stats.evaluations, evaluations])
    return best_tau


def host_pair_scorer(pool, sample_rate_hz, weights: dict) -> Callable[[NDArray, NDArray], NDArray]:
    """A :func:`haas_search` scorer on the host: ``symmetry_aware_objective`` of an LR ``HaasEffect`` per pair."""
    def score(signals, delays):
        return np.array([symmetry_aware_objective(pool[s], HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d),
                                                                      mode='LR'), **weights)
                         for s, d in zip(signals.tolist(), delays.tolist())], np.float64)
    return score


class _DevicePairScorer:
    """A :func:`haas_search` scorer over a float32 ``(B, n, C)`` pool resident on the device: one
    ``vnd_haas_pairs_f64_dev`` launch per call (more only past the workspace budget); pairs go up, moments come
    down, and ``scores_from_moments`` turns them into scores."""

    def __init__(self, ctx, pool, weights: dict):
        self.ctx, self.pool, self.weights = ctx, pool, weights
        import torch
        self.torch = torch
        self.batch, self.n, self.channels = (int(v) for v in pool.shape)
        self.workspace = None

    def _launch(self, signals, delays):
        torch = self.torch
        dev = self.pool.device
        count = int(delays.size)
        ws = _native.haas_pairs_workspace_bytes(self.n, count, int(delays.max()))
        if self.workspace is None or self.workspace.numel() < ws:
            self.workspace = torch.empty(max(ws, 1), dtype=torch.uint8, device=dev)
        pairs = torch.from_numpy(np.stack([signals, delays]).astype(np.int32)).to(dev)
        moments = torch.empty((count, _native.MOMENTS), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev)
        _native.haas_pairs_device(self.ctx, self.pool.data_ptr(), self.batch, self.n, self.channels,
                                  pairs[0].data_ptr(), pairs[1].data_ptr(), count, moments.data_ptr(),
                                  delayed_channel=0, ms_mode=False, width=None,
                                  workspace_ptr=self.workspace.data_ptr(), workspace_bytes=ws,
                                  stream=stream.cuda_stream)
        return moments.cpu().numpy()

    def __call__(self, signals, delays):
        rows: List[NDArray] = []
        first = 0
        chunks = (self.n + delays + 2047) // 2048           # the workspace's partials per pair (vnd_haas_scan.hpp)
        while first < delays.size:                          # launches bounded by their workspace
            need = np.maximum.accumulate(chunks[first:]) * np.arange(1, delays.size - first + 1) * 64
            last = first + min(max(1, int(np.count_nonzero(need <= _HAAS_SCAN_BYTES))), _native.HAAS_PAIRS_MAX)
            rows.append(self._launch(signals[first:last], delays[first:last]))
            first = last
        moments = np.concatenate(rows) if rows else np.zeros((0, _native.MOMENTS))
        return scores_from_moments(moments, **self.weights)


def _haas_pool(input_signals):
    """``(pool, is_torch)``: the pool as ``(B, n, C)`` with C = 1 (mono) or 2, after the shape checks."""
    is_torch = _native.is_torch(input_signals)
    x = input_signals if is_torch else np.asarray(input_signals)
    shape = tuple(x.shape)
    if not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 2)):
        raise ValueError(f'expected a stereo pool (B, n, 2) or a mono pool (B, n), got shape {shape}')
    if shape[0] > 0 and shape[1] == 0:
        raise ValueError(f'the signals of a pool need n > 0 frames, got shape {shape}')
    if is_torch:
        import torch
        if x.is_complex() or x.dtype == torch.bool:
            raise TypeError(f'signals must be real numbers, got {x.dtype}')
    elif x.dtype.kind not in 'biuf':
        raise TypeError(f'signals must be real numbers, got {x.dtype}')
    return x, is_torch


def optimize_haas_delay_batched(*, input_signals, sample_rate_hz: int, max_delay_seconds, grid_size: int = 400,
                                angle_limit: float = np.pi / 4, lambda_mean: float = 5.0, lambda_skew: float = 2.0,
                                lambda_correlation: float = 15.0, lambda_penalty: float = 1e3) -> NDArray[np.float64]:
    """:func:`optimize_haas_delay` for every signal of a pool: ``(B,)`` float64 delays in seconds.

    ``input_signals`` is a stereo pool ``(B, n, 2)`` or a mono pool ``(B, n)`` with n > 0: a NumPy array of any real
    dtype (cast as ``to_float32`` casts it) or a CUDA torch tensor, read in place.  B = 0 gives an empty array.

    Device route (:func:`set_haas_scan_device`: ``None`` with a gfx950 device, or ``True``): the pool goes up once
    (in chunks of whole signals past ``_HAAS_POOL_BYTES``) and stays there.  The grid is one launch over every
    (signal, distinct grid delay) pair; the local minima of every signal are then refined together by
    :func:`minimize_bounded_lockstep`, one launch per round over the distinct (signal, delay) pairs the round needs.
    Only pairs go up and moments come down (:func:`haas_search`, ``vnd_haas_pairs_f64_dev``).
    Parity: the grid scores equal ``grid_scan(x_b, candidates)`` on the device route bit for bit, so the local minima
    are the same; the refinement takes the same iterates, ``nfev`` and tau as ``optimize_local_minima`` through SciPy
    with ``f(tau)`` = the device score of ``round(tau * fs)`` for that signal.  Against the host-refined
    :func:`optimize_haas_delay`, tau is equal unless two distinct delays' scores lie within the device / host score
    difference (<= 7.4e-16 relative on the fixtures): the refinement then may pick the other delay.
    Host route (``False``, or ``None`` without a device): :func:`optimize_haas_delay` signal by signal.
    ``last_haas_search`` records the call's work (:class:`HaasSearchStats`)."""
    global last_haas_search
    weights = dict(angle_limit=angle_limit, lambda_mean=lambda_mean, lambda_skew=lambda_skew,
                   lambda_correlation=lambda_correlation, lambda_penalty=lambda_penalty)
    x, is_torch = _haas_pool(input_signals)
    batch = int(x.shape[0])
    if batch == 0:
        last_haas_search = HaasSearchStats(route='none', signals=0)
        return np.zeros(0, np.float64)
    if not _haas_route():
        if is_torch:
            x = x.detach().cpu().numpy()
        stats = HaasSearchStats(route='host', signals=batch)
        last_haas_search = stats
        out = np.empty(batch, np.float64)
        evaluations = np.empty(batch, np.int64)
        for b in range(batch):
            out[b] = optimize_haas_delay(input_signal=x[b], sample_rate_hz=sample_rate_hz,
                                         max_delay_seconds=max_delay_seconds, grid_size=grid_size, **weights)
            evaluations[b] = last_haas_memo.calls
        stats.evaluations = evaluations
        return out
    taus = np.linspace(0.0, max_delay_seconds, grid_size)
    stats = HaasSearchStats(route='device', signals=batch)
    last_haas_search = stats
    print('Starting Grid Scan')
    print('Starting Local Minima optimization')
    import torch
    if is_torch:
        if not x.is_cuda:
            raise ValueError('a torch pool must be a device tensor (NumPy arrays are uploaded)')
        ctx = _native.context_for(x.device.index if x.device.index is not None else torch.cuda.current_device())
        pool = x.reshape(batch, x.shape[1], -1)
        pool = (pool if pool.dtype == torch.float32 else pool.to(torch.float32)).contiguous()
        return haas_search(_DevicePairScorer(ctx, pool, weights), batch, taus, sample_rate_hz, grid_size, stats)
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    x = x.reshape(batch, x.shape[1], -1)
    per_chunk = max(1, _HAAS_POOL_BYTES // (x.shape[1] * x.shape[2] * 4))
    out = []
    for first in range(0, batch, per_chunk):
        part = np.ascontiguousarray(to_float32(x[first:first + per_chunk]))
        pool = torch.from_numpy(part).to(dev)
        stats.pool_uploads += 1
        out.append(haas_search(_DevicePairScorer(ctx, pool, weights), part.shape[0], taus, sample_rate_hz, grid_size,
                               stats))
    return np.concatenate(out)


# ---- the Haas-delay scan of a voice pool (include/vnd_haas_scan_voice_stream.h) ---------------------------------------
def haas_scan_voice_spans(positions, fills, heads, counts, flags, window_frames: int,
                          max_frames_per_call: Optional[int] = None):
    """``(valid, new_positions, new_fills, new_heads)`` of one push of a :class:`HaasScanVoicePool`
    (``include/vnd_haas_scan_voice_stream.h``), per slot, from the state before the call, the frames pushed and the
    ``VOICE_START`` / ``VOICE_END`` flags alone - what the device computes from its own state::

        p = START ? 0 : position      valid = 1, or 0 for n = 0 without a flag      new position = END ? 0 : p + n
        fill = min(p + n, W)          head = (p + n) mod W                          (of a slot that answers 1)

    The slot's window in time order is then the ring entries ``(head - fill + k) mod W``, ``k in [0, fill)``.  A count
    below 0 (or above ``max_frames_per_call``, when given), or without START a position outside ``[0, 2^60]``, answers -1;
    such a slot and an idle one keep position, fill and head."""
    W = int(window_frames)
    if W < 1:
        raise ValueError(f'window_frames must be >= 1, got {window_frames}')
    valid, new = _valid_voice_spans(positions, counts, flags, max_frames_per_call)
    fills, heads = np.asarray(fills, np.int64), np.asarray(heads, np.int64)
    if not (fills.shape == heads.shape == valid.shape):
        raise ValueError(f'fills and heads of the shape of positions, got {fills.shape} and {heads.shape}')
    answered = valid == 1
    start = (np.asarray(flags, np.int64) & VOICE_START) != 0
    p = np.where(start | ~answered, 0, np.asarray(positions, np.int64))       # (no arithmetic on a bad value)
    q = p + np.where(answered, np.asarray(counts, np.int64), 0)
    return (valid, new, np.where(answered, np.minimum(q, W), fills).astype(np.int64),
            np.where(answered, q % W, heads).astype(np.int64))


class HaasScanVoicePool(_MeterPool):
    """The last ``window_frames`` input frames of ``slots`` voices, each with a life of its own, kept on the device to
    score candidate Haas delays against (:func:`haas_scan_voice_pool`; ``vnd_haas_scan_voice_stream_*``): voices start and
    end on any call and push blocks of any size up to ``max_frames_per_call`` or none, by the slot rule of the other
    meters (:func:`haas_scan_voice_spans`).  The device state keeps a ring of input frames per slot, and beside the
    position how many entries are the voice's (``fill``) and where its next frame goes (``head``): a delay depends on the
    order of the frames.  A (slot, delay) pair's row of moments is ``vnd_haas_pairs_f64_dev``'s for the slot's window as
    a contiguous signal, bit for bit, whatever the schedule.  An END leaves the window readable; the slot's next voice
    drops it.  One ``HaasEffect`` configuration per pool: ``delayed_channel``, ``mode``, ``width``.

    Pushing and scanning are two device entries: blocks arrive a hundred times a second, a voice is re-optimised now and
    then.  Two forms of the push; a pool is used through one of them (mixing them raises ``RuntimeError`` until
    ``reset()``):

    * ``process({slot: block}, start=[slot, ...], end=[slot, ...], discard=False)`` - float32 ``(n, in_channels)`` NumPy
      blocks in, ``{slot: None}`` out for every slot that got a block, started or ended.  One upload, and ``valid`` alone
      comes down.  Every refusal comes before any device call.
    * ``process_dev(x, counts, flags)`` - ``x`` float32 ``(slots, max_frames_per_call, in_channels)`` and int32
      ``(slots,)`` ``counts`` and ``flags`` on the device, a fading pool's own if it has one (``VOICE_SWITCH`` is
      ignored); returns ``valid``.  It only enqueues on the current stream and can be captured with
      ``torch.cuda.graph`` after a ``reset()``.

    The scan reads the state alone and goes with either form: :meth:`scan_dev` and :meth:`pairs_dev` on device tensors,
    :meth:`scan` from NumPy, :meth:`scores` for the objective, :meth:`optimize` for the reference's whole search."""

    _out_dtype = np.float64

    def __init__(self, slots: int, *, in_channels: int, max_frames_per_call: int, window_frames: int, max_delay: int,
                 sample_rate_hz=None, max_delay_seconds=None, delayed_channel: int = 0, ms_mode: bool = False,
                 width: Optional[float] = None):
        _MeterPool.__init__(self, slots, max_frames_per_call, 'float32')
        if isinstance(in_channels, (bool, np.bool_)) or in_channels not in (1, 2):
            raise ValueError(f'a pool of mono (1) or stereo (2) voices is taken, got in_channels={in_channels!r}')
        for name, value in (('window_frames', window_frames), ('max_delay', max_delay)):
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or value < 0:
                raise ValueError(f'{name} must be a non-negative integer, not {value!r}')
        if window_frames < self.max_frames_per_call:
            raise ValueError(f'window_frames {window_frames} below max_frames_per_call {self.max_frames_per_call}: two '
                             'frames of one call would share a ring entry')
        if window_frames > _INT32_MAX or max_delay > _INT32_MAX:
            raise ValueError(f'window_frames {window_frames} and max_delay {max_delay} must stay below 2**31')
        if delayed_channel not in (0, 1) or isinstance(delayed_channel, (bool, np.bool_)):
            raise ValueError(f'delayed_channel must be 0 or 1, got {delayed_channel!r}')
        if width is not None and not np.isfinite(float(width)):
            raise ValueError(f'width must be a finite number or None, got {width!r}')
        self.in_channels = int(in_channels)
        self.window_frames, self.max_delay = int(window_frames), int(max_delay)
        self.sample_rate_hz, self.max_delay_seconds = sample_rate_hz, max_delay_seconds
        self.delayed_channel, self.ms_mode, self.width = int(delayed_channel), bool(ms_mode), width
        if self.slots * -(-self.max_frames_per_call // 1024) > 1 << 23:       # the copy's grid: 1024 frames a workgroup
            raise ValueError(f'{self.slots} slots of {self.max_frames_per_call} frames per call are more than one launch '
                             'takes: split the pool')
        S = self.slots
        self._inputs = (('x', (S, self.max_frames_per_call, self.in_channels), 'float32', None),) \
            + _slot_ints(S, 'counts', 'flags')
        self._valid_spec = (('valid', (S,), 'int32', 'empty'),)
        self._valid = None                    # the pool's own valid, at a fixed address
        self._grids = {}                      # D -> (slot index, delays, moments) of the full grid, on the device
        self._workspace = None
        self._mirror()

    @property
    def chunks_per_pair(self) -> int:
        """The partials a pair can have: ``ceil((window_frames + max_delay) / 2048)``, the scan's grid along the frames."""
        return -(-(self.window_frames + self.max_delay) // 2048)

    # ---- the push ---------------------------------------------------------------------------
    def process(self, blocks=None, *, start=(), end=(), discard: bool = False):
        """One push of the dict form.  ``blocks``: ``{slot: float32 (n, in_channels) array}`` (``(n,)`` as well for
        mono), ``0 <= n <= max_frames_per_call``; ``start``: the slots whose voice begins with this call; ``end``: the
        slots whose voice ends with it.  Returns ``{slot: None}`` for every slot that got a block, started or ended: a
        push computes nothing, :meth:`scan` does.  Raises before any device call, as the other voice pools do:
        ``ValueError`` for a slot outside the pool or named twice, a block or an end for a slot that was never started,
        a start on a live slot (``discard=True`` allows it: the voice it held is dropped), a block above
        ``max_frames_per_call`` or of another channel count; ``TypeError`` for a block that is not float32."""
        return self._process_valid(blocks, start, end, discard, None, False)

    def process_dev(self, x, counts, flags, *, valid=None):
        """One push on device tensors, enqueued on the current stream: ``x`` float32 ``(slots, M, in_channels)``,
        ``counts`` / ``flags`` int32 ``(slots,)``.  Returns ``valid``, int32 ``(slots,)``: the pool's own tensor at a
        fixed address unless ``valid=`` gives the caller's.  No check reads device memory; bad per-slot values answer -1
        (``include/vnd_haas_scan_voice_stream.h``)."""
        if self._form == 'dict':
            self._require_form('dev')
        _check_device_tensors((x, counts, flags), self._inputs)
        _check_device_tensors((valid,), self._valid_spec)
        valid = self._push(_native.torch_module(), (x, counts, flags), valid)
        self._form = 'dev'
        return valid

    def _push(self, torch, inputs, valid):
        ctx, device, state, state_bytes = self._device(torch, inputs)
        x, counts, flags = inputs
        valid = self._valid if valid is None else valid
        _scan_native.haas_scan_voice_stream_push_device(
            ctx, state.data_ptr(), state_bytes, self.max_frames_per_call, self.window_frames, x.data_ptr(),
            self.in_channels, counts.data_ptr(), flags.data_ptr(), valid.data_ptr(), self.slots,
            stream=torch.cuda.current_stream(device).cuda_stream)
        return valid

    def _call_host(self, x, counts, flags, rows: bool = False):
        """One upload (the blocks and the two int32 arrays in one buffer), the push, one download (``valid``)."""
        torch = _native.torch_module()
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        ints = np.stack([counts, flags]).astype(np.int32)
        up = torch.from_numpy(np.concatenate([x.reshape(-1).view(np.uint8), ints.reshape(-1).view(np.uint8)])).to(device)
        self.transfers = {'to_device': 1, 'to_host': 0}
        x_dev = up[:x.nbytes].view(torch.float32).view(x.shape)
        int_rows = up[x.nbytes:].view(torch.int32).view(2, self.slots)
        valid = self._push(torch, (x_dev, int_rows[0], int_rows[1]), None).cpu().numpy()
        self.transfers['to_host'] = 1
        return None, valid

    # ---- the scan ---------------------------------------------------------------------------
    def pairs_dev(self, slot_idx, delays, *, out=None):
        """The raw scan, enqueued on the current stream: ``slot_idx`` and ``delays``, int32 ``(P,)`` device tensors, name
        P (slot, delay) pairs; returns their moments, float64 ``(P, 8)`` (``out=`` takes the caller's).  A pair whose slot
        is outside the pool or whose delay is outside ``[0, max_delay]`` gets a row of NaN; no check reads device memory.
        Pairs sorted by (slot, delay) run fastest; any order, duplicates and any split into calls give the same rows."""
        torch = _native.torch_module()
        for name, t in (('slot_idx', slot_idx), ('delays', delays)):
            if not _native.is_torch(t) or not t.is_cuda or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f'{name} must be a contiguous int32 device tensor of shape (P,)')
        count = int(slot_idx.shape[0])
        if count < 1 or int(delays.shape[0]) != count:
            raise ValueError(f'slot_idx and delays name the same P >= 1 pairs, got {tuple(slot_idx.shape)} and '
                             f'{tuple(delays.shape)}')
        if count > _native.HAAS_PAIRS_MAX:
            raise ValueError(f'{count} pairs, a call takes {_native.HAAS_PAIRS_MAX}: split them')
        if out is not None:
            _check_device_tensors((out,), (('out', (count, _native.MOMENTS), 'float64', None),))
        ctx, device, state, state_bytes = self._device(torch, (slot_idx, delays) + (() if out is None else (out,)))
        if out is None:
            out = torch.empty((count, _native.MOMENTS), dtype=torch.float64, device=device)
        need = count * self.chunks_per_pair * 64
        if self._workspace is None or self._workspace.numel() * 8 < need:
            self._workspace = torch.empty((need // 8,), dtype=torch.float64, device=device)
        _scan_native.haas_scan_voice_stream_pairs_device(
            ctx, state.data_ptr(), state_bytes, self.max_frames_per_call, self.window_frames, self.in_channels, self.slots,
            slot_idx.data_ptr(), delays.data_ptr(), count, out.data_ptr(), max_delay=self.max_delay,
            delayed_channel=self.delayed_channel, ms_mode=self.ms_mode, width=self.width,
            workspace_ptr=self._workspace.data_ptr(), workspace_bytes=self._workspace.numel() * 8,
            stream=torch.cuda.current_stream(device).cuda_stream)
        return out

    def scan_dev(self, delays):
        """Every slot against one grid of delays, enqueued on the current stream: ``delays``, an int32 ``(D,)`` device
        tensor shared by all slots (ascending runs fastest), gives ``moments``, float64 ``(slots, D, 8)`` on the device -
        the pool's own tensor for this ``D`` at a fixed address: read it, do not write it.  The pair arrays of the full
        grid are built once per ``D`` and kept on the device, sorted by (slot, delay); the first call for a ``D``
        allocates them, so make it before a capture."""
        torch = _native.torch_module()
        if not _native.is_torch(delays) or not delays.is_cuda or delays.dtype != torch.int32 or delays.dim() != 1 \
                or not delays.is_contiguous() or delays.shape[0] < 1:
            raise ValueError('delays must be a contiguous int32 device tensor of shape (D,), D >= 1')
        D = int(delays.shape[0])
        if self.slots * D > _native.HAAS_PAIRS_MAX:
            raise ValueError(f'{self.slots} slots x {D} delays are more than the {_native.HAAS_PAIRS_MAX} pairs of a call: '
                             'use pairs_dev on parts of the grid')
        if D not in self._grids:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f'the pair arrays of a grid of {D} delays are allocated on first use: call scan_dev '
                                   'once before the capture')
            device = delays.device
            self._grids[D] = (torch.arange(self.slots, dtype=torch.int32, device=device).repeat_interleave(D),
                              torch.empty((self.slots, D), dtype=torch.int32, device=device),
                              torch.empty((self.slots, D, _native.MOMENTS), dtype=torch.float64, device=device))
            need = self.slots * D * self.chunks_per_pair * 64
            if self._workspace is None or self._workspace.numel() * 8 < need:
                self._workspace = torch.empty((need // 8,), dtype=torch.float64, device=device)
        slot_idx, tiled, moments = self._grids[D]
        tiled.copy_(delays.unsqueeze(0).expand(self.slots, D))
        self.pairs_dev(slot_idx, tiled.view(-1), out=moments.view(-1, _native.MOMENTS))
        return moments

    def scan(self, delays) -> NDArray[np.float64]:
        """The NumPy form of :meth:`scan_dev`: ``delays``, ``(D,)`` integers in ``[0, max_delay]``, up; float64
        ``(slots, D, 8)`` moments down.  It reads the state only, so it goes with either form of the push."""
        d = np.asarray(delays)
        if d.ndim != 1 or not d.size or d.dtype.kind not in 'iu' or d.min() < 0 or d.max() > self.max_delay:
            raise ValueError(f'delays: (D,) integers in [0, {self.max_delay}], D >= 1')
        torch = _native.torch_module()
        device = torch.device('cuda', _native.default_context().device)
        return self.scan_dev(torch.from_numpy(d.astype(np.int32)).to(device)).cpu().numpy()

    def scores(self, moments, *, angle_limit: float = np.pi / 4, lambda_mean: float = 5.0, lambda_skew: float = 2.0,
               lambda_correlation: float = 15.0, lambda_penalty: float = 1e3):
        """``symmetry_aware_objective`` of every row of ``(..., 8)`` moments; lower is better.  NumPy in, NumPy out:
        :func:`scores_from_moments`.  A device tensor in, a device float64 tensor out - the same float64 operations in
        torch, enqueued on the current stream - so ``delays[pool.scores(moments).argmin(-1)]`` is the device int32
        ``(slots,)`` tensor a :class:`~vndecorrelate_amd.streaming.HaasFadeVoicePool` takes as its ``delays``."""
        if not _native.is_torch(moments):
            m = np.asarray(moments, np.float64)
            if m.shape[-1:] != (_native.MOMENTS,):
                raise ValueError(f'moments of shape (..., 8), got {m.shape}')
            return scores_from_moments(m.reshape(-1, _native.MOMENTS), angle_limit=angle_limit, lambda_mean=lambda_mean,
                                       lambda_skew=lambda_skew, lambda_correlation=lambda_correlation,
                                       lambda_penalty=lambda_penalty).reshape(m.shape[:-1])
        torch = _native.torch_module()
        if moments.dtype != torch.float64 or tuple(moments.shape[-1:]) != (_native.MOMENTS,):
            raise ValueError(f'moments: a float64 tensor of shape (..., 8), got {moments.dtype} {tuple(moments.shape)}')
        s0, s1, s2, s3, tmax, lr, ll = (moments[..., k] for k in range(7))
        total = s0 + EPSILON
        spread = s2 / total
        skew = (s3 / total) / (torch.clamp(spread, min=EPSILON) ** 1.5)
        correlation = lr / (torch.sqrt(ll) + EPSILON) ** 2
        exceedance = torch.clamp(tmax - angle_limit, min=0.0)
        objective = (spread - lambda_mean * (s1 / total) ** 2 - lambda_skew * skew ** 2
                     - lambda_correlation * correlation ** 2 - lambda_penalty * exceedance ** 2)
        return -objective

    def optimize(self, slots=None, *, grid_size: int = 400, angle_limit: float = np.pi / 4, lambda_mean: float = 5.0,
                 lambda_skew: float = 2.0, lambda_correlation: float = 15.0,
                 lambda_penalty: float = 1e3) -> NDArray[np.float64]:
        """:func:`optimize_haas_delay_batched` for the windows of ``slots`` (default: every slot): ``(len(slots),)``
        float64 delays in seconds.  It is :func:`haas_search` - the grid of ``grid_size`` taus up to the pool's
        ``max_delay_seconds``, the local minima, their lockstep refinement - with a scorer over the rings: pairs go up,
        moments come down, one pairs launch per round (more only past the workspace budget).  A pair's moments are the
        one-shot's for the slot's window bit for bit, so the result is what :func:`optimize_haas_delay_batched` returns
        on the device route for the same windows.  The optimiser's own configuration only: LR, ``delayed_channel=0``, no
        width, on a pool built with ``sample_rate_hz`` and ``max_delay_seconds``; anything else raises ``ValueError``
        before any device call."""
        if self.ms_mode or self.delayed_channel != 0 or self.width is not None:
            raise ValueError("optimize searches HaasEffect(mode='LR', delayed_channel=0, width=None) as optimize_haas_delay "
                             f'does: this pool scans ms_mode={self.ms_mode}, delayed_channel={self.delayed_channel}, '
                             f'width={self.width!r}')
        if self.sample_rate_hz is None or self.max_delay_seconds is None:
            raise ValueError('optimize needs the pool built with sample_rate_hz and max_delay_seconds')
        chosen = list(range(self.slots)) if slots is None else [self._slot(s, 'optimize') for s in slots]
        if isinstance(grid_size, (bool, np.bool_)) or not isinstance(grid_size, (int, np.integer)) or grid_size < 1:
            raise ValueError(f'grid_size must be a positive integer, not {grid_size!r}')
        if not chosen:
            return np.zeros(0, np.float64)
        weights = dict(angle_limit=angle_limit, lambda_mean=lambda_mean, lambda_skew=lambda_skew,
                       lambda_correlation=lambda_correlation, lambda_penalty=lambda_penalty)
        torch = _native.torch_module()
        device = torch.device('cuda', _native.default_context().device)
        slot_of = np.asarray(chosen, np.int64)
        per_launch = max(1, min(_HAAS_SCAN_BYTES // (self.chunks_per_pair * 64), _native.HAAS_PAIRS_MAX))

        def score(signals, delays):
            rows = []
            for first in range(0, delays.size, per_launch):               # launches bounded by their workspace
                pairs = np.stack([slot_of[signals[first:first + per_launch]], delays[first:first + per_launch]])
                up = torch.from_numpy(pairs.astype(np.int32)).to(device)
                rows.append(self.pairs_dev(up[0], up[1]).cpu().numpy())
            moments = np.concatenate(rows) if rows else np.zeros((0, _native.MOMENTS))
            return scores_from_moments(moments, **weights)

        self.last_search = HaasSearchStats(route='voice pool', signals=len(chosen))
        taus = np.linspace(0.0, self.max_delay_seconds, grid_size)
        return haas_search(score, len(chosen), taus, self.sample_rate_hz, grid_size, self.last_search)

    # ---- the device -------------------------------------------------------------------------
    def _device(self, torch, tensors):
        """``(ctx, device, state, state_bytes)`` after the look at where the tensors live."""
        ctx = _native.default_context()
        device = torch.device('cuda', ctx.device)
        for t in tensors:
            if t.device != device:
                raise ValueError(f'tensor on {t.device}, the pool runs on {device}')
        state, state_bytes = self._ensure_state(torch, ctx)
        return ctx, device, state, state_bytes

    def _state_bytes(self, ctx) -> int:
        return _scan_native.haas_scan_voice_stream_state_bytes(self.slots, self.max_frames_per_call, self.window_frames,
                                                               self.in_channels)

    def _allocate(self, torch, ctx):
        _SlotPool._allocate(self, torch, ctx)
        self._valid = torch.zeros((self.slots,), dtype=torch.int32, device=torch.device('cuda', ctx.device))

    def _reset_entry(self, ctx, state_ptr, state_bytes, stream):
        _scan_native.haas_scan_voice_stream_reset_device(ctx, state_ptr, state_bytes, self.slots, self.max_frames_per_call,
                                                         self.window_frames, self.in_channels, stream=stream)


def haas_scan_voice_pool(slots: int, *, in_channels: int, max_frames_per_call: int, window_frames: int,
                         max_delay_seconds, sample_rate_hz, delayed_channel: int = 0, mode=LayoutMode.LR,
                         width: Optional[float] = None) -> HaasScanVoicePool:
    """A :class:`HaasScanVoicePool`: the last ``window_frames`` input frames (at least ``max_frames_per_call``) of
    ``slots`` mono or stereo voices that start, end and push blocks on their own, kept on the device, and the Haas-delay
    scan over them for delays up to ``round(max_delay_seconds * sample_rate_hz)`` frames (ties to even, as
    ``HaasEffect`` rounds) under the one configuration ``delayed_channel``, ``mode``, ``width``.  There is no host loop:
    whatever the pool does not cover raises ``ValueError`` here."""
    if mode == LayoutMode.MS:
        ms = True
    elif mode == LayoutMode.LR:
        ms = False
    else:
        raise ValueError(f"mode must be 'MS' or 'LR', not {mode!r}")
    if not (np.isfinite(float(sample_rate_hz)) and float(sample_rate_hz) > 0 and np.isfinite(float(max_delay_seconds))
            and float(max_delay_seconds) >= 0):
        raise ValueError(f'sample_rate_hz must be positive and max_delay_seconds non-negative, got {sample_rate_hz!r} '
                         f'and {max_delay_seconds!r}')
    max_delay = int(haas_delays(max_delay_seconds, sample_rate_hz))
    return HaasScanVoicePool(slots, in_channels=in_channels, max_frames_per_call=max_frames_per_call,
                             window_frames=window_frames, max_delay=max_delay, sample_rate_hz=sample_rate_hz,
                             max_delay_seconds=max_delay_seconds, delayed_channel=delayed_channel, ms_mode=ms, width=width)


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


# ---- the batched velvet-noise optimiser -----------------------------------------------------------------------------
# the pairs kernel's workspace is ceil(n / 2048) * P * 64 bytes: keep it under this many bytes per launch
_VELVET_SCAN_BYTES = 1 << 30
# optimize_velvet_noise_batched keeps at most this many bytes of its float32 pool on the device (else chunks of signals)
_VELVET_POOL_BYTES = 4 << 30

_velvet_search_device: Optional[bool] = None


def set_velvet_search_device(enabled: Optional[bool]) -> None:
    """Where :func:`optimize_velvet_noise_batched` runs.

    ``None`` (default): on the GPU when a gfx950 device is present, otherwise :func:`optimize_velvet_noise` signal by
    signal on the host.  ``True``: the device; a call raises ``RuntimeError`` when there is none.  ``False``: always
    the host loop, whose kappa is the reference's."""
    global _velvet_search_device
    if enabled is not None and not isinstance(enabled, (bool, np.bool_)):
        raise TypeError(f'set_velvet_search_device takes True, False or None, not {enabled!r}')
    _velvet_search_device = None if enabled is None else bool(enabled)


def _velvet_route() -> bool:
    return analysis.device_route(_velvet_search_device, True,
                                 'set_velvet_search_device(True): no gfx950 device (or no built extension) to run on')


class VelvetBank:
    """The candidates of :func:`optimize_velvet_noise` at one ``(sample_rate_hz, duration_seconds, num_impulses, seed,
    segment_envelope)``, built for many kappa at once: ``VelvetNoise(log_distribution_strength=kappa, normalizer=None,
    filtered_channels=(0,), mode='LR', num_outs=2)``.

    ``_draw_taps`` makes its two PCG64 draws (signs, then offsets) whatever kappa is, so they are made once here; only
    ``generate_log_distribution``, the cumulative marks and ``apply_log_distribution`` depend on kappa, and those are
    the same float64 operations broadcast over a kappa axis (``np.cumsum`` along the row adds in the same order).
    ``positions`` therefore equals ``_draw_taps`` position for position, and ``arrays`` equals
    ``class_path_bank_arrays([VelvetNoise(kappa)._tap_member() ...])`` array for array.  (``seed=None`` draws once for
    the whole bank, where ``VelvetNoise`` draws afresh per candidate.)"""

    def __init__(self, *, sample_rate_hz, duration_seconds: float, num_impulses: int, seed=1,
                 segment_envelope: Sequence[float] = _dec.DEFAULT_SEGMENT_ENVELOPE):
        self.sample_rate_hz, self.duration_seconds, self.num_impulses = sample_rate_hz, duration_seconds, int(num_impulses)
        self.fir_length = int(round(sample_rate_hz * duration_seconds))
        if self.num_impulses >= self.fir_length * 0.2:            # VelvetNoise.__post_init__'s refusal
            raise ValueError(f'Velvet Noise Filter of length {self.fir_length} with {self.num_impulses} impulses is '
                             'not sparse.\n\tnum_impulses must be less than 20% the FIR length in samples.')
        self.envelope = segment_envelope if segment_envelope else _dec.IDENTITY_ENVELOPE
        self.apply_gain = self.envelope != _dec.IDENTITY_ENVELOPE
        rng = np.random.default_rng(seed)
        sign_draw = rng.uniform(low=0, high=1, size=(self.num_impulses, 1))
        self.offset_draw = rng.uniform(low=0, high=1, size=(self.num_impulses + 1, 1))[:, 0]
        signs = ((2 * np.round(sign_draw)) - 1)[:, 0]
        self.mean_gap = sample_rate_hz / (self.num_impulses / duration_seconds)
        # table order: per segment the negative taps, then the positive ones, each in generation order
        num_segments = len(self.envelope)
        segment = np.array([_dec._segment_index(k, self.num_impulses, num_segments) for k in range(self.num_impulses)])
        positive = ((signs + 1) / 2).astype(np.int64)
        self.order = np.lexsort((np.arange(self.num_impulses), positive, segment))
        self.weights = np.where(positive[self.order] == 1, 1.0, -1.0).astype(np.float32)
        self.seg_end = np.cumsum(np.bincount(segment, minlength=num_segments)).astype(np.int64)
        self.seg_gain = np.asarray([float(self.envelope[s]) if self.apply_gain else 1.0 for s in range(num_segments)],
                                   np.float32)

    def positions(self, kappas) -> NDArray[np.int32]:
        """``(K, num_impulses + 1)`` int32: row j is ``_draw_taps(..., strength=kappas[j])[0][:, 0]``."""
        kappa = np.asarray(kappas, np.float64).reshape(-1, 1)
        size = self.num_impulses
        ramp = np.arange(size + 1.0) / size
        weights = (10.0 ** (2.0 * kappa * ramp)) / (100.0 * ((1.0 + (kappa * 99.0)) / 100.0))
        marks = np.cumsum(weights, axis=1)
        marks[kappa[:, 0] == 0.0] -= 1.0
        marks *= self.fir_length / marks[:, -1:]
        spread = np.fmax(0.0, weights * self.mean_gap - 1)
        return np.round(self.offset_draw * spread + marks).astype(np.int32)

    def keys(self, kappas) -> NDArray[np.int32]:
        """``(K, num_impulses)``: what a candidate's table depends on kappa through - its taps' positions."""
        return self.positions(kappas)[:, :self.num_impulses]

    def arrays_of_keys(self, keys) -> TapArrays:
        """The class-path bank of the candidates whose :meth:`keys` rows are ``keys``: candidate t owns channels
        ``2t`` (filtered) and ``2t + 1`` (copied through)."""
        keys = np.asarray(keys, np.int32).reshape(-1, self.num_impulses)
        count, taps, segs = keys.shape[0], self.num_impulses, len(self.seg_end)
        if count == 0:
            return class_path_bank_arrays([])
        first = np.arange(count, dtype=np.int64)
        tap_offsets = np.concatenate([[0], np.repeat((first + 1) * taps, 2)])
        seg_offsets = np.concatenate([[0], np.repeat((first + 1) * segs, 2)])
        return TapArrays(tap_offsets.astype(np.int32), np.ascontiguousarray(keys[:, self.order]).reshape(-1),
                         np.tile(self.weights, count), seg_offsets.astype(np.int32),
                         (first[:, None] * taps + self.seg_end).reshape(-1).astype(np.int32),
                         np.tile(self.seg_gain, count), np.tile(np.array([0, 1], np.uint8), count), self.apply_gain)

    def arrays(self, kappas) -> TapArrays:
        return self.arrays_of_keys(self.keys(kappas))


def velvet_bank_arrays(kappas, *, sample_rate_hz, duration_seconds: float, num_impulses: int, seed=1,
                       segment_envelope: Sequence[float] = _dec.DEFAULT_SEGMENT_ENVELOPE) -> TapArrays:
    """The ``TapArrays`` of :func:`optimize_velvet_noise`'s candidates at the K values ``kappas``, vectorised over
    kappa (:class:`VelvetBank`): equal to ``class_path_bank_arrays([VelvetNoise(kappa)._tap_member() ...])``."""
    return VelvetBank(sample_rate_hz=sample_rate_hz, duration_seconds=duration_seconds, num_impulses=num_impulses,
                      seed=seed, segment_envelope=segment_envelope).arrays(kappas)


@dataclass
class VelvetSearchStats:
    """The work of one :func:`optimize_velvet_noise_batched` call (tools, tests), in the shape of
    :class:`HaasSearchStats`.  ``rounds`` counts the lockstep refinement's rounds, the first points of every minimum
    included; ``pairs_per_round`` / ``tables_per_round`` the distinct (signal, table) pairs and distinct tables each
    round scored; ``grid_pairs`` / ``grid_tables`` those of the grid; ``evaluations[b]`` the objective evaluations of
    signal b's refinements; ``minimum_signal``, ``minimum_nfev``, ``minimum_x`` and ``minimum_fun`` the signal, ``nfev``,
    kappa and score of each refined minimum in order; ``evaluated`` per round the (signal, kappa) of every lane; ``pool_uploads`` how many chunks of the pool went
    to the device.  Device route: ``grid_launches`` and ``launches`` count ``vnd_velvet_pairs_f32_dev`` calls,
    ``launch_pairs`` / ``launch_ms`` / ``launch_pool`` their pairs, device-event milliseconds and pool pointer, and
    ``bank_seconds`` the host time spent building banks (their arrays, ``TapTable.create``'s device images and uploads)."""
    route: str
    signals: int
    rounds: int = 0
    pairs_per_round: List[int] = field(default_factory=list)
    tables_per_round: List[int] = field(default_factory=list)
    grid_pairs: int = 0
    grid_tables: int = 0
    evaluations: NDArray = field(default_factory=lambda: np.zeros(0, np.int64))
    minimum_signal: NDArray = field(default_factory=lambda: np.zeros(0, np.int64))
    minimum_nfev: NDArray = field(default_factory=lambda: np.zeros(0, np.int64))
    minimum_x: NDArray = field(default_factory=lambda: np.zeros(0, np.float64))
    minimum_fun: NDArray = field(default_factory=lambda: np.zeros(0, np.float64))
    evaluated: List[Tuple[NDArray, NDArray]] = field(default_factory=list)
    pool_uploads: int = 0
    grid_launches: int = 0
    launches: int = 0
    launch_pairs: List[int] = field(default_factory=list)
    launch_ms: List[float] = field(default_factory=list)
    launch_pool: List[int] = field(default_factory=list)
    bank_seconds: float = 0.0


last_velvet_search: Optional[VelvetSearchStats] = None   # the last optimize_velvet_noise_batched call's work


def _distinct_rows(keys: NDArray) -> Tuple[NDArray, NDArray]:
    """``(distinct rows in lexicographic order, index of each row among them)``: tables deduplicated by content."""
    unique, inverse = np.unique(keys, axis=0, return_inverse=True)
    return unique, np.asarray(inverse, np.int64).reshape(-1)


def velvet_search(score_pairs: Callable[[NDArray, NDArray, NDArray], NDArray], num_signals: int, kappas: NDArray,
                  table_keys: Callable[[NDArray], NDArray], grid_size: int,
                  stats: Optional[VelvetSearchStats] = None) -> NDArray[np.float64]:
    """``optimize_velvet_noise``'s search for ``num_signals`` signals at once, given a scorer.

    ``table_keys(values)`` gives one integer row per value: everything the candidate's table depends on the value
    through (:meth:`VelvetBank.keys`); equal rows are one table.  ``score_pairs(signals, tables, keys)`` returns the
    objective of table ``keys[tables[p]]`` on signal ``signals[p]`` for distinct (signal, table) pairs sorted by
    (signal, table); ``keys`` holds the call's distinct tables.  The grid is one call over every signal and distinct
    grid table; each refinement round is one call over the distinct pairs its lanes ask for.  Per signal: the grid's
    local minima (:func:`get_local_minima`), each refined over its neighbours by :func:`minimize_bounded_lockstep`
    (SciPy's bounded method, ``xatol=1e-4``), and :func:`optimize_local_minima`'s choice among them."""
    kappas = np.asarray(kappas, np.float64)
    stats = VelvetSearchStats(route='custom', signals=num_signals) if stats is None else stats

    def score(signals, tables, keys):
        return np.asarray(score_pairs(signals, tables, keys), np.float64)

    keys, inverse = _distinct_rows(np.asarray(table_keys(kappas)))
    count = keys.shape[0]
    launches_before = stats.launches
    grid = score(np.repeat(np.arange(num_signals, dtype=np.int64), count),
                 np.tile(np.arange(count, dtype=np.int64), num_signals), keys)
    scores = grid.reshape(num_signals, count)[:, inverse]
    stats.grid_pairs += num_signals * count
    stats.grid_tables = count                            # (the same for every chunk of a pool)
    stats.grid_launches += stats.launches - launches_before
    lane_signal, lower, upper = [], [], []
    for b in range(num_signals):
        for i in get_local_minima(scores[b], grid_size):
            lane_signal.append(b)
            lower.append(kappas[max(0, i - 1)])
            upper.append(kappas[min(grid_size - 1, i + 1)])
    lane_signal = np.asarray(lane_signal, np.int64)

    def objective(lanes, x):
        tables, which = _distinct_rows(np.asarray(table_keys(x)))
        pairs, back = np.unique(lane_signal[lanes] * tables.shape[0] + which, return_inverse=True)
        stats.pairs_per_round.append(int(pairs.size))
        stats.tables_per_round.append(int(tables.shape[0]))
        stats.evaluated.append((lane_signal[lanes] + stats.evaluations.size, np.array(x, np.float64)))
        return score(pairs // tables.shape[0], pairs % tables.shape[0], tables)[np.asarray(back).reshape(-1)]

    result = minimize_bounded_lockstep(objective, lower, upper, xatol=1e-4)
    stats.rounds += result.rounds
    best_kappa, best_score = np.zeros(num_signals), np.full(num_signals, np.inf)
    evaluations = np.zeros(num_signals, np.int64)
    for lane, b in enumerate(lane_signal):               # minima in order, strict <, from (0.0, inf)
        evaluations[b] += result.nfev[lane]
        if result.fun[lane] < best_score[b]:
            best_score[b], best_kappa[b] = result.fun[lane], result.x[lane]
    stats.minimum_signal = np.concatenate([stats.minimum_signal, lane_signal + stats.evaluations.size])
    stats.minimum_nfev = np.concatenate([stats.minimum_nfev, result.nfev])
    stats.minimum_x = np.concatenate([stats.minimum_x, result.x])
    stats.minimum_fun = np.concatenate([stats.minimum_fun, result.fun])
    stats.evaluations = np.concatenate([stats.evaluations, evaluations])
    return best_kappa


class _VelvetUnsupported(Exception):
    """A bank outside the pairs kernel's scope (largest tap index): the call takes the host route."""


class _DeviceVelvetScorer:
    """A :func:`velvet_search` scorer over a float32 ``(B, n, C)`` pool resident on the device: per call one bank of
    the call's distinct tables (:meth:`VelvetBank.arrays_of_keys`) and one ``vnd_velvet_pairs_f32_dev`` launch (more
    only past the workspace budget, the pair limit or the 32767 candidates a tap table holds); tables and pairs go up,
    moments come down, and ``scores_from_moments`` turns them into scores.  Always ``VND_MODE_EXACT``."""

    def __init__(self, ctx, pool, weights: dict, bank: VelvetBank, stats: VelvetSearchStats):
        self.ctx, self.pool, self.weights, self.bank, self.stats = ctx, pool, weights, bank, stats
        import torch
        self.torch = torch
        self.batch, self.n, self.channels = (int(v) for v in pool.shape)
        self.workspace = None
        tiles = (self.n + _native.VELVET_PAIRS_TILE - 1) // _native.VELVET_PAIRS_TILE
        self.per_launch = min(_native.VELVET_PAIRS_MAX, max(1, _VELVET_SCAN_BYTES // (tiles * 64)))

    def _launch(self, table, signals, candidates):
        torch, stats = self.torch, self.stats
        dev = self.pool.device
        count = int(signals.size)
        ws = _native.velvet_pairs_workspace_bytes(self.n, count)
        if self.workspace is None or self.workspace.numel() < ws:
            self.workspace = None                                  # the old one goes before the new one comes
            self.workspace = torch.empty(max(ws, 1), dtype=torch.uint8, device=dev)
        pairs = torch.from_numpy(np.stack([signals, candidates]).astype(np.int32)).to(dev)
        moments = torch.empty((count, _native.MOMENTS), dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev)
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record(stream)
        _native.velvet_pairs_device(self.ctx, table, self.pool.data_ptr(), self.batch, self.n, self.channels,
                                    pairs[0].data_ptr(), pairs[1].data_ptr(), count, moments.data_ptr(),
                                    workspace_ptr=self.workspace.data_ptr(), workspace_bytes=ws,
                                    mode=_native.MODE_EXACT, stream=stream.cuda_stream)
        end.record(stream)
        out = moments.cpu().numpy()                                # (synchronises the stream)
        stats.launches += 1
        stats.launch_pairs.append(count)
        stats.launch_ms.append(float(begin.elapsed_time(end)))
        stats.launch_pool.append(int(self.pool.data_ptr()))
        return out

    def _bank_rows(self, keys, signals, candidates):
        """Moments of the pairs (signals[p], candidates[p]) of one bank, built from its tables' ``keys``."""
        import time
        started = time.perf_counter()
        arrays = self.bank.arrays_of_keys(keys)
        table = _native.TapTable.create(self.ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight,
                                        **arrays.kwargs())
        self.stats.bank_seconds += time.perf_counter() - started       # arrays, device images and their uploads
        try:
            rows = [self._launch(table, signals[first:first + self.per_launch], candidates[first:first + self.per_launch])
                    for first in range(0, signals.size, self.per_launch)]
        finally:
            table.close()
        return np.concatenate(rows)

    def __call__(self, signals, tables, keys):
        if keys.size and int(keys.max()) > _native.VELVET_PAIRS_MAX_TAP_INDEX:
            raise _VelvetUnsupported(f'tap index {int(keys.max())} is above {_native.VELVET_PAIRS_MAX_TAP_INDEX}')
        moments = np.zeros((signals.size, _native.MOMENTS))
        # A tap table holds at most VELVET_BANK_MAX_CANDIDATES candidates: more distinct tables go in several banks.  A row
        # does not depend on its candidate's bank or place in it, so the split changes no bit.
        limit = _native.VELVET_BANK_MAX_CANDIDATES
        for first in range(0, keys.shape[0], limit):
            mine = np.flatnonzero((tables >= first) & (tables < first + limit))      # (keeps the (signal, table) order)
            if mine.size:
                moments[mine] = self._bank_rows(keys[first:first + limit], signals[mine], tables[mine] - first)
        return scores_from_moments(moments, **self.weights)


def optimize_velvet_noise_batched(*, input_signals, sample_rate_hz: int, duration_seconds: float, num_impulses: int,
                                  seed: int = 1, grid_size: int = 400, angle_limit: float = np.pi / 4,
                                  lambda_mean: float = 5.0, lambda_skew: float = 2.0, lambda_correlation: float = 15.0,
                                  lambda_penalty: float = 1e3) -> NDArray[np.float64]:
    """:func:`optimize_velvet_noise` for every signal of a pool: ``(B,)`` float64 ``log_distribution_strength``.

    ``input_signals`` is a stereo pool ``(B, n, 2)`` or a mono pool ``(B, n)`` with n > 0: a NumPy array of any real
    dtype (cast as ``to_float32`` casts it) or a CUDA torch tensor, read in place.  B = 0 gives an empty array.

    Device route (:func:`set_velvet_search_device`: ``None`` with a gfx950 device, or ``True``): the pool goes up once
    (in chunks of whole signals past ``_VELVET_POOL_BYTES``) and stays there.  The kappa grid's tables are built at
    once (:class:`VelvetBank`) and deduplicated by content; the grid is one launch over every (signal, distinct table)
    pair (more only past the workspace budget or the pair limit).  The local minima of every signal
    (:func:`get_local_minima`) are then refined together by :func:`minimize_bounded_lockstep` (``xatol=1e-4``): each
    round builds one bank of the round's distinct tables and makes one launch over its distinct (signal, table) pairs
    (:func:`velvet_search`, ``vnd_velvet_pairs_f32_dev``).  Only tables and pairs go up and moments come down;
    ``scores_from_moments`` scores them; the choice among a signal's minima is :func:`optimize_local_minima`'s.  The
    kernel runs in ``VND_MODE_EXACT`` whatever ``set_default_mode`` says: every frame is the exact-mode
    ``VelvetNoise.convolve`` output bit for bit, polar maths in float32, sums in float64.  A filter whose taps reach
    past ``VND_VELVET_PAIRS_MAX_TAP_INDEX`` (4094 frames) is outside the kernel: such a call takes the host route.

    **kappa may differ from** :func:`optimize_velvet_noise`'s, whose refinement runs ``symmetry_aware_objective`` on the
    host and reproduces the reference's kappa.  The objective is piecewise constant in kappa (tap positions are rounded
    to integers) and Brent's parabolic steps use the score values themselves, so score differences far below any
    tolerance steer the minimiser elsewhere.  Measured on the ``viola_excerpt`` fixture at grid 9, feeding the exact
    frames through this route's arithmetic (float32 element maths, float64 sums): every score moved by at most 5.6e-5 on
    scores of about 619 and the grid's local minima stayed [2, 4, 6], but ``nfev`` became [12, 16, 11] against the
    host's [12, 15, 20] and kappa 0.75965 against the reference's 0.75804 - with a lower score, 618.306 against
    618.404.  The returned kappa is, bit for bit, what ``optimize_local_minima`` returns through SciPy when its
    objective is this route's device score.  A caller who needs the reference's kappa uses
    :func:`optimize_velvet_noise`.

    Host route (``False``, or ``None`` without a device): :func:`optimize_velvet_noise` signal by signal.
    ``last_velvet_search`` records the call's work (:class:`VelvetSearchStats`)."""
    global last_velvet_search
    weights = dict(angle_limit=angle_limit, lambda_mean=lambda_mean, lambda_skew=lambda_skew,
                   lambda_correlation=lambda_correlation, lambda_penalty=lambda_penalty)
    x, is_torch = _haas_pool(input_signals)
    batch = int(x.shape[0])
    if batch == 0:
        last_velvet_search = VelvetSearchStats(route='none', signals=0)
        return np.zeros(0, np.float64)

    def on_host():
        global last_velvet_search
        pool = x.detach().cpu().numpy() if is_torch else x
        last_velvet_search = VelvetSearchStats(route='host', signals=batch)
        return np.array([optimize_velvet_noise(input_signal=pool[b], sample_rate_hz=sample_rate_hz,
                                               duration_seconds=duration_seconds, num_impulses=num_impulses, seed=seed,
                                               grid_size=grid_size, **weights) for b in range(batch)], np.float64)

    if not _velvet_route():
        return on_host()
    bank = VelvetBank(sample_rate_hz=sample_rate_hz, duration_seconds=duration_seconds, num_impulses=num_impulses,
                      seed=seed)
    kappas = np.linspace(0.0, 1.0, grid_size)
    if int(bank.keys(kappas).max()) > _native.VELVET_PAIRS_MAX_TAP_INDEX:      # outside the kernel's window: nothing printed yet
        return on_host()
    stats = VelvetSearchStats(route='device', signals=batch)
    last_velvet_search = stats
    print('Starting Grid Scan')
    print('Starting Local Minima optimization')
    import torch
    try:
        if is_torch:
            if not x.is_cuda:
                raise ValueError('a torch pool must be a device tensor (NumPy arrays are uploaded)')
            ctx = _native.context_for(x.device.index if x.device.index is not None else torch.cuda.current_device())
            pool = x.reshape(batch, x.shape[1], -1)
            pool = (pool if pool.dtype == torch.float32 else pool.to(torch.float32)).contiguous()
            return velvet_search(_DeviceVelvetScorer(ctx, pool, weights, bank, stats), batch, kappas, bank.keys,
                                 grid_size, stats)
        ctx = _native.default_context()
        dev = torch.device('cuda', ctx.device)
        x3 = x.reshape(batch, x.shape[1], -1)
        per_chunk = max(1, _VELVET_POOL_BYTES // (x3.shape[1] * x3.shape[2] * 4))
        out = []
        for first in range(0, batch, per_chunk):
            part = np.ascontiguousarray(to_float32(x3[first:first + per_chunk]))
            pool = torch.from_numpy(part).to(dev)
            stats.pool_uploads += 1
            out.append(velvet_search(_DeviceVelvetScorer(ctx, pool, weights, bank, stats), part.shape[0], kappas,
                                     bank.keys, grid_size, stats))
        return np.concatenate(out)
    except _VelvetUnsupported:
        return on_host()
