"""CPU tier of the batched Haas-delay optimiser (include/vnd_haas_search.h, bounded.py,
optimization.optimize_haas_delay_batched): the lockstep bounded minimiser against SciPy lane by lane, the vectorised
delay rounding against Python's round, the search driver with the host objective against optimize_haas_delay and the
reference's tau, the header and its binding, and the routing rules - no device call."""
import contextlib
import ctypes
import io
import json
import math
import pathlib
import re
import subprocess
import warnings

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / 'tests' / 'golden'
HEADER = REPO / 'include' / 'vnd_haas_search.h'


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_haas_scan_golden', REPO / 'tools' / 'gen_haas_scan_golden.py')
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def golden():
    return json.loads((GOLDEN / 'haas_scan_manifest.json').read_text())


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


@pytest.fixture
def host_only():
    from vndecorrelate_amd import optimization
    optimization.set_haas_scan_device(False)
    yield optimization
    optimization.set_haas_scan_device(None)


# ---- the lockstep minimiser against SciPy ----------------------------------------------------------------------------
def _problems(rng, count):
    """(f, lower, upper) of every kind the issue names: smooth, integer-delay steps with plateaus and exact ties,
    equal bounds, NaN, and constants (every comparison a tie)."""
    out = []
    for k in range(count):
        kind = k % 6
        c, w = rng.uniform(-1, 2), rng.uniform(0.5, 3)
        lo = rng.uniform(-1, 0.5)
        hi = lo + rng.uniform(1e-3, 1.5)
        fs = int(rng.choice([50, 997, 16000, 44100]))
        if kind == 0:
            f = (lambda x, c=c, w=w: w * (x - c) ** 2 + math.sin(5 * x))
        elif kind == 1:                             # a score of round(tau * fs): plateaus, exact ties between delays
            f = (lambda x, c=c, fs=fs: float(abs(round(x * fs) - round(c * fs)) // 3))
        elif kind == 2:
            f = (lambda x, c=c, fs=fs: float((round(x * fs) * 7919) % 13) - 0.5 * (round(x * fs) == round(c * fs)))
        elif kind == 3:
            f = (lambda x, c=c: float('nan') if x > c else x * x)
        elif kind == 4:
            f = (lambda x, c=c: math.cos(13 * x + c))
            hi = lo                                 # equal bounds
        else:
            f = (lambda x: 1.0)
        out.append((f, lo, hi))
    return out


def _scipy(f, lo, hi, maxiter):
    from scipy.optimize import minimize_scalar
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return minimize_scalar(f, bounds=(lo, hi), method='bounded', options={'xatol': 1e-4, 'maxiter': maxiter})


@pytest.mark.parametrize('maxiter', [500, 6])
def test_lockstep_equals_scipy_lane_by_lane(maxiter):
    from vndecorrelate_amd.bounded import minimize_bounded_lockstep
    problems = _problems(np.random.default_rng(3), 240)
    calls = []

    def fun(lanes, x):
        calls.append(lanes.size)
        return [problems[i][0](float(v)) for i, v in zip(lanes, x)]
    got = minimize_bounded_lockstep(fun, [p[1] for p in problems], [p[2] for p in problems], xatol=1e-4,
                                    maxiter=maxiter)
    statuses = set()
    for lane, (f, lo, hi) in enumerate(problems):
        want = _scipy(f, lo, hi, maxiter)
        assert np.float64(want.x).tobytes() == got.x[lane].tobytes(), (lane, want.x, got.x[lane])
        assert np.float64(want.fun).tobytes() == got.fun[lane].tobytes(), (lane, want.fun, got.fun[lane])
        assert (want.nfev, want.status) == (got.nfev[lane], got.status[lane]), lane
        statuses.add(int(want.status))
    assert statuses == ({0, 1, 2} if maxiter == 6 else {0, 2})
    assert calls == got.evaluations and calls[0] == len(problems) and sum(calls) == int(got.nfev.sum())
    assert got.rounds == int(got.nfev.max())


def test_lockstep_bounds_and_empty():
    from vndecorrelate_amd.bounded import minimize_bounded_lockstep
    out = minimize_bounded_lockstep(lambda lanes, x: x, [], [])
    assert out.x.size == 0 and out.rounds == 0
    with pytest.raises(ValueError, match='lower bound exceeds'):
        minimize_bounded_lockstep(lambda lanes, x: x, [1.0], [0.0])
    with pytest.raises(ValueError, match='finite'):
        minimize_bounded_lockstep(lambda lanes, x: x, [0.0], [np.inf])


def test_rounding_equals_python_round():
    from vndecorrelate_amd.bounded import minimize_bounded_lockstep
    from vndecorrelate_amd.optimization import haas_delays
    seen = []
    rng = np.random.default_rng(9)
    lo = rng.uniform(0, 0.02, 300)
    minimize_bounded_lockstep(lambda lanes, x: seen.append(x.copy()) or np.sin(x * 1e3), lo, lo + 0.0007, xatol=1e-4)
    taus = np.concatenate(seen)
    for fs in (8000, 16000, 44100, 48000, 96000):
        half = [(k + 0.5) / fs for k in range(0, 4000, 7)]
        half = [t for t in half if t * fs == math.floor(t * fs) + 0.5]      # exact ties in float64
        assert len(half) > 100
        values = np.concatenate([taus, half, np.nextafter(half, 0), np.nextafter(half, 1)])
        got = haas_delays(values, fs)
        assert got.dtype == np.int64
        assert got.tolist() == [round(float(t) * fs) for t in values], fs
        assert got.tolist() == [round(np.float64(t) * fs) for t in values], fs


# ---- the driver with the host objective ----------------------------------------------------------------------------
def test_driver_with_host_objective_equals_optimize_haas_delay(golden, host_only):
    gen = generator()
    for name, case in golden['optimize'].items():
        x = gen.fixture_input(case['input'])
        fs, grid = case['sample_rate_hz'], case['grid_size']
        taus = np.linspace(0.0, case['max_delay_seconds'], grid)
        stats = host_only.HaasSearchStats(route='host-scorer', signals=1)
        got = quiet(host_only.haas_search, host_only.host_pair_scorer(x[None], fs, golden['weights']), 1, taus, fs,
                    grid, stats)
        want = quiet(host_only.optimize_haas_delay, input_signal=x, sample_rate_hz=fs,
                     max_delay_seconds=case['max_delay_seconds'], grid_size=grid, **golden['weights'])
        assert got.dtype == np.float64 and got.shape == (1,)
        assert got[0].tobytes() == np.float64(want).tobytes(), name
        assert float(got[0]) == case['tau'], name
        assert stats.evaluations.tolist() == [host_only.last_haas_memo.calls], name
        assert stats.rounds == len(stats.pairs_per_round) and stats.minimum_nfev.sum() == stats.evaluations.sum()


def test_driver_sends_distinct_sorted_pairs_and_scatters_back(host_only):
    """A round's lanes that ask for the same (signal, delay) share one scored pair; the scatter gives each lane its
    own signal's score."""
    fs, grid = 1000, 41
    taus = np.linspace(0.0, 0.04, grid)
    rng = np.random.default_rng(2)
    table = rng.uniform(0, 1, (5, 41))                   # score of (signal, delay)
    table[:, 17] = -1.0                                  # a shared minimum at 17 ms
    table[3, 29] = -2.0
    seen = []

    def scorer(signals, delays):
        key = list(zip(signals.tolist(), delays.tolist()))
        assert key == sorted(set(key))
        seen.append(len(key))
        return table[signals, delays]
    stats = host_only.HaasSearchStats(route='table', signals=5)
    got = quiet(host_only.haas_search, scorer, 5, taus, fs, grid, stats)
    assert seen[0] == 5 * 41 and stats.grid_pairs == 5 * 41
    assert seen[1:] == stats.pairs_per_round and all(p <= 5 * 41 for p in seen[1:])
    for b in range(5):
        want_tau = 0.029 if b == 3 else 0.017
        assert round(got[b] * fs) == round(want_tau * fs), b
    # each signal alone gives the same tau and nfev
    for b in range(5):
        alone = host_only.HaasSearchStats(route='table', signals=1)
        one = quiet(host_only.haas_search, lambda s, d, b=b: table[b + 0 * s, d], 1, taus, fs, grid, alone)
        assert one[0].tobytes() == got[b].tobytes()
        assert alone.minimum_nfev.tolist() == stats.minimum_nfev[stats.minimum_signal == b].tolist()


# ---- header and binding ----------------------------------------------------------------------------------------------
def test_haas_search_header_is_plain_c():
    src = ('#include "vnd_haas_search.h"\nint main(void){int64_t b = 0;\n'
           'return vnd_haas_pairs_workspace_bytes(441000, 16, 1323, &b) == VND_OK && VND_HAAS_PAIRS_MAX > 0 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_haas_search_symbols_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == ['vnd_haas_pairs_f64_dev', 'vnd_haas_pairs_f64_host', 'vnd_haas_pairs_workspace_bytes']
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_haas_search.h but not exported'
    for other in ('vnd_amd.h', 'vnd_scan.h', 'vnd_analysis.h', 'vnd_haas_stream.h'):
        assert not set(names) & set(_declared(REPO / 'include' / other)), other
    assert _native.HAAS_PAIRS_MAX == int(re.search(r'#define VND_HAAS_PAIRS_MAX (\d+)', HEADER.read_text()).group(1))


def test_workspace_query_and_argument_checks(lib):
    from vndecorrelate_amd import _native
    b = ctypes.c_int64(-1)
    assert lib.vnd_haas_pairs_workspace_bytes(441000, 16, 1323, ctypes.byref(b)) == 0
    assert b.value == ((441000 + 1323 + 2047) // 2048) * 16 * 8 * 8
    assert b.value == _native.haas_scan_workspace_bytes(441000, 16, 1323)
    for args in ((-1, 1, 0), (10, -1, 0), (10, 1, -1)):
        assert lib.vnd_haas_pairs_workspace_bytes(*args, ctypes.byref(b)) == 1, args
    # refusals that come before any device work: no context, bad shapes, too many pairs
    assert lib.vnd_haas_pairs_f64_host(None, None, 1, 10, 2, None, None, 1, 0, 0, 0, 0.0, None) == 1
    assert lib.vnd_haas_pairs_f64_dev(None, None, 1, 10, 2, None, None, 1, 0, 0, 0, 0.0, None, None, 0, None) == 1


# ---- routing and shapes ------------------------------------------------------------------------------------------
def _pool(b=3, n=1500, channels=2, seed=0):
    x = np.random.default_rng(seed).uniform(-1, 1, (b, n, channels))
    return x[..., 0].copy() if channels == 1 else x


KW = dict(sample_rate_hz=16000, max_delay_seconds=0.004, grid_size=24)


@pytest.mark.parametrize('channels', [1, 2])
def test_host_route_equals_the_per_signal_loop(channels, monkeypatch):
    from vndecorrelate_amd import analysis, optimization
    monkeypatch.setattr(analysis, '_gpu_present', lambda: False)     # None without a device: the host route
    optimization.set_haas_scan_device(None)
    pool = _pool(channels=channels, seed=channels)
    got = quiet(optimization.optimize_haas_delay_batched, input_signals=pool, **KW)
    want = [quiet(optimization.optimize_haas_delay, input_signal=pool[b], **KW) for b in range(pool.shape[0])]
    assert got.dtype == np.float64 and got.tobytes() == np.asarray(want, np.float64).tobytes()
    assert optimization.last_haas_search.route == 'host' and optimization.last_haas_search.evaluations.size == 3


def test_forced_device_without_one_raises(monkeypatch):
    from vndecorrelate_amd import analysis, optimization
    monkeypatch.setattr(analysis, '_gpu_present', lambda: False)
    optimization.set_haas_scan_device(True)
    try:
        with pytest.raises(RuntimeError, match='no gfx950 device'):
            quiet(optimization.optimize_haas_delay_batched, input_signals=_pool(), **KW)
    finally:
        optimization.set_haas_scan_device(None)


def test_shapes(host_only):
    f = host_only.optimize_haas_delay_batched
    for shape in [(4,), (2, 10, 1), (2, 10, 3), (2, 10, 2, 1), (), (2, 0), (2, 0, 2)]:
        with pytest.raises(ValueError):
            quiet(f, input_signals=np.zeros(shape, np.float32), **KW)
    for empty in [np.zeros((0, 10, 2)), np.zeros((0, 10)), np.zeros((0, 0, 2))]:
        out = f(input_signals=empty, **KW)
        assert out.shape == (0,) and out.dtype == np.float64
    with pytest.raises(TypeError):
        quiet(f, input_signals=np.zeros((2, 10), complex), **KW)
    # any real dtype takes the host route as optimize_haas_delay takes it
    ints = (_pool(b=2, n=800) * 1000).astype(np.int16)
    got = quiet(f, input_signals=ints, **KW)
    assert got.tolist() == [quiet(host_only.optimize_haas_delay, input_signal=ints[b], **KW) for b in range(2)]
