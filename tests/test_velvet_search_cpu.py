"""CPU tier of the batched velvet-noise optimiser (include/vnd_velvet_search.h, optimization.velvet_search,
optimization.optimize_velvet_noise_batched): the header and its binding, the argument checks that come before any
device work, the vectorised bank builder against the per-candidate tables, the search driver with a host scorer
against SciPy lane by lane, and the routing rules - no device call."""
import contextlib
import ctypes
import dataclasses
import io
import pathlib
import re
import subprocess
import warnings

import numpy as np
import pytest

from oracle import vnd_oracle as O

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_velvet_search.h'
WEIGHTS = dict(angle_limit=np.pi / 4, lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0, lambda_penalty=1e3)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


@pytest.fixture
def opt():
    from vndecorrelate_amd import optimization
    yield optimization
    optimization.set_velvet_search_device(None)


# ---- header and binding ----------------------------------------------------------------------------------------------
def test_velvet_search_header_is_plain_c():
    src = ('#include "vnd_velvet_search.h"\nint main(void){int64_t b = 0;\n'
           'return vnd_velvet_pairs_workspace_bytes(441000, 16, &b) == VND_OK && VND_VELVET_PAIRS_MAX > 0\n'
           '       && VND_VELVET_PAIRS_MAX_TAP_INDEX > 0 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_velvet_search_symbols_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == ['vnd_velvet_pairs_f32_dev', 'vnd_velvet_pairs_f32_host', 'vnd_velvet_pairs_workspace_bytes']
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_velvet_search.h but not exported'
        assert getattr(lib, name).argtypes is not None, f'{name} is not bound'
    assert not set(names) & set(_native.SIGNATURES)
    for other in ('vnd_amd.h', 'vnd_scan.h', 'vnd_analysis.h', 'vnd_haas_search.h', 'vnd_stream.h'):
        assert not set(names) & set(_declared(REPO / 'include' / other)), other
    text = HEADER.read_text()
    assert _native.VELVET_PAIRS_MAX == int(re.search(r'#define VND_VELVET_PAIRS_MAX (\d+)', text).group(1))
    assert _native.VELVET_PAIRS_MAX_TAP_INDEX == int(re.search(r'#define VND_VELVET_PAIRS_MAX_TAP_INDEX (\d+)', text).group(1))


def test_workspace_query_and_argument_checks(lib):
    from vndecorrelate_amd import _native
    b = ctypes.c_int64(-1)
    assert lib.vnd_velvet_pairs_workspace_bytes(441000, 16, ctypes.byref(b)) == 0
    assert b.value == ((441000 + 2047) // 2048) * 16 * 8 * 8 == _native.velvet_pairs_workspace_bytes(441000, 16)
    assert _native.VELVET_PAIRS_TILE == 2048
    assert lib.vnd_velvet_pairs_workspace_bytes(0, 16, ctypes.byref(b)) == 0 and b.value == 0
    for args in ((-1, 1), (10, -1)):
        assert lib.vnd_velvet_pairs_workspace_bytes(*args, ctypes.byref(b)) == 1, args
    assert lib.vnd_velvet_pairs_workspace_bytes(10, 1, None) == 1
    # refusals that come before any device work: no context, no bank
    assert lib.vnd_velvet_pairs_f32_host(None, None, None, 1, 10, 2, None, None, 1, 0, None) == 1
    assert lib.vnd_velvet_pairs_f32_dev(None, None, None, 1, 10, 2, None, None, 1, 0, None, None, 0, None) == 1
    assert b'null context' in lib.vnd_last_error()


# ---- the vectorised bank ---------------------------------------------------------------------------------------------
SETTINGS = [(44100, 0.03, 30, 1, None), (48000, 0.03, 30, 7, (1.0,)), (96000, 0.05, 64, 3, (1.0, 0.5, 0.25)),
            (16000, 0.02, 15, 1, None)]


@pytest.mark.parametrize('fs,duration,impulses,seed,envelope', SETTINGS)
def test_vectorised_bank_equals_per_candidate_tables(opt, fs, duration, impulses, seed, envelope):
    from vndecorrelate_amd.decorrelation import VelvetNoise, _draw_taps
    from vndecorrelate_amd.taps import class_path_bank_arrays
    kw = {} if envelope is None else dict(segment_envelope=envelope)
    kappas = np.concatenate([np.linspace(0.0, 1.0, 400), np.random.default_rng(seed).uniform(0, 1, 120), [0.0, 1.0]])
    assert kappas[0] == 0.0
    got = opt.velvet_bank_arrays(kappas, sample_rate_hz=fs, duration_seconds=duration, num_impulses=impulses, seed=seed,
                                 **kw)
    members = [VelvetNoise(sample_rate_hz=fs, duration_seconds=duration, num_impulses=impulses,
                           log_distribution_strength=k, normalizer=None, filtered_channels=(0,), mode='LR', seed=seed,
                           **kw)._tap_member() for k in kappas]
    want = class_path_bank_arrays(members)
    for f in dataclasses.fields(want):
        a, b = getattr(got, f.name), getattr(want, f.name)
        if isinstance(b, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f.name
        else:
            assert type(a) is type(b) and a == b, f.name
    assert got.num_channels == 2 * kappas.size and got.chan_flags.tolist() == [0, 1] * kappas.size
    bank = opt.VelvetBank(sample_rate_hz=fs, duration_seconds=duration, num_impulses=impulses, seed=seed, **kw)
    positions = bank.positions(kappas)
    fir_length = int(round(fs * duration))
    for j in (0, 1, 57, 399, 400, kappas.size - 1):
        ref = _draw_taps(seed, impulses, 1, fir_length, fs, duration, kappas[j])[0][:, 0]
        assert positions.dtype == np.int32 and np.array_equal(positions[j], ref), j


def test_bank_refuses_what_velvet_noise_refuses(opt):
    with pytest.raises(ValueError, match='not sparse'):
        opt.VelvetBank(sample_rate_hz=1000, duration_seconds=0.03, num_impulses=30)
    assert opt.VelvetBank(sample_rate_hz=44100, duration_seconds=0.03, num_impulses=30).arrays([]).num_channels == 0


# ---- the driver with a host scorer against SciPy ----------------------------------------------------------------------
FS, DURATION, IMPULSES, SEED = 16000, 0.02, 15, 1


def _moments(y):
    """float32 element maths as NumPy, float64 sums: the quantities of the device rows."""
    left, right = y[:, 0], y[:, 1]
    th = np.arctan2(left - right, left + right)
    th = np.where(th < -np.pi / 2, th + np.pi, np.where(th > np.pi / 2, th - np.pi, th))
    r = np.sqrt(left**2 + right**2)
    d = np.float64
    return np.array([r.sum(dtype=d), (r * th).sum(dtype=d), (r * th**2).sum(dtype=d), (r * (th**2 * th)).sum(dtype=d),
                     np.max(np.abs(th)), (left * right).sum(dtype=d), (left * left).sum(dtype=d),
                     (right * right).sum(dtype=d)])


class OracleScorer:
    """(signal, table) pairs scored from the oracle: generate_class_taps at a kappa that has the table's key,
    class_convolve, float64-sum moments, scores_from_moments."""

    def __init__(self, opt, pool):
        self.opt, self.pool = opt, pool
        self.bank = opt.VelvetBank(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED)
        self.kappa_of, self.memo, self.calls = {}, {}, []

    def keys(self, values):
        rows = self.bank.keys(values)
        for row, value in zip(rows, np.asarray(values, np.float64).reshape(-1)):
            self.kappa_of.setdefault(row.tobytes(), float(value))
        return rows

    def one(self, signal, key):
        memo = (signal, key.tobytes())
        if memo not in self.memo:
            taps = O.generate_class_taps(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES,
                                         log_distribution_strength=self.kappa_of[key.tobytes()],
                                         filtered_channels=(0,), seed=SEED)
            assert sorted(i for seg in taps[0] for part in seg for i in part) == sorted(key.tolist())
            y = O.class_convolve(self.pool[signal], taps, O.DEFAULT_ENVELOPE, 2)
            self.memo[memo] = float(self.opt.scores_from_moments(_moments(y)[None], **WEIGHTS)[0])
        return self.memo[memo]

    def __call__(self, signals, tables, keys):
        pairs = list(zip(signals.tolist(), tables.tolist()))
        assert pairs == sorted(set(pairs)), 'pairs must be distinct and sorted by (signal, table)'
        assert len({k.tobytes() for k in keys}) == len(keys), 'tables must be distinct'
        assert max(tables.tolist()) < len(keys)
        self.calls.append(len(pairs))
        return np.array([self.one(s, keys[t]) for s, t in pairs])


def _pool(batch=3, n=2500, seed=5):
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1, 1, (batch, n, 1))
    return (base * np.array([1.0, 0.6]) + 0.4 * rng.uniform(-1, 1, (batch, n, 2))).astype(np.float32)


def test_driver_equals_scipy_lane_by_lane(opt):
    from scipy.optimize import minimize_scalar
    grid = 33
    pool = _pool()
    scorer = OracleScorer(opt, pool)
    kappas = np.linspace(0.0, 1.0, grid)
    stats = opt.VelvetSearchStats(route='oracle', signals=pool.shape[0])
    got = quiet(opt.velvet_search, scorer, pool.shape[0], kappas, scorer.keys, grid, stats)
    assert got.dtype == np.float64 and got.shape == (3,)
    distinct = len({k.tobytes() for k in scorer.bank.keys(kappas)})
    assert scorer.calls[0] == 3 * distinct and stats.grid_pairs == 3 * distinct and stats.grid_tables == distinct
    assert scorer.calls[1:] == stats.pairs_per_round and stats.rounds == len(stats.pairs_per_round)
    assert all(t <= p for t, p in zip(stats.tables_per_round, stats.pairs_per_round))
    lane = 0
    for b in range(pool.shape[0]):
        def f(kappa, b=b):
            return scorer.one(b, scorer.keys(np.array([kappa]))[0])
        scores = np.array([f(k) for k in kappas])
        minima = opt.get_local_minima(scores, grid)
        for i in minima:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                want = minimize_scalar(f, bounds=(kappas[max(0, i - 1)], kappas[min(grid - 1, i + 1)]), method='bounded',
                                       options={'xatol': 1e-4})
            assert stats.minimum_signal[lane] == b
            assert stats.minimum_x[lane].tobytes() == np.float64(want.x).tobytes(), (b, i)
            assert stats.minimum_fun[lane].tobytes() == np.float64(want.fun).tobytes(), (b, i)
            assert stats.minimum_nfev[lane] == want.nfev, (b, i)
            lane += 1
        choice = quiet(opt.optimize_local_minima, minima, kappas, grid, f)
        assert got[b].tobytes() == np.float64(choice).tobytes(), b
        assert stats.evaluations[b] == stats.minimum_nfev[stats.minimum_signal == b].sum()
    assert lane == stats.minimum_signal.size
    evaluated = sum(len(k) for _, k in stats.evaluated)
    assert evaluated == stats.evaluations.sum()


def test_driver_sends_distinct_sorted_pairs_and_scatters_back(opt):
    """Lanes of a round that ask for the same (signal, table) share one scored pair; equal keys are one table; the
    scatter gives each lane its own signal's score."""
    grid = 41
    kappas = np.linspace(0.0, 1.0, grid)
    rng = np.random.default_rng(2)
    table = rng.uniform(0, 1, (5, 21))                   # score of (signal, key): keys are round(20 * kappa)
    table[:, 9] = -1.0
    table[3, 13] = -2.0                                  # (keys 9 and 13 each have one grid point: strict minima)
    seen = []

    def keys(values):
        return np.rint(np.asarray(values, np.float64) * 20).astype(np.int32).reshape(-1, 1)

    def scorer(signals, tables, rows):
        pairs = list(zip(signals.tolist(), tables.tolist()))
        assert pairs == sorted(set(pairs)) and rows[:, 0].tolist() == sorted(set(rows[:, 0].tolist()))
        seen.append(len(pairs))
        return table[signals, rows[tables, 0]]
    stats = opt.VelvetSearchStats(route='table', signals=5)
    got = quiet(opt.velvet_search, scorer, 5, kappas, keys, grid, stats)
    assert seen[0] == 5 * 21 and stats.grid_pairs == 5 * 21 and stats.grid_tables == 21
    assert seen[1:] == stats.pairs_per_round
    for b in range(5):
        assert int(keys([got[b]])[0, 0]) == (13 if b == 3 else 9), b
    for b in range(5):                                   # each signal alone: the same kappa and nfev
        alone = opt.VelvetSearchStats(route='table', signals=1)
        one = quiet(opt.velvet_search, lambda s, t, rows, b=b: table[b + 0 * s, rows[t, 0]], 1, kappas, keys, grid, alone)
        assert one[0].tobytes() == got[b].tobytes()
        assert alone.minimum_nfev.tolist() == stats.minimum_nfev[stats.minimum_signal == b].tolist()


# ---- routing and shapes ------------------------------------------------------------------------------------------
KW = dict(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, grid_size=7)


def test_switch_takes_only_booleans_and_none(opt):
    for bad in (1, 'yes', 0.0):
        with pytest.raises(TypeError):
            opt.set_velvet_search_device(bad)


def test_forced_device_without_one_raises(opt, monkeypatch):
    from vndecorrelate_amd import analysis
    monkeypatch.setattr(analysis, '_gpu_present', lambda: False)
    opt.set_velvet_search_device(True)
    with pytest.raises(RuntimeError, match='no gfx950 device'):
        quiet(opt.optimize_velvet_noise_batched, input_signals=_pool(), **KW)


def test_host_route_is_the_per_signal_loop(opt, monkeypatch):
    from vndecorrelate_amd import analysis
    monkeypatch.setattr(analysis, '_gpu_present', lambda: False)     # None without a device: the host route
    calls = []
    monkeypatch.setattr(opt, 'optimize_velvet_noise', lambda **kw: calls.append(kw) or 0.25 * len(calls))
    pool = _pool(n=300)
    got = opt.optimize_velvet_noise_batched(input_signals=pool, **KW)
    assert got.dtype == np.float64 and got.tolist() == [0.25, 0.5, 0.75]
    assert opt.last_velvet_search.route == 'host' and opt.last_velvet_search.signals == 3
    for b, kw in enumerate(calls):
        assert np.array_equal(kw.pop('input_signal'), pool[b]), b
        assert kw == dict(KW, **WEIGHTS)


def test_shapes(opt):
    opt.set_velvet_search_device(False)
    f = opt.optimize_velvet_noise_batched
    for shape in [(4,), (2, 10, 1), (2, 10, 3), (2, 10, 2, 1), (), (2, 0), (2, 0, 2)]:
        with pytest.raises(ValueError) as ours:
            quiet(f, input_signals=np.zeros(shape, np.float32), **KW)
        with pytest.raises(ValueError) as theirs:
            opt._haas_pool(np.zeros(shape, np.float32))
        assert str(ours.value) == str(theirs.value)
    for empty in [np.zeros((0, 10, 2)), np.zeros((0, 10)), np.zeros((0, 0, 2))]:
        out = f(input_signals=empty, **KW)
        assert out.shape == (0,) and out.dtype == np.float64 and opt.last_velvet_search.route == 'none'
    with pytest.raises(TypeError, match='real numbers'):
        quiet(f, input_signals=np.zeros((2, 10), complex), **KW)


# ---- more distinct tables than one tap table holds --------------------------------------------------------------------
def test_scorer_splits_tables_past_one_banks_capacity(opt):
    """A call with more than 32767 distinct tables (a large pool's refinement round, a long filter's grid) goes in
    several banks of at most VELVET_BANK_MAX_CANDIDATES candidates; every pair gets its own table's row back."""
    from vndecorrelate_amd import _native
    limit = _native.VELVET_BANK_MAX_CANDIDATES
    assert limit == 65535 // 2
    banks = []

    class FakeDevice(opt._DeviceVelvetScorer):
        def __init__(self):
            self.weights = WEIGHTS
            self.stats = opt.VelvetSearchStats(route='fake', signals=3)

        def _bank_rows(self, keys, signals, candidates):
            assert 0 < keys.shape[0] <= limit and candidates.min() >= 0 and candidates.max() < keys.shape[0]
            pairs = list(zip(signals.tolist(), candidates.tolist()))
            assert pairs == sorted(pairs), 'a bank keeps the (signal, candidate) order'
            banks.append(keys.shape[0])
            m = np.ones((signals.size, _native.MOMENTS))
            m[:, 2] = 1e-3 * keys[candidates, 0] + 10.0 * signals      # the spread carries (table content, signal)
            return m

    count = 2 * limit + 1000
    keys = np.arange(count, dtype=np.int32)[:, None] % 4000 + np.array([[0, 1]], np.int32) * (np.arange(count)[:, None] // 4000)
    assert len({k.tobytes() for k in keys}) == count and keys.max() <= _native.VELVET_PAIRS_MAX_TAP_INDEX
    rng = np.random.default_rng(1)
    tables = np.sort(rng.choice(count, 50000, replace=False))
    signals = np.concatenate([np.zeros(20000, np.int64), np.ones(20000, np.int64), np.full(10000, 2)])
    order = np.lexsort((tables, signals))
    signals, tables = signals[order], tables[order]
    got = FakeDevice()(signals, tables, keys)
    assert banks == [limit, limit, 1000]
    m = np.ones((signals.size, _native.MOMENTS))
    m[:, 2] = 1e-3 * keys[tables, 0] + 10.0 * signals
    assert got.tobytes() == opt.scores_from_moments(m, **WEIGHTS).tobytes()
    # and through the driver: a grid with more distinct tables than one bank holds
    grid = limit + 500
    kappas = np.linspace(0.0, 1.0, grid)
    banks.clear()

    def table_keys(values):
        return np.rint(np.asarray(values, np.float64) * (grid - 1) * 4).astype(np.int32).reshape(-1, 1) % 4000 \
            + np.array([[0, 1]], np.int32) * (np.rint(np.asarray(values, np.float64) * (grid - 1) * 4).astype(np.int32).reshape(-1, 1) // 4000)
    scorer = FakeDevice()
    stats = opt.VelvetSearchStats(route='fake', signals=2)
    out = quiet(opt.velvet_search, scorer, 2, kappas, table_keys, grid, stats)
    assert stats.grid_tables == grid and banks[:2] == [limit, 500] and out.shape == (2,)


def test_out_of_window_filters_take_the_host_route_before_anything_is_printed(opt, monkeypatch, capsys):
    """A filter whose taps reach past VELVET_PAIRS_MAX_TAP_INDEX is outside the kernel: the call is the host loop, and it
    prints what the host loop prints - the device route's two lines do not come first."""
    from vndecorrelate_amd import analysis
    monkeypatch.setattr(analysis, '_gpu_present', lambda: True)      # the device route is chosen ...
    monkeypatch.setattr(opt, 'optimize_velvet_noise', lambda **kw: print('host search') or 0.5)
    opt.set_velvet_search_device(True)
    got = opt.optimize_velvet_noise_batched(input_signals=_pool(batch=2, n=300), sample_rate_hz=44100, duration_seconds=0.1,
                                            num_impulses=30, seed=1, grid_size=5)           # ... for 4410-frame filters
    assert got.tolist() == [0.5, 0.5] and opt.last_velvet_search.route == 'host'
    assert capsys.readouterr().out == 'host search\nhost search\n'
