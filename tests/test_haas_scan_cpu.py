"""CPU tier of the Haas-delay scan: the reference's fixture (sha256), the routing rule, the delay dedupe and its
scatter back, the host route against the reference bit for bit, and the refinement's memo."""
import contextlib
import hashlib
import io
import json
import pathlib

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / 'tests' / 'golden'


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_haas_scan_golden', REPO / 'tools' / 'gen_haas_scan_golden.py')
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN / 'haas_scan.npz'), json.loads((GOLDEN / 'haas_scan_manifest.json').read_text())


@pytest.fixture
def host_only():
    from vndecorrelate_amd import optimization
    optimization.set_haas_scan_device(False)
    yield optimization
    optimization.set_haas_scan_device(None)


def candidates(case):
    from vndecorrelate_amd.decorrelation import HaasEffect
    taus = np.linspace(0.0, case['max_delay_seconds'], case['grid_size'])
    return [HaasEffect(sample_rate_hz=case['sample_rate_hz'], delay_time_seconds=t, **case['config']) for t in taus]


def test_manifest_matches_the_arrays(golden):
    g, m = golden
    assert (GOLDEN / 'haas_scan.npz').stat().st_size < 1 << 20
    names = set()
    for name, case in m['scans'].items():
        for part in ('scores', 'minima'):
            assert sha(g[f'{name}__{part}']) == case['sha256'][part], (name, part)
            names.add(f'{name}__{part}')
        assert g[f'{name}__scores'].shape == (case['grid_size'],)
    assert names == set(g.files)
    assert any(c['distinct_delays'] < c['grid_size'] for c in m['scans'].values())
    configs = {(c['config']['mode'], c['config']['delayed_channel'], c['config']['width'] is None, c['input']['kind'])
               for c in m['scans'].values()}
    assert {(mode, ch) for mode, ch, _, _ in configs} == {('LR', 0), ('LR', 1), ('MS', 0), ('MS', 1)}
    assert {k for _, _, _, k in configs} == {'mono', 'stereo', 'stereo_zeros'}
    assert {w for _, _, w, _ in configs} == {True, False}
    for case in m['optimize'].values():
        assert float.fromhex(case['tau_hex']) == case['tau']


def test_zero_recipe_has_signed_zeros(golden):
    _, m = golden
    x = generator().fixture_input(m['scans']['lr_c0_zeros']['input'])
    assert x.dtype == np.float32 and x.shape == (3000, 2)
    assert np.all(x[1200:1700] == 0) and np.all(np.signbit(x[300:340]))
    assert np.signbit(x[400, 0]) and not np.signbit(x[400, 1])
    assert not np.signbit(x[420, 0]) and np.signbit(x[420, 1])


def test_routing_predicate():
    from vndecorrelate_amd.decorrelation import HaasEffect, VelvetNoise
    from vndecorrelate_amd.optimization import haas_scan_covers
    h = HaasEffect(sample_rate_hz=48000, delay_time_seconds=0.01)
    assert haas_scan_covers(np.zeros(10, np.float32), h)
    assert haas_scan_covers(np.zeros((10, 2), np.float32), h)
    assert haas_scan_covers(np.zeros((10, 2), np.float64), h)
    assert haas_scan_covers(np.zeros((1, 2), np.float32), h)
    for shape in [(0,), (0, 2), (10, 1), (10, 3), (10, 2, 2), ()]:
        assert not haas_scan_covers(np.zeros(shape, np.float32), h), shape
    x = np.zeros((10, 2), np.float32)
    for kw in (dict(mode='MS'), dict(delayed_channel=1), dict(width=0.5), dict(width=1), dict(width=np.float64(0.2)),
               dict(delay_time_seconds=0.0)):
        assert haas_scan_covers(x, HaasEffect(sample_rate_hz=48000, **kw)), kw
    for kw in (dict(delayed_channel=2), dict(delayed_channel=True), dict(mode='XY'), dict(width=np.float32(0.5)),
               dict(width=float('nan')), dict(delay_time_seconds=-0.01), dict(delay_time_seconds=1e6)):
        assert not haas_scan_covers(x, HaasEffect(sample_rate_hz=48000, **kw)), kw
    assert not haas_scan_covers(x, VelvetNoise(sample_rate_hz=48000, seed=1))

    class Sub(HaasEffect):
        pass
    assert not haas_scan_covers(x, Sub(sample_rate_hz=48000))


def test_without_the_device_route_nothing_reaches_the_kernel(monkeypatch, host_only):
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.decorrelation import HaasEffect

    def boom(*a, **k):
        raise AssertionError('the device route was taken')
    monkeypatch.setattr(_native, 'haas_scan_host', boom)
    x = np.random.default_rng(0).uniform(-1, 1, (500, 2)).astype(np.float32)
    cands = [HaasEffect(sample_rate_hz=16000, delay_time_seconds=t) for t in (0.0, 0.001, 0.002)]
    kw = dict(angle_limit=0.7, lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0, lambda_penalty=1e3)
    got = quiet(host_only.grid_scan, x, cands, **kw)
    assert np.array_equal(got, [host_only.symmetry_aware_objective(x, c, **kw) for c in cands])
    with pytest.raises(ValueError):                       # (n, 3): the host path and its exception, as upstream
        quiet(host_only.grid_scan, np.zeros((50, 3), np.float32), cands, **kw)


def test_dedupe_and_scatter_keep_candidate_order(monkeypatch):
    from vndecorrelate_amd import _native, optimization
    from vndecorrelate_amd.decorrelation import HaasEffect
    calls = []

    def fake(ctx, x, delays, *, delayed_channel, ms_mode, width):
        delays = np.asarray(delays)
        calls.append((delays.copy(), delayed_channel, ms_mode, width))
        assert np.all(np.diff(delays) > 0)                # distinct and ascending
        rows = np.zeros((delays.size, _native.MOMENTS))
        rows[:, 0] = delays
        rows[:, 1] = delayed_channel + 10 * ms_mode + 100 * (width or 0)
        return rows
    monkeypatch.setattr(_native, 'haas_scan_host', fake)
    monkeypatch.setattr(_native, 'default_context', lambda: None)
    fs = 8000
    taus = list(np.linspace(0.0, 0.005, 300))
    cands = [HaasEffect(sample_rate_hz=fs, delay_time_seconds=t) for t in taus[::-1]]
    cands += [HaasEffect(sample_rate_hz=fs, delay_time_seconds=t, mode='MS', delayed_channel=1, width=0.5)
              for t in taus[::7]]
    x = np.zeros((100, 2), np.float32)
    got = optimization.scan_haas_moments(x, cands)
    assert len(calls) == 2
    assert sum(c[0].size for c in calls) == len({round(t * fs) for t in taus}) + len({round(t * fs) for t in taus[::7]})
    for i, c in enumerate(cands):
        assert got[i, 0] == round(c.delay_time_seconds * fs)
        assert got[i, 1] == (0 if c.mode == 'LR' else 1 + 10 + 50)


def test_host_route_equals_the_reference_bit_for_bit(golden, host_only):
    g, m = golden
    gen = generator()
    for name, case in m['scans'].items():
        x = gen.fixture_input(case['input'])
        got = quiet(host_only.grid_scan, x, candidates(case), **m['weights'])
        assert np.array_equal(got, g[f'{name}__scores']), name
        assert np.array_equal(host_only.get_local_minima(got, case['grid_size']), g[f'{name}__minima']), name


def test_optimize_haas_delay_on_the_host_equals_the_reference(golden, host_only):
    _, m = golden
    gen = generator()
    for name, case in m['optimize'].items():
        tau = quiet(host_only.optimize_haas_delay, input_signal=gen.fixture_input(case['input']),
                    sample_rate_hz=case['sample_rate_hz'], max_delay_seconds=case['max_delay_seconds'],
                    grid_size=case['grid_size'], **m['weights'])
        assert float(tau) == case['tau'], name


def test_the_memo_returns_the_unmemoised_tau(golden, host_only):
    _, m = golden
    gen = generator()
    for name, case in m['optimize'].items():
        x = gen.fixture_input(case['input'])
        fs, grid = case['sample_rate_hz'], case['grid_size']
        taus = np.linspace(0.0, case['max_delay_seconds'], grid)

        def make(t):
            return host_only.HaasEffect(sample_rate_hz=fs, delay_time_seconds=t, mode='LR')

        def plain(t):
            return host_only.symmetry_aware_objective(x, make(t), **m['weights'])
        scores = quiet(host_only.grid_scan, x, [make(t) for t in taus], **m['weights'])
        minima = host_only.get_local_minima(scores, grid)
        memo = host_only.DelayMemo(plain, fs)
        want = quiet(host_only.optimize_local_minima, minima, taus, grid, plain)
        got = quiet(host_only.optimize_local_minima, minima, taus, grid, memo)
        assert float(got) == float(want), name
        assert memo.evaluations <= memo.calls


def test_memo_counts_saved_evaluations():
    from vndecorrelate_amd.optimization import DelayMemo
    seen = []
    memo = DelayMemo(lambda t: seen.append(t) or float(round(t * 100)), 100)
    assert [memo(t) for t in (0.011, 0.012, 0.0149, 0.02, 0.0201)] == [1.0, 1.0, 1.0, 2.0, 2.0]
    assert memo.calls == 5 and memo.evaluations == 2 and seen == [0.011, 0.02]
