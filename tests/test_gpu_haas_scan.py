"""GPU tier of the Haas-delay scan (vnd_haas_scan_f64_*, include/vnd_scan.h): grid_scan's HaasEffect candidates never
reach the host objective, the reference's fixture scores, minima and optimised delays, every moment against float64
NumPy moments of HaasEffect.decorrelate, determinism across runs and launch splits, the device-buffer form on a
non-default stream, and argument checks."""
import contextlib
import io
import json
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / 'tests' / 'golden'
SCORE_REL = 1e-9            # |device - reference| <= SCORE_REL * max(1, |reference|)
SUM_REL = 1e-12             # a moment sum against NumPy's, relative to the sum of its terms' magnitudes
THETA_ABS = 4e-15           # max |theta|: a few ulps of pi/2 (atan2 may differ in the last bit)

CONFIGS = [dict(delayed_channel=c, mode=m, width=w) for c in (0, 1) for m in ('LR', 'MS') for w in (None, 0.35)]


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
def opt():
    from vndecorrelate_amd import _native, optimization
    assert 'gfx950' in _native.default_context().info()['name']
    optimization.set_haas_scan_device(True)
    yield optimization
    optimization.set_haas_scan_device(None)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN / 'haas_scan.npz'), json.loads((GOLDEN / 'haas_scan_manifest.json').read_text())


def candidates(case):
    from vndecorrelate_amd.decorrelation import HaasEffect
    taus = np.linspace(0.0, case['max_delay_seconds'], case['grid_size'])
    return [HaasEffect(sample_rate_hz=case['sample_rate_hz'], delay_time_seconds=t, **case['config']) for t in taus]


def numpy_terms(y):
    """The eight moments' terms of a float64 (n, 2) signal, as the reference's polar_coordinates computes them."""
    l, r = y[:, 0], y[:, 1]
    th = np.arctan2(l - r, l + r)
    th = np.where(th < -np.pi / 2, th + np.pi, np.where(th > np.pi / 2, th - np.pi, th))
    rad = np.sqrt(l ** 2 + r ** 2)
    return [rad, rad * th, rad * th * th, rad * th * th * th, None, l * r, l * l, r * r], th


def check_row(row, y, what):
    terms, th = numpy_terms(y)
    for k, t in enumerate(terms):
        if t is None:
            want = float(np.max(np.abs(th))) if th.size else 0.0
            assert abs(row[4] - want) <= THETA_ABS, (what, k, row[4], want)
            continue
        bound = SUM_REL * float(np.sum(np.abs(t))) + 1e-300
        assert abs(row[k] - float(np.sum(t))) <= bound, (what, k, row[k], float(np.sum(t)), bound)


def test_grid_scan_never_calls_the_host_objective(opt, monkeypatch):
    from vndecorrelate_amd.decorrelation import HaasEffect

    def boom(*a, **k):
        raise AssertionError('symmetry_aware_objective was called')
    monkeypatch.setattr(opt, 'symmetry_aware_objective', boom)
    x = np.random.default_rng(0).uniform(-1, 1, (4000, 2)).astype(np.float32)
    cands = [HaasEffect(sample_rate_hz=16000, delay_time_seconds=t, **cfg)
             for cfg in CONFIGS for t in np.linspace(0, 0.01, 9)]
    kw = dict(angle_limit=float(np.pi / 4), lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0, lambda_penalty=1e3)
    scores = quiet(opt.grid_scan, x, cands, **kw)
    assert scores.shape == (len(cands),) and np.all(np.isfinite(scores))
    mono = quiet(opt.grid_scan, x[:, 0].copy(), cands, **kw)
    assert np.all(np.isfinite(mono))


def test_fixture_scores_and_minima(opt, golden):
    g, m = golden
    gen = generator()
    worst = 0.0
    for name, case in m['scans'].items():
        x = gen.fixture_input(case['input'])
        got = quiet(opt.grid_scan, x, candidates(case), **m['weights'])
        ref = g[f'{name}__scores']
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(err.max()))
        assert err.max() <= SCORE_REL, (name, float(err.max()))
        assert np.array_equal(opt.get_local_minima(got, case['grid_size']), g[f'{name}__minima']), name
    print(f'worst score error: {worst:.3e} of max(1, |ref|)')


def test_optimize_haas_delay_returns_the_reference_tau(opt, golden):
    _, m = golden
    gen = generator()
    for name, case in m['optimize'].items():
        tau = quiet(opt.optimize_haas_delay, input_signal=gen.fixture_input(case['input']),
                    sample_rate_hz=case['sample_rate_hz'], max_delay_seconds=case['max_delay_seconds'],
                    grid_size=case['grid_size'], **m['weights'])
        assert float(tau) == case['tau'], name
        assert opt.last_haas_memo.evaluations <= opt.last_haas_memo.calls


@pytest.mark.parametrize('n,channels', [(1, 1), (1, 2), (3, 2), (777, 1), (2048, 2), (2049, 1), (65541, 2),
                                        (1_000_003, 2), (999_999, 1)])
def test_moments_match_numpy(opt, n, channels):
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.decorrelation import HaasEffect
    rng = np.random.default_rng(n * 3 + channels)
    x = rng.uniform(-1, 1, (n, channels)).astype(np.float32)
    if n > 100:
        x[n // 4: n // 3] = 0.0                                 # a silent stretch
        x[n // 2: n // 2 + 7] = -0.0
    sig = x[:, 0] if channels == 1 else x
    delays = np.unique(np.concatenate([[0, 1, 2000], rng.integers(0, 2001, 5)]))
    configs = CONFIGS if n < 100_000 else CONFIGS[::3]
    for cfg in configs:
        got = _native.haas_scan_host(_native.default_context(), x, delays, delayed_channel=cfg['delayed_channel'],
                                     ms_mode=cfg['mode'] == 'MS', width=cfg['width'])
        for row, d in zip(got, delays):
            y = HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d), **cfg).decorrelate(sig)
            assert y.shape == (n + d, 2)
            check_row(row, y, (n, channels, cfg, int(d)))


def test_unstaged_blocks_and_any_order(opt):
    """Delays more than a tile apart in one block read the delayed column from global memory: the same bits."""
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    x = np.random.default_rng(7).uniform(-1, 1, (50_000, 2)).astype(np.float32)
    wide = np.array([0, 4500, 3000, 17, 9000, 1], np.int64)
    together = _native.haas_scan_host(ctx, x, wide, delayed_channel=1, ms_mode=True, width=0.5)
    for i, d in enumerate(wide):
        alone = _native.haas_scan_host(ctx, x, [d], delayed_channel=1, ms_mode=True, width=0.5)
        assert np.array_equal(alone[0], together[i]), int(d)
    from vndecorrelate_amd.decorrelation import HaasEffect
    for i, d in enumerate(wide):
        y = HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d), delayed_channel=1, mode='MS', width=0.5).decorrelate(x)
        check_row(together[i], y, int(d))


def test_bit_identical_across_runs_and_launch_splits(opt):
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (300_001, 2)).astype(np.float32)
    delays = np.unique(rng.integers(0, 1400, 120))
    kw = dict(delayed_channel=0, ms_mode=False, width=None)
    a = _native.haas_scan_host(ctx, x, delays, **kw)
    assert np.array_equal(a, _native.haas_scan_host(ctx, x, delays, **kw))
    cuts = [0, 1, 17, 40, 41, 99, delays.size]
    pieces = np.concatenate([_native.haas_scan_host(ctx, x, delays[p:q], **kw) for p, q in zip(cuts, cuts[1:])])
    assert np.array_equal(a, pieces)
    perm = rng.permutation(delays.size)
    assert np.array_equal(a[perm], _native.haas_scan_host(ctx, x, delays[perm], **kw))
    moments = opt.scan_haas_moments(x, [opt.HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d)) for d in delays])
    assert np.array_equal(a, moments)


def test_device_buffers_on_a_side_stream(opt):
    import torch
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (123_457, 1)).astype(np.float32)
    delays = np.array([0, 5, 700, 1323, 2000], np.int32)
    want = _native.haas_scan_host(ctx, x, delays, delayed_channel=1, ms_mode=True, width=None)
    ws = _native.haas_scan_workspace_bytes(x.shape[0], delays.size, int(delays.max()))
    dev = torch.device('cuda:0')
    xd = torch.from_numpy(x).to(dev)
    dd = torch.from_numpy(delays).to(dev)
    md = torch.full((delays.size, _native.MOMENTS), -1.0, dtype=torch.float64, device=dev)
    wd = torch.empty(ws, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _native.haas_scan_device(ctx, xd.data_ptr(), x.shape[0], 1, dd.data_ptr(), delays.size, md.data_ptr(),
                                 delayed_channel=1, ms_mode=True, width=None, workspace_ptr=wd.data_ptr(),
                                 workspace_bytes=ws, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(md.cpu().numpy(), want)
    # a delay above what the workspace was sized for, and a negative one: NaN rows, the others unchanged
    bad = torch.tensor([0, 2001 + 2048, -3, 700], dtype=torch.int32, device=dev)
    ws4 = _native.haas_scan_workspace_bytes(x.shape[0], 4, 2000)
    wd4 = torch.empty(ws4, dtype=torch.uint8, device=dev)
    m4 = torch.zeros((4, _native.MOMENTS), dtype=torch.float64, device=dev)
    with torch.cuda.stream(side):
        _native.haas_scan_device(ctx, xd.data_ptr(), x.shape[0], 1, bad.data_ptr(), 4, m4.data_ptr(),
                                 delayed_channel=1, ms_mode=True, width=None, workspace_ptr=wd4.data_ptr(),
                                 workspace_bytes=ws4, stream=side.cuda_stream)
    side.synchronize()
    got = m4.cpu().numpy()
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[2])


def test_invalid_arguments(opt):
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    lib = _native.load_library()
    x = np.zeros((10, 2), np.float32)
    with pytest.raises(ValueError, match='negative'):
        _native.haas_scan_host(ctx, x, [0, -1], delayed_channel=0, ms_mode=False, width=None)
    with pytest.raises(ValueError, match='mono or stereo'):
        _native.haas_scan_host(ctx, np.zeros((10, 3), np.float32), [0], delayed_channel=0, ms_mode=False, width=None)
    with pytest.raises(ValueError, match='delayed_channel'):
        _native.haas_scan_host(ctx, x, [0], delayed_channel=2, ms_mode=False, width=None)
    with pytest.raises(ValueError):
        _native.haas_scan_workspace_bytes(10, 1, -1)
    with pytest.raises(ValueError):
        _native.haas_scan_workspace_bytes(-1, 1, 0)
    d = np.zeros(1, np.int32)
    m = np.zeros((1, 8))
    import ctypes
    rc = lib.vnd_haas_scan_f64_host(ctx.handle, _native._ptr(x, ctypes.c_float), -1, 2, _native._ptr(d, ctypes.c_int32),
                                    1, 0, 0, 0, 0.0, _native._ptr(m, ctypes.c_double))
    assert rc == 1 and b'negative' in lib.vnd_last_error()
    for args in ((-1, 2, 0), (10, 0, 0), (10, 2, 5)):       # n_frames, in_channels, delayed_channel
        rc = lib.vnd_haas_scan_f64_dev(ctx.handle, None, args[0], args[1], None, 1, args[2], 0, 0, 0.0, None, None, 0,
                                       None)
        assert rc == 1, args
    rc = lib.vnd_haas_scan_f64_dev(ctx.handle, None, 10, 2, None, 1, 0, 0, 0, 0.0, None, None, 0, None)
    assert rc == 1 and b'null' in lib.vnd_last_error()
    rc = lib.vnd_haas_scan_f64_dev(ctx.handle, None, 10, 2, None, 1, 0, 0, 0, 0.0, None, None, -8, None)
    assert rc == 1
    rc = lib.vnd_haas_scan_f64_dev(ctx.handle, None, 10, 2, None, 1048561, 0, 0, 0, 0.0, None, None, 0, None)
    assert rc == 4
    assert np.array_equal(_native.haas_scan_host(ctx, x, [], delayed_channel=0, ms_mode=False, width=None),
                          np.zeros((0, 8)))


def test_mixed_candidates_take_both_routes(opt):
    from vndecorrelate_amd.decorrelation import HaasEffect, VelvetNoise
    x = np.random.default_rng(48).uniform(-1, 1, (20000, 2)).astype(np.float32)
    kw = dict(angle_limit=float(np.pi / 4), lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0, lambda_penalty=1e3)
    cands = [VelvetNoise(sample_rate_hz=48000, seed=1),
             HaasEffect(sample_rate_hz=48000, delay_time_seconds=0.01, mode='LR'),
             HaasEffect(sample_rate_hz=48000, delay_time_seconds=0.004, mode='MS', width=np.float32(0.5)),
             HaasEffect(sample_rate_hz=48000, delay_time_seconds=0.002, delayed_channel=1)]
    got = quiet(opt.grid_scan, x, cands, **kw)
    for i, c in enumerate(cands):
        ref = opt.symmetry_aware_objective(x, c, **kw)
        assert abs(got[i] - ref) <= SCORE_REL * max(1.0, abs(ref)), i
    with pytest.raises(ValueError):
        quiet(opt.grid_scan, np.zeros((50, 3), np.float32), cands[1:], **kw)
