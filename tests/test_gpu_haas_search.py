"""GPU tier of the batched Haas-delay optimiser (vnd_haas_pairs_f64_*, include/vnd_haas_search.h, and
optimize_haas_delay_batched): pairs moments against the single-signal scan bit for bit, bad pairs, the device-buffer
form on a side stream, the reference's tau alone and inside pools, the device scorer through SciPy, batch
independence, and that the work stays on the device."""
import contextlib
import ctypes
import io
import json
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = REPO / 'tests' / 'golden'
CONFIGS = [dict(delayed_channel=c, mode=m, width=w) for c in (0, 1) for m in ('LR', 'MS') for w in (None, 0.35)]


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def generator():
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_haas_scan_golden', REPO / 'tools' / 'gen_haas_scan_golden.py')
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


@pytest.fixture(scope='module')
def opt():
    from vndecorrelate_amd import _native, optimization
    assert 'gfx950' in _native.default_context().info()['name']
    optimization.set_haas_scan_device(True)
    yield optimization
    optimization.set_haas_scan_device(None)


@pytest.fixture(scope='module')
def golden():
    return json.loads((GOLDEN / 'haas_scan_manifest.json').read_text())


def _kw(cfg):
    return dict(delayed_channel=cfg['delayed_channel'], ms_mode=cfg['mode'] == 'MS', width=cfg['width'])


@pytest.mark.parametrize('channels', [1, 2])
def test_pairs_equal_the_single_signal_scan(opt, channels):
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    rng = np.random.default_rng(40 + channels)
    B, n = 5, 9001
    pool = rng.uniform(-1, 1, (B, n, channels)).astype(np.float32)
    pool[2, 1000:3000] = 0.0
    delays = np.array([0, 1, 2, 17, 300, 2047, 2048, 2049, 4500, 9000, 13000], np.int64)   # 9000, 13000: unstaged
    for cfg in CONFIGS:
        want = {s: _native.haas_scan_host(ctx, np.ascontiguousarray(pool[s]), delays, **_kw(cfg)) for s in range(B)}
        sig = np.repeat(np.arange(B), delays.size)
        dl = np.tile(delays, B)
        perm = rng.permutation(sig.size)
        sig = np.concatenate([sig[perm], sig[:9]])                       # shuffled, with duplicate pairs
        dl = np.concatenate([dl[perm], dl[:9]])
        got = _native.haas_pairs_host(ctx, pool, sig, dl, **_kw(cfg))
        for p, (s, d) in enumerate(zip(sig, dl)):
            assert got[p].tobytes() == want[s][list(delays).index(d)].tobytes(), (cfg, channels, int(s), int(d))
        cuts = [0, 1, 16, 17, 40, sig.size]                              # split across launches
        parts = np.concatenate([_native.haas_pairs_host(ctx, pool, sig[a:b], dl[a:b], **_kw(cfg))
                                for a, b in zip(cuts, cuts[1:])])
        assert parts.tobytes() == got.tobytes(), cfg


def test_bad_pairs(opt):
    import torch
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    lib = _native.load_library()
    rng = np.random.default_rng(8)
    B, n = 3, 7000
    pool = rng.uniform(-1, 1, (B, n, 2)).astype(np.float32)
    kw = dict(delayed_channel=0, ms_mode=False, width=None)
    for sig, dl in (([0, 3], [5, 5]), ([0, -1], [5, 5]), ([1, 1], [5, -2])):
        with pytest.raises(ValueError):
            _native.haas_pairs_host(ctx, pool, sig, dl, **kw)
    m = np.zeros((1, 8))
    s = np.array([3], np.int32)
    d = np.array([5], np.int32)
    rc = lib.vnd_haas_pairs_f64_host(ctx.handle, _native._ptr(pool, ctypes.c_float), B, n, 2,
                                     _native._ptr(s, ctypes.c_int32), _native._ptr(d, ctypes.c_int32), 1, 0, 0, 0, 0.0,
                                     _native._ptr(m, ctypes.c_double))
    assert rc == 1 and b'outside' in lib.vnd_last_error() and not m.any()
    # on _dev: NaN rows for a bad signal, a negative delay or one above the workspace; the others as alone
    dev = torch.device('cuda', ctx.device)
    xd = torch.from_numpy(pool).to(dev)
    sig = np.array([0, 3, 1, -1, 2, 1, 2], np.int32)
    dl = np.array([0, 10, -3, 10, 700 + 4096, 700, 9], np.int32)
    sd, dd = torch.from_numpy(sig).to(dev), torch.from_numpy(dl).to(dev)
    ws = _native.haas_pairs_workspace_bytes(n, sig.size, 700)
    wd = torch.empty(ws, dtype=torch.uint8, device=dev)
    md = torch.zeros((sig.size, 8), dtype=torch.float64, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _native.haas_pairs_device(ctx, xd.data_ptr(), B, n, 2, sd.data_ptr(), dd.data_ptr(), sig.size, md.data_ptr(),
                                  workspace_ptr=wd.data_ptr(), workspace_bytes=ws, stream=side.cuda_stream, **kw)
    side.synchronize()
    got = md.cpu().numpy()
    for p in (1, 2, 3, 4):
        assert np.isnan(got[p]).all(), p
    for p in (0, 5, 6):
        want = _native.haas_scan_host(ctx, np.ascontiguousarray(pool[sig[p]]), [dl[p]], **kw)
        assert got[p].tobytes() == want[0].tobytes(), p


def test_reference_tau_alone_and_in_pools(opt, golden):
    gen = generator()
    for name, case in golden['optimize'].items():
        x = gen.fixture_input(case['input'])
        kw = dict(sample_rate_hz=case['sample_rate_hz'], max_delay_seconds=case['max_delay_seconds'],
                  grid_size=case['grid_size'], **golden['weights'])
        alone = quiet(opt.optimize_haas_delay_batched, input_signals=x[None], **kw)
        assert alone.shape == (1,) and float(alone[0]) == case['tau'], name
        others = np.random.default_rng(len(name)).uniform(-1, 1, (7,) + x.shape).astype(x.dtype)
        for at in (0, 3, 7):
            pool = np.insert(others, at, x, axis=0)
            got = quiet(opt.optimize_haas_delay_batched, input_signals=pool, **kw)
            assert float(got[at]) == case['tau'], (name, at)


def test_device_scorer_through_scipy(opt):
    """tau and each minimum's nfev equal optimize_local_minima driven through SciPy one tau at a time by the same
    device score of round(tau * fs)."""
    from scipy.optimize import minimize_scalar
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    weights = dict(angle_limit=float(np.pi / 4), lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0,
                   lambda_penalty=1e3)
    fs, max_delay, grid = 16000, 0.01, 40
    pool = np.random.default_rng(77).uniform(-1, 1, (16, 3000, 2)).astype(np.float32)
    pool[5, :, 1] = pool[5, :, 0]                                        # a correlated one
    got = quiet(opt.optimize_haas_delay_batched, input_signals=pool, sample_rate_hz=fs, max_delay_seconds=max_delay,
                grid_size=grid, **weights)
    stats = opt.last_haas_search
    taus = np.linspace(0.0, max_delay, grid)
    for b in range(pool.shape[0]):
        def f(t, b=b):
            m = _native.haas_scan_host(ctx, pool[b], [round(t * fs)], delayed_channel=0, ms_mode=False, width=None)
            return opt.scores_from_moments(m, **weights)[0]
        cands = [opt.HaasEffect(sample_rate_hz=fs, delay_time_seconds=t, mode='LR') for t in taus]
        scores = quiet(opt.grid_scan, pool[b], cands, **weights)
        minima = opt.get_local_minima(scores, grid)
        nfev, best, best_tau = [], np.inf, 0.0
        for i in minima:
            r = minimize_scalar(f, bounds=(taus[max(0, i - 1)], taus[min(grid - 1, i + 1)]), method='bounded',
                                options={'xatol': 1e-4})
            nfev.append(r.nfev)
            if r.fun < best:
                best, best_tau = r.fun, r.x
        assert got[b].tobytes() == np.float64(best_tau).tobytes(), b
        assert stats.minimum_nfev[stats.minimum_signal == b].tolist() == nfev, b
        assert stats.evaluations[b] == sum(nfev)


def test_batch_independence_and_chunking(opt, monkeypatch):
    kw = dict(sample_rate_hz=8000, max_delay_seconds=0.02, grid_size=50)
    pool = np.random.default_rng(5).uniform(-1, 1, (9, 2500, 2))
    full = quiet(opt.optimize_haas_delay_batched, input_signals=pool, **kw)
    assert opt.last_haas_search.pool_uploads == 1
    perm = np.random.default_rng(6).permutation(9)
    shuffled = quiet(opt.optimize_haas_delay_batched, input_signals=pool[perm], **kw)
    assert shuffled.tobytes() == full[perm].tobytes()
    part = quiet(opt.optimize_haas_delay_batched, input_signals=pool[2:5], **kw)
    assert part.tobytes() == full[2:5].tobytes()
    monkeypatch.setattr(opt, '_HAAS_POOL_BYTES', 2 * 2500 * 2 * 4)       # two signals per chunk
    chunked = quiet(opt.optimize_haas_delay_batched, input_signals=pool, **kw)
    assert opt.last_haas_search.pool_uploads == 5
    assert chunked.tobytes() == full.tobytes()
    mono = quiet(opt.optimize_haas_delay_batched, input_signals=pool[..., 0], **kw)
    for b in (0, 4):
        alone = quiet(opt.optimize_haas_delay_batched, input_signals=pool[b:b + 1, :, 0], **kw)
        assert alone[0].tobytes() == mono[b].tobytes()


def test_work_stays_on_the_device(opt, monkeypatch):
    import torch
    from vndecorrelate_amd import _native

    def boom(*a, **k):
        raise AssertionError('symmetry_aware_objective was called')
    monkeypatch.setattr(opt, 'symmetry_aware_objective', boom)
    launches = []
    real = _native.haas_pairs_device

    def spy(ctx, x_ptr, batch, n, channels, signals_ptr, delays_ptr, n_pairs, *a, **k):
        launches.append((x_ptr, batch, n, channels, n_pairs))
        return real(ctx, x_ptr, batch, n, channels, signals_ptr, delays_ptr, n_pairs, *a, **k)
    monkeypatch.setattr(_native, 'haas_pairs_device', spy)
    kw = dict(sample_rate_hz=16000, max_delay_seconds=0.01, grid_size=40)
    pool = np.random.default_rng(12).uniform(-1, 1, (6, 4000, 2)).astype(np.float32)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        got = opt.optimize_haas_delay_batched(input_signals=pool, **kw)
    assert out.getvalue() == 'Starting Grid Scan\nStarting Local Minima optimization\n'
    stats = opt.last_haas_search
    assert stats.route == 'device' and stats.pool_uploads == 1
    assert len({l[0] for l in launches}) == 1                           # one resident pool
    assert len(launches) == 1 + stats.rounds                            # the grid, then one launch per round
    assert [l[4] for l in launches] == [stats.grid_pairs] + stats.pairs_per_round
    assert all(l[1:4] == (6, 4000, 2) for l in launches)
    # a device tensor is read in place: no upload, the same pointer in every launch
    launches.clear()
    xd = torch.from_numpy(pool).to(torch.device('cuda', _native.default_context().device))
    again = quiet(opt.optimize_haas_delay_batched, input_signals=xd, **kw)
    assert again.tobytes() == got.tobytes()
    assert opt.last_haas_search.pool_uploads == 0 and {l[0] for l in launches} == {xd.data_ptr()}
