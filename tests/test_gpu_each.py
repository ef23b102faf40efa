"""GPU tier of decorrelate_each (vnd_convolve_each_f32_*, vnd_decorrelate_each_f32_*, vnd_haas_each_f64_*,
include/vnd_each.h): a pool through one filter or one delay per signal.  Every comparison is bit for bit: the frames
against the oracle's class-path and function-path convolutions and against the per-signal entry points, the stage
against the loop of VelvetNoise.decorrelate with NumPy's epilogue and against the oracle's decorrelate, the independence
contract, the bounds, the Haas rows against NumPy's HaasEffect, the optimisers' results applied, and residency."""
import contextlib
import io

import numpy as np
import pytest

from oracle import vnd_oracle as O

pytestmark = pytest.mark.gpu

FS, DURATION, IMPULSES, SEED = 16000, 0.02, 15, 1        # a small filter: 320 frames, 15 taps
TILE = 2048
SIZES = (1, 200, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5000)   # 200: shorter than the largest tap index


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


@pytest.fixture(scope='module')
def ctx():
    from vndecorrelate_amd import _native
    context = _native.default_context()
    assert 'gfx950' in context.info()['name']
    return context


@pytest.fixture
def dec(ctx):
    import vndecorrelate_amd.decorrelation as decorrelation
    decorrelation.set_each_device(True)
    yield decorrelation
    decorrelation.set_each_device(None)
    decorrelation.set_device_epilogue(None)


def _taps(kappa, *, filtered=(0,), envelope=O.DEFAULT_ENVELOPE, seed=SEED):
    return O.generate_class_taps(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES,
                                 segment_envelope=envelope, log_distribution_strength=kappa,
                                 filtered_channels=filtered, seed=seed)


def _class_bank(ctx, members, envelope):
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import class_path_bank_arrays
    env = tuple(envelope)
    arrays = class_path_bank_arrays([(taps, env, env != (1.0,)) for taps in members])
    return _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight, **arrays.kwargs())


def _stereo(x):
    return np.repeat(x, 2, axis=1) if x.shape[1] == 1 else x


def _noise(rng, shape):
    return rng.uniform(-1, 1, shape).astype(np.float32)


# ---- 1. frames -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('envelope', [(1.0,), (1.0, 0.5, 0.25)])
def test_frames_are_the_oracles_and_the_per_signal_entrys(ctx, channels, envelope):
    from vndecorrelate_amd import _native
    rng = np.random.default_rng(100 + channels + len(envelope))
    members = [_taps(0.0, envelope=envelope), _taps(0.4, envelope=envelope), _taps(1.0, envelope=envelope),
               _taps(0.7, filtered=(0, 1), envelope=envelope, seed=5),        # both channels filtered
               _taps(0.2, filtered=(0, 1), envelope=envelope, seed=9)]
    bank = _class_bank(ctx, members, envelope)
    alone = [_class_bank(ctx, [m], envelope) for m in members]
    try:
        assert bank.max_index > 200
        for i, n in enumerate(SIZES):
            pool = _noise(rng, (5, n, channels))
            tables = np.roll(np.array([3, 0, 4, 1, 2]), i)
            got = _native.convolve_each_host(ctx, bank, pool, tables)
            assert got.shape == (5, n, 2) and got.dtype == np.float32
            for b, t in enumerate(tables):
                want = O.class_convolve(_stereo(pool[b]), members[t], envelope, 2)
                assert got[b].tobytes() == want.tobytes(), (n, b, int(t))
                own = alone[t].convolve_host(np.ascontiguousarray(pool[b]))
                assert got[b].tobytes() == own.tobytes(), (n, b, int(t))
    finally:
        bank.close()
        for t in alone:
            t.close()


@pytest.mark.parametrize('channels', [1, 2])
def test_function_path_bank_frames(ctx, channels):
    from vndecorrelate_amd import _native
    from vndecorrelate_amd.taps import function_path_arrays
    rng = np.random.default_rng(7 + channels)
    fir = O.generate_velvet_noise(duration_seconds=DURATION, num_impulses=IMPULSES, num_outs=6, sample_rate_hz=FS,
                                  segment_envelope=(1.0, 0.5, 0.25), log_distribution_strength=0.6, seed=3)
    arrays = function_path_arrays(fir)
    bank = _native.TapTable.create(ctx, arrays.tap_offsets, arrays.tap_index, arrays.tap_weight)
    alone = []
    for c in range(3):
        a = function_path_arrays(fir[:, 2 * c:2 * c + 2])
        alone.append(_native.TapTable.create(ctx, a.tap_offsets, a.tap_index, a.tap_weight))
    try:
        for n in (150, TILE, TILE + 77, 4500):
            pool = _noise(rng, (4, n, channels))
            tables = np.array([2, 0, 1, 2])
            got = _native.convolve_each_host(ctx, bank, pool, tables)
            for b, c in enumerate(tables):
                want = O.convolve_velvet_noise(_stereo(pool[b]), fir[:, 2 * c:2 * c + 2])
                assert got[b].tobytes() == want.tobytes(), (n, b, int(c))
                assert got[b].tobytes() == alone[c].convolve_host(np.ascontiguousarray(pool[b])).tobytes(), (n, b)
    finally:
        bank.close()
        for t in alone:
            t.close()


# ---- 2. the stage ----------------------------------------------------------------------------------------------------
KAPPAS = (0.0, 0.3, 0.55, 0.3, 0.8, 1.0)                  # signals 1 and 3 share a kappa: one candidate for both


def _velvets(dec, kappas, **kw):
    return [dec.VelvetNoise(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED,
                            log_distribution_strength=k, **kw) for k in kappas]


@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('width', [None, 0.3])
@pytest.mark.parametrize('mode', ['MS', 'LR'])
def test_stage_equals_the_loop_with_numpys_epilogue(dec, mode, width, normalize, channels):
    rng = np.random.default_rng(200 + 8 * (mode == 'MS') + 4 * (width is not None) + 2 * normalize + channels)
    kw = dict(mode=mode, width=width) if normalize else dict(mode=mode, width=width, normalizer=None)
    stages = _velvets(dec, KAPPAS, **kw)
    for n in (1, TILE + 1, 5000):
        pool = _noise(rng, (6, n, 2) if channels == 2 else (6, n))
        got = dec.decorrelate_each(pool, stages)
        assert dec.last_each.route == 'device' and dec.last_each.kind == 'velvet'
        assert dec.last_each.tables == 5 and dec.last_each.launches == 1
        assert got.shape == (6, n, 2) and got.dtype == np.float32
        dec.set_device_epilogue(False)                     # the loop: device convolution, NumPy's epilogue on the host
        try:
            want = np.stack([d.decorrelate(pool[b]) for b, d in enumerate(stages)])
        finally:
            dec.set_device_epilogue(None)
        assert got.tobytes() == want.tobytes(), (n, np.flatnonzero((got != want).any(axis=(1, 2))))
        for b, k in enumerate(KAPPAS):
            ref = O.decorrelate(pool[b], sample_rate_hz=FS, width=width, duration_seconds=DURATION,
                                num_impulses=IMPULSES, log_distribution_strength=k, normalize=normalize, mode=mode,
                                seed=SEED)
            assert got[b].tobytes() == ref.tobytes(), (n, b)
    if channels == 1:                                      # a mono pool as (B, n, 1) is the same pool
        assert dec.decorrelate_each(pool[:, :, None], stages).tobytes() == got.tobytes()


# ---- 3. independence -------------------------------------------------------------------------------------------------
STAGE = dict(ms_encode=True, width=0.3, normalize=2)


def _device_rows(ctx, bank, pool, tables, *, stage=None, side=True):
    import torch
    from vndecorrelate_amd import _native
    dev = torch.device('cuda', ctx.device)
    batch, n, channels = pool.shape
    xd = torch.from_numpy(pool).to(dev)
    td = torch.from_numpy(np.asarray(tables, np.int32)).to(dev)
    yd = torch.full((batch, n, 2), -7.0, dtype=torch.float32, device=dev)
    ws = _native.decorrelate_workspace_bytes(batch, n, 2)
    wd = torch.empty(max(ws, 1), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev) if side else torch.cuda.current_stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        if stage is None:
            _native.convolve_each_device(ctx, bank, xd.data_ptr(), td.data_ptr(), yd.data_ptr(), batch, n, channels,
                                         stream=stream.cuda_stream)
        else:
            _native.decorrelate_each_device(ctx, bank, xd.data_ptr(), td.data_ptr(), yd.data_ptr(), batch, n, channels,
                                            workspace_ptr=wd.data_ptr(), workspace_bytes=ws, stream=stream.cuda_stream,
                                            **stage)
    stream.synchronize()
    return yd.cpu().numpy()


@pytest.mark.parametrize('channels', [1, 2])
def test_rows_depend_on_signal_and_table_only(ctx, channels):
    from vndecorrelate_amd import _native
    rng = np.random.default_rng(50 + channels)
    a, b, c = _taps(0.1), _taps(0.6), _taps(0.9, filtered=(0, 1), seed=2)
    bank = _class_bank(ctx, [a, b, c, a, b], O.DEFAULT_ENVELOPE)          # one table at two bank positions
    alone = [_class_bank(ctx, [m], O.DEFAULT_ENVELOPE) for m in (a, b, c)]
    try:
        n = 2 * TILE + 333
        pool = _noise(rng, (4, n, channels))
        pool[3] = pool[0]                                  # one signal at two pool indices
        for stage in (None, STAGE):
            def host(table, x, tables):
                if stage is None:
                    return _native.convolve_each_host(ctx, table, x, tables)
                return _native.decorrelate_each_host(ctx, table, x, tables, **stage)
            base = {(s, k): host(alone[k], np.ascontiguousarray(pool[s:s + 1]), [0])[0]
                    for s in range(3) for k in range(3)}
            if stage is not None:                          # ... and the per-signal entry, normaliser included
                for (s, k), row in base.items():
                    own = alone[k].decorrelate_host(np.ascontiguousarray(pool[s]), ms_encode=True, width=0.3, normalize=2)
                    assert row.tobytes() == own.tobytes(), (s, k)
            for tables in ([0, 1, 2, 3], [3, 4, 2, 0], [2, 2, 1, 4], [4, 3, 0, 1]):      # shuffled
                got = host(bank, pool, tables)
                for s, k in enumerate(tables):
                    assert got[s].tobytes() == base[(s % 3, k % 3)].tobytes(), (tables, s)
                halves = np.concatenate([host(bank, np.ascontiguousarray(pool[:1]), tables[:1]),
                                         host(bank, np.ascontiguousarray(pool[1:]), tables[1:])])
                assert halves.tobytes() == got.tobytes()                               # a pool split into two calls
                assert _device_rows(ctx, bank, pool, tables, stage=stage).tobytes() == got.tobytes()   # _dev, side stream
    finally:
        bank.close()
        for t in alone:
            t.close()


# ---- 4. bounds -------------------------------------------------------------------------------------------------------
def test_window_limit(ctx, dec):
    from vndecorrelate_amd import _native
    limit = _native.VELVET_PAIRS_MAX_TAP_INDEX
    inside = _native.TapTable.create(ctx, [0, 2, 3], [limit, 0, 7], [0.5, 1.0, -1.0])
    outside = _native.TapTable.create(ctx, [0, 1, 2], [limit + 1, 0], [1.0, 1.0])
    try:
        pool = _noise(np.random.default_rng(3), (2, 6000, 2))
        got = _native.convolve_each_host(ctx, inside, pool, [0, 0])       # the largest window the kernel stages
        for b in range(2):
            assert got[b].tobytes() == inside.convolve_host(np.ascontiguousarray(pool[b])).tobytes(), b
        with pytest.raises(_native.NativeError, match='largest tap index'):         # VND_ERR_UNSUPPORTED
            _native.convolve_each_host(ctx, outside, pool, [0, 0])
        with pytest.raises(_native.NativeError, match='VND_MODE_EXACT only'):
            _native.convolve_each_host(ctx, inside, pool, [0, 0], mode=_native.MODE_FAST)
        with pytest.raises(_native.NativeError, match='VND_MODE_EXACT only'):
            _native.decorrelate_each_host(ctx, inside, pool, [0, 0], mode=_native.MODE_FMA, **STAGE)
    finally:
        inside.close()
        outside.close()
    # the Python call with filters past the window: the loop's result
    long = [dec.VelvetNoise(sample_rate_hz=44100, duration_seconds=0.1, num_impulses=30, seed=1,
                            log_distribution_strength=k) for k in (0.2, 0.9)]            # 4410-frame filters
    small = _noise(np.random.default_rng(4), (2, 900, 2))
    assert not dec.each_covers(small, long)
    got = dec.decorrelate_each(small, long)
    assert dec.last_each.route == 'host'
    assert got.tobytes() == np.stack([d.decorrelate(small[b]) for b, d in enumerate(long)]).tobytes()


def test_bad_tables(ctx):
    from vndecorrelate_amd import _native
    lib = _native.load_library()
    rng = np.random.default_rng(8)
    members = [_taps(0.2), _taps(0.8)]
    bank = _class_bank(ctx, members, O.DEFAULT_ENVELOPE)
    try:
        for n in (TILE + 5, 5001):                          # 5001: an odd row length, rows on 8-byte boundaries
            pool = _noise(rng, (4, n, 2))
            for tables, word in (([0, -1, 1, 0], 'table -1 of signal 1'), ([0, 1, 1, 2], 'table 2 of signal 3')):
                for stage in (None, STAGE):
                    with pytest.raises(ValueError, match=word):
                        if stage is None:
                            _native.convolve_each_host(ctx, bank, pool, tables)
                        else:
                            _native.decorrelate_each_host(ctx, bank, pool, tables, **stage)
                    assert word.encode() in lib.vnd_last_error()
                    got = _device_rows(ctx, bank, pool, tables, stage=stage)     # _dev: NaN rows from the bounds check
                    bad = [b for b, t in enumerate(tables) if not 0 <= t < 2]
                    good = [b for b in range(4) if b not in bad]
                    assert np.isnan(got[bad]).all(), (n, tables)
                    fine = np.ascontiguousarray(pool[good])
                    kept = [tables[b] for b in good]
                    want = _native.convolve_each_host(ctx, bank, fine, kept) if stage is None else \
                        _native.decorrelate_each_host(ctx, bank, fine, kept, **stage)
                    assert got[good].tobytes() == want.tobytes(), (n, tables)
        with pytest.raises(ValueError, match='mono or stereo'):
            _native.convolve_each_host(ctx, bank, np.zeros((1, 10, 3), np.float32), [0])
        odd = _native.TapTable.create(ctx, [0, 1, 2, 3], [0, 1, 2], [1.0, 1.0, 1.0])
        try:
            with pytest.raises(ValueError, match='stereo pairs'):
                _native.convolve_each_host(ctx, odd, pool, [0, 0, 0, 0])
        finally:
            odd.close()
    finally:
        bank.close()


# ---- 5. Haas ---------------------------------------------------------------------------------------------------------
def _haas(dec, delays, **kw):
    return [dec.HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d), **kw) for d in delays]


@pytest.mark.parametrize('n', [300, 1000])
@pytest.mark.parametrize('channels', [1, 2])
@pytest.mark.parametrize('mode', ['LR', 'MS'])
@pytest.mark.parametrize('delayed_channel', [0, 1])
@pytest.mark.parametrize('width', [None, 0.3])
def test_haas_rows_are_numpys(ctx, dec, n, channels, mode, delayed_channel, width):
    from vndecorrelate_amd import _native
    rng = np.random.default_rng(n + channels)
    delays = (0, 1, 255, 256, 257, n - 1, n, n + 5)
    stages = _haas(dec, delays, mode=mode, delayed_channel=delayed_channel, width=width)
    pool = _noise(rng, (8, n, 2) if channels == 2 else (8, n))
    got = dec.decorrelate_each(pool, stages)
    assert dec.last_each.route == 'device' and dec.last_each.kind == 'haas' and dec.last_each.launches == 1
    assert isinstance(got, list) and len(got) == 8
    for b, (d, stage) in enumerate(zip(delays, stages)):
        want = stage.decorrelate(pool[b])                  # NumPy on the host
        assert got[b].shape == (n + d, 2) and got[b].dtype == np.float64
        assert got[b].tobytes() == want.tobytes(), (b, d)
    block = _native.haas_each_host(ctx, np.ascontiguousarray(pool.reshape(8, n, -1)), delays, max_delay=n + 9,
                                   delayed_channel=delayed_channel, ms_mode=mode == 'MS', width=width)
    assert block.shape == (8, 2 * n + 9, 2)
    for b, d in enumerate(delays):
        assert block[b, :n + d].tobytes() == got[b].tobytes(), (b, d)
        assert block[b, n + d:].tobytes() == np.zeros((n + 9 - d, 2)).tobytes(), (b, d)      # padding: +0.0


def test_haas_bad_delays(ctx):
    import torch
    from vndecorrelate_amd import _native
    n, max_delay = 700, 40
    pool = _noise(np.random.default_rng(5), (4, n, 2))
    settings = dict(max_delay=max_delay, delayed_channel=1, ms_mode=True, width=0.3)
    for delays, word in (([3, 41, 0, 40], 'delay 41 of signal 1'), ([0, 1, 2, -1], 'delay -1 of signal 3')):
        with pytest.raises(ValueError, match=word):
            _native.haas_each_host(ctx, pool, delays, **settings)
        dev = torch.device('cuda', ctx.device)
        xd = torch.from_numpy(pool).to(dev)
        dd = torch.from_numpy(np.asarray(delays, np.int32)).to(dev)
        yd = torch.full((4, n + max_delay, 2), -7.0, dtype=torch.float64, device=dev)
        _native.haas_each_device(ctx, xd.data_ptr(), yd.data_ptr(), 4, n, 2, dd.data_ptr(),
                                 stream=torch.cuda.current_stream(dev).cuda_stream, **settings)
        got = yd.cpu().numpy()
        bad = [b for b, d in enumerate(delays) if not 0 <= d <= max_delay]
        good = [b for b in range(4) if b not in bad]
        assert np.isnan(got[bad]).all()
        want = _native.haas_each_host(ctx, np.ascontiguousarray(pool[good]), [delays[b] for b in good], **settings)
        assert got[good].tobytes() == want.tobytes()


# ---- 6. closing the loop ---------------------------------------------------------------------------------------------
def test_the_optimisers_results_applied(ctx, dec):
    from vndecorrelate_amd import optimization as opt
    rng = np.random.default_rng(6)
    base = rng.uniform(-1, 1, (4, 4000, 1))
    pool = (base * np.array([1.0, 0.6]) + 0.4 * rng.uniform(-1, 1, (4, 4000, 2))).astype(np.float32)
    kw = dict(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED)
    kappas = quiet(opt.optimize_velvet_noise_batched, input_signals=pool, grid_size=9, **kw)
    taus = quiet(opt.optimize_haas_delay_batched, input_signals=pool, sample_rate_hz=FS, max_delay_seconds=0.01, grid_size=9)
    assert opt.last_velvet_search.route == 'device' and opt.last_haas_search.route == 'device'
    velvets = [dec.VelvetNoise(log_distribution_strength=float(k), **kw) for k in kappas]
    got = dec.decorrelate_each(pool, velvets)
    assert dec.last_each.route == 'device'
    dec.set_device_epilogue(False)
    try:
        want = np.stack([d.decorrelate(pool[b]) for b, d in enumerate(velvets)])
    finally:
        dec.set_device_epilogue(None)
    assert got.tobytes() == want.tobytes()
    haas = [dec.HaasEffect(sample_rate_hz=FS, delay_time_seconds=float(t)) for t in taus]
    rows = dec.decorrelate_each(pool, haas)
    assert dec.last_each.route == 'device'
    for b, d in enumerate(haas):
        assert rows[b].tobytes() == d.decorrelate(pool[b]).tobytes(), b


# ---- 7. residency ----------------------------------------------------------------------------------------------------
def test_a_resident_pool_stays_on_the_device(ctx, dec, monkeypatch):
    import torch
    from vndecorrelate_amd import _native
    rng = np.random.default_rng(13)
    pool = _noise(rng, (5, 2 * TILE + 77, 2))
    velvets = _velvets(dec, (0.1, 0.9, 0.5, 0.1, 0.7), width=0.3)
    haas = _haas(dec, (0, 17, 300, 5, 17), mode='MS')
    want = dec.decorrelate_each(pool, velvets)
    assert dec.last_each.pool_uploads == 1 and dec.last_each.result_downloads == 1
    want_haas = dec.decorrelate_each(pool, haas)
    want_mono = dec.decorrelate_each(np.ascontiguousarray(pool[:, :, 0]), velvets)

    def refuse(*args, **kwargs):
        raise AssertionError('a host copy of the pool or the result was made')
    for name in ('decorrelate_each_host', 'convolve_each_host', 'haas_each_host'):
        monkeypatch.setattr(_native, name, refuse)
    monkeypatch.setattr(dec.VelvetNoise, 'decorrelate', refuse)
    monkeypatch.setattr(dec.HaasEffect, 'decorrelate', refuse)
    tensor = torch.from_numpy(pool).to(torch.device('cuda', ctx.device))
    got = dec.decorrelate_each(tensor, velvets)
    stats = dec.last_each
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert stats.route == 'device' and stats.pool_uploads == 0 and stats.result_downloads == 0
    assert stats.launches == 1 and stats.launch_pool == [tensor.data_ptr()] and stats.tables == 4      # read in place
    assert got.cpu().numpy().tobytes() == want.tobytes()
    rows = dec.decorrelate_each(tensor, haas)
    stats = dec.last_each
    assert stats.pool_uploads == 0 and stats.result_downloads == 0 and stats.launch_pool == [tensor.data_ptr()]
    for b, row in enumerate(rows):
        assert isinstance(row, torch.Tensor) and row.is_cuda and row.dtype == torch.float64
        assert row.cpu().numpy().tobytes() == want_haas[b].tobytes(), b
    mono = dec.decorrelate_each(tensor[:, :, 0].contiguous(), velvets)                   # a mono pool, fanned out
    assert mono.is_cuda and mono.cpu().numpy().tobytes() == want_mono.tobytes()
