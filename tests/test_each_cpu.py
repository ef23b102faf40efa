"""CPU tier of decorrelate_each (include/vnd_each.h, decorrelation.decorrelate_each): the header and its binding, the
argument checks that come before any device work, what each_covers accepts and refuses, the bank builder against
class_path_bank_arrays, the split into calls with a fake device under the real driver, and the routing rules - no
device call."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_each.h'
FS, DURATION, IMPULSES, SEED = 16000, 0.02, 15, 1


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
def dec():
    import vndecorrelate_amd.decorrelation as decorrelation
    yield decorrelation
    decorrelation.set_each_device(None)
    decorrelation.set_default_mode(decorrelation.MODE_EXACT)


def _velvets(dec, kappas, **kw):
    base = dict(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED)
    base.update(kw)
    return [dec.VelvetNoise(log_distribution_strength=k, **base) for k in kappas]


def _haas(dec, delays, **kw):
    return [dec.HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d), **kw) for d in delays]


# ---- header and binding ----------------------------------------------------------------------------------------------
def test_each_header_is_plain_c():
    src = '#include "vnd_each.h"\nint main(void){return VND_VELVET_PAIRS_MAX_TAP_INDEX == 4094 ? 0 : 1;}\n'
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = _declared(HEADER)
    assert names == ['vnd_convolve_each_f32_dev', 'vnd_convolve_each_f32_host', 'vnd_decorrelate_each_f32_dev',
                     'vnd_decorrelate_each_f32_host', 'vnd_haas_each_f64_dev', 'vnd_haas_each_f64_host']
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_each.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))       # vnd_amd.h keeps its fixed set


def test_checks_that_need_no_device(lib):
    """A null context is refused before anything else (VND_ERR_INVALID = 1) by every entry."""
    null = ctypes.c_void_p(None)
    stage = (0, 1, 0, 0.0, 0, ctypes.c_float(0.0))
    assert lib.vnd_convolve_each_f32_dev(null, null, null, null, null, 1, 10, 2, 0, null) == 1
    assert b'null context' in lib.vnd_last_error()
    assert lib.vnd_convolve_each_f32_host(null, null, None, None, None, 1, 10, 2, 0) == 1
    assert lib.vnd_decorrelate_each_f32_dev(null, null, null, null, null, 1, 10, 2, *stage, null, 0, null) == 1
    assert lib.vnd_decorrelate_each_f32_host(null, null, None, None, None, 1, 10, 2, *stage) == 1
    assert lib.vnd_haas_each_f64_dev(null, null, null, 1, 10, 2, null, 5, 0, 0, 0, 0.0, null) == 1
    assert lib.vnd_haas_each_f64_host(null, None, None, 1, 10, 2, None, 5, 0, 0, 0, 0.0) == 1
    assert b'null context' in lib.vnd_last_error()


def test_wrappers_check_their_arrays(lib):
    from vndecorrelate_amd import _native
    x = np.zeros((2, 10, 2), np.float32)
    for bad, tables in ((x.astype(np.float64), [0, 0]), (x[0], [0]), (x[:, :, ::-1], [0, 0]), (x, [0]), (x, [[0, 0]]),
                        (x, [0, 2 ** 31])):
        with pytest.raises(ValueError):
            _native.convolve_each_host(None, None, bad, tables)
        with pytest.raises(ValueError):
            _native.decorrelate_each_host(None, None, bad, tables, ms_encode=True, width=None, normalize=2)
        with pytest.raises(ValueError):
            _native.haas_each_host(None, bad, tables, max_delay=3, delayed_channel=0, ms_mode=False, width=None)


# ---- coverage --------------------------------------------------------------------------------------------------------
def test_each_covers_velvet(dec):
    x = np.zeros((3, 50, 2), np.float32)
    ks = (0.1, 0.5, 0.9)
    assert dec.each_covers(x, _velvets(dec, ks))
    assert dec.each_covers(x[:, :, 0], _velvets(dec, ks)) and dec.each_covers(x[:, :, :1], _velvets(dec, ks))
    assert dec.each_covers(x.astype(np.int16), _velvets(dec, ks, mode='LR', width=0.3, normalizer=None))
    assert dec.each_covers(x, _velvets(dec, ks, width=np.float64(0.25), filtered_channels=(0,)))
    assert dec.each_covers(x, _velvets(dec, ks, segment_envelope=()))            # the identity envelope
    # refused: the pool
    assert not dec.each_covers(x[:2], _velvets(dec, ks))                          # length mismatch
    assert not dec.each_covers(np.zeros((3, 0, 2), np.float32), _velvets(dec, ks))     # n == 0
    assert not dec.each_covers(np.zeros((3, 50, 3), np.float32), _velvets(dec, ks))
    assert not dec.each_covers(np.zeros((0, 50, 2), np.float32), [])
    # refused: the list
    assert not dec.each_covers(x, _velvets(dec, ks, num_outs=3, filtered_channels=(0, 1, 2), mode='LR'))
    mixed = _velvets(dec, ks)
    mixed[1].mode = 'LR'
    assert not dec.each_covers(x, mixed)                                          # mode differs across the list
    mixed = _velvets(dec, ks, width=0.3)
    mixed[2].width = 0.31
    assert not dec.each_covers(x, mixed)                                          # width differs
    mixed = _velvets(dec, ks)
    mixed[0].normalizer = None
    assert not dec.each_covers(x, mixed)                                          # normaliser differs
    assert not dec.each_covers(x, _velvets(dec, ks, normalizer=lambda a, b: None))     # a custom normaliser
    assert not dec.each_covers(x, _velvets(dec, ks, width=np.float32(0.3)))      # NumPy's 1.0 - width would be float32
    assert not dec.each_covers(x, _velvets(dec, ks, width=float('nan')))
    assert not dec.each_covers(x, _velvets(dec, ks, sample_rate_hz=44100, duration_seconds=0.1, num_impulses=30))  # 4410 frames
    assert not dec.each_covers(x, _velvets(dec, ks, segment_envelope=(1.0, float('inf'))))

    class Mine(dec.VelvetNoise):
        pass
    assert not dec.each_covers(x, [Mine(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES)] * 3)
    assert not dec.each_covers(x, _velvets(dec, ks[:2]) + _haas(dec, [3]))
    short = _velvets(dec, ks)
    short[1].segment_envelope = (0.5,)                    # shorter than the generated segments: the loop's IndexError
    assert not dec.each_covers(x, short)
    dec.set_default_mode(dec.MODE_FMA)
    assert not dec.each_covers(x, _velvets(dec, ks))                              # the default mode is not exact
    dec.set_default_mode(dec.MODE_EXACT)
    # the largest index the window holds, and one past it (a tap moved: the table keeps its impulse count)
    edge = _velvets(dec, ks)
    taps = next(seg.positive_impulse_indexes for seg in edge[0]._velvet_noise.output_channels[0]
                if seg.positive_impulse_indexes)
    taps[-1] = 4094
    assert dec.each_covers(x, edge)
    taps[-1] = 4095
    assert not dec.each_covers(x, edge)
    assert dec._member_in_window(([[([], [4094])], None], (1.0,), False))
    assert not dec._member_in_window(([[([4095], [3])], None], (1.0,), False))


def test_each_covers_haas(dec):
    x = np.zeros((3, 50, 2), np.float32)
    assert dec.each_covers(x, _haas(dec, (0, 7, 60)))
    assert dec.each_covers(x[:, :, 0], _haas(dec, (0, 7, 60), mode='MS', delayed_channel=1, width=0.3))
    assert not dec.each_covers(x, _haas(dec, (0, 7)))
    assert not dec.each_covers(x, _haas(dec, (0, 7, -1)))
    assert not dec.each_covers(x, _haas(dec, (0, 7, 2 ** 31)))
    assert not dec.each_covers(x, _haas(dec, (0, 7, 3), width=np.float32(0.3)))
    assert not dec.each_covers(x, _haas(dec, (0, 7, 3), delayed_channel=2))
    for field, other in (('mode', 'MS'), ('delayed_channel', 1), ('width', 0.5)):
        mixed = _haas(dec, (0, 7, 3))
        setattr(mixed[1], field, other)
        assert not dec.each_covers(x, mixed), field
    assert not dec.each_covers(x, _haas(dec, (0, 7, dec._EACH_HAAS_BYTES // 16)))      # a padded block past the budget


# ---- the bank --------------------------------------------------------------------------------------------------------
def test_bank_builder(dec):
    from vndecorrelate_amd.taps import class_path_bank_arrays
    stages = _velvets(dec, (0.2, 0.7, 0.2, 1.0, 0.7, 0.2)) + _velvets(dec, (0.2,), filtered_channels=(0,)) \
        + _velvets(dec, (0.2,), segment_envelope=(1.0, 0.5, 0.25, 0.1)) + _velvets(dec, (0.2,), segment_envelope=())
    members, tables = dec.each_velvet_members(stages)
    assert tables.dtype == np.int32 and tables.tolist() == [0, 1, 0, 2, 1, 0, 3, 4, 5]
    assert len(members) == 6
    for b, d in enumerate(stages):                        # every signal is mapped to its own member
        assert dec._member_key(members[tables[b]]) == dec._member_key(d._tap_member()), b
    distinct = [stages[i] for i in (0, 1, 3, 6, 7, 8)]
    got = class_path_bank_arrays(members)
    want = class_path_bank_arrays([d._tap_member() for d in distinct])
    assert got.to_bytes() == want.to_bytes() and got.num_channels == 12


def test_ranges(dec):
    f = dec._each_ranges
    assert f(np.array([], np.int32), 4, 4) == []
    assert f(np.arange(10) % 3, 4, 9) == [(0, 4), (4, 8), (8, 10)]               # the signal limit
    assert f(np.array([0, 1, 0, 1, 2, 2, 3, 0]), 100, 2) == [(0, 4), (4, 7), (7, 8)]   # the table limit
    assert f(np.array([5, 5, 5, 5]), 100, 1) == [(0, 4)]


def test_split_past_the_limits_with_a_fake_device(dec):
    """More than 32767 distinct tables, and more than VND_MAX_STREAMS signals: the real driver cuts the pool into calls,
    each with the bank of its own distinct members and local indices; every signal gets its own table's row back."""
    from vndecorrelate_amd import _native
    bank_limit, stream_limit = _native.VELVET_BANK_MAX_CANDIDATES, _native.MAX_STREAMS_PER_CALL
    assert (bank_limit, stream_limit) == (32767, 65535)
    calls = []

    class FakeDevice(dec._EachVelvet):
        def __init__(self, batch):
            self.stats = dec.EachStats(route='fake', signals=batch)
            self.batch, self.n, self.channels, self.is_torch = batch, 1, 1, False

        def _call(self, arrays, local, first, last, out):
            assert arrays.num_channels % 2 == 0 and 0 < arrays.num_channels // 2 <= bank_limit
            assert local.dtype == np.int32 and local.size == last - first <= stream_limit
            assert local.min() >= 0 and local.max() < arrays.num_channels // 2
            calls.append((first, last, arrays.num_channels // 2))
            # the "row" of a signal: the first tap index of its candidate's left channel, and its weight
            at = arrays.tap_offsets[2 * local]
            out[first:last, 0, 0] = arrays.tap_index[at]
            out[first:last, 0, 1] = arrays.tap_weight[at]

    count = 2 * bank_limit + 1000                          # distinct members: one tap each, at index i % 4000, sign by i // 4000 parity
    members = [([[([i % 4000], []) if (i // 4000) % 2 else ([], [i % 4000])], None], (1.0,), False) for i in range(count)]
    rng = np.random.default_rng(1)
    tables = np.concatenate([np.arange(count), rng.integers(0, count, 30000)]).astype(np.int32)
    out = FakeDevice(tables.size).run(members, tables)
    assert calls[0] == (0, bank_limit, bank_limit) and calls[1] == (bank_limit, 2 * bank_limit, bank_limit)
    assert [c[0] for c in calls[1:]] == [c[1] for c in calls[:-1]] and calls[-1][1] == tables.size
    assert out[:, 0, 0].tolist() == (tables % 4000).tolist()
    assert out[:, 0, 1].tolist() == np.where((tables // 4000) % 2 == 1, -1.0, 1.0).tolist()
    # few tables, many signals: the stream limit cuts
    calls.clear()
    tables = (np.arange(2 * stream_limit + 10) % 7).astype(np.int32)
    driver = FakeDevice(tables.size)
    out = driver.run(members[:7], tables)
    assert calls == [(0, stream_limit, 7), (stream_limit, 2 * stream_limit, 7), (2 * stream_limit, tables.size, 7)]
    assert out[:, 0, 0].tolist() == tables.tolist()
    assert driver.stats.launches == 3 and driver.stats.launch_tables == [7, 7, 7] and driver.stats.tables == 7


# ---- routing ---------------------------------------------------------------------------------------------------------
def test_switch_takes_only_booleans_and_none(dec):
    for bad in (1, 'yes', 0.0):
        with pytest.raises(TypeError):
            dec.set_each_device(bad)


def test_forced_device_without_one_raises(dec, monkeypatch):
    from vndecorrelate_amd import analysis
    monkeypatch.setattr(analysis, '_gpu_present', lambda: False)
    dec.set_each_device(True)
    with pytest.raises(RuntimeError, match='no gfx950 device'):
        dec.decorrelate_each(np.zeros((2, 30, 2), np.float32), _haas(dec, (1, 2)))
    # a call without a device form is the loop even then
    got = dec.decorrelate_each(np.ones((2, 30, 2), np.float32), _haas(dec, (1, 2), width=np.float32(0.5)))
    assert dec.last_each.route == 'host' and [g.shape for g in got] == [(31, 2), (32, 2)]


def test_host_route_is_the_loop(dec, monkeypatch):
    from vndecorrelate_amd import analysis
    monkeypatch.setattr(analysis, '_gpu_present', lambda: False)      # None without a device: the loop
    rng = np.random.default_rng(2)
    pool = rng.uniform(-1, 1, (3, 40, 2))
    stages = _haas(dec, (0, 5, 45), mode='MS', width=0.3)
    got = dec.decorrelate_each(pool, stages)
    assert dec.last_each.route == 'host' and dec.last_each.signals == 3 and isinstance(got, list)
    for b, d in enumerate(stages):
        assert got[b].tobytes() == d.decorrelate(pool[b]).tobytes(), b
    mono = dec.decorrelate_each(pool[:, :, :1], stages)               # (B, n, 1): each signal as (n,)
    for b, d in enumerate(stages):
        assert mono[b].tobytes() == d.decorrelate(pool[b, :, 0]).tobytes(), b
    # velvet noise: the loop's rows, stacked (the convolution itself needs a device: a stand-in here)
    seen = []
    monkeypatch.setattr(dec.VelvetNoise, 'decorrelate',
                        lambda self, x: seen.append((self.log_distribution_strength, x)) or np.full((len(x), 2), len(seen), np.float32))
    velvets = _velvets(dec, (0.1, 0.5, 0.9))
    for switch in (None, False):
        seen.clear()
        dec.set_each_device(switch)
        out = dec.decorrelate_each(pool[:, :, 0], velvets)
        assert out.shape == (3, 40, 2) and out.dtype == np.float32 and out[:, 0, 0].tolist() == [1, 2, 3]
        assert [k for k, _ in seen] == [0.1, 0.5, 0.9]
        assert all(np.array_equal(x, pool[b, :, 0]) for b, (_, x) in enumerate(seen))
    monkeypatch.setattr(analysis, '_gpu_present', lambda: True)       # False wins over a device
    dec.set_each_device(False)
    assert dec.decorrelate_each(pool, velvets)[:, 0, 0].tolist() == [4, 5, 6] and dec.last_each.route == 'host'


def test_argument_errors(dec):
    dec.set_each_device(False)
    pool = np.zeros((3, 20, 2), np.float32)
    with pytest.raises(ValueError, match='2 decorrelators for a pool of 3 signals'):
        dec.decorrelate_each(pool, _haas(dec, (1, 2)))
    with pytest.raises(TypeError, match='one type'):
        dec.decorrelate_each(pool, _haas(dec, (1, 2)) + _velvets(dec, (0.5,)))
    for shape in [(4,), (2, 10, 3), (2, 10, 2, 1), ()]:
        with pytest.raises(ValueError, match='expected a stereo pool'):
            dec.decorrelate_each(np.zeros(shape, np.float32), [])
    with pytest.raises(TypeError, match='real numbers'):
        dec.decorrelate_each(np.zeros((2, 10), complex), _haas(dec, (1, 2)))
    out = dec.decorrelate_each(np.zeros((0, 10, 2)), [])
    assert out.shape == (0, 10, 2) and out.dtype == np.float32 and dec.last_each.route == 'none'


def test_exported_from_the_package():
    import vndecorrelate_amd
    for name in ('decorrelate_each', 'each_covers', 'set_each_device'):
        assert callable(getattr(vndecorrelate_amd, name))
