"""CPU tier of decorrelate_each_stream (include/vnd_each_stream.h, decorrelation.decorrelate_each_stream): the header and
its binding, the argument checks that come before any device work, every refusal of the Python entry before the device
is touched, and the output counts of random schedules against output_span at the bank's latency - no device call."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_each_stream.h'
FS, DURATION, IMPULSES, SEED = 16000, 0.02, 15, 1
NAMES = ['vnd_each_stream_f32_dev', 'vnd_each_stream_f32_host', 'vnd_each_stream_state_bytes',
         'vnd_haas_each_stream_f64_dev', 'vnd_haas_each_stream_f64_host', 'vnd_haas_each_stream_state_bytes']
INVALID, UNSUPPORTED = 1, 4


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
    return decorrelation


@pytest.fixture
def no_device(monkeypatch):
    """Any touch of the device raises: the refusals and the counts below come before it."""
    from vndecorrelate_amd import _native

    def touched(*args, **kwargs):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(_native, 'default_context', touched)
    monkeypatch.setattr(_native, 'context_for', touched)


def _velvets(dec, kappas, **kw):
    base = dict(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None)
    base.update(kw)
    return [dec.VelvetNoise(log_distribution_strength=k, **base) for k in kappas]


def _haas(dec, delays, **kw):
    return [dec.HaasEffect(sample_rate_hz=1, delay_time_seconds=float(d), **kw) for d in delays]


# ---- header and binding ----------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    src = ('#include "vnd_each_stream.h"\n'
           'int main(void){return VND_VELVET_PAIRS_MAX_TAP_INDEX == 4094 && VND_MAX_STREAMS == 65535 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    text = HEADER.read_text()
    assert '#include "vnd_each.h"' in text and '#include "vnd_stream.h"' in text


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_each_stream.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))       # vnd_amd.h keeps its fixed set
    # the planner's description: declared beside the stream's, exported and bound
    internal = _declared(REPO / 'include' / 'vnd_amd_internal.h')
    assert 'vnd_describe_each_stream_launch' in internal and 'vnd_describe_stream_launch' in internal
    assert hasattr(lib, 'vnd_describe_each_stream_launch')
    assert 'vnd_describe_each_stream_launch' in _native.INTERNAL_SIGNATURES
    for wrapper in ('each_stream_device', 'each_stream_host', 'each_stream_state_bytes', 'haas_each_stream_device',
                    'haas_each_stream_host', 'haas_each_stream_state_bytes'):
        assert callable(getattr(_native, wrapper))
    assert callable(_native.TapTable.describe_each_stream)


def test_checks_that_need_no_device(lib):
    null = ctypes.c_void_p(None)
    got = ctypes.c_int64(-7)
    velvet = (null, null, 0, 480, null, null, 1, 0, 10, 2, 0, 0, 0, 0, 0.0)
    # a null context or bank is refused before anything else, by every entry
    assert lib.vnd_each_stream_f32_dev(null, null, *velvet, ctypes.byref(got), null) == INVALID
    assert b'null context' in lib.vnd_last_error()
    assert lib.vnd_each_stream_f32_host(null, null, *velvet, ctypes.byref(got)) == INVALID
    assert lib.vnd_each_stream_state_bytes(null, 1, 2, 480, ctypes.byref(got)) == INVALID
    haas = (null, 0, 480, null, null, 1, 0, 10, 2, 0, null, 5, 0, 0, 0, 0.0)
    assert lib.vnd_haas_each_stream_f64_dev(null, *haas, ctypes.byref(got), null) == INVALID
    assert b'null context' in lib.vnd_last_error()
    assert lib.vnd_haas_each_stream_f64_host(null, *haas, ctypes.byref(got)) == INVALID
    text = ctypes.create_string_buffer(64)
    assert lib.vnd_describe_each_stream_launch(null, null, 480, 1, 0, 10, 2, 0, 0, 0, text, 64) == INVALID
    # the Haas state query is all scalars
    need = ctypes.c_int64(-1)
    assert lib.vnd_haas_each_stream_state_bytes(3, 2, 7, 480, ctypes.byref(need)) == 0
    assert need.value == 3 * (7 + 480) * 2 * 4                                    # capacity max_delay + max_frames_per_call
    assert lib.vnd_haas_each_stream_state_bytes(3, 1, 0, 480, ctypes.byref(need)) == 0 and need.value == 0
    assert lib.vnd_haas_each_stream_state_bytes(3, 2, 7, 480, None) == INVALID
    for bad in ((-1, 2, 7, 480), (3, 3, 7, 480), (3, 0, 7, 480), (3, 2, -1, 480), (3, 2, 7, -1)):
        need.value = -1
        assert lib.vnd_haas_each_stream_state_bytes(*bad, ctypes.byref(need)) == INVALID, bad
        assert need.value == 0
    assert lib.vnd_haas_each_stream_state_bytes(65536, 2, 7, 480, ctypes.byref(need)) == UNSUPPORTED
    assert b'split the pool' in lib.vnd_last_error()


def test_wrappers_check_their_arrays(lib):
    from vndecorrelate_amd import _native
    x = np.zeros((2, 10, 2), np.float32)
    for bad, each in ((x.astype(np.float64), [0, 0]), (x[0], [0]), (x[:, :, ::-1], [0, 0]), (x, [0]), (x, [[0, 0]]),
                      (x, [0, 2 ** 31])):
        with pytest.raises(ValueError):
            _native.each_stream_host(None, None, each, 0, 0, 480, bad, 0, 0, final=False, ms_encode=False, width=None)
        with pytest.raises(ValueError):
            _native.haas_each_stream_host(None, 0, 0, 480, bad, each, 0, final=False, max_delay=3, delayed_channel=0,
                                          ms_mode=False, width=None)


# ---- the Python entry's refusals -------------------------------------------------------------------------------------
def test_refusals_come_before_the_device(dec, no_device):
    make = dec.decorrelate_each_stream
    ks = (0.1, 0.5, 0.9)
    with pytest.raises(ValueError, match='at least one decorrelator'):
        make([])
    with pytest.raises(TypeError, match='one type'):
        make(_velvets(dec, ks[:2]) + _haas(dec, [3]))
    with pytest.raises(TypeError, match='WhiteNoise'):
        make([dec.WhiteNoise(sample_rate_hz=FS)] * 2)

    class Mine(dec.VelvetNoise):
        pass
    with pytest.raises(TypeError, match='Mine'):
        make([Mine(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, normalizer=None)])
    for bad in (0, 3, True, 2.5, None):
        with pytest.raises(ValueError, match='in_channels'):
            make(_velvets(dec, ks), in_channels=bad)
        with pytest.raises(ValueError, match='in_channels'):
            make(_haas(dec, (1, 2)), in_channels=bad)
    for bad in (0, -1, 2.0):
        with pytest.raises(ValueError, match='max_frames_per_call'):
            make(_velvets(dec, ks), max_frames_per_call=bad)
    # velvet noise
    with pytest.raises(ValueError, match='VelvetNoise.stream needs normalizer=None'):
        make(_velvets(dec, ks, normalizer=dec.rms_normalize))
    for field, first, other in (('mode', 'MS', 'LR'), ('width', 0.3, 0.31), ('width', None, 0.3),
                                ('normalizer', None, dec.rms_normalize)):
        mixed = _velvets(dec, ks, **{field: first})
        setattr(mixed[2], field, other)
        with pytest.raises(ValueError, match=f'{field} differs across the list'):
            make(mixed)
    with pytest.raises(ValueError, match='num_outs'):
        make(_velvets(dec, ks, num_outs=3, filtered_channels=(0, 1, 2), mode='LR'))
    with pytest.raises(ValueError, match='float64 width'):
        make(_velvets(dec, ks, width=np.float32(0.3)))
    with pytest.raises(ValueError, match=r'stream 0: its table reaches past 4094 frames.*\.stream\(\)'):
        make(_velvets(dec, ks, sample_rate_hz=44100, duration_seconds=0.1, num_impulses=30))      # 4410 frames
    with pytest.raises(ValueError, match=r'not finite.*\.stream\(\)'):
        make(_velvets(dec, ks, segment_envelope=(1.0, float('inf'))))
    edge = _velvets(dec, ks)
    taps = next(seg.positive_impulse_indexes for seg in edge[1]._velvet_noise.output_channels[0]
                if seg.positive_impulse_indexes)
    taps[-1] = 4094
    assert make(edge).latency_frames == 4094
    taps[-1] = 4095
    with pytest.raises(ValueError, match='stream 1: its table reaches past 4094'):
        make(edge)
    # Haas
    for field, other in (('mode', 'MS'), ('delayed_channel', 1), ('width', 0.5)):
        mixed = _haas(dec, (0, 7, 3))
        setattr(mixed[1], field, other)
        with pytest.raises(ValueError, match=f'{field} differs across the list'):
            make(mixed)
    for bad in (_haas(dec, (0, 7, -1)), _haas(dec, (0, 7, 2 ** 31)), _haas(dec, (0, 7), delayed_channel=2),
                _haas(dec, (0, 7), width=np.float32(0.3))):
        with pytest.raises(ValueError, match='covers a plain HaasEffect'):
            make(bad)


def test_too_many_streams_or_tables(dec, no_device, monkeypatch):
    from vndecorrelate_amd import _native
    one = _haas(dec, (1,))[0]
    with pytest.raises(ValueError, match='split the pool'):
        dec.decorrelate_each_stream([one] * (_native.MAX_STREAMS_PER_CALL + 1))
    v = _velvets(dec, (0.2,))[0]
    with pytest.raises(ValueError, match='split the pool'):
        dec.decorrelate_each_stream([v] * (_native.MAX_STREAMS_PER_CALL + 1))
    monkeypatch.setattr(_native, 'VELVET_BANK_MAX_CANDIDATES', 2)
    assert dec.decorrelate_each_stream(_velvets(dec, (0.1, 0.5, 0.1))).num_streams == 3
    with pytest.raises(ValueError, match='3 distinct tap tables.*split the pool'):
        dec.decorrelate_each_stream(_velvets(dec, (0.1, 0.5, 0.9)))


# ---- what the streams report, and their counts -----------------------------------------------------------------------
def test_velvet_stream_properties(dec, no_device):
    from vndecorrelate_amd import streaming
    from vndecorrelate_amd.taps import class_path_bank_arrays
    short = _velvets(dec, (0.3, 0.8), duration_seconds=0.01, num_impulses=8)          # 160 frames
    long_ = _velvets(dec, (0.3, 0.8, 0.3))                                             # 320 frames; 0 and 2 share a table
    stages = [short[0], long_[0], short[1], long_[1], long_[2]]
    own = [int(class_path_bank_arrays([d._tap_member()]).tap_index.max()) for d in stages]
    assert len(set(own)) > 2 and max(own[1], own[3]) > max(own[0], own[2])
    s = dec.decorrelate_each_stream(stages, in_channels=1, max_frames_per_call=480)
    assert type(s) is streaming.EachStream and isinstance(s, streaming.Stream)
    assert s.num_streams == 5 and s.in_channels == 1 and s.num_channels == 2 and s.max_frames_per_call == 480
    assert s.latency_frames == max(own)                                    # the bank's: the shorter filters wait
    assert s.tables.dtype == np.int32 and s.tables.tolist() == [0, 1, 2, 3, 1]
    assert s.arrays.num_channels == 8 and s.mode == dec.MODE_EXACT
    assert (s.ms_encode, s.width) == (True, None)                          # the VelvetNoise defaults: MS, no width
    lr = dec.decorrelate_each_stream(_velvets(dec, (0.1,), mode='LR', width=0.35))
    assert (lr.ms_encode, lr.width, lr.in_channels, lr.max_frames_per_call) == (False, 0.35, 2, 4800)


def test_haas_stream_properties(dec, no_device):
    from vndecorrelate_amd import streaming
    s = dec.decorrelate_each_stream(_haas(dec, (5, 0, 257, 12), mode='MS', delayed_channel=1, width=0.3), in_channels=1,
                                    max_frames_per_call=256)
    assert type(s) is streaming.HaasEachStream and isinstance(s, streaming.HaasStream)
    assert s.num_streams == 4 and s.latency_frames == 0 and s.tail_frames == 257
    assert s.tail_frames_each.tolist() == [5, 0, 257, 12] and s.tail_frames_each.dtype.kind == 'i'
    assert (s.delayed_channel, s.ms_mode, s.width, s.num_channels) == (1, True, 0.3, 2)


class _Recorder:
    """Stands for the device under a real stream: records every call the lifecycle makes and answers with zeros."""

    def __init__(self, stream):
        self.calls = []
        stream._call_host = self._call
        self.width, self.dtype, self.streams = stream._out_width, stream._out_dtype, stream.num_streams

    def _call(self, block, n_in, n_out, final):
        self.calls.append((n_in, n_out, bool(final)))
        return np.zeros((self.streams, n_out, self.width), self.dtype)


@pytest.mark.parametrize('seed', range(6))
def test_counts_over_random_schedules(dec, no_device, seed):
    from vndecorrelate_amd.streaming import output_span
    rng = np.random.default_rng(seed)
    M = 96
    velvet = dec.decorrelate_each_stream(_velvets(dec, (0.3, 0.8), duration_seconds=0.002, num_impulses=4)       # 32 frames
                                         + _velvets(dec, (0.5,), duration_seconds=0.004, num_impulses=6),        # 64 frames
                                         max_frames_per_call=M)
    haas = dec.decorrelate_each_stream(_haas(dec, (3, 40, 0)), max_frames_per_call=M)
    H, D = velvet.latency_frames, haas.tail_frames
    assert 32 < H < 64 and D == 40
    for stream, dtype in ((velvet, np.float32), (haas, np.float64)):
        record = _Recorder(stream)
        for round_ in range(2):                               # the second signal follows a reset
            sizes = [int(v) for v in rng.choice([0, 0, 1, H, H + 1, M, int(rng.integers(1, M))], 12)]
            ending = ('flush', 'final')[(seed + round_) % 2]
            pos, total = 0, 0
            for i, b in enumerate(sizes):
                final = ending == 'final' and i == len(sizes) - 1
                x = rng.uniform(-1, 1, (3, b, 2))
                out = stream.process(x, final=final) if final else stream.process(x)
                if stream is velvet:
                    first, end = output_span(pos, b, H, final)
                    want = end - first
                else:
                    want = b + (D if final else 0)
                assert out.shape == (3, want, 2) and out.dtype == dtype, (i, b, out.shape)
                pos += b
                total += want
                assert stream.position == pos
            if ending == 'flush':
                out = stream.flush()
                want = (pos - max(0, pos - H)) if stream is velvet else D
                assert out.shape == (3, want, 2)
                total += want
            assert total == pos + (0 if stream is velvet else D)
            with pytest.raises(RuntimeError):
                stream.process(np.zeros((3, 1, 2)))
            stream.reset()
        # every recorded call agrees with the span it was given, and a call of no frames and no outputs made none
        for n_in, n_out, final in record.calls:
            assert n_in or n_out
            assert n_in <= M


def test_block_checks(dec, no_device):
    s = dec.decorrelate_each_stream(_velvets(dec, (0.1, 0.5)), in_channels=2, max_frames_per_call=100)
    for bad in (np.zeros((3, 10, 2)), np.zeros((2, 10, 1)), np.zeros((10, 2)), np.zeros((2, 101, 2))):
        with pytest.raises(ValueError):
            s.process(bad)
    with pytest.raises(TypeError):
        s.process(np.zeros((2, 10, 2), complex))
    assert s.process(np.zeros((2, 0, 2), np.int16)).shape == (2, 0, 2)      # any real dtype; no frames, no device call
    assert s.position == 0


def test_exported_from_the_package():
    import vndecorrelate_amd
    assert callable(vndecorrelate_amd.decorrelate_each_stream)
    assert issubclass(vndecorrelate_amd.EachStream, vndecorrelate_amd.Stream)
    assert issubclass(vndecorrelate_amd.HaasEachStream, vndecorrelate_amd.HaasStream)
