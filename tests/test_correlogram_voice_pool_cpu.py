"""CPU tier of the correlogram voice pool (include/vnd_correlogram_voice_stream.h, analysis.cross_correlogram_voice_pool,
analysis.CorrelogramVoicePool): correlogram_voice_spans against every voice alone through analysis.stream_rows, the bound
on the rows of a call over an exhaustive grid, the dict form's bookkeeping and every refusal over a fake native, and the
header against its binding - no device call."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_correlogram_voice_stream.h'
NAMES = ['vnd_correlogram_voice_stream_f32_dev', 'vnd_correlogram_voice_stream_f64_dev',
         'vnd_correlogram_voice_stream_reset_dev', 'vnd_correlogram_voice_stream_state_bytes']
INVALID, UNSUPPORTED = 1, 4
START, END = 1, 2


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
def an():
    from vndecorrelate_amd import analysis
    return analysis


@pytest.fixture
def no_device(monkeypatch):
    """Any touch of the device raises: the refusals and the bookkeeping below come before it."""
    from vndecorrelate_amd import _native

    def touched(*args, **kwargs):
        raise AssertionError('the device was touched')
    for name in ('default_context', 'context_for', 'correlogram_voice_stream_device', 'correlogram_voice_stream_reset_device',
                 'correlogram_voice_stream_state_bytes'):
        monkeypatch.setattr(_native, name, touched)


# ---- correlogram_voice_spans -----------------------------------------------------------------------------------------
class _Voice:
    """One voice alone, as a lockstep stream sees it: a position in Python integers and analysis.stream_rows."""

    def __init__(self, W, H, pos=0):
        self.W, self.H, self.pos = W, H, pos

    def call(self, n, flags):
        from vndecorrelate_amd.analysis import stream_rows
        if flags & START:
            self.pos = 0                                   # whatever the slot held is dropped
        first, end = stream_rows(self.pos, n, self.W, self.H)
        self.pos = 0 if flags & END else self.pos + n
        return end - first


@pytest.mark.parametrize('W,H', [(64, 24), (100, 250), (64, 1), (1, 1), (1, 7), (882, 441), (5, 5)])
@pytest.mark.parametrize('seed', range(3))
def test_spans_equal_every_voice_alone(an, W, H, seed):
    rng = np.random.default_rng(1000 * seed + W + H)
    S, M = 7, 96
    voices = [_Voice(W, H) for _ in range(S)]
    pos = np.zeros(S, np.int64)
    menu = [0, 0, 1, min(H, M), min(max(W - 1, 0), M), M, 17]
    for call in range(80):
        counts = np.array([int(rng.choice(menu + [int(rng.integers(0, M + 1))])) for _ in range(S)], np.int32)
        flags = rng.choice([0, 0, 0, 0, START, END, START | END, 4, 8 | START], S).astype(np.int32)     # other bits are ignored
        counts[rng.random(S) < 0.25] = 0                                  # idle slots, flagged or not
        out, new = an.correlogram_voice_spans(pos, counts, flags, W, H, M)
        assert out.dtype == new.dtype == np.int64
        want = [v.call(int(n), int(f)) for v, n, f in zip(voices, counts, flags)]
        assert out.tolist() == want, (call, counts, flags)
        assert new.tolist() == [v.pos for v in voices], call
        assert (out >= 0).all() and (out <= -(-M // H)).all()
        idle = (counts == 0) & ((flags & 3) == 0)
        assert (out[idle] == 0).all() and (new[idle] == pos[idle]).all()  # an idle slot does nothing: its position stays
        pos = new


def test_spans_edge_rows(an):
    W, H = 64, 24

    def one(p, n, f, M=600):
        out, new = an.correlogram_voice_spans([p], [n], [f], W, H, M)
        return int(out[0]), int(new[0])
    assert one(0, 63, 0) == (0, 63) and one(0, 64, 0) == (1, 64) and one(63, 1, 0) == (1, 64)
    assert one(64, 23, 0) == (0, 87) and one(64, 24, 0) == (1, 88)
    # END has no tail: what this call's frames completed, and the position back to 0; END with n = 0 returns 0 rows
    assert one(0, 0, END) == (0, 0) and one(87, 0, END) == (0, 0) and one(1000, 0, END) == (0, 0)
    assert one(87, 1, END) == (1, 0) and one(63, 0, END) == (0, 0)
    # START with END: a whole voice in one block, whatever the slot held; START alone drops it
    assert one(777, 64, START | END) == (1, 0) and one(777, 600, START | END) == (23, 0) and one(777, 0, START | END) == (0, 0)
    assert one(777, 63, START) == (0, 63) and one(777, 112, START) == (3, 112)
    # idle
    assert one(777, 0, 0) == (0, 777)
    # bad counts answer -1 and leave the position
    out, new = an.correlogram_voice_spans([40, 40, 40, 40, 40], [-1, 97, 96, 2 ** 31 - 1, -2 ** 31], [0, START, 0, END, 0], W, H, 96)
    assert out.tolist() == [-1, -1, 4, -1, -1] and new.tolist() == [40, 40, 136, 40, 40]   # wc(136) = 72 // 24 + 1
    with pytest.raises(ValueError):
        an.correlogram_voice_spans([0, 0], [1], [0], W, H)
    with pytest.raises(ValueError):
        an.correlogram_voice_spans([0], [1], [0], W, 0)


def test_spans_at_the_positions_of_a_long_lived_voice(an):
    """Around 2^31, 2^32 and at the last position taken, 2^60, against Python's own integers; 2^60 + 1 is refused unless
    the call STARTs over it."""
    top = 1 << 60
    for W, H, M in ((882, 441, 480), (64, 1, 600), (100, 250, 333), (1, 1, 7)):
        positions = [2 ** 31 - 7, 2 ** 31, 2 ** 32 - 300, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 2 ** 40 + 3, 2 ** 53 + 1,
                     top - M, top - 1, top]
        for n, f in ((0, 0), (7, 0), (M, 0), (0, END), (M, END), (min(M, W), START), (M, START | END)):
            out, new = an.correlogram_voice_spans(positions, [n] * len(positions), [f] * len(positions), W, H, M)
            for p, got, after in zip(positions, out.tolist(), new.tolist()):
                v = _Voice(W, H, p)
                assert (got, after) == (v.call(n, f), v.pos), (p, n, f)
        out, new = an.correlogram_voice_spans([top], [M], [0], W, H, M)
        assert new[0] == top + M                                       # the next call of that slot is the refused one
        bad = [top + 1, top + M, 2 ** 62, -1, -2 ** 63]
        out, new = an.correlogram_voice_spans(bad, [M] * 5, [0, END, 0, 0, END], W, H, M)
        assert out.tolist() == [-1] * 5 and new.tolist() == bad
        out, new = an.correlogram_voice_spans(bad, [M] * 5, [START, START | END, START, START, START], W, H, M)
        whole = _Voice(W, H).call(M, 0)
        assert out.tolist() == [whole] * 5 and new.tolist() == [M, 0, M, M, M]


def test_rows_per_call_bound_over_a_grid(an):
    """out_counts <= RC = ceil(M / H) for every p, H > W included - and the bound is met."""
    for W in (1, 2, 3, 5, 8):
        for H in (1, 2, 3, 4, 7, 11):
            for M in (1, 2, 3, 5, 9, 12):
                rc = -(-M // H)
                p = np.repeat(np.arange(0, 3 * (W + H) + 2), M + 1)
                n = np.tile(np.arange(0, M + 1), len(p) // (M + 1))
                out, new = an.correlogram_voice_spans(p, n, np.zeros_like(p), W, H, M)
                assert (out >= 0).all() and out.max() == rc, (W, H, M)
                assert (new == p + n).all()
    pool = an.CorrelogramVoicePool(3, window=5, hop=7, num_lags=9, epsilon=1e-10, max_frames_per_call=15)
    assert pool.rows_per_call == 3


# ---- the dict form over a fake native --------------------------------------------------------------------------------
class _FakeNative:
    """Stands for the device under a real pool: records what every call uploads and answers with the spans of a position
    of its own per slot (the device's), and rows that name the slot and the call."""

    def __init__(self, pool):
        self.pool, self.calls = pool, []
        self.pos = np.zeros(pool.slots, np.int64)
        pool._call_host = self._call

    def _call(self, x, counts, flags):
        from vndecorrelate_amd.analysis import correlogram_voice_spans
        p = self.pool
        assert x.shape == (p.slots, p.max_frames_per_call, 2) and x.dtype == np.float32
        assert counts.dtype == flags.dtype == np.int32
        self.calls.append((x.copy(), counts.copy(), flags.copy()))
        out, self.pos = correlogram_voice_spans(self.pos, counts, flags, p.window, p.hop, p.max_frames_per_call)
        y = np.full((p.slots, p.rows_per_call, p.num_lags), np.nan, np.float32)
        for b, n in enumerate(out):
            y[b, :n] = 1000 * len(self.calls) + b
        return y, out.astype(np.int32)


def _pool(an, slots=4, M=100, **kw):
    return an.CorrelogramVoicePool(slots, window=64, hop=24, num_lags=127, epsilon=1e-10, max_frames_per_call=M, **kw)


def test_bookkeeping_over_a_schedule(an, no_device):
    pool = _pool(an)
    assert pool.rows_per_call == 5 and pool.in_channels == 2
    fake = _FakeNative(pool)
    rng = np.random.default_rng(0)

    def block(n, dtype=np.float32):
        return rng.uniform(-1, 1, (n, 2)).astype(dtype)
    assert pool.process({}) == {} and not fake.calls                  # nothing pushed, started or ended: no device call
    a, b = block(100), block(7, np.float64)
    out = pool.process({0: a, 2: b}, start=[0, 2])
    assert sorted(out) == [0, 2] and out[0].shape == (2, 127) and out[2].shape == (0, 127) and out[0].dtype == np.float32
    x, counts, flags = fake.calls[-1]
    assert counts.tolist() == [100, 0, 7, 0] and flags.tolist() == [START, 0, START, 0]
    assert x[0].tobytes() == a.tobytes() and x[2, :7].tobytes() == b.astype(np.float32).tobytes()     # float64: cast as astype
    assert not x[2, 7:].any() and not x[1].any()
    for _ in range(3):                                                # slot 0 advances alone; slot 2 is idle
        out = pool.process({0: block(100)})
    assert sorted(out) == [0] and out[0].shape == ((400 - 64) // 24 + 1 - ((300 - 64) // 24 + 1), 127)
    assert pool.positions.tolist() == [400, 0, 7, 0] and pool.live.tolist() == [True, False, True, False]
    out = pool.process({0: block(0)})                                 # an empty block of a live voice: no device call
    assert out[0].shape == (0, 127) and len(fake.calls) == 4
    # slot 2 ends with no block (no tail: 0 rows), slot 1 is a whole voice in one call, slot 0 ends with its last block
    out = pool.process({1: block(88), 0: block(5)}, start=[1], end=[2, 1, 0])
    assert {s: o.shape[0] for s, o in out.items()} == {0: 0, 1: 2, 2: 0}
    assert (out[1] == 1000 * len(fake.calls) + 1).all()               # rows of slot 1, of this call
    assert fake.calls[-1][1].tolist() == [5, 88, 0, 0] and fake.calls[-1][2].tolist() == [END, START | END, END, 0]
    assert not pool.live.any() and not pool.positions.any()
    # a live voice is dropped only on request
    pool.process({2: block(10)}, start=[2])
    with pytest.raises(ValueError, match='slot 2 holds a live voice'):
        pool.process({2: block(10)}, start=[2])
    pool.process({2: block(10)}, start=[2], discard=True)
    assert fake.calls[-1][2].tolist() == [0, 0, START, 0] and pool.positions[2] == 10
    assert pool.positions.tolist() == fake.pos.tolist()               # the mirror is the device's


def test_every_refusal_comes_before_the_native(an, no_device):
    pool = _pool(an, slots=3)
    fake = _FakeNative(pool)
    ok = np.zeros((10, 2), np.float32)
    pool.process({0: ok}, start=[0])
    before = (pool.positions.copy(), pool.live.copy(), len(fake.calls))
    for kwargs, error, text in (
            (dict(blocks={1: ok}), ValueError, 'slot 1, which was never started'),
            (dict(end=[1]), ValueError, 'end of slot 1, which was never started'),
            (dict(blocks={0: ok}, start=[0]), ValueError, 'holds a live voice'),
            (dict(blocks={0: np.zeros((101, 2), np.float32)}), ValueError, 'above max_frames_per_call=100'),
            (dict(blocks={0: np.zeros((10, 2), np.int16)}), TypeError, 'float32'),
            (dict(blocks={0: np.zeros((10, 2), np.complex64)}), TypeError, 'float32'),
            (dict(blocks={0: np.zeros((10, 1), np.float32)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={0: np.zeros(10, np.float32)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={0: np.zeros((1, 10, 2), np.float64)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={3: ok}), ValueError, 'outside the pool of 3 slots'),
            (dict(blocks={-1: ok}), ValueError, 'outside the pool'),
            (dict(start=[3]), ValueError, 'outside the pool'),
            (dict(start=[True]), ValueError, 'outside the pool'),
            (dict(start=[1.0]), ValueError, 'outside the pool'),
            (dict(start=[1, 1]), ValueError, 'named twice'),
            (dict(end=[0, 0]), ValueError, 'named twice'),
            (dict(blocks={0: ok, 1: ok}, start=[2]), ValueError, 'slot 1, which was never started')):
        with pytest.raises(error, match=text):
            pool.process(kwargs.get('blocks'), start=kwargs.get('start', ()), end=kwargs.get('end', ()))
        assert len(fake.calls) == before[2], kwargs
        assert pool.positions.tolist() == before[0].tolist() and pool.live.tolist() == before[1].tolist()
    # a native that answers other counts than the spans is an error, and the mirror stays
    pool._call_host = lambda x, c, f: (np.zeros((3, pool.rows_per_call, 127), np.float32), np.array([1, 0, 0], np.int32))
    from vndecorrelate_amd import _native
    with pytest.raises(_native.NativeError, match='the spans are'):
        pool.process({0: ok})
    assert pool.positions.tolist() == before[0].tolist()


def test_mixing_the_forms(an, no_device):
    pool = _pool(an, slots=2)
    _FakeNative(pool)
    pool.process({1: np.zeros((5, 2), np.float32)}, start=[1])
    with pytest.raises(RuntimeError, match='runs through process'):
        pool.process_dev(None, None, None)                            # refused before the tensors are looked at
    other = _pool(an, slots=2, dtype='float64')
    other._form = 'dev'                                               # what a process_dev call leaves behind
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        other.process({0: np.zeros((5, 2), np.float32)}, start=[0])
    with pytest.raises(ValueError, match='x must be a device tensor'):
        other.process_dev(np.zeros((2, 100, 2), np.float64), None, None)


def test_construction_refusals(an, no_device):
    make = an.cross_correlogram_voice_pool
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='slots'):
            make(bad)
        with pytest.raises(ValueError, match='max_frames_per_call'):
            make(2, max_frames_per_call=bad)
    with pytest.raises(ValueError, match='split the pool'):
        make(65536)
    with pytest.raises(ValueError, match='counts are int32'):
        make(2, max_frames_per_call=2 ** 31)
    with pytest.raises(ValueError, match='correlogram_covers'):
        make(2, window_size_seconds=1.0)                              # 44100 samples: above MAX_WINDOW
    with pytest.raises(ValueError, match='correlogram_covers'):
        make(2, epsilon=np.float32(1e-10))                            # a NumPy scalar changes the promotion
    with pytest.raises(ValueError, match='correlogram_covers'):
        an.CorrelogramVoicePool(2, window=64, hop=0, num_lags=127, epsilon=1e-10, max_frames_per_call=100)
    for bad in ('float16', 'int32', None, 'nothing'):
        with pytest.raises(ValueError, match='dtype'):
            make(2, dtype=bad)
    with pytest.raises(ValueError, match='more than one launch takes'):
        an.CorrelogramVoicePool(2, window=64, hop=1, num_lags=127, epsilon=1e-10, max_frames_per_call=2 ** 20)
    pool = make(5, sample_rate_hz=16000, max_frames_per_call=480, dtype=np.float64)
    assert (pool.slots, pool.window, pool.hop, pool.num_lags, pool.rows_per_call) == (5, 320, 160, 641, 3)
    assert pool.dtype == np.float64 and make(1).dtype == np.float32 and make(1).max_frames_per_call == 4800


def test_exported_from_the_package():
    import vndecorrelate_amd
    assert callable(vndecorrelate_amd.cross_correlogram_voice_pool) and callable(vndecorrelate_amd.correlogram_voice_spans)
    assert vndecorrelate_amd.CorrelogramVoicePool.__name__ == 'CorrelogramVoicePool'
    from vndecorrelate_amd import analysis
    assert {'cross_correlogram_voice_pool', 'CorrelogramVoicePool', 'correlogram_voice_spans'} <= set(analysis.__all__)


# ---- header and binding ----------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    src = ('#include "vnd_correlogram_voice_stream.h"\n'
           'int main(void){return VND_VOICE_START == 1 && VND_VOICE_END == 2 && VND_CORRELOGRAM_MAX_WINDOW == 16384 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_correlogram_voice_stream.h but not exported'
    for fixed in ('vnd_amd.h', 'vnd_analysis.h'):                                     # both keep their fixed sets
        assert not set(names) & set(_declared(REPO / 'include' / fixed))
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    assert '#include "vnd_correlogram_stream.h"' in text and '#include "vnd_voice_stream.h"' in text
    for wrapper in ('correlogram_voice_stream_state_bytes', 'correlogram_voice_stream_reset_device',
                    'correlogram_voice_stream_device', 'describe_correlogram_voice_stream'):
        assert callable(getattr(_native, wrapper))
    internal = _declared(REPO / 'include' / 'vnd_amd_internal.h')
    assert 'vnd_describe_correlogram_voice_stream_launch' in internal and 'vnd_describe_voice_stream_launch' in internal
    assert hasattr(lib, 'vnd_describe_correlogram_voice_stream_launch')
    assert 'vnd_describe_correlogram_voice_stream_launch' in _native.INTERNAL_SIGNATURES


def test_checks_and_plans_that_need_no_device(lib):
    from vndecorrelate_amd import _native
    null = ctypes.c_void_p(None)
    for fn in (lib.vnd_correlogram_voice_stream_f32_dev, lib.vnd_correlogram_voice_stream_f64_dev):
        assert fn(null, null, 0, 480, null, null, 960, 2, null, null, null, null, 4, 64, 24, 127, 1e-10, null) == INVALID
        assert b'null context' in lib.vnd_last_error()
    assert lib.vnd_correlogram_voice_stream_reset_dev(null, null, 0, 4, 64, 480, null) == INVALID
    got = ctypes.c_int64(-7)
    assert lib.vnd_correlogram_voice_stream_state_bytes(4, 64, 480, ctypes.byref(got)) == 0
    assert got.value == 32 + 4 * (63 + 480) * 8
    assert lib.vnd_correlogram_voice_stream_state_bytes(3, 1, 5, ctypes.byref(got)) == 0
    assert got.value == 32 + 3 * 5 * 8                                                # 24 bytes of positions, padded to 32
    assert lib.vnd_correlogram_voice_stream_state_bytes(0, 64, 480, ctypes.byref(got)) == INVALID and got.value == 0
    assert lib.vnd_correlogram_voice_stream_state_bytes(4, 64, 480, None) == INVALID
    assert lib.vnd_correlogram_voice_stream_state_bytes(65536, 64, 480, ctypes.byref(got)) == UNSUPPORTED
    assert lib.vnd_correlogram_voice_stream_state_bytes(4, 16385, 480, ctypes.byref(got)) == UNSUPPORTED
    text = _native.describe_correlogram_voice_stream(512, 882, 441, 1765, 480)
    assert text == ('correlogram_voice_stream rows_per_call=2 groups=1 tiles=2 nblocks=1024 threads=256 advance_groups=2')
    assert 'rows_per_call=11 groups=3 tiles=2 nblocks=12288' in _native.describe_correlogram_voice_stream(2048, 882, 441, 1765, 4800)
    buf = ctypes.create_string_buffer(64)
    assert lib.vnd_describe_correlogram_voice_stream_launch(4, 64, 24, 127, 480, None, 64) == INVALID
    assert b'null text' in lib.vnd_last_error()
    assert lib.vnd_describe_correlogram_voice_stream_launch(4, 64, 0, 127, 480, buf, 64) == INVALID and not buf.value
    assert lib.vnd_describe_correlogram_voice_stream_launch(4, 64, 1, 127, 2 ** 20, buf, 64) == UNSUPPORTED and not buf.value
