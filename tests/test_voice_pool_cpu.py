"""CPU tier of the voice pool (include/vnd_voice_stream.h, decorrelation.decorrelate_voice_pool, streaming.VoicePool):
voice_spans against a brute-force model that runs every voice alone through streaming.output_span, the dict form's
bookkeeping and every refusal over a fake native, and the header against its binding - no device call."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_voice_stream.h'
FS, DURATION, IMPULSES, SEED = 16000, 0.02, 15, 1
NAMES = ['vnd_voice_stream_f32_dev', 'vnd_voice_stream_f32_host', 'vnd_voice_stream_reset_dev', 'vnd_voice_stream_state_bytes']
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
def dec():
    import vndecorrelate_amd.decorrelation as decorrelation
    return decorrelation


@pytest.fixture
def no_device(monkeypatch):
    """Any touch of the device raises: the refusals and the bookkeeping below come before it."""
    from vndecorrelate_amd import _native

    def touched(*args, **kwargs):
        raise AssertionError('the device was touched')
    for name in ('default_context', 'context_for', 'voice_stream_host', 'voice_stream_device', 'voice_stream_reset_device',
                 'voice_stream_state_bytes'):
        monkeypatch.setattr(_native, name, touched)


def _velvets(dec, kappas, **kw):
    base = dict(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None)
    base.update(kw)
    return [dec.VelvetNoise(log_distribution_strength=k, **base) for k in kappas]


# ---- voice_spans -----------------------------------------------------------------------------------------------------
class _Voice:
    """One voice alone, as a lockstep stream sees it: a position and streaming.output_span."""

    def __init__(self, H):
        self.H, self.pos = H, 0

    def call(self, n, flags):
        from vndecorrelate_amd.streaming import output_span
        if flags & START:
            self.pos = 0                                   # whatever the slot held is discarded, unflushed
        first, end = output_span(self.pos, n, self.H, bool(flags & END))
        self.pos = 0 if flags & END else self.pos + n
        return end - first


@pytest.mark.parametrize('seed', range(8))
def test_voice_spans_equal_every_voice_alone(seed):
    from vndecorrelate_amd.streaming import voice_spans
    rng = np.random.default_rng(seed)
    S, H, M = 7, int(rng.choice([0, 1, 37, 300])), 96
    voices = [_Voice(H) for _ in range(S)]
    pos = np.zeros(S, np.int64)
    menu = [0, 0, 1, H, H + 1, M, 17]
    for call in range(60):
        counts = np.array([min(M, int(rng.choice(menu + [int(rng.integers(0, M + 1))]))) for _ in range(S)], np.int32)
        flags = rng.choice([0, 0, 0, 0, START, END, START | END], S).astype(np.int32)
        counts[rng.random(S) < 0.25] = 0                                  # idle slots, flagged or not
        out, new = voice_spans(pos, counts, flags, H)
        want = [v.call(int(n), int(f)) for v, n, f in zip(voices, counts, flags)]
        assert out.tolist() == want, (call, counts, flags)
        assert new.tolist() == [v.pos for v in voices], call
        assert (out <= counts + np.minimum(np.where(flags & START, 0, pos), H)).all() and (out >= 0).all()
        idle = (counts == 0) & (flags == 0)
        assert (out[idle] == 0).all() and (new[idle] == pos[idle]).all()  # an idle slot does nothing: its position stays
        pos = new


def test_voice_spans_edge_rows():
    from vndecorrelate_amd.streaming import voice_spans
    H = 300

    def one(p, n, f):
        out, new = voice_spans([p], [n], [f], H)
        assert out.dtype == np.int64 and new.dtype == np.int64
        return int(out[0]), int(new[0])
    # END with n = 0 flushes the tail, min(p, H) frames
    assert one(0, 0, END) == (0, 0)
    assert one(200, 0, END) == (200, 0)
    assert one(300, 0, END) == (300, 0)
    assert one(1000, 0, END) == (300, 0)
    # START with END in one call: a whole voice in one block, whatever the slot held
    assert one(0, 50, START | END) == (50, 0)
    assert one(777, 50, START | END) == (50, 0)
    assert one(777, 0, START | END) == (0, 0)
    # START alone discards: the position restarts
    assert one(777, 50, START) == (0, 50)
    assert one(777, 350, START) == (50, 350)
    # a plain call below, across and above the latency
    assert one(0, 300, 0) == (0, 300)
    assert one(0, 301, 0) == (1, 301)
    assert one(250, 100, 0) == (50, 350)
    assert one(1000, 480, 0) == (480, 1480)
    assert one(1000, 480, END) == (780, 0)
    # a bad count answers -1 and leaves the position
    out, new = voice_spans([40, 40, 40], [-1, 97, 96], [0, START, 0], H, max_frames_per_call=96)
    assert out.tolist() == [-1, -1, 0] and new.tolist() == [40, 40, 136]
    with pytest.raises(ValueError):
        voice_spans([0, 0], [1], [0], H)


def test_voice_spans_at_the_positions_of_a_long_lived_voice():
    """Around 2^31, 2^32 and at the last position taken, 2^60, against Python's own integers; 2^60 + 1 is refused unless
    the call STARTs over it."""
    from vndecorrelate_amd.streaming import output_span, voice_spans
    H, M = 300, 480
    top = 1 << 60
    positions = [2 ** 31 - 7, 2 ** 31, 2 ** 32 - 300, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 2 ** 40 + 3, 2 ** 53 + 1,
                 top - M, top - 1, top]
    for n, f in ((0, 0), (7, 0), (M, 0), (0, END), (M, END), (301, START), (M, START | END)):
        out, new = voice_spans(positions, [n] * len(positions), [f] * len(positions), H, M)
        assert out.dtype == new.dtype == np.int64
        for p, got, after in zip(positions, out.tolist(), new.tolist()):
            at = 0 if f & START else p
            first, end = output_span(at, n, H, bool(f & END))
            assert (got, after) == (end - first, 0 if f & END else at + n), (p, n, f)
    # a steady-state call returns what it was given; an END returns the tail too - at any of these positions
    out, new = voice_spans(positions, [M] * len(positions), [0] * len(positions), H, M)
    assert out.tolist() == [M] * len(positions) and (new - np.array(positions) == M).all()
    assert new[-1] == top + M                                          # the next call of that slot is the refused one
    # outside [0, 2^60] without START: -1 and the position stays; START discards it like any other position
    bad = [top + 1, top + M, 2 ** 62, -1, -2 ** 63]
    out, new = voice_spans(bad, [7] * 5, [0, END, 0, 0, END], H, M)
    assert out.tolist() == [-1] * 5 and new.tolist() == bad
    out, new = voice_spans(bad, [7] * 5, [START, START | END, START, START, START], H, M)
    assert out.tolist() == [0, 7, 0, 0, 0] and new.tolist() == [7, 0, 7, 7, 7]


# ---- VoicePool over a fake native ------------------------------------------------------------------------------------
class _FakeNative:
    """Stands for the device under a real pool: records what every call uploads and answers with the spans of a
    position of its own per slot (the device's), and rows that name the slot and the call."""

    def __init__(self, pool):
        self.pool, self.calls = pool, []
        self.pos = np.zeros(pool.slots, np.int64)
        pool._call_host = self._call

    def _call(self, x, counts, flags, tables):
        from vndecorrelate_amd.streaming import voice_spans
        p = self.pool
        assert x.shape == (p.slots, p.max_frames_per_call, p.in_channels) and x.dtype == np.float32
        assert counts.dtype == flags.dtype == tables.dtype == np.int32
        self.calls.append((x.copy(), counts.copy(), flags.copy(), tables.copy()))
        out, self.pos = voice_spans(self.pos, counts, flags, p.latency_frames, p.max_frames_per_call)
        y = np.full((p.slots, p.row_frames, 2), np.nan, np.float32)
        for b, n in enumerate(out):
            y[b, :n] = 1000 * len(self.calls) + b
        return y, out.astype(np.int32)


def test_bookkeeping_over_a_schedule(dec, no_device):
    bank = _velvets(dec, (0.1, 0.5, 0.9, 0.5))                       # 1 and 3 share a table: 3 candidates
    pool = dec.decorrelate_voice_pool(bank, slots=4, in_channels=2, max_frames_per_call=100)
    assert pool.bank_tables.tolist() == [0, 1, 2, 1] and pool.num_tables == 3
    H = pool.latency_frames
    assert 200 < H < 320 and pool.row_frames == 100 + H
    fake = _FakeNative(pool)
    rng = np.random.default_rng(0)

    def block(n):
        return rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    assert pool.process({}) == {} and not fake.calls                  # nothing pushed, started or ended: no device call
    a, b = block(100), block(7)
    out = pool.process({0: a, 2: b}, start={0: 3, 2: 2})
    assert sorted(out) == [0, 2] and out[0].shape == (0, 2) and out[2].shape == (0, 2)
    x, counts, flags, tables = fake.calls[-1]
    assert counts.tolist() == [100, 0, 7, 0] and flags.tolist() == [START, 0, START, 0]
    assert tables[0] == 1 and tables[2] == 2
    assert x[0].tobytes() == a.tobytes() and x[2, :7].tobytes() == b.tobytes() and not x[2, 7:].any() and not x[1].any()
    for _ in range(3):                                                # slot 0 advances alone; slot 2 is idle
        out = pool.process({0: block(100)})
    assert sorted(out) == [0] and out[0].shape == (400 - H - max(0, 300 - H), 2)
    assert fake.calls[-1][1].tolist() == [100, 0, 0, 0] and not fake.calls[-1][2].any()
    assert pool.positions.tolist() == [400, 0, 7, 0] and pool.live.tolist() == [True, False, True, False]
    out = pool.process({0: block(0)})                                 # an empty block of a live voice: no device call
    assert out[0].shape == (0, 2) and len(fake.calls) == 4
    # slot 2 ends with no block (its tail: 7 frames), slot 1 is a whole voice in one call, slot 0 ends with its last block
    out = pool.process({1: block(33), 0: block(5)}, start={1: 0}, end=[2, 1, 0])
    assert {s: o.shape[0] for s, o in out.items()} == {0: 5 + H, 1: 33, 2: 7}
    assert (out[1] == 1000 * len(fake.calls) + 1).all()               # rows of slot 1, of this call
    assert fake.calls[-1][1].tolist() == [5, 33, 0, 0] and fake.calls[-1][2].tolist() == [END, START | END, END, 0]
    assert not pool.live.any() and not pool.positions.any()
    # the slot goes to another voice with another table; the table of the ended voice is not sent again by name
    pool.process({2: block(10)}, start={2: 0})
    assert fake.calls[-1][3][2] == 0 and fake.calls[-1][2].tolist() == [0, 0, START, 0]
    # a live voice is dropped, unflushed, only on request
    with pytest.raises(ValueError, match='slot 2 holds a live voice'):
        pool.process({2: block(10)}, start={2: 1})
    pool.process({2: block(10)}, start={2: 1}, discard=True)
    assert fake.calls[-1][3][2] == 1 and pool.positions[2] == 10
    assert pool.positions.tolist() == fake.pos.tolist()               # the mirror is the device's


def test_every_refusal_comes_before_the_native(dec, no_device):
    pool = dec.decorrelate_voice_pool(_velvets(dec, (0.1, 0.5)), slots=3, in_channels=2, max_frames_per_call=100)
    fake = _FakeNative(pool)
    ok = np.zeros((10, 2), np.float32)
    pool.process({0: ok}, start={0: 0})
    before = (pool.positions.copy(), pool.live.copy(), pool.tables.copy(), len(fake.calls))
    for kwargs, error, text in (
            (dict(blocks={1: ok}), ValueError, 'slot 1, which was never started'),
            (dict(end=[1]), ValueError, 'end of slot 1, which was never started'),
            (dict(blocks={0: ok}, start={0: 1}), ValueError, 'holds a live voice'),
            (dict(blocks={0: np.zeros((101, 2), np.float32)}), ValueError, 'above max_frames_per_call=100'),
            (dict(blocks={0: np.zeros((10, 2), np.float64)}), TypeError, 'float32'),
            (dict(blocks={0: np.zeros((10, 2), np.int16)}), TypeError, 'float32'),
            (dict(blocks={0: np.zeros((10, 1), np.float32)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={0: np.zeros(10, np.float32)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={0: np.zeros((1, 10, 2), np.float32)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={3: ok}), ValueError, 'outside the pool of 3 slots'),
            (dict(blocks={-1: ok}), ValueError, 'outside the pool'),
            (dict(start={1: 2}), ValueError, 'outside the bank of 2'),
            (dict(start={1: -1}), ValueError, 'outside the bank'),
            (dict(start={1: 0.0}), ValueError, 'outside the bank'),
            (dict(start={True: 0}), ValueError, 'outside the pool'),
            (dict(end=[0, 0]), ValueError, 'named twice'),
            (dict(blocks={0: ok, 1: ok}, start={2: 0}), ValueError, 'slot 1, which was never started')):
        with pytest.raises(error, match=text):
            pool.process(kwargs.get('blocks'), start=kwargs.get('start'), end=kwargs.get('end', ()))
        assert len(fake.calls) == before[3], kwargs
        assert pool.positions.tolist() == before[0].tolist() and pool.live.tolist() == before[1].tolist()
        assert pool.tables.tolist() == before[2].tolist()
    # a native that answers other counts than the spans is an error, and the mirror stays
    pool._call_host = lambda x, c, f, t: (np.zeros((3, pool.row_frames, 2), np.float32), np.array([1, 0, 0], np.int32))
    from vndecorrelate_amd import _native
    with pytest.raises(_native.NativeError, match='the spans are'):
        pool.process({0: ok})
    assert pool.positions.tolist() == before[0].tolist()


def test_mono_blocks_and_mixing_the_forms(dec, no_device):
    pool = dec.decorrelate_voice_pool(_velvets(dec, (0.3,)), slots=2, in_channels=1, max_frames_per_call=64)
    fake = _FakeNative(pool)
    a = np.arange(5, dtype=np.float32)
    pool.process({1: a}, start={1: 0})                               # (n,) for a mono pool
    pool.process({1: a[:, None]})
    assert fake.calls[0][0][1, :5, 0].tolist() == a.tolist() and fake.calls[1][0].shape == (2, 64, 1)
    with pytest.raises(RuntimeError, match='runs through process'):
        pool.process_dev(None, None, None, None)                      # refused before the tensors are looked at
    other = dec.decorrelate_voice_pool(_velvets(dec, (0.3,)), slots=2, in_channels=1, max_frames_per_call=64)
    other._form = 'dev'                                               # what a process_dev call leaves behind
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        other.process({0: a}, start={0: 0})
    with pytest.raises(ValueError, match='x must be a device tensor'):
        other.process_dev(np.zeros((2, 64, 1), np.float32), None, None, None)


def test_the_entry_checks_its_bank_like_decorrelate_each_stream(dec, no_device):
    make = dec.decorrelate_voice_pool
    ks = (0.1, 0.5, 0.9)
    with pytest.raises(ValueError, match='at least one decorrelator'):
        make([], slots=2)
    with pytest.raises(TypeError, match='HaasEffect'):
        make(_velvets(dec, ks[:2]) + [dec.HaasEffect(sample_rate_hz=FS)], slots=2)
    for bad in (0, 3, True, None):
        with pytest.raises(ValueError, match='in_channels'):
            make(_velvets(dec, ks), slots=2, in_channels=bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match='slots'):
            make(_velvets(dec, ks), slots=bad)
        with pytest.raises(ValueError, match='max_frames_per_call'):
            make(_velvets(dec, ks), slots=2, max_frames_per_call=bad)
    with pytest.raises(ValueError, match='split the pool'):
        make(_velvets(dec, ks), slots=65536)
    with pytest.raises(ValueError, match='normalizer=None'):
        make(_velvets(dec, ks, normalizer=dec.rms_normalize), slots=2)
    mixed = _velvets(dec, ks)
    mixed[2].width = 0.3
    with pytest.raises(ValueError, match='decorrelate_voice_pool: width differs across the list.*bank entry 2'):
        make(mixed, slots=2)
    with pytest.raises(ValueError, match='bank entry 0: its table reaches past 4094'):
        make(_velvets(dec, ks, sample_rate_hz=44100, duration_seconds=0.1, num_impulses=30), slots=2)
    pool = make(_velvets(dec, ks, mode='LR', width=0.35), slots=5, in_channels=1, max_frames_per_call=480)
    assert (pool.slots, pool.in_channels, pool.max_frames_per_call, pool.num_channels) == (5, 1, 480, 2)
    assert (pool.ms_encode, pool.width, pool.mode) == (False, 0.35, dec.MODE_EXACT)
    assert make(_velvets(dec, ks), slots=1).ms_encode is True


def test_exported_from_the_package():
    import vndecorrelate_amd
    assert callable(vndecorrelate_amd.decorrelate_voice_pool) and callable(vndecorrelate_amd.voice_spans)
    assert vndecorrelate_amd.VoicePool.__name__ == 'VoicePool'


# ---- header and binding ----------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    src = ('#include "vnd_voice_stream.h"\n'
           'int main(void){return VND_VOICE_START == 1 && VND_VOICE_END == 2 && VND_MAX_STREAMS == 65535 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_voice_stream.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))       # vnd_amd.h keeps its fixed set
    assert (_native.VOICE_START, _native.VOICE_END) == (START, END)
    for wrapper in ('voice_stream_state_bytes', 'voice_stream_reset_device', 'voice_stream_device', 'voice_stream_host'):
        assert callable(getattr(_native, wrapper))
    # the planner's description: declared beside the each-stream's, exported and bound
    internal = _declared(REPO / 'include' / 'vnd_amd_internal.h')
    assert 'vnd_describe_voice_stream_launch' in internal and 'vnd_describe_each_stream_launch' in internal
    assert hasattr(lib, 'vnd_describe_voice_stream_launch')
    assert 'vnd_describe_voice_stream_launch' in _native.INTERNAL_SIGNATURES
    assert callable(_native.TapTable.describe_voice_stream)


def test_checks_that_need_no_device(lib):
    null = ctypes.c_void_p(None)
    call = (null, 0, 480, null, null, null, null, null, null, 4, 2, 0, 0, 0, 0.0)
    assert lib.vnd_voice_stream_f32_dev(null, null, *call, null) == INVALID
    assert b'null context' in lib.vnd_last_error()
    assert lib.vnd_voice_stream_f32_host(null, null, *call) == INVALID
    assert b'null context' in lib.vnd_last_error()
    assert lib.vnd_voice_stream_reset_dev(null, null, 0, 4, 2, null, 480, null) == INVALID
    got = ctypes.c_int64(-7)
    assert lib.vnd_voice_stream_state_bytes(null, 4, 2, 480, ctypes.byref(got)) == INVALID
    assert b'null tap table' in lib.vnd_last_error()
    text = ctypes.create_string_buffer(64)
    assert lib.vnd_describe_voice_stream_launch(null, null, 480, 4, 2, 0, 0, text, 64) == INVALID
    assert b'null context' in lib.vnd_last_error() and not text.value
    assert lib.vnd_describe_voice_stream_launch(null, null, 480, 4, 2, 0, 0, None, 64) == INVALID
    assert b'null text' in lib.vnd_last_error()
