"""CPU tier of the Haas and chain voice pools (include/vnd_haas_voice_stream.h, decorrelation.decorrelate_voice_pool,
streaming.HaasVoicePool / ChainVoicePool): haas_voice_spans against a brute-force model that runs every voice alone through
streaming.haas_output_span, the dict forms' bookkeeping and every refusal over a fake native, the bank refusals, and the
header against its binding - no device call."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_haas_voice_stream.h'
FS, DURATION, IMPULSES, SEED = 16000, 0.02, 15, 1
NAMES = ['vnd_haas_voice_stream_f64_dev', 'vnd_haas_voice_stream_f64_host', 'vnd_haas_voice_stream_reset_dev',
         'vnd_haas_voice_stream_state_bytes']
INVALID, UNSUPPORTED = 1, 4
START, END = 1, 2
TOP = 1 << 60


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
                 'voice_stream_state_bytes', 'haas_voice_stream_host', 'haas_voice_stream_device',
                 'haas_voice_stream_reset_device', 'haas_voice_stream_state_bytes', 'torch_module'):
        monkeypatch.setattr(_native, name, touched)


def _haases(dec, delays, **kw):
    base = dict(sample_rate_hz=1000, delayed_channel=1, mode='LR')
    base.update(kw)
    return [dec.HaasEffect(delay_time_seconds=d / 1000, **base) for d in delays]


def _chains(dec, kappas, delays, velvet=None, haas=None):
    out = []
    for k, d in zip(kappas, delays):
        v = dict(duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None, log_distribution_strength=k)
        v.update(velvet or {})
        h = dict(delay_time_seconds=d / FS, delayed_channel=1, mode='LR')
        h.update(haas or {})
        out.append(dec.SignalChain(sample_rate_hz=FS).velvet_noise(**v).haas_effect(**h))
    return out


# ---- haas_voice_spans ------------------------------------------------------------------------------------------------
class _Voice:
    """One voice alone, as a lockstep Haas stream sees it: a position and streaming.haas_output_span."""

    def __init__(self):
        self.pos = 0

    def call(self, n, flags, d):
        from vndecorrelate_amd.streaming import haas_output_span
        if flags & START:
            self.pos = 0                                   # whatever the slot held is discarded, unflushed
        first, end = haas_output_span(self.pos, n, d, bool(flags & END))
        assert first == self.pos
        self.pos = 0 if flags & END else self.pos + n
        return end - first


@pytest.mark.parametrize('seed', range(8))
def test_spans_equal_every_voice_alone(seed):
    from vndecorrelate_amd.streaming import haas_voice_spans
    rng = np.random.default_rng(seed)
    S, D, M = 7, int(rng.choice([0, 1, 37, 300])), 96
    voices = [_Voice() for _ in range(S)]
    pos = np.zeros(S, np.int64)
    delays = rng.integers(0, D + 1, S).astype(np.int32)
    for call in range(60):
        counts = np.array([min(M, int(rng.choice([0, 0, 1, D, D + 1, M, 17, int(rng.integers(0, M + 1))]))) for _ in range(S)],
                          np.int32)
        flags = rng.choice([0, 0, 0, 0, START, END, START | END], S).astype(np.int32)
        counts[rng.random(S) < 0.25] = 0                                  # idle slots, flagged or not
        fresh = (flags & START) != 0                                      # the delay changes with START only
        delays[fresh] = rng.integers(0, D + 1, int(fresh.sum()))
        out, new = haas_voice_spans(pos, counts, flags, delays, D, M)
        want = [v.call(int(n), int(f), int(d)) for v, n, f, d in zip(voices, counts, flags, delays)]
        assert out.tolist() == want, (call, counts, flags, delays)
        assert new.tolist() == [v.pos for v in voices], call
        assert (out <= counts + delays).all() and (out >= 0).all() and (out <= M + D).all()
        idle = (counts == 0) & (flags == 0)
        assert (out[idle] == 0).all() and (new[idle] == pos[idle]).all()  # an idle slot does nothing: its position stays
        pos = new


def test_spans_edge_rows():
    from vndecorrelate_amd.streaming import haas_voice_spans
    D, M = 300, 96

    def one(p, n, f, d):
        out, new = haas_voice_spans([p], [n], [f], [d], D, M)
        assert out.dtype == np.int64 and new.dtype == np.int64
        return int(out[0]), int(new[0])
    # idle: nothing, whatever the delay says
    assert one(40, 0, 0, 7) == (0, 40)
    assert one(40, 0, 0, -1) == (0, 40) and one(40, 0, 0, D + 1) == (0, 40)
    # END alone flushes the voice's own d tail frames - not max_delay, and whatever the position is
    assert one(0, 0, END, 7) == (7, 0)
    assert one(3, 0, END, 7) == (7, 0)
    assert one(1000, 0, END, 300) == (300, 0)
    assert one(1000, 0, END, 0) == (0, 0)
    # START with END: a whole voice in one block, one shorter than its delay included, whatever the slot held
    assert one(0, 50, START | END, 7) == (57, 0)
    assert one(777, 5, START | END, 300) == (305, 0)
    assert one(777, 0, START | END, 300) == (300, 0)
    # START over a live slot discards: the position restarts and nothing of the old voice comes out
    assert one(777, 50, START, 300) == (50, 50)
    assert one(777, 0, START, 300) == (0, 0)
    # d = 0, n below d, a plain call
    assert one(10, 96, 0, 0) == (96, 106) and one(10, 96, END, 0) == (96, 0)
    assert one(0, 5, 0, 300) == (5, 5) and one(5, 5, END, 300) == (305, 0)
    assert one(1000, 96, 0, 37) == (96, 1096)
    # a bad count answers -1 and leaves the position, with any flags
    out, new = haas_voice_spans([40] * 4, [-1, 97, 96, 97], [0, START, 0, START | END], [1] * 4, D, M)
    assert out.tolist() == [-1, -1, 96, -1] and new.tolist() == [40, 40, 136, 40]
    # a bad delay on a slot with work - frames, START or END - does the same
    out, new = haas_voice_spans([40] * 6, [5, 5, 0, 0, 0, 5], [0, 0, START, END, 0, END], [-1, D + 1, -1, D + 1, D + 1, D], D, M)
    assert out.tolist() == [-1, -1, -1, -1, 0, 5 + D] and new.tolist() == [40, 40, 40, 40, 40, 0]
    # without max_frames_per_call only a negative count is bad
    out, _ = haas_voice_spans([0, 0], [10 ** 6, -1], [0, 0], [0, 0], D)
    assert out.tolist() == [10 ** 6, -1]
    with pytest.raises(ValueError):
        haas_voice_spans([0, 0], [1, 1], [0, 0], [0], D)
    with pytest.raises(ValueError):
        haas_voice_spans([0, 0], [1], [0], [0, 0], D)


def test_spans_at_the_positions_of_a_long_lived_voice():
    """Around 2^31, 2^32 and at the last position taken, 2^60, against Python's own integers; 2^60 + 1 is refused unless
    the call STARTs over it."""
    from vndecorrelate_amd.streaming import haas_output_span, haas_voice_spans
    D, M, d = 300, 480, 257
    positions = [2 ** 31 - 7, 2 ** 31, 2 ** 32 - 300, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 2 ** 40 + 3, 2 ** 53 + 1,
                 TOP - M, TOP - 1, TOP]
    k = len(positions)
    for n, f in ((0, 0), (7, 0), (M, 0), (0, END), (M, END), (301, START), (M, START | END)):
        out, new = haas_voice_spans(positions, [n] * k, [f] * k, [d] * k, D, M)
        assert out.dtype == new.dtype == np.int64
        for p, got, after in zip(positions, out.tolist(), new.tolist()):
            at = 0 if f & START else p
            first, end = haas_output_span(at, n, d, bool(f & END))
            assert (got, after) == (end - first, 0 if f & END else at + n), (p, n, f)
    out, new = haas_voice_spans(positions, [M] * k, [0] * k, [d] * k, D, M)
    assert out.tolist() == [M] * k and (new - np.array(positions) == M).all()
    assert new[-1] == TOP + M                                          # the next call of that slot is the refused one
    bad = [TOP + 1, TOP + M, 2 ** 62, -1, -2 ** 63]
    out, new = haas_voice_spans(bad, [7] * 5, [0, END, 0, 0, END], [d] * 5, D, M)
    assert out.tolist() == [-1] * 5 and new.tolist() == bad
    out, new = haas_voice_spans(bad, [7] * 5, [START, START | END, START, START, START], [d] * 5, D, M)
    assert out.tolist() == [7, 7 + d, 7, 7, 7] and new.tolist() == [7, 0, 7, 7, 7]


# ---- HaasVoicePool over a fake native --------------------------------------------------------------------------------
class _FakeHaas:
    """Stands for the device under a real pool: records what every call uploads and answers with the spans of a
    position of its own per slot (the device's), and rows that name the slot and the call."""

    def __init__(self, pool):
        self.pool, self.calls = pool, []
        self.pos = np.zeros(pool.slots, np.int64)
        pool._call_host = self._call

    def _call(self, x, counts, flags, delays):
        from vndecorrelate_amd.streaming import haas_voice_spans
        p = self.pool
        assert x.shape == (p.slots, p.max_frames_per_call, p.in_channels) and x.dtype == np.float32
        assert counts.dtype == flags.dtype == delays.dtype == np.int32
        self.calls.append((x.copy(), counts.copy(), flags.copy(), delays.copy()))
        out, self.pos = haas_voice_spans(self.pos, counts, flags, delays, p.max_delay, p.max_frames_per_call)
        y = np.full((p.slots, p.row_frames, 2), np.nan, np.float64)
        for b, n in enumerate(out):
            y[b, :n] = 1000 * len(self.calls) + b
        return y, out.astype(np.int32)


def test_haas_bookkeeping_over_a_schedule(dec, no_device):
    from vndecorrelate_amd.streaming import HaasVoicePool
    bank = _haases(dec, (0, 30, 250, 30), width=0.4, mode='MS')
    pool = dec.decorrelate_voice_pool(bank, slots=4, in_channels=2, max_frames_per_call=100)
    assert type(pool) is HaasVoicePool and pool.bank_delays.tolist() == [0, 30, 250, 30] and pool.bank_delays.dtype == np.int32
    assert (pool.latency_frames, pool.tail_frames, pool.row_frames, pool.num_channels) == (0, 250, 350, 2)
    assert (pool.delayed_channel, pool.ms_mode, pool.width) == (1, True, 0.4)
    fake = _FakeHaas(pool)
    rng = np.random.default_rng(0)

    def block(n):
        return rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    assert pool.process({}) == {} and not fake.calls                  # nothing pushed, started or ended: no device call
    a, b = block(100), block(7)
    out = pool.process({0: a, 2: b}, start={0: 3, 2: 2})
    assert sorted(out) == [0, 2] and out[0].shape == (100, 2) and out[2].shape == (7, 2) and out[0].dtype == np.float64
    x, counts, flags, delays = fake.calls[-1]
    assert counts.tolist() == [100, 0, 7, 0] and flags.tolist() == [START, 0, START, 0]
    assert delays[0] == 30 and delays[2] == 250
    assert x[0].tobytes() == a.tobytes() and x[2, :7].tobytes() == b.tobytes() and not x[2, 7:].any() and not x[1].any()
    for _ in range(3):                                                # slot 0 advances alone; slot 2 is idle
        out = pool.process({0: block(100)})
    assert sorted(out) == [0] and out[0].shape == (100, 2)
    assert pool.positions.tolist() == [400, 0, 7, 0] and pool.live.tolist() == [True, False, True, False]
    out = pool.process({0: block(0)})                                 # an empty block of a live voice: no device call
    assert out[0].shape == (0, 2) and out[0].dtype == np.float64 and len(fake.calls) == 4
    # slot 2 ends with no block (its own tail: 250 frames), slot 1 is a whole voice shorter than its delay, slot 0 ends
    out = pool.process({1: block(3), 0: block(5)}, start={1: 1}, end=[2, 1, 0])
    assert {s: o.shape[0] for s, o in out.items()} == {0: 5 + 30, 1: 3 + 30, 2: 250}
    assert (out[1] == 1000 * len(fake.calls) + 1).all()               # rows of slot 1, of this call
    assert fake.calls[-1][1].tolist() == [5, 3, 0, 0] and fake.calls[-1][2].tolist() == [END, START | END, END, 0]
    assert not pool.live.any() and not pool.positions.any()
    pool.process({2: block(10)}, start={2: 0})                        # the slot goes to another voice with another delay
    assert fake.calls[-1][3][2] == 0 and fake.calls[-1][2].tolist() == [0, 0, START, 0]
    with pytest.raises(ValueError, match='slot 2 holds a live voice'):
        pool.process({2: block(10)}, start={2: 1})
    pool.process({2: block(10)}, start={2: 1}, discard=True)
    assert fake.calls[-1][3][2] == 30 and pool.positions[2] == 10
    assert pool.positions.tolist() == fake.pos.tolist()               # the mirror is the device's


REFUSALS = lambda ok: (
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
    (dict(blocks={0: ok, 1: ok}, start={2: 0}), ValueError, 'slot 1, which was never started'))


def _every_refusal(pool, fake, answer):
    from vndecorrelate_amd import _native
    ok = np.zeros((10, 2), np.float32)
    pool.process({0: ok}, start={0: 0})
    before = (pool.positions.copy(), pool.live.copy(), pool.tables.copy(), len(fake.calls))
    for kwargs, error, text in REFUSALS(ok):
        with pytest.raises(error, match=text):
            pool.process(kwargs.get('blocks'), start=kwargs.get('start'), end=kwargs.get('end', ()))
        assert len(fake.calls) == before[3], kwargs
        assert pool.positions.tolist() == before[0].tolist() and pool.live.tolist() == before[1].tolist()
        assert pool.tables.tolist() == before[2].tolist()
    # a native that answers other counts than the spans is an error, and the mirror stays
    pool._call_host = answer
    with pytest.raises(_native.NativeError, match='the spans are'):
        pool.process({0: ok})
    assert pool.positions.tolist() == before[0].tolist()


def test_every_haas_refusal_comes_before_the_native(dec, no_device):
    pool = dec.decorrelate_voice_pool(_haases(dec, (5, 50)), slots=3, in_channels=2, max_frames_per_call=100)
    _every_refusal(pool, _FakeHaas(pool),
                   lambda x, c, f, d: (np.zeros((3, pool.row_frames, 2), np.float64), np.array([1, 0, 0], np.int32)))


def test_haas_mono_blocks_and_mixing_the_forms(dec, no_device):
    make = lambda: dec.decorrelate_voice_pool(_haases(dec, (9,)), slots=2, in_channels=1, max_frames_per_call=64)
    pool = make()
    fake = _FakeHaas(pool)
    a = np.arange(5, dtype=np.float32)
    pool.process({1: a}, start={1: 0})                               # (n,) for a mono pool
    pool.process({1: a[:, None]})
    assert fake.calls[0][0][1, :5, 0].tolist() == a.tolist() and fake.calls[1][0].shape == (2, 64, 1)
    with pytest.raises(RuntimeError, match='runs through process'):
        pool.process_dev(None, None, None, None)                      # refused before the tensors are looked at
    other = make()
    other._form = 'dev'                                               # what a process_dev call leaves behind
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        other.process({0: a}, start={0: 0})
    with pytest.raises(ValueError, match='x must be a device tensor'):
        other.process_dev(np.zeros((2, 64, 1), np.float32), None, None, None)


# ---- ChainVoicePool over a fake native -------------------------------------------------------------------------------
class _FakeChain:
    """Both stages of the device: stage 1's spans feed stage 2 as its counts, each with positions of its own."""

    def __init__(self, pool):
        self.pool, self.calls = pool, []
        self.pos1, self.pos2 = np.zeros(pool.slots, np.int64), np.zeros(pool.slots, np.int64)
        pool._call_host = self._call

    def _call(self, x, counts, flags, tables, delays):
        from vndecorrelate_amd.streaming import haas_voice_spans, voice_spans
        p = self.pool
        assert x.shape == (p.slots, p.max_frames_per_call, p.in_channels) and x.dtype == np.float32
        assert counts.dtype == flags.dtype == tables.dtype == delays.dtype == np.int32
        self.calls.append((x.copy(), counts.copy(), flags.copy(), tables.copy(), delays.copy()))
        H, M = p.latency_frames, p.max_frames_per_call
        mid, self.pos1 = voice_spans(self.pos1, counts, flags, H, M)
        out, self.pos2 = haas_voice_spans(self.pos2, mid, flags, delays, p.max_delay, M + H)
        y = np.full((p.slots, p.row_frames, 2), np.nan, np.float64)
        for b, n in enumerate(out):
            y[b, :n] = 1000 * len(self.calls) + b
        return y, out.astype(np.int32)


def test_chain_bookkeeping_over_a_schedule(dec, no_device):
    from vndecorrelate_amd.streaming import ChainVoicePool
    bank = _chains(dec, (0.1, 0.5, 0.9, 0.5), (0, 100, 441, 882))     # velvets 1 and 3 share a table: 3 candidates, 4 entries
    pool = dec.decorrelate_voice_pool(bank, slots=4, in_channels=2, max_frames_per_call=100)
    assert type(pool) is ChainVoicePool
    assert pool.bank_tables.tolist() == [0, 1, 2, 1] and pool.bank_delays.tolist() == [0, 100, 441, 882]
    H = pool.latency_frames
    assert 200 < H < 320 and pool.tail_frames == 882 and pool.row_frames == 100 + H + 882
    assert pool.haas.max_frames_per_call == 100 + H and pool.haas.in_channels == 2
    assert (pool.ms_encode, pool.width, pool.haas.delayed_channel, pool.haas.ms_mode, pool.haas.width) == (True, None, 1, False, None)
    fake = _FakeChain(pool)
    rng = np.random.default_rng(0)

    def block(n):
        return rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    assert pool.process({}) == {} and not fake.calls
    a, b = block(100), block(7)
    out = pool.process({0: a, 2: b}, start={0: 3, 2: 2})
    assert sorted(out) == [0, 2] and out[0].shape == (0, 2) and out[2].shape == (0, 2) and out[0].dtype == np.float64
    x, counts, flags, tables, delays = fake.calls[-1]
    assert counts.tolist() == [100, 0, 7, 0] and flags.tolist() == [START, 0, START, 0]
    assert (tables[0], delays[0], tables[2], delays[2]) == (1, 882, 2, 441)       # the entry's table and delay go up together
    assert x[0].tobytes() == a.tobytes() and x[2, :7].tobytes() == b.tobytes() and not x[2, 7:].any() and not x[1].any()
    for _ in range(3):
        out = pool.process({0: block(100)})
    assert sorted(out) == [0] and out[0].shape == (400 - H - max(0, 300 - H), 2)
    assert pool.positions.tolist() == [400, 0, 7, 0] and pool.haas_positions.tolist() == [400 - H, 0, 0, 0]
    # slot 2 ends with no block: stage 1 flushes its 7 frames, stage 2 adds its 441; slot 1 is a whole voice; slot 0 ends
    out = pool.process({1: block(33), 0: block(5)}, start={1: 0}, end=[2, 1, 0])
    assert {s: o.shape[0] for s, o in out.items()} == {0: 5 + H + 882, 1: 33, 2: 7 + 441}
    assert fake.calls[-1][1].tolist() == [5, 33, 0, 0] and fake.calls[-1][2].tolist() == [END, START | END, END, 0]
    assert not pool.live.any() and not pool.positions.any() and not pool.haas_positions.any()
    pool.process({2: block(10)}, start={2: 0})
    with pytest.raises(ValueError, match='slot 2 holds a live voice'):
        pool.process({2: block(10)}, start={2: 1})
    pool.process({2: block(10)}, start={2: 1}, discard=True)                      # START reaches both stages
    assert (fake.calls[-1][3][2], fake.calls[-1][4][2]) == (1, 100) and pool.positions[2] == 10
    assert pool.positions.tolist() == fake.pos1.tolist() and pool.haas_positions.tolist() == fake.pos2.tolist()


def test_every_chain_refusal_comes_before_the_native(dec, no_device):
    pool = dec.decorrelate_voice_pool(_chains(dec, (0.1, 0.5), (5, 50)), slots=3, in_channels=2, max_frames_per_call=100)
    _every_refusal(pool, _FakeChain(pool),
                   lambda x, c, f, t, d: (np.zeros((3, pool.row_frames, 2), np.float64), np.array([1, 0, 0], np.int32)))
    assert not pool.haas_positions.any()                              # (the first block is still below the latency)


def test_chain_mixing_the_forms(dec, no_device):
    make = lambda: dec.decorrelate_voice_pool(_chains(dec, (0.3,), (9,)), slots=2, in_channels=1, max_frames_per_call=64)
    pool = make()
    fake = _FakeChain(pool)
    a = np.arange(5, dtype=np.float32)
    pool.process({1: a}, start={1: 0})
    assert fake.calls[0][0][1, :5, 0].tolist() == a.tolist() and fake.calls[0][0].shape == (2, 64, 1)
    with pytest.raises(RuntimeError, match='runs through process'):
        pool.process_dev(None, None, None, None, None)
    other = make()
    other._form = 'dev'
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        other.process({0: a}, start={0: 0})
    with pytest.raises(ValueError, match='x must be a device tensor'):
        other.process_dev(np.zeros((2, 64, 1), np.float32), None, None, None, None)


# ---- the bank ----------------------------------------------------------------------------------------------------------
def test_bank_refusals(dec, no_device):
    make = dec.decorrelate_voice_pool
    velvet = dec.VelvetNoise(sample_rate_hz=FS, duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None)
    haas = _haases(dec, (5, 50))
    chains = _chains(dec, (0.1, 0.5), (5, 50))
    # a mixed bank lists its types
    with pytest.raises(TypeError, match='HaasEffect, VelvetNoise'):
        make([velvet] + haas, slots=2)
    with pytest.raises(TypeError, match='HaasEffect, SignalChain'):
        make(chains + haas, slots=2)
    with pytest.raises(TypeError, match='WhiteNoise'):
        make([dec.WhiteNoise(sample_rate_hz=FS)], slots=2)
    # Haas settings that differ across the bank
    for field, kw in (('delayed_channel', dict(delayed_channel=0)), ('mode', dict(mode='MS')), ('width', dict(width=0.3))):
        with pytest.raises(ValueError, match=rf'decorrelate_voice_pool: {field} differs across the list.*bank entry 1'):
            make([haas[0]] + _haases(dec, (50,), **kw), slots=2)
        with pytest.raises(ValueError, match=rf'decorrelate_voice_pool: {field} differs across the list.*bank entry 1'):
            make([chains[0]] + _chains(dec, (0.5,), (50,), haas=kw), slots=2)
    # an uncovered HaasEffect: a float32 width, a delayed channel that is no channel, a delay that is no frame count
    for kw in (dict(width=np.float32(0.3)), dict(delayed_channel=2), dict(delay_time_seconds=-0.001),
               dict(delay_time_seconds=float('nan'))):
        with pytest.raises(ValueError, match='decorrelate_voice_pool covers a plain HaasEffect'):
            make(_haases(dec, (5,), **kw) if 'delay_time_seconds' not in kw
                 else [dec.HaasEffect(sample_rate_hz=1000, **kw)], slots=2)
        with pytest.raises(ValueError, match='decorrelate_voice_pool covers a plain HaasEffect'):
            make(_chains(dec, (0.1,), (5,), haas=kw), slots=2)
    # a chain with a normaliser; velvet settings that differ across the bank
    with pytest.raises(ValueError, match='normalizer=None'):
        make(_chains(dec, (0.1, 0.5), (5, 50), velvet=dict(normalizer=dec.rms_normalize)), slots=2)
    with pytest.raises(ValueError, match='decorrelate_voice_pool: width differs across the list.*bank entry 1'):
        make([chains[0]] + _chains(dec, (0.5,), (50,), velvet=dict(width=0.3)), slots=2)
    # a chain of another stage count or order names the bank entry
    sc = lambda: dec.SignalChain(sample_rate_hz=FS)
    v = dict(duration_seconds=DURATION, num_impulses=IMPULSES, seed=SEED, normalizer=None)
    with pytest.raises(ValueError, match='bank entry 1: a chain of 1 stages'):
        make([chains[0], sc().velvet_noise(**v)], slots=2)
    with pytest.raises(ValueError, match='bank entry 1: a chain of 3 stages'):
        make([chains[0], sc().velvet_noise(**v).haas_effect().haas_effect()], slots=2)
    with pytest.raises(ValueError, match='bank entry 0: a chain of 0 stages'):
        make([sc()], slots=2)
    with pytest.raises(TypeError, match='bank entry 1: a chain of HaasEffect then VelvetNoise'):
        make([chains[0], sc().haas_effect().velvet_noise(**v)], slots=2)
    with pytest.raises(TypeError, match='bank entry 0: a chain of VelvetNoise then WhiteNoise'):
        make([sc().velvet_noise(**v).white_noise()], slots=2)
    with pytest.raises(TypeError, match='bank entry 0: a chain of VelvetNoise then partial'):
        make([sc().velvet_noise(**v).stateless(dec.convolve_velvet_noise, velvet_noise_filters=np.zeros((4, 2), np.float32))],
             slots=2)
    # the scalars, for both kinds
    for bank in (haas, chains):
        for bad in (0, 3, True, None):
            with pytest.raises(ValueError, match='in_channels'):
                make(bank, slots=2, in_channels=bad)
        for bad in (0, -1, 2.0, True):
            with pytest.raises(ValueError, match='slots'):
                make(bank, slots=bad)
            with pytest.raises(ValueError, match='max_frames_per_call'):
                make(bank, slots=2, max_frames_per_call=bad)
        with pytest.raises(ValueError, match='split the pool'):
            make(bank, slots=65536)
    with pytest.raises(ValueError, match='make a row above 16776960 frames'):
        make(haas, slots=2, max_frames_per_call=16776960 - 50 + 1)
    assert make(haas, slots=2, max_frames_per_call=16776960 - 50).row_frames == 16776960
    # the velvet bank is what it was
    from vndecorrelate_amd.streaming import VoicePool
    assert type(make([velvet], slots=2)) is VoicePool


def test_exported_from_the_package():
    import vndecorrelate_amd
    assert callable(vndecorrelate_amd.haas_voice_spans)
    assert vndecorrelate_amd.HaasVoicePool.__name__ == 'HaasVoicePool'
    assert vndecorrelate_amd.ChainVoicePool.__name__ == 'ChainVoicePool'


# ---- header and binding ----------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    src = ('#include "vnd_haas_voice_stream.h"\n'
           'int main(void){return VND_VOICE_START == 1 && VND_VOICE_END == 2 && VND_HAAS_VOICE_MAX_ROW_FRAMES == 65535 * 256 '
           '? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vndecorrelate_amd import _native, streaming
    names = _declared(HEADER)
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_haas_voice_stream.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))       # vnd_amd.h keeps its fixed set
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_voice_stream.h'))
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    assert streaming.HAAS_VOICE_MAX_ROW_FRAMES == int(re.search(r'VND_HAAS_VOICE_MAX_ROW_FRAMES\s+(\d+)', text).group(1))
    for wrapper in ('haas_voice_stream_state_bytes', 'haas_voice_stream_reset_device', 'haas_voice_stream_device',
                    'haas_voice_stream_host'):
        assert callable(getattr(_native, wrapper))


def test_checks_that_need_no_device(lib):
    null = ctypes.c_void_p(None)
    call = (null, 0, 480, null, null, null, null, null, null, 4, 2, 100, 0, 0, 0, 0.0)
    assert lib.vnd_haas_voice_stream_f64_dev(null, *call, null) == INVALID
    assert b'null context' in lib.vnd_last_error()
    assert lib.vnd_haas_voice_stream_f64_host(null, *call) == INVALID
    assert b'null context' in lib.vnd_last_error()
    assert lib.vnd_haas_voice_stream_reset_dev(null, null, 0, 4, 2, 100, 480, null) == INVALID
    assert lib.vnd_haas_voice_stream_state_bytes(4, 2, 100, 480, None) == INVALID
    assert b'null bytes' in lib.vnd_last_error()
    got = ctypes.c_int64(-7)
    for args, status, text in (((4, 2, 100, 480), 0, b''), ((0, 1, 0, 0), 0, b''), ((-1, 2, 100, 480), INVALID, b'negative'),
                               ((4, 3, 100, 480), INVALID, b'mono or stereo'), ((4, 2, -1, 480), INVALID, b'negative max_delay'),
                               ((4, 2, 100, -1), INVALID, b'max_frames_per_call'),
                               ((65536, 2, 100, 480), UNSUPPORTED, b'split the pool'),
                               ((4, 2, 100, 16776960 - 99), UNSUPPORTED, b'one grid dimension')):
        assert lib.vnd_haas_voice_stream_state_bytes(*args, ctypes.byref(got)) == status, args
        if status:
            assert got.value == 0 and text in lib.vnd_last_error(), args
    assert lib.vnd_haas_voice_stream_state_bytes(4, 2, 100, 480, ctypes.byref(got)) == 0 and got.value == 32 + 4 * 580 * 2 * 4
    assert lib.vnd_haas_voice_stream_state_bytes(3, 1, 0, 480, ctypes.byref(got)) == 0 and got.value == 32   # positions only
    assert lib.vnd_haas_voice_stream_state_bytes(4, 1, 2 ** 31 - 1, 0, ctypes.byref(got)) == UNSUPPORTED
