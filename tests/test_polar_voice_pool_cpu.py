"""CPU tier of the polar-moments voice pool (include/vnd_polar_voice_stream.h, analysis.stereo_image_voice_pool,
analysis.PolarVoicePool): polar_voice_spans against every voice alone, the streamed form of polar_moments_ordered against
its one-shot form bit for bit, the dict form's bookkeeping and every refusal over a fake native, pool.scores against
optimization.score_from_moments, and the header against its binding - no device call."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_polar_voice_stream.h'
NAMES = ['vnd_polar_voice_stream_f32_dev', 'vnd_polar_voice_stream_f64_dev', 'vnd_polar_voice_stream_reset_dev',
         'vnd_polar_voice_stream_state_bytes']
INVALID, UNSUPPORTED = 1, 4
START, END = 1, 2
WEIGHTS = dict(angle_limit=np.pi / 4, lambda_mean=5.0, lambda_skew=2.0, lambda_correlation=15.0, lambda_penalty=1e3)


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
    for name in ('default_context', 'context_for', 'polar_voice_stream_device', 'polar_voice_stream_reset_device',
                 'polar_voice_stream_state_bytes'):
        monkeypatch.setattr(_native, name, touched)


# ---- polar_voice_spans -----------------------------------------------------------------------------------------------
class _Voice:
    """One voice alone: a position in Python integers."""

    def __init__(self, pos=0):
        self.pos = pos

    def call(self, n, flags, M):
        p = 0 if flags & START else self.pos               # START: whatever the slot held is dropped
        if not 0 <= n <= M or not 0 <= p <= 1 << 60:
            return -1                                      # ... unless the call is refused: nothing changes
        if n == 0 and not flags & (START | END):
            return 0
        self.pos = 0 if flags & END else p + n
        return 1


@pytest.mark.parametrize('seed', range(4))
def test_spans_equal_every_voice_alone(an, seed):
    rng = np.random.default_rng(seed)
    S, M = 9, 96
    voices = [_Voice() for _ in range(S)]
    pos = np.zeros(S, np.int64)
    menu = [0, 0, 1, M, 17, M + 1, -1, 2 ** 31 - 1, -2 ** 31]
    seen = set()
    for call in range(120):
        counts = np.array([int(rng.choice(menu + [int(rng.integers(0, M + 1))])) for _ in range(S)], np.int64)
        flags = rng.choice([0, 0, 0, 0, START, END, START | END, 4, 8 | START], S).astype(np.int32)     # other bits are ignored
        counts[rng.random(S) < 0.25] = 0                                  # idle slots, flagged or not
        live = pos > 0
        valid, new = an.polar_voice_spans(pos, counts.astype(np.int32), flags, M)
        assert valid.dtype == new.dtype == np.int64
        want = [v.call(int(n), int(f), M) for v, n, f in zip(voices, counts, flags)]
        assert valid.tolist() == want, (call, counts, flags)
        assert new.tolist() == [v.pos for v in voices], call
        untouched = valid != 1
        assert (new[untouched] == pos[untouched]).all()                   # idle and bad slots keep their position
        for b in range(S):
            seen.add((int(valid[b]), int(flags[b]) & 3, int(counts[b]) == 0, bool(live[b])))
        pos = new
    # idle, END alone, START + END, START over a live slot, and bad counts on live and idle slots were all drawn
    assert {(0, 0, True, True), (1, END, True, True), (1, START | END, False, True), (1, START, False, True),
            (-1, 0, False, True), (-1, START, False, False)} <= seen


def test_spans_edge_rows(an):
    def one(p, n, f, M=600):
        valid, new = an.polar_voice_spans([p], [n], [f], M)
        return int(valid[0]), int(new[0])
    assert one(0, 63, 0) == (1, 63) and one(63, 1, 0) == (1, 64) and one(511, 600, 0) == (1, 1111)
    assert one(0, 0, END) == (1, 0) and one(87, 0, END) == (1, 0) and one(87, 1, END) == (1, 0)      # END alone answers
    assert one(777, 64, START | END) == (1, 0) and one(777, 0, START | END) == (1, 0) and one(777, 0, START) == (1, 0)
    assert one(777, 63, START) == (1, 63)
    assert one(777, 0, 0) == (0, 777) and one(777, 0, 4) == (0, 777)                                   # idle
    valid, new = an.polar_voice_spans([40] * 5, [-1, 97, 96, 2 ** 31 - 1, -2 ** 31], [0, START, 0, END, 0], 96)
    assert valid.tolist() == [-1, -1, 1, -1, -1] and new.tolist() == [40, 40, 136, 40, 40]
    with pytest.raises(ValueError):
        an.polar_voice_spans([0, 0], [1], [0], 96)


def test_spans_at_the_positions_of_a_long_lived_voice(an):
    """Around 2^31, 2^32 and at the last position taken, 2^60, against Python's own integers; 2^60 + 1 is refused unless
    the call STARTs over it."""
    top = 1 << 60
    for M in (480, 600, 7):
        positions = [2 ** 31 - 7, 2 ** 31, 2 ** 32 - 300, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 2 ** 40 + 3, 2 ** 53 + 1,
                     top - M, top - 1, top]
        for n, f in ((0, 0), (7, 0), (M, 0), (0, END), (M, END), (M, START), (M, START | END)):
            valid, new = an.polar_voice_spans(positions, [n] * len(positions), [f] * len(positions), M)
            for p, got, after in zip(positions, valid.tolist(), new.tolist()):
                v = _Voice(p)
                assert (got, after) == (v.call(n, f, M), v.pos), (p, n, f)
        valid, new = an.polar_voice_spans([top], [M], [0], M)
        assert valid[0] == 1 and new[0] == top + M                     # the next call of that slot is the refused one
        bad = [top + 1, top + M, 2 ** 62, -1, -2 ** 63]
        valid, new = an.polar_voice_spans(bad, [M] * 5, [0, END, 0, 0, END], M)
        assert valid.tolist() == [-1] * 5 and new.tolist() == bad
        valid, new = an.polar_voice_spans(bad, [M] * 5, [START, START | END, START, START, START], M)
        assert valid.tolist() == [1] * 5 and new.tolist() == [M, 0, M, M, M]


# ---- polar_moments_ordered: streamed against one-shot ----------------------------------------------------------------
LENGTHS = [0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 131071, 131072, 131073, 131585]
_terms_cache = {}


def _terms(n):
    """Per-frame terms whose magnitudes run over 1e-8 .. 1e8 with both signs, so that sums cancel and the order of the
    additions shows in the last bits; |theta| (column 4) is not negative."""
    if n not in _terms_cache:
        rng = np.random.default_rng(n)
        t = rng.standard_normal((n, 8)) * 10.0 ** rng.integers(-8, 9, (n, 8))
        t[:, 4] = np.abs(t[:, 4])
        _terms_cache[n] = (t, None)
    return _terms_cache[n][0]


def _one_shot(an, n):
    t = _terms(n)
    if _terms_cache[n][1] is None:
        _terms_cache[n] = (t, an.polar_moments_ordered(t))
    return _terms_cache[n][1]


def _bits(a):
    return np.asarray(a, np.float64).tobytes()


def test_the_order_matters_for_these_terms(an):
    """The test below could not tell two orders apart if plain sums gave the same bits."""
    t = _terms(1025)
    got = _one_shot(an, 1025)
    plain = t.sum(axis=0)
    assert got[4] == t[:, 4].max()
    assert any(got[k] != plain[k] for k in (0, 1, 2, 3, 5, 6, 7))
    assert np.allclose(np.delete(got, 4), np.delete(plain, 4), rtol=0, atol=1e-6 * np.abs(t).sum(axis=0).max())
    assert _bits(an.polar_moments_ordered(np.zeros((0, 8)))) == _bits(np.zeros(8))           # one chunk of zeros


def _schedules(n, M, rng):
    yield 'whole blocks', [M] * (n // M) + ([n % M] if n % M else [])
    sizes, left = [], n
    while left:
        k = int(min(left, rng.integers(0, M + 1)))
        sizes.append(k)
        left -= k
    yield 'random', sizes + [0]
    # p mod 512 = 511 before every full block: a call of M frames then touches ceil(M / 512) + 1 chunks
    sizes, p = [], 0
    while p < n:
        k = min(n - p, M if p % 512 == 511 else min(M, (511 - p) % 512 or M))
        sizes.append(k)
        p += k
    yield '511 then M', sizes


@pytest.mark.parametrize('M', [100, 600, 132096])
def test_streamed_equals_one_shot_bit_for_bit(an, M):
    rng = np.random.default_rng(M)
    for n in LENGTHS:
        t, want = _terms(n), _one_shot(an, n)
        for name, sizes in _schedules(n, M, rng):
            assert sum(sizes) == n and all(0 <= k <= M for k in sizes)
            state = an.PolarMomentsState()
            got, p = an.polar_moments_ordered(t[:0], state), 0
            for i, k in enumerate(sizes):
                got = an.polar_moments_ordered(t[p:p + k], state)
                p += k
                if i in (0, len(sizes) // 2):                              # on the way: the one-shot form of the prefix
                    assert _bits(got) == _bits(an.polar_moments_ordered(t[:p])), (n, name, i)
            assert state.position == n and len(state.pending) == n % 512
            assert _bits(got) == _bits(want), (n, M, name)
            if name == '511 then M' and n >= 511 + M:
                at = np.cumsum([0] + sizes[:-1])
                assert any(k == M and p % 512 == 511 for k, p in zip(sizes, at)), (n, M)


@pytest.mark.parametrize('n', LENGTHS)
def test_streamed_in_blocks_of_one(an, n):
    t, want = _terms(n), _one_shot(an, n)
    state = an.PolarMomentsState()
    for row in t:
        state.push(row[None])
    assert _bits(state.moments()) == _bits(want)


def test_a_state_planted_at_a_large_position(an):
    """The state depends on the position through floor(p / 512) mod 256 and p mod 512 alone once every lane has a chunk: a
    state moved from p to p + 131072 k answers the same bits - at 2^31, 2^32, 2^40 and up to 2^60 in Python integers."""
    rng = np.random.default_rng(5)
    t = _terms(131585)
    for target in (2 ** 31 - 7, 2 ** 32 - 300, 2 ** 40 + 3, 2 ** 60 - 600):
        small = target % 131072 + 131072
        a = an.PolarMomentsState()
        a.push(t[:small - 131072])
        a.push(_terms(131072))
        assert a.position == small
        b = an.PolarMomentsState(target, a.lanes, a.pending)
        p = 0
        for k in (1, 600, 0, 511, 513, 600):
            more = t[p:p + k] * 3.0
            p += k
            assert _bits(an.polar_moments_ordered(more, a)) == _bits(an.polar_moments_ordered(more, b)), (target, k)
        assert b.position == target + p and isinstance(b.position, int)
    with pytest.raises(ValueError):
        an.PolarMomentsState(5, None, np.zeros((4, 8)))
    del rng


# ---- the dict form over a fake native --------------------------------------------------------------------------------
class _FakeNative:
    """Stands for the device under a real pool: records what every call uploads and answers with the spans of a position
    of its own per slot (the device's), and moments that name the slot and the call."""

    def __init__(self, pool):
        self.pool, self.calls = pool, []
        self.pos = np.zeros(pool.slots, np.int64)
        pool._call_host = self._call

    def _call(self, x, counts, flags):
        from vndecorrelate_amd.analysis import polar_voice_spans
        p = self.pool
        assert x.shape == (p.slots, p.max_frames_per_call, 2) and x.dtype == p.dtype
        assert counts.dtype == flags.dtype == np.int32
        self.calls.append((x.copy(), counts.copy(), flags.copy()))
        valid, self.pos = polar_voice_spans(self.pos, counts, flags, p.max_frames_per_call)
        m = np.full((p.slots, 8), np.nan)
        for b, v in enumerate(valid):
            if v == 1:
                m[b] = 1000 * len(self.calls) + b
        return m, valid.astype(np.int32)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_bookkeeping_over_a_schedule(an, no_device, dtype):
    pool = an.stereo_image_voice_pool(4, max_frames_per_call=100, dtype=dtype)
    assert pool.chunks_per_call == 2 and pool.in_channels == 2 and pool._out_width == 8 and pool._out_dtype == np.float64
    assert pool._bank_len() == 1
    fake = _FakeNative(pool)
    rng = np.random.default_rng(0)

    def block(n):
        return rng.uniform(-1, 1, (n, 2)).astype(dtype)
    assert pool.process({}) == {} and not fake.calls                  # nothing pushed, started or ended: no device call
    a, b = block(100), block(7)
    out = pool.process({0: a, 2: b}, start=[0, 2])
    assert sorted(out) == [0, 2] and out[0].shape == (8,) and out[0].dtype == np.float64
    x, counts, flags = fake.calls[-1]
    assert counts.tolist() == [100, 0, 7, 0] and flags.tolist() == [START, 0, START, 0]
    assert x[0].tobytes() == a.tobytes() and x[2, :7].tobytes() == b.tobytes() and not x[2, 7:].any() and not x[1].any()
    for _ in range(3):                                                # slot 0 advances alone; slot 2 is idle
        out = pool.process({0: block(100)})
    assert sorted(out) == [0] and (out[0] == 1000 * 4 + 0).all()
    assert pool.positions.tolist() == [400, 0, 7, 0] and pool.live.tolist() == [True, False, True, False]
    assert pool.process({0: block(0)}) == {} and len(fake.calls) == 4             # an empty block alone: no device call
    out = pool.process({0: block(0), 2: block(3)})                                # ... beside a neighbour's block: idle
    assert sorted(out) == [2] and len(fake.calls) == 5
    # slot 2 ends with no block (its final moments), slot 1 is a whole voice in one call, slot 0 ends with its last block,
    # slot 3 starts with no block (eight zeros on the device)
    out = pool.process({1: block(88), 0: block(5)}, start=[1, 3], end=[2, 1, 0])
    assert sorted(out) == [0, 1, 2, 3] and (out[1] == 1000 * len(fake.calls) + 1).all()
    assert fake.calls[-1][1].tolist() == [5, 88, 0, 0] and fake.calls[-1][2].tolist() == [END, START | END, END, START]
    assert pool.live.tolist() == [False, False, False, True] and not pool.positions.any()
    pool.process({2: block(10)}, start=[2])
    with pytest.raises(ValueError, match='slot 2 holds a live voice'):
        pool.process({2: block(10)}, start=[2])
    pool.process({2: block(10)}, start=[2], discard=True)             # a live voice is dropped only on request
    assert fake.calls[-1][2].tolist() == [0, 0, START, 0] and pool.positions[2] == 10
    assert pool.positions.tolist() == fake.pos.tolist()               # the mirror is the device's


def test_every_refusal_comes_before_the_native(an, no_device):
    pool = an.stereo_image_voice_pool(3, max_frames_per_call=100)
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
            (dict(blocks={0: np.zeros((10, 2), np.float64)}), TypeError, 'float32'),
            (dict(blocks={0: np.zeros((10, 1), np.float32)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={0: np.zeros(10, np.float32)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={0: np.zeros((1, 10, 2), np.float32)}), ValueError, r'expected \(frames, 2\)'),
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
    other = an.stereo_image_voice_pool(3, max_frames_per_call=100, dtype='float64')
    _FakeNative(other)
    with pytest.raises(TypeError, match='float64'):
        other.process({0: ok}, start=[0])
    # a native that answers otherwise than the spans is an error, and the mirror stays
    pool._call_host = lambda x, c, f: (np.zeros((3, 8)), np.array([0, 0, 0], np.int32))
    from vndecorrelate_amd import _native
    with pytest.raises(_native.NativeError, match='the spans are'):
        pool.process({0: ok})
    assert pool.positions.tolist() == before[0].tolist()


def test_mixing_the_forms(an, no_device):
    pool = an.stereo_image_voice_pool(2, max_frames_per_call=100)
    _FakeNative(pool)
    pool.process({1: np.zeros((5, 2), np.float32)}, start=[1])
    with pytest.raises(RuntimeError, match='runs through process'):
        pool.process_dev(None, None, None)                            # refused before the tensors are looked at
    other = an.stereo_image_voice_pool(2, max_frames_per_call=100, dtype='float64')
    other._form = 'dev'                                               # what a process_dev call leaves behind
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        other.process({0: np.zeros((5, 2), np.float64)}, start=[0])
    with pytest.raises(ValueError, match='y must be a device tensor'):
        other.process_dev(np.zeros((2, 100, 2), np.float64), None, None)


def test_construction_refusals(an, no_device):
    make = an.stereo_image_voice_pool
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='slots'):
            make(bad)
        with pytest.raises(ValueError, match='max_frames_per_call'):
            make(2, max_frames_per_call=bad)
    with pytest.raises(ValueError, match='split the pool'):
        make(65536)
    with pytest.raises(ValueError, match='counts are int32'):
        make(2, max_frames_per_call=2 ** 31)
    for bad in ('float16', 'int32', None, 'nothing'):
        with pytest.raises(ValueError, match='dtype'):
            make(2, dtype=bad)
    with pytest.raises(ValueError, match='more than one launch takes'):
        make(2, max_frames_per_call=512 * 65535)                      # 65536 chunk workgroups per slot
    with pytest.raises(ValueError, match='more than one launch takes'):
        make(40000, max_frames_per_call=512 * 256)                    # 257 x 40000 workgroups, above 2^23
    pool = make(5, max_frames_per_call=480, dtype=np.float64)
    assert (pool.slots, pool.max_frames_per_call, pool.chunks_per_call) == (5, 480, 2)
    assert pool.dtype == np.float64 and make(1).dtype == np.float32 and make(1).max_frames_per_call == 4800
    assert make(2, max_frames_per_call=512 * 65534).chunks_per_call == 65535


def test_scores_are_score_from_moments_row_by_row(an, no_device):
    from vndecorrelate_amd import optimization
    pool = an.stereo_image_voice_pool(3, max_frames_per_call=100)
    rng = np.random.default_rng(2)
    m = np.abs(rng.standard_normal((6, 8))) * np.array([100, 10, 30, 5, 1, 20, 50, 50.0])
    m[:, 1] *= -1
    m[0] = 0.0                                                        # a voice of no frames
    got = pool.scores(m, **WEIGHTS)
    assert got.shape == (6,) and got.dtype == np.float64
    for row, s in zip(m, got):
        want = optimization.score_from_moments(row, **WEIGHTS)
        assert abs(s - want) <= 1e-15 * max(1.0, abs(want))           # (array ** and float ** may differ in the last bit)
    assert pool.scores(m[3], **WEIGHTS) == got[3]
    with pytest.raises(ValueError, match='moments of shape'):
        pool.scores(np.zeros((2, 7)), **WEIGHTS)


def test_exported_from_the_package():
    import vndecorrelate_amd
    assert callable(vndecorrelate_amd.stereo_image_voice_pool) and callable(vndecorrelate_amd.polar_voice_spans)
    assert callable(vndecorrelate_amd.polar_moments_ordered)
    assert vndecorrelate_amd.PolarVoicePool.__name__ == 'PolarVoicePool'
    from vndecorrelate_amd import analysis
    assert {'stereo_image_voice_pool', 'PolarVoicePool', 'polar_voice_spans', 'polar_moments_ordered',
            'PolarMomentsState'} <= set(analysis.__all__)


# ---- header and binding ----------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    src = ('#include "vnd_polar_voice_stream.h"\n'
           'int main(void){return VND_VOICE_START == 1 && VND_VOICE_END == 2 && VND_MAX_STREAMS == 65535 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_polar_voice_stream.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))            # vnd_amd.h keeps its fixed set
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    assert '#include "vnd_voice_stream.h"' in text
    for wrapper in ('polar_voice_stream_state_bytes', 'polar_voice_stream_reset_device', 'polar_voice_stream_device',
                    'describe_polar_voice_stream'):
        assert callable(getattr(_native, wrapper))
    assert 'vnd_describe_polar_voice_stream_launch' in _declared(REPO / 'include' / 'vnd_amd_internal.h')
    assert hasattr(lib, 'vnd_describe_polar_voice_stream_launch')
    assert 'vnd_describe_polar_voice_stream_launch' in _native.INTERNAL_SIGNATURES


def test_checks_and_plans_that_need_no_device(lib):
    from vndecorrelate_amd import _native
    null = ctypes.c_void_p(None)
    for fn in (lib.vnd_polar_voice_stream_f32_dev, lib.vnd_polar_voice_stream_f64_dev):
        assert fn(null, null, 0, 480, null, null, 960, 2, null, null, null, null, 4, null) == INVALID
        assert b'null context' in lib.vnd_last_error()
    assert lib.vnd_polar_voice_stream_reset_dev(null, null, 0, 4, 480, 4, null) == INVALID
    got = ctypes.c_int64(-7)
    # positions, 256 x 8 lane sums a slot, (ceil(M / 512) + 1) x 8 partials a slot, 511 + M pairs of ring a slot
    assert lib.vnd_polar_voice_stream_state_bytes(4, 480, 4, ctypes.byref(got)) == 0
    assert got.value == 32 + 4 * 256 * 64 + 4 * 2 * 64 + 4 * (511 + 480) * 8
    assert lib.vnd_polar_voice_stream_state_bytes(3, 513, 8, ctypes.byref(got)) == 0
    assert got.value == 32 + 3 * 256 * 64 + 3 * 3 * 64 + 3 * (511 + 513) * 16         # 24 bytes of positions, padded to 32
    assert _native.polar_voice_stream_state_bytes(3, 513, 8) == got.value
    for args in ((0, 480, 4), (4, 0, 4), (4, 480, 2), (4, 480, 0), (4, 2 ** 31, 4), (-1, 480, 8)):
        assert lib.vnd_polar_voice_stream_state_bytes(*args, ctypes.byref(got)) == INVALID and got.value == 0, args
    assert lib.vnd_polar_voice_stream_state_bytes(4, 480, 4, None) == INVALID
    assert lib.vnd_polar_voice_stream_state_bytes(65536, 480, 4, ctypes.byref(got)) == UNSUPPORTED
    assert lib.vnd_polar_voice_stream_state_bytes(4, 512 * 65535, 4, ctypes.byref(got)) == UNSUPPORTED
    assert lib.vnd_polar_voice_stream_state_bytes(40000, 512 * 256, 4, ctypes.byref(got)) == UNSUPPORTED and got.value == 0
    text = _native.describe_polar_voice_stream(512, 480)
    assert text == f'polar_voice_stream groups=2 nblocks=1024 finish_groups=512 threads=256 state_bytes={_native.polar_voice_stream_state_bytes(512, 480)}'
    assert 'groups=11 nblocks=22528 finish_groups=2048' in _native.describe_polar_voice_stream(2048, 4800, 8)
    assert 'groups=259 ' in _native.describe_polar_voice_stream(2, 132096)
    buf = ctypes.create_string_buffer(64)
    assert lib.vnd_describe_polar_voice_stream_launch(4, 480, 4, None, 64) == INVALID
    assert b'null text' in lib.vnd_last_error()
    assert lib.vnd_describe_polar_voice_stream_launch(4, 0, 4, buf, 64) == INVALID and not buf.value
    assert lib.vnd_describe_polar_voice_stream_launch(4, 512 * 65535, 4, buf, 64) == UNSUPPORTED and not buf.value
