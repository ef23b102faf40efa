"""CPU tier of the spectrum voice pool (include/vnd_spectrum_voice_stream.h, spectral.spectrum_voice_pool,
spectral.SpectrumVoicePool): spectrum_voice_spans against a scalar restatement, the bound on the rows of a call over an
exhaustive grid, the total / partial fold against spectrum_cases.replay_mean bit for bit, the dict form's bookkeeping and
every refusal over a fake native, the header against its binding and every ABI refusal with a null context - no device call."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

import spectrum_cases as sc
import spectrum_voice_cases as sv
from spectrum_voice_cases import END, INVALID, START, UNSUPPORTED

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_spectrum_voice_stream.h'
NAMES = ['vnd_spectrum_voice_stream_f32_dev', 'vnd_spectrum_voice_stream_f64_dev', 'vnd_spectrum_voice_stream_reset_dev',
         'vnd_spectrum_voice_stream_state_bytes']


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
def sp(lib):
    from vndecorrelate_amd import spectral
    return spectral


@pytest.fixture
def no_device(monkeypatch):
    """Any touch of the device raises: the refusals and the bookkeeping below come before it."""
    from vndecorrelate_amd import _native

    def touched(*args, **kwargs):
        raise AssertionError('the device was touched')
    for name in ('default_context', 'context_for', 'spectrum_voice_stream_device', 'spectrum_voice_stream_reset_device',
                 'spectrum_voice_stream_state_bytes'):
        monkeypatch.setattr(_native, name, touched)


# ---- spectrum_voice_spans ----------------------------------------------------------------------------------------------
def _check_against_scalar(sp, pos, counts, flags, W, H, M):
    out, seg, new = sp.spectrum_voice_spans(pos, counts, flags, W, H, M)
    assert out.dtype == seg.dtype == new.dtype == np.int64
    for b in range(len(pos)):
        want = sv.scalar_span(int(pos[b]), int(counts[b]), int(flags[b]), W, H, M)
        assert (int(out[b]), int(seg[b]), int(new[b])) == want, (b, int(pos[b]), int(counts[b]), int(flags[b]), W, H, M)
    return out, new


@pytest.mark.parametrize('W,H', [(64, 32), (63, 63), (99, 1), (256, 128), (2, 1), (2, 2), (513, 256)])
@pytest.mark.parametrize('seed', range(3))
def test_spans_equal_the_scalar_rule_over_random_schedules(sp, W, H, seed):
    """Idle calls, END alone, START + END, START over a live slot, hop = nperseg and hop = 1, counts below hop, bad counts."""
    rng = np.random.default_rng(1000 * W + 10 * H + seed)
    S, M = 12, 3 * W + 5
    pos = np.zeros(S, np.int64)
    seen = set()
    for call in range(60):
        counts = rng.choice([0, 1, max(H - 1, 0), H, W - 1, W, W + 1, M, M + 1, -1, int(rng.integers(0, M + 1))], S).astype(np.int64)
        flags = rng.choice([0, 0, 0, START, END, START | END, 4, 4 | START], S).astype(np.int64)
        out, new = _check_against_scalar(sp, pos, counts, flags, W, H, M)
        for b in range(S):
            idle = counts[b] == 0 and not flags[b] & 3
            seen.add(('bad' if out[b] < 0 else 'idle' if idle else 'end-alone' if counts[b] == 0 and flags[b] & 3 == END
                      else 'whole' if flags[b] & 3 == 3 else 'start-over-live' if flags[b] & START and pos[b] > 0
                      else 'below-hop' if 0 < counts[b] < H else 'none' if out[b] == 0 else 'rows'))
        assert (out <= -(-M // H)).all()
        pos = new
    assert {'bad', 'idle', 'end-alone', 'whole', 'start-over-live', 'rows'} <= seen, seen
    assert H == 1 or 'below-hop' in seen or H > M


@pytest.mark.parametrize('base', [2 ** 31, 2 ** 32, 2 ** 60])
def test_spans_at_large_positions(sp, base):
    W, H, M = 256, 128, 600
    rng = np.random.default_rng(base % 1009)
    pos = base + rng.integers(-700, 700, 64).astype(np.int64)
    pos[:4] = [base, base - 1, base + 1, base - M]
    counts = rng.integers(0, M + 1, 64).astype(np.int64)
    counts[:4] = [0, 1, M, M]
    for flags in (np.zeros(64, np.int64), rng.choice([0, START, END, START | END], 64).astype(np.int64)):
        out, new = _check_against_scalar(sp, pos, counts, flags, W, H, M)
        if base == 2 ** 60:
            late = (pos > 2 ** 60) & (flags & START == 0)
            assert late.any() and (out[late] == -1).all() and (new[late] == pos[late]).all()
            assert (out[~late] >= 0).all()                   # 2^60 itself goes on
    out, seg, new = sp.spectrum_voice_spans([2 ** 60 + 1, -1, 5], [0, 0, 0], [0, 0, 0], W, H, M)
    assert out.tolist() == [-1, -1, 0] and seg.tolist() == [-1, -1, -1] and new.tolist() == [2 ** 60 + 1, -1, 5]
    with pytest.raises(ValueError, match='one shape'):
        sp.spectrum_voice_spans([0, 0], [1], [0], W, H)
    with pytest.raises(ValueError, match='nperseg and hop'):
        sp.spectrum_voice_spans([0], [1], [0], W, 0)


def test_rows_per_call_bound_over_a_grid(sp):
    """out_counts <= RC = ceil(M / H) for every p - and the bound is met."""
    for W in (2, 3, 5, 8):
        for H in range(1, W + 1):
            for M in (1, 2, 3, 5, 9, 12):
                rc = -(-M // H)
                p = np.repeat(np.arange(0, 3 * (W + H) + 2), M + 1)
                n = np.tile(np.arange(0, M + 1), len(p) // (M + 1))
                out, seg, new = sp.spectrum_voice_spans(p, n, np.full_like(p, 4), W, H, M)      # bit 2 is ignored
                assert (out >= 0).all() and out.max() == rc, (W, H, M)
                assert (new == p + n).all()
                assert ((seg == -1) == (n == 0)).all()
    pool = sp.spectrum_voice_pool(3, 15, nperseg=64, noverlap=57)
    assert pool.rows_per_call == 3 and pool.hop == 7


# ---- the order of the sums ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('run', [1, 2, 3, 8, 32])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_fold_equals_the_replayed_mean_at_every_split(run, dtype):
    """total / partial, pushed call by call, against the one-shot order (spectrum_cases.replay_mean) bit for bit: R - 1, R,
    R + 1, 2 R and 2 R + 1 segments, split into two calls at every boundary, and into single segments."""
    rng = np.random.default_rng(run)
    bins = 5
    for count in sorted({max(run - 1, 1), run, run + 1, 2 * run, 2 * run + 1}):
        cols = (rng.uniform(0, 1, (bins, count)) * 10.0 ** rng.integers(-6, 6, (bins, count))).astype(dtype)
        want = sc.replay_mean(cols, run, dtype)
        for cut in list(range(count + 1)) + [None]:
            fold = sv.Fold(run, (bins,))
            calls = [range(count)[i:i + 1] for i in range(count)] if cut is None else [range(0, cut), range(cut, count)]
            for call in calls:
                for t in call:
                    fold.push(cols[:, t])
                got = fold.mean(dtype)                        # after every call: the mean of the segments so far
                ref = sc.replay_mean(cols[:, :fold.count], run, dtype) if fold.count else np.zeros(bins, dtype)
                assert got.tobytes() == ref.tobytes(), (run, count, cut, fold.count)
            assert fold.mean(dtype).tobytes() == want.tobytes()


# ---- the dict form over a fake native ----------------------------------------------------------------------------------
class _FakeNative:
    """Stands for the device under a real pool: records what every call uploads and answers with the spans of a position
    of its own per slot (the device's), and columns that name the slot and the call."""

    def __init__(self, pool):
        self.pool, self.calls = pool, []
        self.pos = np.zeros(pool.slots, np.int64)
        pool._call_host = self._call

    def _call(self, x, counts, flags):
        from vndecorrelate_amd.spectral import spectrum_voice_spans
        p = self.pool
        assert x.shape == (p.slots, p.max_frames_per_call, p.in_channels) and x.dtype == p.dtype
        assert counts.dtype == flags.dtype == np.int32
        self.calls.append((x.copy(), counts.copy(), flags.copy()))
        out, _, self.pos = spectrum_voice_spans(self.pos, counts, flags, p.nperseg, p.hop, p.max_frames_per_call)
        y = np.full((p.slots, p.rows_per_call if p.columns else 0, p.in_channels, p.bins), np.nan, p.dtype)
        for b, n in enumerate(out):
            y[b, :n] = 1000 * len(self.calls) + b
        return y, out.astype(np.int32)


def _pool(sp, slots=4, M=100, **kw):
    return sp.spectrum_voice_pool(slots, M, nperseg=64, noverlap=40, **kw)


def test_bookkeeping_over_a_schedule(sp, no_device):
    pool = _pool(sp)
    assert (pool.rows_per_call, pool.in_channels, pool.hop, pool.bins, pool.nfft) == (5, 2, 24, 33, 64)
    assert pool.dtype == np.float32 and pool.f.tobytes() == sp.bin_frequencies(64, 1.0).tobytes()
    fake = _FakeNative(pool)
    rng = np.random.default_rng(0)

    def block(n):
        return rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    assert pool.process({}) == {} and not fake.calls                  # nothing pushed, started or ended: no device call
    a, b = block(100), block(7)
    out = pool.process({0: a, 2: b}, start=[0, 2])
    assert sorted(out) == [0, 2] and out[0].shape == (2, 2, 33) and out[2].shape == (0, 2, 33) and out[0].dtype == np.float32
    x, counts, flags = fake.calls[-1]
    assert counts.tolist() == [100, 0, 7, 0] and flags.tolist() == [START, 0, START, 0]
    assert x[0].tobytes() == a.tobytes() and x[2, :7].tobytes() == b.tobytes() and not x[2, 7:].any() and not x[1].any()
    for _ in range(3):                                                # slot 0 advances alone; slot 2 is idle
        out = pool.process({0: block(100)})
    assert sorted(out) == [0] and out[0].shape == ((400 - 64) // 24 + 1 - ((300 - 64) // 24 + 1), 2, 33)
    assert pool.positions.tolist() == [400, 0, 7, 0] and pool.live.tolist() == [True, False, True, False]
    out = pool.process({0: block(0)})                                 # an empty block of a live voice: no device call
    assert out[0].shape == (0, 2, 33) and out[0].dtype == np.float32 and len(fake.calls) == 4
    out = pool.process({1: block(88), 0: block(5)}, start=[1], end=[2, 1, 0])
    assert {s: o.shape[0] for s, o in out.items()} == {0: 0, 1: 2, 2: 0}
    assert (out[1] == 1000 * len(fake.calls) + 1).all()               # columns of slot 1, of this call
    assert fake.calls[-1][1].tolist() == [5, 88, 0, 0] and fake.calls[-1][2].tolist() == [END, START | END, END, 0]
    assert not pool.live.any() and not pool.positions.any()
    pool.process({2: block(10)}, start=[2])
    with pytest.raises(ValueError, match='slot 2 holds a live voice'):
        pool.process({2: block(10)}, start=[2])
    pool.process({2: block(10)}, start=[2], discard=True)
    assert fake.calls[-1][2].tolist() == [0, 0, START, 0] and pool.positions[2] == 10
    assert pool.positions.tolist() == fake.pos.tolist()               # the mirror is the device's
    # one channel, float64, no columns
    mono = _pool(sp, slots=2, channels=1, dtype='float64', columns=False)
    fake = _FakeNative(mono)
    out = mono.process({1: np.zeros(100)}, start=[1], end=[1])        # (n,) for one channel
    assert out[1].shape == (0, 1, 33) and out[1].dtype == np.float64 and fake.calls[-1][1].tolist() == [0, 100]


def test_every_refusal_comes_before_the_native(sp, no_device):
    pool = _pool(sp, slots=3)
    fake = _FakeNative(pool)
    ok = np.zeros((10, 2), np.float32)
    pool.process({0: ok}, start=[0])
    before = (pool.positions.copy(), pool.live.copy(), len(fake.calls))
    for kwargs, error, text in (
            (dict(blocks={1: ok}), ValueError, 'slot 1, which was never started'),
            (dict(end=[1]), ValueError, 'end of slot 1, which was never started'),
            (dict(blocks={0: ok}, start=[0]), ValueError, 'holds a live voice'),
            (dict(blocks={0: np.zeros((101, 2), np.float32)}), ValueError, 'above max_frames_per_call=100'),
            (dict(blocks={0: np.zeros((10, 2), np.float64)}), TypeError, 'float32'),
            (dict(blocks={0: np.zeros((10, 2), np.int16)}), TypeError, 'float32'),
            (dict(blocks={0: np.zeros((10, 1), np.float32)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={0: np.zeros(10, np.float32)}), ValueError, r'expected \(frames, 2\)'),
            (dict(blocks={3: ok}), ValueError, 'outside the pool of 3 slots'),
            (dict(start=[3]), ValueError, 'outside the pool'),
            (dict(start=[True]), ValueError, 'outside the pool'),
            (dict(start=[1, 1]), ValueError, 'named twice'),
            (dict(end=[0, 0]), ValueError, 'named twice')):
        with pytest.raises(error, match=text):
            pool.process(kwargs.get('blocks'), start=kwargs.get('start', ()), end=kwargs.get('end', ()))
        assert len(fake.calls) == before[2], kwargs
        assert pool.positions.tolist() == before[0].tolist() and pool.live.tolist() == before[1].tolist()
    pool._call_host = lambda x, c, f: (np.zeros((3, pool.rows_per_call, 2, 33), np.float32), np.array([1, 0, 0], np.int32))
    from vndecorrelate_amd import _native
    with pytest.raises(_native.NativeError, match='the spans are'):
        pool.process({0: ok})
    assert pool.positions.tolist() == before[0].tolist()
    with pytest.raises(RuntimeError, match='runs through process'):
        pool.process_dev(None, None, None)
    other = _pool(sp, slots=2)
    other._form = 'dev'
    with pytest.raises(RuntimeError, match='runs through process_dev'):
        other.process({0: ok}, start=[0])
    with pytest.raises(ValueError, match='y must be a device tensor'):
        other.process_dev(np.zeros((2, 100, 2), np.float32), None, None)
    with pytest.raises(RuntimeError, match='no means yet'):
        other.coherence()
    with pytest.raises(RuntimeError, match='no means yet'):
        other.welch(0)
    with pytest.raises(ValueError, match='outside the pool'):
        other.welch(2)
    with pytest.raises(ValueError, match='two channels'):
        _pool(sp, channels=1).coherence()


def test_construction_refusals(sp, no_device):
    make = sp.spectrum_voice_pool
    for bad in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='slots'):
            make(bad, 480)
        with pytest.raises(ValueError, match='max_frames_per_call'):
            make(2, bad)
    with pytest.raises(ValueError, match='split the pool'):
        make(65536, 480)
    with pytest.raises(ValueError, match='counts are int32'):
        make(2, 2 ** 31)
    for bad in ('float16', 'int32', None, 'nothing'):
        with pytest.raises(ValueError, match='dtype'):
            make(2, 480, dtype=bad)
    for bad in (0, 3, True, None):
        with pytest.raises(ValueError, match='channels'):
            make(2, 480, channels=bad)
    with pytest.raises(ValueError, match='columns'):
        make(2, 480, columns=1)
    for kw in (dict(nperseg=100), dict(nperseg=32), dict(nperseg=8192), dict(nfft=300), dict(nperseg=256, nfft=128),
               dict(noverlap=256), dict(noverlap=-1), dict(detrend='linear'), dict(detrend=True), dict(scaling='power'),
               dict(nperseg=2.0), dict(nperseg=1, nfft=64), dict(window=np.ones(100)), dict(window=np.ones((2, 128))),
               dict(window=np.ones(256, np.complex64))):
        with pytest.raises(ValueError, match='spectrum_covers'):
            make(2, 480, **kw)
    with pytest.raises(ValueError, match='not positive and finite'):
        make(2, 480, window=np.zeros(256))
    with pytest.raises(ValueError, match='not positive and finite'):
        make(2, 480, fs=1e60)
    with pytest.raises(ValueError, match='more than one launch takes'):
        make(2, 2 ** 22, noverlap=255)                                # 2^22 segments a call: 2^17 runs per slot
    with pytest.raises(ValueError, match='more than one launch takes'):
        make(300, 2 ** 20, noverlap=255)                              # 32769 runs x 300 slots
    with pytest.raises(ValueError, match='more than one launch takes'):
        make(2048, 131040 * 64, nperseg=4096, noverlap=4096 - 64)     # 2^23 workgroups exactly, columns above 2^40 values
    pool = make(5, 480, fs=48000.0, dtype=np.float64, channels=1, nperseg=128, nfft=256, window=('tukey', 0.25))
    assert (pool.slots, pool.nperseg, pool.noverlap, pool.hop, pool.nfft, pool.bins, pool.rows_per_call) == (5, 128, 64, 64, 256, 129, 8)
    assert pool.dtype == np.float64 and make(1, 480).dtype == np.float32 and make(1, 480).hop == 128
    assert make(1, 480).run == 32 and make(1, 480, nperseg=4096, dtype='float64').run == 1
    win = np.hanning(64)
    assert make(1, 10, window=win, nperseg=None).nperseg == 64        # nperseg from an array window


def test_exported_from_the_package():
    import vndecorrelate_amd
    from vndecorrelate_amd import spectral
    assert callable(vndecorrelate_amd.spectrum_voice_pool) and callable(vndecorrelate_amd.spectrum_voice_spans)
    assert vndecorrelate_amd.SpectrumVoicePool is spectral.SpectrumVoicePool
    assert {'spectrum_voice_pool', 'SpectrumVoicePool', 'spectrum_voice_spans'} <= set(spectral.__all__)


# ---- header and binding ------------------------------------------------------------------------------------------------
def test_header_is_plain_c():
    src = ('#include "vnd_spectrum_voice_stream.h"\n'
           'int main(void){return VND_VOICE_START == 1 && VND_VOICE_END == 2 && VND_SPECTRUM_RUN == 32 ? 0 : 1;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == NAMES
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_spectrum_voice_stream.h but not exported'
    for fixed in ('vnd_amd.h', 'vnd_analysis.h', 'vnd_spectrum.h'):                   # they keep their fixed sets
        assert not set(names) & set(_declared(REPO / 'include' / fixed))
    text = re.sub(r'/\*.*?\*/', '', HEADER.read_text(), flags=re.S)
    assert '#include "vnd_spectrum.h"' in text and '#include "vnd_voice_stream.h"' in text
    for wrapper in ('spectrum_voice_stream_state_bytes', 'spectrum_voice_stream_reset_device', 'spectrum_voice_stream_device',
                    'describe_spectrum_voice_stream'):
        assert callable(getattr(_native, wrapper))
    internal = _declared(REPO / 'include' / 'vnd_amd_internal.h')
    assert 'vnd_describe_spectrum_voice_stream_launch' in internal
    assert hasattr(lib, 'vnd_describe_spectrum_voice_stream_launch')
    assert 'vnd_describe_spectrum_voice_stream_launch' in _native.INTERNAL_SIGNATURES


def test_plans_and_state_sizes_that_need_no_device(lib):
    from vndecorrelate_amd import _native
    got = ctypes.c_int64(-7)
    for S, C, W, H, nfft, M, f64 in ((4, 2, 256, 128, 256, 480, 0), (3, 1, 63, 63, 64, 5, 1), (6, 2, 513, 256, 1024, 600, 1),
                                     (2, 2, 4096, 2048, 4096, 5000, 1), (7, 1, 99, 1, 128, 600, 0)):
        R = _native.spectrum_run_length(nfft, W, H, bool(f64), C)
        assert R == sc.spectrum_run(nfft, W, H, 8 if f64 else 4, C)
        lay = sv.layout(S, C, W, H, nfft, M, 8 if f64 else 4, R)
        assert lib.vnd_spectrum_voice_stream_state_bytes(S, C, W, H, nfft, M, f64, ctypes.byref(got)) == 0
        assert got.value == lay['need'], (S, C, W, H, nfft, M, f64)
        text = _native.describe_spectrum_voice_stream(S, C, W, H, nfft, M, bool(f64))
        assert text == (f'spectrum_voice_stream rows_per_call={lay["rc"]} run={R} groups={lay["G"]} nblocks={S * lay["G"]} '
                        f'threads=256 advance_groups={S} state_bytes={lay["need"]}')
    assert 'run=1 groups=4 ' in _native.describe_spectrum_voice_stream(2, 2, 4096, 2048, 4096, 5000, True)    # R = 1
    assert 'rows_per_call=4 run=32 groups=2 nblocks=4096 ' in _native.describe_spectrum_voice_stream(2048, 2, 256, 128, 256, 480)
    for args, status in (((0, 2, 256, 128, 256, 480, 0), INVALID), ((4, 3, 256, 128, 256, 480, 0), INVALID),
                         ((4, 2, 1, 1, 256, 480, 0), INVALID), ((4, 2, 256, 0, 256, 480, 0), INVALID),
                         ((4, 2, 256, 128, 256, 0, 0), INVALID), ((4, 2, 256, 128, 256, 2 ** 31, 0), INVALID),
                         ((4, 2, 256, 128, 100, 480, 0), UNSUPPORTED), ((4, 2, 256, 128, 128, 480, 0), UNSUPPORTED),
                         ((4, 2, 256, 257, 256, 480, 0), UNSUPPORTED), ((65536, 2, 256, 128, 256, 480, 0), UNSUPPORTED),
                         ((2, 2, 256, 1, 256, 2 ** 22, 0), UNSUPPORTED), ((300, 2, 256, 1, 256, 2 ** 20, 0), UNSUPPORTED),
                         ((2048, 2, 4096, 64, 4096, 131040 * 64, 0), UNSUPPORTED)):
        got.value = -7
        assert lib.vnd_spectrum_voice_stream_state_bytes(*args, ctypes.byref(got)) == status and got.value == 0, args
        buf = ctypes.create_string_buffer(256)
        assert lib.vnd_describe_spectrum_voice_stream_launch(*args, buf, 256) == status and not buf.value, args
    assert b'2^40' in lib.vnd_last_error()
    assert lib.vnd_spectrum_voice_stream_state_bytes(4, 2, 256, 128, 256, 480, 0, None) == INVALID
    assert lib.vnd_describe_spectrum_voice_stream_launch(4, 2, 256, 128, 256, 480, 0, None, 64) == INVALID
    assert b'null text' in lib.vnd_last_error()


@pytest.mark.parametrize('f64', [False, True], ids=['f32', 'f64'])
def test_every_abi_refusal_is_reached_with_a_null_context_and_nothing_written(lib, f64):
    """The arguments are checked before the context: host buffers stand for the device's, and no byte of them changes."""
    from vndecorrelate_amd import _native
    S, C, W, H, nfft, M = 3, 2, 64, 32, 64, 100
    dt = np.float64 if f64 else np.float32
    item = np.dtype(dt).itemsize
    R = _native.spectrum_run_length(nfft, W, H, f64, C)
    lay = sv.layout(S, C, W, H, nfft, M, item, R)
    F, rc = lay['F'], lay['rc']
    bufs = dict(state=np.full(lay['need'] // 8 + 2, 0x7FF4A5A5A5A5A5A5, np.uint64), x=np.ones((S, M, C), dt),
                counts=np.full(S, M, np.int32), flags=np.full(S, START, np.int32), win=np.ones(W, dt), tw=np.ones((nfft, 2), dt),
                cols=np.full((S, rc, C, F), 7, dt), oc=np.full(S, -77, np.int32), pxx=np.full((S, F), 7, dt),
                pyy=np.full((S, F), 7, dt), pxy=np.full((S, F, 2), 7, dt), segments=np.full(S, -77, np.int64))
    image = {k: v.tobytes() for k, v in bufs.items()}
    a = {k: v.ctypes.data for k, v in bufs.items()}
    a['state'] += -a['state'] % 16
    a.update(ctx=0, state_bytes=lay['need'], M=M, ss=M * C, fs=C, C=C, W=W, H=H, nfft=nfft, detrend=1, scale=0.5, S=S, stream=0)
    assert sv.raw_call(lib, f64, a) == INVALID and b'null context' in lib.vnd_last_error()     # every argument is good
    for kw in (dict(cols=0), dict(pxx=0, pyy=0, pxy=0, segments=0), dict(C=1, fs=1, pyy=0, pxy=0), dict(C=1, fs=2, ss=2 * M)):
        assert sv.raw_call(lib, f64, dict(a, **kw)) == INVALID and b'null context' in lib.vnd_last_error(), kw  # the nullable ones
    cases = sv.refusals(a, item)
    assert len(cases) > 50
    for kw, status in cases:
        assert sv.raw_call(lib, f64, dict(a, **kw)) == status, (kw, lib.vnd_last_error())
        assert lib.vnd_last_error() and b'null context' not in lib.vnd_last_error(), kw
    null = ctypes.c_void_p(None)
    state = ctypes.c_void_p(a['state'])
    reset = lib.vnd_spectrum_voice_stream_reset_dev
    assert reset(null, state, lay['need'], S, C, W, H, nfft, M, int(f64), null) == INVALID and b'null context' in lib.vnd_last_error()
    for args, status in (((null, lay['need'], S, C, W, H, nfft, M), INVALID), ((state, lay['need'] - 1, S, C, W, H, nfft, M), INVALID),
                         ((ctypes.c_void_p(a['state'] + 4), lay['need'], S, C, W, H, nfft, M), INVALID),
                         ((state, lay['need'], 0, C, W, H, nfft, M), INVALID), ((state, lay['need'], S, C, W, H, 100, M), UNSUPPORTED),
                         ((state, 2 ** 60, 65536, C, W, H, nfft, M), UNSUPPORTED)):
        assert reset(null, *args, int(f64), null) == status, args
        assert b'null context' not in lib.vnd_last_error()
    assert {k: v.tobytes() for k, v in bufs.items()} == image
