"""CPU tier of the streamed cross-correlogram (include/vnd_correlogram_stream.h, analysis.cross_correlogram_stream): the
header, the binding, the row arithmetic, the state size and every refusal - all before any device call, so no GPU is
needed."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_correlogram_stream.h'


def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


def test_header_is_plain_c():
    src = ('#include "vnd_correlogram_stream.h"\nint main(void){int64_t b = 0, r = 0;\n'
           'vnd_status (*f)(vnd_ctx *, void *, int64_t, int64_t, const float *, const float *, int64_t, int32_t, float *,'
           ' int64_t, int64_t, int64_t, int32_t, int32_t, int32_t, float, int64_t *, void *) ='
           ' vnd_correlogram_stream_f32_dev;\n'
           'return f != 0 && vnd_correlogram_stream_state_bytes(1, 882, 4800, &b) == VND_OK && r == 0 ? 1 : 0;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_symbols_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    names = _declared(HEADER)
    assert names == ['vnd_correlogram_stream_f32_dev', 'vnd_correlogram_stream_state_bytes']
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_correlogram_stream.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_analysis.h'))
    assert not set(names) & set(_native.ANALYSIS_SIGNATURES)


def _schedule(rng, n, W, H):
    sched, left = [], n
    while left > 0:           # blocks of 0 and 1 frames, of H, of W - 1, larger ones and the whole rest
        b = int(min(left, rng.choice([0, 1, H, max(1, W - 1), W + 3, 3 * H + 7, int(rng.integers(0, 2 * W + 2)), left])))
        sched.append(b)
        left -= b
    return sched


SIZES = [(882, 441), (320, 160), (100, 250), (64, 1), (1000, 300), (1, 1), (1, 5), (7, 7), (16384, 8192)]


@pytest.mark.parametrize('W,H', SIZES)
@pytest.mark.parametrize('seed', range(4))
def test_rows_over_random_schedules(W, H, seed):
    """Rows per call sum to the one-shot window count, and follow on from one another, whatever the schedule."""
    from vndecorrelate_amd.analysis import stream_rows
    rng = np.random.default_rng(seed * 1000 + W + H)
    for n in (0, 1, max(0, W - 1), W, W + H - 1, W + H, int(rng.integers(0, 5 * W + 3 * H))):
        want = len(np.arange(0, n - W + 1, H))
        pos, nxt, total = 0, 0, 0
        for b in _schedule(rng, n, W, H) + [0]:
            first, end = stream_rows(pos, b, W, H)
            assert first == nxt and end >= first, (n, pos, b)
            if b == 0:
                assert end == first
            nxt, total, pos = end, total + end - first, pos + b
        assert pos == n and total == want, (n, W, H, total, want)


def test_rows_small_cases():
    from vndecorrelate_amd.analysis import stream_rows
    assert stream_rows(0, 881, 882, 441) == (0, 0)          # n < W: no window
    assert stream_rows(881, 1, 882, 441) == (0, 1)          # the first window completes on its last frame
    assert stream_rows(882, 440, 882, 441) == (1, 1)
    assert stream_rows(882, 441, 882, 441) == (1, 2)
    assert stream_rows(0, 1000, 100, 250) == (0, 4)         # H > W: starts 0, 250, 500, 750
    assert stream_rows(0, 5, 1, 1) == (0, 5)


def test_state_bytes(lib):
    b = ctypes.c_int64(-1)
    assert lib.vnd_correlogram_stream_state_bytes(3, 882, 4800, ctypes.byref(b)) == 0
    assert b.value == 3 * (882 - 1 + 4800) * 8
    assert lib.vnd_correlogram_stream_state_bytes(1, 1, 1, ctypes.byref(b)) == 0 and b.value == 8
    assert lib.vnd_correlogram_stream_state_bytes(65535, 16384, 4800, ctypes.byref(b)) == 0
    assert b.value == 65535 * (16383 + 4800) * 8
    for args in ((0, 882, 4800), (-1, 882, 4800), (3, 0, 4800), (3, 882, 0), (3, 882, -5),
                 (2 ** 62, 882, 4800), (3, 882, 2 ** 62), (2 ** 40, 882, 2 ** 30)):
        assert lib.vnd_correlogram_stream_state_bytes(*args, ctypes.byref(b)) == 1 and b.value == 0, args
    assert lib.vnd_correlogram_stream_state_bytes(3, 16385, 4800, ctypes.byref(b)) == 4            # VND_ERR_UNSUPPORTED
    assert lib.vnd_correlogram_stream_state_bytes(3, 882, 4800, None) == 1
    from vndecorrelate_amd import _native
    assert _native.correlogram_stream_state_bytes(2, 320, 64) == 2 * (319 + 64) * 8
    with pytest.raises(ValueError):
        _native.correlogram_stream_state_bytes(2, 320, 0)


@pytest.fixture
def no_device(monkeypatch):
    """Any device call fails the test: the refusals must come first."""
    from vndecorrelate_amd import _native, analysis

    def refuse(*a, **k):
        raise AssertionError('a device call before the refusal')
    monkeypatch.setattr(_native, 'default_context', refuse)
    monkeypatch.setattr(_native, 'correlogram_stream_device', refuse)
    monkeypatch.setattr(_native, 'correlogram_stream_state_bytes', refuse)
    monkeypatch.setattr(analysis, '_torch', refuse)
    return analysis


def test_construction_refusals(no_device):
    an = no_device
    s = an.cross_correlogram_stream()
    assert (s.window, s.hop, s.num_lags, s.position, s.num_streams) == (882, 441, 1765, 0, 1)
    assert isinstance(s, an.CorrelogramStream) and 'cross_correlogram_stream' in an.__all__
    for kw, match in ((dict(stride_seconds=0.0), 'correlogram_covers'),           # hop 0
                      (dict(window_size_seconds=0.0), 'correlogram_covers'),      # window 0
                      (dict(window_size_seconds=1.0), 'correlogram_covers'),      # above the cap
                      (dict(max_lag_seconds=-0.01), 'correlogram_covers'),        # negative lag count
                      (dict(epsilon=np.float64(1e-10)), 'correlogram_covers'),    # promotion changes
                      (dict(epsilon=1e40), 'correlogram_covers'),
                      (dict(max_frames_per_call=0), 'max_frames_per_call'),
                      (dict(max_frames_per_call=2.5), 'max_frames_per_call'),
                      (dict(max_frames_per_call=True), 'max_frames_per_call')):
        with pytest.raises(ValueError, match=match):
            an.cross_correlogram_stream(**kw)
    for n, match in ((0, 'num_streams'), (-1, 'num_streams'), (1.0, 'num_streams'), (65536, 'split the pool')):
        with pytest.raises(ValueError, match=match):
            an.cross_correlogram_stream(n)


def test_block_refusals(no_device):
    an = no_device
    s = an.cross_correlogram_stream(max_frames_per_call=16)
    z = lambda *shape: np.zeros(shape, np.float32)
    with pytest.raises(ValueError, match='max_frames_per_call'):
        s.process(z(17, 2))
    with pytest.raises(ValueError, match='max_frames_per_call'):
        s.process(z(17), z(17))
    for bad in (z(4, 3), z(4), z(2, 4, 2), z(1, 4, 3), z(4, 2, 1)):
        with pytest.raises(ValueError):
            s.process(bad)
    for bx, by in ((z(4), z(5)), (z(4, 2), z(4)), (z(2, 4), z(2, 4)), (z(1, 4, 2), z(1, 4, 2))):
        with pytest.raises(ValueError):
            s.process(bx, by)
    with pytest.raises(TypeError):
        s.process(np.zeros((4, 2), np.complex64))
    with pytest.raises(TypeError):
        s.process(np.array([['a', 'b']]))
    p = an.cross_correlogram_stream(3, max_frames_per_call=8)
    for bad in (z(4, 2), z(2, 4, 2), z(3, 4, 3), z(3, 9, 2)):
        with pytest.raises(ValueError):
            p.process(bad)
    with pytest.raises(ValueError):
        p.process(z(4), z(4))                                   # the unbatched form needs a pool of one
    with pytest.raises(ValueError):
        p.process(z(3, 9), z(3, 9))
    assert s.position == 0 and p.position == 0


def test_empty_blocks_and_flush_need_no_device(no_device):
    an = no_device
    s = an.cross_correlogram_stream(max_frames_per_call=16)
    out = s.process(np.zeros((0, 2), np.float32))
    assert out.shape == (0, 1765) and out.dtype == np.float32
    assert s.process(np.zeros(0), np.zeros(0)).shape == (0, 1765)
    p = an.cross_correlogram_stream(3, max_frames_per_call=16)
    assert p.process(np.zeros((3, 0, 2))).shape == (3, 0, 1765)
    assert p.flush().shape == (3, 0, 1765)
    with pytest.raises(RuntimeError, match='reset'):
        p.process(np.zeros((3, 0, 2)))
    with pytest.raises(RuntimeError):
        p.flush()
    p.reset()
    assert p.process(np.zeros((3, 0), np.float64), np.zeros((3, 0))).shape == (3, 0, 1765) and p.position == 0
    assert s.flush().shape == (0, 1765)


def test_without_a_device_the_first_call_that_needs_one_raises(monkeypatch):
    """No device (here: a context that cannot be made, as on a host without one): blocks of 0 frames still answer, the
    first block with frames raises RuntimeError and leaves the position alone."""
    from vndecorrelate_amd import _native, analysis

    def no_context():
        raise _native.NativeError('no gfx950 device')
    monkeypatch.setattr(_native, 'default_context', no_context)
    s = analysis.cross_correlogram_stream(2, max_frames_per_call=16)
    assert s.process(np.zeros((2, 0, 2), np.float32)).shape == (2, 0, 1765)
    with pytest.raises(RuntimeError):
        s.process(np.zeros((2, 8, 2), np.float32))
    assert s.position == 0 and s._state is None
