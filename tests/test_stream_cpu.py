"""CPU tier of the chunked stream (include/vnd_stream.h, vndecorrelate_amd/streaming.py): the header, the binding, the
output-count arithmetic and every argument check - all before any device call, so no GPU is needed."""
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
STREAM_HEADER = REPO / 'include' / 'vnd_stream.h'


def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


def test_stream_header_is_plain_c():
    src = ('#include "vnd_stream.h"\nint main(void){int64_t b = 0;\n'
           'return vnd_stream_state_bytes((const vnd_taps *)0, 1, 2, 480, &b) == VND_OK ? 1 : 0;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_stream_symbols_exported_and_bound(lib):
    names = _declared(STREAM_HEADER)
    assert names == ['vnd_stream_f32_dev', 'vnd_stream_f32_host', 'vnd_stream_state_bytes']
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_stream.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))


def _vn(**kw):
    import vndecorrelate_amd.decorrelation as d
    kw.setdefault('normalizer', None)
    return d.VelvetNoise(sample_rate_hz=48000, seed=1, **kw)


def test_latency_is_the_largest_tap_index():
    import vndecorrelate_amd.decorrelation as d
    from vndecorrelate_amd.streaming import convolve_velvet_noise_stream
    fir = d.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, sample_rate_hz=48000, seed=1)
    want = int(max(np.flatnonzero(fir[:, c]).max() for c in range(fir.shape[1])))
    assert convolve_velvet_noise_stream(fir).latency_frames == want
    assert convolve_velvet_noise_stream(fir, in_channels=1).latency_frames == int(np.flatnonzero(fir[:, 0]).max())
    vn = _vn()
    idx = [i for seq in vn.velvet_noise for seg in seq for side in (seg.negative_impulse_indexes,
                                                                     seg.positive_impulse_indexes) for i in side]
    assert vn.stream().latency_frames == int(max(idx))
    assert vn.stream(in_channels=1).latency_frames == int(max(idx))
    assert 1200 < want < 1440


@pytest.mark.parametrize('seed', range(6))
def test_output_counts_over_random_schedules(seed):
    from vndecorrelate_amd.streaming import output_span
    rng = np.random.default_rng(seed)
    latency = int(rng.choice([0, 1, 7, 1439, 5000]))
    n = int(rng.choice([0, 1, latency // 2, latency, latency + 1, 20000]))
    sched, left = [], n
    while left > 0:          # B = 0, B < H, B > H, and the whole rest at once
        b = int(min(left, rng.choice([0, 1, max(1, latency // 3), latency + 5, 4 * latency + 17, left])))
        sched.append(b)
        left -= b
    pos, expect_first, total = 0, 0, 0
    for b in sched + [None]:
        final = b is None
        first, end = output_span(pos, 0 if final else b, latency, final)
        assert first == expect_first and end >= first
        if not final:
            assert end == max(0, pos + b - latency)                # final once frame n + H has arrived
        total += end - first
        expect_first = end
        pos += 0 if final else b
    assert total == n
    # a signal shorter than the latency returns nothing before the flush
    if 0 < n <= latency:
        assert output_span(0, n, latency, False) == (0, 0)


@pytest.mark.parametrize('position', [2 ** 31 - 7, 2 ** 31, 2 ** 32 - 300, 2 ** 32, 2 ** 40 + 3, 2 ** 53 + 1, 2 ** 60 - 480, 2 ** 60])
def test_output_span_at_the_positions_of_a_long_lived_stream(position):
    """The span arithmetic around 2^31 and 2^32 and up to the last position a call takes, 2^60: exact integers, and one
    call's end is the next call's start."""
    from vndecorrelate_amd.streaming import haas_output_span, output_span
    H = 1439
    expect_first, pos, total = position - H, position, 0
    blocks = [0, 1, H, H + 1, 480] if position < 2 ** 60 - 480 else ([480] if position < 2 ** 60 else [])
    for b in blocks + [None]:
        final = b is None
        first, end = output_span(pos, 0 if final else b, H, final)
        assert isinstance(first, int) and isinstance(end, int)
        assert first == expect_first == pos - H and end == (pos if final else pos + b - H)
        total += end - first
        expect_first = end
        pos += 0 if final else b
    assert pos <= 2 ** 60 and total == sum(blocks) + H                # every frame pushed, and the H held before them
    # a steady-state block returns as many frames as it was given, a Haas block too
    assert output_span(position, 480, H, False) == (position - H, position + 480 - H)
    first, end = haas_output_span(position, 480, 700, False)
    assert end - first == 480
    first, end = haas_output_span(position, 0, 700, True)
    assert end - first == 700


def test_errors_without_a_device():
    import vndecorrelate_amd.decorrelation as d
    from vndecorrelate_amd.streaming import convolve_velvet_noise_stream
    fir = d.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, sample_rate_hz=48000, seed=1)
    with pytest.raises(ValueError, match='normalizer=None'):
        d.VelvetNoise(sample_rate_hz=48000, seed=1).stream()
    with pytest.raises(ValueError):
        _vn().stream(in_channels=3)
    with pytest.raises(ValueError):
        _vn(num_outs=4, filtered_channels=(0, 1, 2, 3), mode='MS', width=None).stream()
    with pytest.raises(ValueError):
        _vn().stream(num_streams=0)
    with pytest.raises(ValueError):
        _vn().stream(num_streams=70000)
    with pytest.raises(ValueError):
        _vn().stream(max_frames_per_call=0)
    with pytest.raises(ValueError):
        _vn().stream(mode=7)
    with pytest.raises(TypeError, match='convolve_velvet_noise'):
        convolve_velvet_noise_stream(fir.astype(np.float64))
    with pytest.raises(ValueError):
        convolve_velvet_noise_stream(fir, in_channels=3)
    s = convolve_velvet_noise_stream(fir, num_streams=3, max_frames_per_call=480)
    for bad in (np.zeros((3, 10), np.float32), np.zeros((2, 10, 2), np.float32), np.zeros((3, 10, 1), np.float32),
                np.zeros((10, 2), np.float32), np.zeros((3, 481, 2), np.float32)):
        with pytest.raises(ValueError):
            s.process(bad)
    for dtype in (np.float64, np.int32, np.int64):
        with pytest.raises(TypeError, match='convolve_velvet_noise'):
            s.process(np.zeros((3, 10, 2), dtype))
    # zero-frame pushes and a flush of nothing need no device; process after flush raises until reset
    assert s.process(np.zeros((3, 0, 2), np.float32)).shape == (3, 0, 2)
    assert s.process(np.zeros((3, 0, 2), np.int16)).shape == (3, 0, 2)
    assert s.flush().shape == (3, 0, 2)
    with pytest.raises(RuntimeError):
        s.process(np.zeros((3, 0, 2), np.float32))
    with pytest.raises(RuntimeError):
        s.flush()
    s.reset()
    assert s.process(np.zeros((3, 0, 2), np.float32)).shape == (3, 0, 2) and s.position == 0
    one = _vn().stream(in_channels=1)
    assert one.process(np.zeros(0)).shape == (0, 2)          # mono blocks of any real dtype (decorrelate casts them)
    with pytest.raises(ValueError):
        one.process(np.zeros((5, 2), np.float32))
