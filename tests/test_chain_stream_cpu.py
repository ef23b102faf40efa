"""CPU tier of the Haas and chain streams (include/vnd_haas_stream.h, streaming.HaasStream / ChainStream): the header, the
binding, the span arithmetic, a NumPy model of the ring protocol against HaasEffect.decorrelate, chain planning and every
refusal - all before any device call, so no GPU is needed."""
import pathlib
import re
import subprocess

import numpy as np
import pytest

REPO = pathlib.Path(__file__).resolve().parents[1]
HEADER = REPO / 'include' / 'vnd_haas_stream.h'
FS = 48000


def _declared(header):
    text = re.sub(r'/\*.*?\*/', '', header.read_text(), flags=re.S)
    return sorted(set(re.findall(r'\b(vnd_[a-z0-9_]+)\s*\(', text)))


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


@pytest.fixture(scope='module')
def vnd():
    import vndecorrelate_amd.decorrelation as d
    return d


def test_haas_stream_header_is_plain_c():
    src = ('#include "vnd_haas_stream.h"\nint main(void){int64_t b = 0;\n'
           'return vnd_haas_stream_state_bytes(1, 2, 960, 480, &b) == VND_OK ? 1 : 0;}\n')
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', str(REPO / 'include'),
                        '-x', 'c', '-'], input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()


def test_haas_stream_symbols_exported_and_bound(lib):
    names = _declared(HEADER)
    assert names == ['vnd_haas_stream_f64_dev', 'vnd_haas_stream_f64_host', 'vnd_haas_stream_state_bytes']
    for name in names:
        assert hasattr(lib, name), f'{name} declared in vnd_haas_stream.h but not exported'
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_amd.h'))
    assert not set(names) & set(_declared(REPO / 'include' / 'vnd_stream.h'))


def test_state_bytes_query(lib):
    import ctypes
    b = ctypes.c_int64(-1)
    assert lib.vnd_haas_stream_state_bytes(3, 2, 960, 480, ctypes.byref(b)) == 0 and b.value == 3 * (960 + 480) * 2 * 4
    assert lib.vnd_haas_stream_state_bytes(3, 1, 960, 480, ctypes.byref(b)) == 0 and b.value == 3 * (960 + 480) * 4
    assert lib.vnd_haas_stream_state_bytes(3, 2, 0, 480, ctypes.byref(b)) == 0 and b.value == 0
    for args in ((3, 3, 960, 480), (3, 2, -1, 480), (-1, 2, 960, 480), (65536, 2, 960, 480), (3, 2, 960, -1)):
        assert lib.vnd_haas_stream_state_bytes(*args, ctypes.byref(b)) == 1, args


def _schedule(rng, n, d):
    sched, left = [], n
    while left > 0:           # B = 0, B < d, B > d, and the whole rest at once
        b = int(min(left, rng.choice([0, 1, max(1, d // 3), d + 5, 4 * d + 17, left])))
        sched.append(b)
        left -= b
    return sched


@pytest.mark.parametrize('seed', range(8))
def test_haas_spans_over_random_schedules(seed):
    from vndecorrelate_amd.streaming import haas_output_span
    rng = np.random.default_rng(seed)
    d = int(rng.choice([0, 1, 7, 144, 960]))
    n = int(rng.choice([0, 1, max(0, d // 2), d, d + 1, 5000]))      # d // 2: a whole signal shorter than the delay
    pos, total = 0, 0
    for b in _schedule(rng, n, d) + [None]:
        final = b is None
        first, end = haas_output_span(pos, 0 if final else b, d, final)
        assert first == pos == total
        assert end - first == (d if final else b)
        total = end
        pos += 0 if final else b
    assert total == n + d


class RingModel:
    """The kernel's protocol in NumPy: ring of capacity d + M, slot = frame mod capacity, reads below the position from
    the ring, the chunk's last min(n_in, d) frames written after; each output frame through the one-shot's float64 steps."""

    def __init__(self, d, ch, ms, width, cx, M):
        self.d, self.ch, self.ms, self.width, self.cx, self.M = d, ch, ms, width, cx, M
        self.cap = d + M
        self.ring = np.full((self.cap, cx), np.nan, np.float32)      # never read before written
        self.pos = 0

    def frame(self, f, chunk):
        if f < 0 or f >= self.pos + len(chunk):
            return None
        return chunk[f - self.pos] if f >= self.pos else self.ring[f % self.cap]

    def column(self, c, fr):
        if fr is None:
            return 0.0
        if self.cx == 1:
            return float(np.float64(fr[0]))
        l, r = np.float64(fr[0]), np.float64(fr[1])
        if not self.ms:
            return l if c == 0 else r
        return (l + r) * 0.5 if c == 0 else (l - r) * 0.5

    def call(self, chunk, final):
        assert len(chunk) <= self.M
        n_out = len(chunk) + (self.d if final else 0)
        y = np.empty((n_out, 2))
        for k in range(n_out):
            t = self.pos + k
            c = [self.column(j, self.frame(t - self.d if j == self.ch else t, chunk)) for j in range(2)]
            v = np.array(c, np.float64)
            if self.ms:
                v = np.array([v[0] + v[1], v[0] - v[1]])
                if self.cx == 1:
                    v = v * 0.5
            if self.width is not None:
                m, s = (v[0] + v[1]) * 0.5 * (1.0 - self.width), (v[0] - v[1]) * 0.5 * self.width
                v = np.array([m + s, m - s])
            y[k] = v
        w = 0 if final else min(len(chunk), self.d)
        for f in range(self.pos + len(chunk) - w, self.pos + len(chunk)):
            self.ring[f % self.cap] = chunk[f - self.pos]
        self.pos += len(chunk)
        return y


@pytest.mark.parametrize('seed', range(10))
def test_ring_model_reproduces_haas_effect(vnd, seed):
    rng = np.random.default_rng(100 + seed)
    d = int(rng.choice([0, 1, 13, 48]))
    cx = int(rng.choice([1, 2]))
    n = int(rng.choice([0, 1, max(1, d // 2), 3 * d + 40]))
    ms, ch = bool(rng.integers(2)), int(rng.integers(2))
    width = [None, 0.3, 0.7][int(rng.integers(3))]
    M = int(rng.choice([max(1, d // 3), d + 5, 64]))
    x = rng.uniform(-1, 1, (n, cx) if cx == 2 else (n,)).astype(np.float32)
    stage = vnd.HaasEffect(sample_rate_hz=1000, delay_time_seconds=d / 1000, delayed_channel=ch,
                           mode='MS' if ms else 'LR', width=width)
    want = stage.decorrelate(x)
    model = RingModel(d, ch, ms, width, cx, M)
    x2 = x.reshape(n, cx)
    outs, pos = [], 0
    for b in _schedule(rng, n, d):
        b = min(b, M)
        outs.append(model.call(x2[pos:pos + b], False))
        pos += b
    while pos < n:
        b = min(M, n - pos)
        outs.append(model.call(x2[pos:pos + b], False))
        pos += b
    outs.append(model.call(x2[:0], True))
    got = np.concatenate(outs)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))


def _fir():
    import vndecorrelate_amd.decorrelation as d
    return d.generate_velvet_noise(duration_seconds=0.03, num_impulses=30, sample_rate_hz=FS, seed=1)


def test_chain_planning(vnd):
    chain = (vnd.SignalChain(sample_rate_hz=FS).velvet_noise(duration_seconds=0.02, seed=1, normalizer=None)
             .haas_effect(delay_time_seconds=0.02, delayed_channel=1, mode='LR'))
    cs = chain.stream(num_streams=5, max_frames_per_call=480)
    H = cs.streams[0].latency_frames
    assert 0 < H < 960
    assert [p.kind for p in cs.plan] == ['velvet', 'haas']
    assert [p.in_channels for p in cs.plan] == [2, 2]
    assert [p.in_dtype for p in cs.plan] == [None, 'float32']
    assert [p.max_frames_per_call for p in cs.plan] == [480, max(480, H)]
    assert (cs.latency_frames, cs.tail_frames) == (H, 960)

    fir = _fir()
    H1 = int(max(np.flatnonzero(fir[:, c]).max() for c in range(2)))
    chain = (vnd.SignalChain(sample_rate_hz=FS).haas_effect(delay_time_seconds=0.01, delayed_channel=1)
             .velvet_noise(seed=2, normalizer=None).haas_effect(delay_time_seconds=0.001)
             .stateless(vnd.convolve_velvet_noise, velvet_noise_filters=fir))
    with pytest.raises(TypeError, match='stage 3'):
        chain.stream()
    chain = (vnd.SignalChain(sample_rate_hz=FS).stateless(vnd.convolve_velvet_noise, velvet_noise_filters=fir)
             .haas_effect(delay_time_seconds=0.01).velvet_noise(seed=2, normalizer=None)
             .haas_effect(delay_time_seconds=0.001))
    cs = chain.stream(num_streams=2, max_frames_per_call=64)
    H2 = cs.streams[2].latency_frames
    assert [p.kind for p in cs.plan] == ['convolve', 'haas', 'velvet', 'haas']
    assert [p.in_dtype for p in cs.plan] == [None, 'float32', 'float64', 'float32']
    assert [p.max_frames_per_call for p in cs.plan] == [64, H1, H1 + 480, H1 + 480 + H2]
    assert (cs.latency_frames, cs.tail_frames) == (H1 + H2, 480 + 48)
    mono = (vnd.SignalChain(sample_rate_hz=FS).haas_effect(delay_time_seconds=0.001)
            .velvet_noise(seed=2, normalizer=None)).stream(in_channels=1)
    assert [p.in_channels for p in mono.plan] == [1, 2]
    mono = vnd.SignalChain(sample_rate_hz=FS).velvet_noise(seed=2, normalizer=None).stream(in_channels=1)
    assert mono.plan[0].in_channels == 1 and mono.num_channels == 2


def test_haas_stream_coverage(vnd):
    s = vnd.HaasEffect(sample_rate_hz=FS, delay_time_seconds=0.02, delayed_channel=1).stream(num_streams=3)
    assert (s.latency_frames, s.tail_frames, s.num_streams, s.in_channels) == (0, 960, 3, 2)
    for bad in (dict(delayed_channel=2), dict(width=np.float32(0.5)), dict(width=float('nan')),
                dict(delay_time_seconds=-0.01), dict(mode='XY')):
        with pytest.raises(ValueError):
            vnd.HaasEffect(sample_rate_hz=FS, **bad).stream()
    for bad in (dict(in_channels=3), dict(num_streams=0), dict(max_frames_per_call=0), dict(num_streams=65536)):
        with pytest.raises(ValueError):
            vnd.HaasEffect(sample_rate_hz=FS).stream(**bad)
    s = vnd.HaasEffect(sample_rate_hz=FS).stream(max_frames_per_call=16)
    with pytest.raises(ValueError, match='max_frames_per_call'):
        s.process(np.zeros((17, 2), np.float32))
    with pytest.raises(ValueError):
        s.process(np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError):
        s.process(np.zeros((4, 2), np.complex64))


def test_chain_refusals_raise_before_any_device_call(vnd):
    fir = _fir()
    sc = lambda: vnd.SignalChain(sample_rate_hz=FS)
    cases = [
        (sc().velvet_noise(seed=1), ValueError, 'stage 0.*normalizer=None'),
        (sc().haas_effect().velvet_noise(seed=1), ValueError, 'stage 1.*normalizer=None'),
        (sc().white_noise(), ValueError, 'stage 0.*WhiteNoise'),
        (sc().haas_effect().stateless(vnd.convolve_velvet_noise, velvet_noise_filters=fir), TypeError, 'stage 1.*float64'),
        (sc().stateless(vnd.convolve_velvet_noise, velvet_noise_filters=fir.astype(np.float64)), TypeError, 'stage 0'),
        (sc().stateless(vnd.convolve_velvet_noise, fir), TypeError, 'stage 0'),
        (sc().stateless(np.abs), TypeError, 'stage 0'),
        (sc().haas_effect(delayed_channel=3), ValueError, 'stage 0'),
        (sc().velvet_noise(num_outs=1, seed=1, normalizer=None, mode='LR').haas_effect(), ValueError, 'stage 0'),
    ]
    for chain, exc, match in cases:
        with pytest.raises(exc, match=match):
            chain.stream()
    # channel counts the next stage cannot take
    with pytest.raises(ValueError, match='stage 1.*1 channels'):
        (sc().velvet_noise(num_outs=1, seed=1, normalizer=None, mode='LR').haas_effect()).stream(in_channels=1)
    with pytest.raises(ValueError, match='stage 0.*IndexError'):
        sc().stateless(vnd.convolve_velvet_noise, velvet_noise_filters=fir).stream(in_channels=1)
    with pytest.raises(ValueError, match='stage 0'):
        sc().haas_effect().stream(in_channels=3)
    for kw in (dict(num_streams=0), dict(mode=7), dict(max_frames_per_call=-1)):
        with pytest.raises(ValueError):
            sc().haas_effect().stream(**kw)
    # a float64 chunk into a convolve-first chain: refused by the first stage's rule, before the upload
    cs = sc().stateless(vnd.convolve_velvet_noise, velvet_noise_filters=fir).stream()
    with pytest.raises(TypeError):
        cs.process(np.zeros((10, 2)))
    with pytest.raises(ValueError):
        cs.process(np.zeros((4801, 2), np.float32))
