"""GPU tier of the device cross-correlogram (vnd_correlogram_f32_dev, include/vnd_analysis.h): the reference's fixtures
under the bounds of DESIGN.md §3.8, randomised shapes against R (the same formula with exact sums) within one float32
ulp, the batched, strided and device-tensor forms bit for bit against the per-stream call, an output above 2^31 floats,
argument checks and the window cap."""
import json
import pathlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parents[1]
GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden'


def fixture_inputs(case, g):
    """A fixture case's (x, y), rebuilt from its manifest recipe by the generator's own function."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('gen_correlogram_golden', REPO / 'tools' / 'gen_correlogram_golden.py')
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen.fixture_inputs(case['input'], g)


@pytest.fixture(scope='module')
def an():
    from vndecorrelate_amd import _native, analysis
    ctx = _native.default_context()
    assert 'gfx950' in ctx.info()['name']
    yield analysis
    analysis.set_correlogram_device(None)


@pytest.fixture(scope='module')
def torch():
    import torch as t
    return t


def exact_R(x, y, W, hop, num_lags, eps):
    """The contract's R for every window of (x, y): sums in float128 (exact products of float32, 64-bit sums), each
    rounded to float32, then NumPy 2's float32 normaliser."""
    x = np.asarray(x, np.float32)
    y = np.asarray(y, np.float32)
    n = len(x)
    windows = (n - W) // hop + 1 if n >= W else 0
    out = np.zeros((windows, num_lags), np.float32)
    keep = min(num_lags, 2 * W - 1)
    for w in range(windows):
        xw = x[w * hop:w * hop + W].astype(np.longdouble)
        yw = y[w * hop:w * hop + W].astype(np.longdouble)
        num = np.correlate(xw, yw, 'full')[:keep].astype(np.float32)
        exx, eyy = np.float32(np.sum(xw * xw)), np.float32(np.sum(yw * yw))
        with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
            d = np.float32(np.sqrt(np.float32(exx * eyy)) + np.float32(eps))
            out[w, :keep] = num / d
    return out


def ulps(a, b):
    """Distance in float32 ulps (on the monotone integer line of the bit patterns)."""
    def line(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(line(a) - line(b))


def device(torch, an, x, y, W, hop, num_lags, eps=1e-10, frame_stride=1):
    """x, y float32 (B, n) through the C entry point; float32 (B, windows, num_lags) on the host."""
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    xd = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    yd = torch.from_numpy(np.ascontiguousarray(y, np.float32)).to(dev)
    out = an._launch(torch, ctx, xd.data_ptr(), yd.data_ptr(), x.shape[0], x.shape[1], x.shape[1], 1, W, hop, num_lags,
                     eps, dev)
    return out.cpu().numpy()


def test_fixtures_within_bounds(an):
    from vndecorrelate_amd.utils import dsp
    g = np.load(GOLDEN / 'correlogram.npz')
    manifest = json.loads((GOLDEN / 'correlogram_manifest.json').read_text())
    an.set_correlogram_device(True)
    try:
        for name, case in manifest['cases'].items():
            (x, y), ref = fixture_inputs(case, g), g[name + '__out']
            got = dsp.cross_correlogram(x, y, **case['kwargs'])
            assert got.dtype == np.float32 and got.shape == ref.shape, name
            fs = case['kwargs'].get('sample_rate_hz', 44100)
            W, hop, lag = dsp.correlogram_sizes(fs, case['kwargs'].get('max_lag_seconds', 0.02),
                                                case['kwargs'].get('window_size_seconds', 0.02),
                                                case['kwargs'].get('stride_seconds', 0.01))
            diff = np.abs(got.astype(np.float64) - ref)
            assert diff.max(initial=0) <= (2 * W + 4) * 2.0 ** -24, name
            assert diff.max(initial=0) <= 1e-6, name
            R = exact_R(x, y, W, hop, 2 * lag + 1, 1e-10)
            assert ulps(got, R).max(initial=0) <= 1, name
            if name == 'huge_16k':
                assert not got.any()
    finally:
        an.set_correlogram_device(None)


SHAPES = [  # W, hop, num_lags, n
    (1, 1, 1, 7), (1, 3, 5, 10), (2, 1, 3, 9), (2, 5, 2, 23), (15, 15, 29, 100), (16, 7, 31, 131), (17, 40, 40, 300),
    (64, 32, 127, 640), (100, 1, 50, 260), (255, 100, 509, 1500), (256, 256, 600, 1300), (257, 300, 513, 2000),
    (320, 160, 1601, 3333), (500, 1000, 999, 4321), (882, 441, 1765, 5000), (1023, 511, 2045, 4000),
    (1024, 1024, 2047, 5121), (1025, 2000, 3000, 6000), (1500, 700, 101, 5000), (2047, 999, 4093, 7000),
    (3000, 1500, 5999, 9001), (2999, 4000, 7000, 12000),
]


@pytest.mark.parametrize('W,hop,num_lags,n', SHAPES)
def test_random_shapes_against_exact(torch, an, W, hop, num_lags, n):
    rng = np.random.default_rng(W * 7919 + hop)
    x = rng.uniform(-1, 1, (2, n)).astype(np.float32)
    y = rng.standard_normal((2, n)).astype(np.float32)
    x[1, : n // 3] *= 1e-3                                        # a quieter stretch in the second stream
    got = device(torch, an, x, y, W, hop, num_lags)
    for b in range(2):
        R = exact_R(x[b], y[b], W, hop, num_lags, 1e-10)
        assert got[b].shape == R.shape
        assert ulps(got[b], R).max(initial=0) <= 1, (W, hop, num_lags, n, b)
        if num_lags > 2 * W - 1:
            assert not got[b][:, 2 * W - 1:].any()


@pytest.mark.parametrize('amplitude', [0.0, 1e-20, 3e-12, 1e17, 1e19])
def test_quiet_and_overflow_windows(torch, an, amplitude):
    rng = np.random.default_rng(3)
    x = (rng.uniform(-1, 1, (1, 4000)) * amplitude).astype(np.float32)
    y = (rng.uniform(-1, 1, (1, 4000)) * amplitude).astype(np.float32)
    got = device(torch, an, x, y, 320, 160, 641)
    R = exact_R(x[0], y[0], 320, 160, 641, 1e-10)
    if amplitude >= 1e19:                                          # sums beyond float32: NaN where R is NaN
        assert np.array_equal(np.isnan(got[0]), np.isnan(R))
        fin = ~np.isnan(R)
        assert ulps(got[0][fin], R[fin]).max(initial=0) <= 1
    else:
        assert ulps(got[0], R).max(initial=0) <= 1
    if amplitude in (0.0, 1e17):
        assert not got.any()


def test_batched_equals_per_stream_and_is_deterministic(an):
    from vndecorrelate_amd.utils import dsp
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (5, 9000)).astype(np.float32)
    y = rng.uniform(-1, 1, (5, 9000)).astype(np.float32)
    y[3] = x[1]
    kw = dict(sample_rate_hz=16000, max_lag_seconds=0.03, window_size_seconds=0.02, stride_seconds=0.013)
    an.set_correlogram_device(True)
    try:
        got = an.cross_correlogram_batched(x, y, **kw)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32
        for b in range(5):
            assert np.array_equal(got[b], dsp.cross_correlogram(x[b], y[b], **kw)), b
        again = an.cross_correlogram_batched(x[::-1].copy(), y[::-1].copy(), **kw)
        assert np.array_equal(again[::-1], got)                       # stream position and runs
    finally:
        an.set_correlogram_device(None)
    an.set_correlogram_device(False)
    try:
        host = an.cross_correlogram_batched(x, y, **kw)
    finally:
        an.set_correlogram_device(None)
    assert np.abs(host.astype(np.float64) - got).max() <= 1e-6


def test_interleaved_stereo_equals_deinterleaved(an):
    rng = np.random.default_rng(12)
    st = rng.uniform(-1, 1, (3, 22050, 2)).astype(np.float32)
    an.set_correlogram_device(True)
    try:
        inplace = an.cross_correlogram_batched(st)
        split = an.cross_correlogram_batched(np.ascontiguousarray(st[:, :, 0]), np.ascontiguousarray(st[:, :, 1]))
    finally:
        an.set_correlogram_device(None)
    assert inplace.shape == (3, 49, 1765)
    assert np.array_equal(inplace, split)


def test_device_tensor_in_device_tensor_out(torch, an):
    from vndecorrelate_amd import _native
    dev = torch.device('cuda', _native.default_context().device)
    rng = np.random.default_rng(13)
    st = rng.uniform(-1, 1, (2, 13230, 2)).astype(np.float32)
    xd = torch.from_numpy(st).to(dev)
    got = an.cross_correlogram_batched(xd)
    assert isinstance(got, torch.Tensor) and got.device == dev and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy(), an.cross_correlogram_batched(st))
    pair = an.cross_correlogram_batched(xd[:, :, 0].contiguous(), xd[:, :, 1].contiguous())
    assert torch.equal(pair, got)


def test_output_above_2_to_31_floats(torch, an):
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    B, n, W, hop, lags = 4, 4_300_000, 64, 1, 127
    windows = (n - W) // hop + 1
    assert B * windows * lags > 2 ** 31
    rng = np.random.default_rng(14)
    x = rng.uniform(-1, 1, (B, n)).astype(np.float32)
    y = rng.uniform(-1, 1, (B, n)).astype(np.float32)
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    out = an._launch(torch, ctx, xd.data_ptr(), yd.data_ptr(), B, n, n, 1, W, hop, lags, 1e-10, dev)
    first = out[0, :3].cpu().numpy()
    last = out[B - 1, -3:].cpu().numpy()
    del out
    torch.cuda.empty_cache()
    assert ulps(first, exact_R(x[0, :W + 2], y[0, :W + 2], W, hop, lags, 1e-10)).max() <= 1
    tail = slice(n - W - 2, n)
    assert ulps(last, exact_R(x[B - 1, tail], y[B - 1, tail], W, hop, lags, 1e-10)).max() <= 1


def test_bad_arguments_launch_nothing(torch, an):
    from vndecorrelate_amd import _native
    ctx = _native.default_context()
    dev = torch.device('cuda', ctx.device)
    x = torch.zeros((2, 100), dtype=torch.float32, device=dev)
    out = torch.full((2, 9, 21), float('nan'), dtype=torch.float32, device=dev)
    good = dict(batch=2, n=100, stream_stride=100, frame_stride=1, window=20, hop=10, num_lags=21)
    for key in good:
        for bad in (0, -1):
            a = dict(good, **{key: bad})
            with pytest.raises(ValueError):
                _native.correlogram_device(ctx, x.data_ptr(), x.data_ptr(), out.data_ptr(), a['batch'], a['n'],
                                           a['stream_stride'], a['frame_stride'], window=a['window'], hop=a['hop'],
                                           num_lags=a['num_lags'], eps=1e-10)
    with pytest.raises(ValueError):                               # out overlapping the input
        _native.correlogram_device(ctx, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 100, 100, 1, window=20, hop=90,
                                   num_lags=1, eps=1e-10)
    with pytest.raises(_native.NativeError):                      # above the cap: VND_ERR_UNSUPPORTED
        _native.correlogram_device(ctx, x.data_ptr(), x.data_ptr(), out.data_ptr(), 1, 20000, 20000, 1,
                                   window=an.MAX_WINDOW + 1, hop=1, num_lags=1, eps=1e-10)
    torch.cuda.synchronize(dev)
    assert torch.isnan(out).all()


def test_window_above_cap_is_numpy(an):
    from vndecorrelate_amd.utils import dsp
    rng = np.random.default_rng(15)
    x = rng.uniform(-1, 1, 40000).astype(np.float32)
    y = rng.uniform(-1, 1, 40000).astype(np.float32)
    kw = dict(sample_rate_hz=an.MAX_WINDOW + 1, max_lag_seconds=0.0005, window_size_seconds=1.0, stride_seconds=0.5)
    assert not an.correlogram_covers(40000, an.MAX_WINDOW + 1, 8192, 17, 1e-10)
    an.set_correlogram_device(True)
    try:
        got = dsp.cross_correlogram(x, y, **kw)
    finally:
        an.set_correlogram_device(None)
    assert np.array_equal(got, dsp._correlogram_numpy(x, y, an.MAX_WINDOW + 1, 8192, 8, 1e-10))
