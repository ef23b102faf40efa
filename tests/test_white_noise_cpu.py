"""CPU tier of WhiteNoise on the device: the C entry point is declared, exported and bound, refuses bad arguments
without a device, and the Python switch and routing behave; on a box without a GPU the NumPy code runs."""
import ctypes

import numpy as np
import pytest

from test_abi import declared_functions


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as entry
    entry.build()
    from vndecorrelate_amd import _native
    return _native.load_library()


@pytest.fixture
def vnd():
    import vndecorrelate_amd.decorrelation as d
    yield d
    d.set_white_noise_device(None)


def test_entry_point_is_declared_exported_and_bound(lib):
    from vndecorrelate_amd import _native
    import vndecorrelate_amd as pkg
    assert 'vnd_white_noise_f32_dev' in declared_functions()
    assert hasattr(lib, 'vnd_white_noise_f32_dev')
    assert 'vnd_white_noise_f32_dev' in _native.SIGNATURES
    assert callable(_native.white_noise_device)
    assert pkg.set_white_noise_device is pkg.decorrelation.set_white_noise_device


def _call(lib, ctx, *, x=1, h=1, y=1, batch=1, n=100, cx=2, c=2, m=10, use_width=0, normalize=0, ws=None, ws_bytes=0):
    p = lambda v: ctypes.c_void_p(v) if v else None     # noqa: E731 - fake, never dereferenced device addresses
    return lib.vnd_white_noise_f32_dev(ctx, p(x), p(h), p(y), batch, n, cx, c, m, use_width, 0.5, normalize,
                                       ctypes.c_float(1e-10), p(ws), ws_bytes, None)


def test_bad_arguments_are_invalid_without_a_device(lib):
    from vndecorrelate_amd import _native
    fake_ctx = ctypes.c_void_p(0x1000)            # validation happens before the context is touched
    assert _call(lib, None) == 1
    assert b'null context' in lib.vnd_last_error()
    base = dict(x=0x10000, h=0x20000, y=0x30000)
    cases = [
        dict(n=9, m=10),                          # shorter than the filter
        dict(m=0),                                # no taps
        dict(batch=-1),
        dict(cx=3, c=2),                          # channel mismatch
        dict(cx=1, c=3),                          # fan-out only to stereo
        dict(c=0, cx=0),
        dict(c=3, cx=3, use_width=1),             # width needs two channels
        dict(normalize=7),
        dict(normalize=1),                        # normaliser without a workspace
        dict(x=None),                             # null pointers
        dict(h=None),
        dict(y=0x10000 + 400),                    # y overlaps x (100 frames x 2 channels x 4 bytes)
        dict(h=0x30000 + 8),                      # h overlaps y
    ]
    for case in cases:
        kw = {**base, **case}
        assert _call(lib, fake_ctx, **kw) == 1, case
        assert lib.vnd_last_error(), case
    # an empty batch is a no-op, whatever the pointers
    assert _call(lib, fake_ctx, batch=0, x=None, h=None, y=None) == 0
    # and the wrapper maps the status to ValueError
    with pytest.raises(ValueError):
        _native.white_noise_device(type('C', (), {'_lib': lib, 'handle': None})(), 1, 1, 1, 1, 100, 2, 2, 10,
                                   width=None, normalize=0)


def test_switch_rejects_other_values(vnd):
    for bad in (1, 0, 'yes', 2.0, [True]):
        with pytest.raises(TypeError):
            vnd.set_white_noise_device(bad)
    vnd.set_white_noise_device(True)
    vnd.set_white_noise_device(False)
    vnd.set_white_noise_device(None)


def _numpy_white_noise(wn, x):
    from vndecorrelate_amd.utils.dsp import apply_stereo_width, mono_to_stereo, rms_normalize
    x = x.astype(np.float32)
    if x.ndim == 1:
        x = mono_to_stereo(x)
    out = np.zeros((len(x), wn.num_outs), np.float32)
    for c in range(wn.num_outs):
        out[:, c] = np.convolve(x[:, c], wn.white_noise_filter[:, c], mode='same')
    if wn.width is not None:
        apply_stereo_width(out, wn.width)
    rms_normalize(x, out)
    return out


def test_policy_without_a_gpu(vnd):
    from vndecorrelate_amd import _native
    if _native.device_count() > 0:
        pytest.skip('a GPU is present')
    wn = vnd.WhiteNoise(sample_rate_hz=8000, duration_seconds=0.01, seed=3, width=0.5)
    x = np.random.default_rng(1).standard_normal((1000, 2)).astype(np.float32)
    vnd.set_white_noise_device(True)
    with pytest.raises(RuntimeError):
        wn.decorrelate(x)
    with pytest.raises(RuntimeError):
        wn.decorrelate_batched(x[None])
    vnd.set_white_noise_device(None)
    assert np.array_equal(wn.decorrelate(x), _numpy_white_noise(wn, x))
    xb = np.random.default_rng(2).standard_normal((3, 500)).astype(np.float32)
    got = wn.decorrelate_batched(xb)
    assert got.shape == (3, 500, 2) and got.dtype == np.float32
    assert np.array_equal(got, np.stack([_numpy_white_noise(wn, s) for s in xb]))
    vnd.set_white_noise_device(False)
    assert np.array_equal(wn.decorrelate(x), _numpy_white_noise(wn, x))


def test_forced_device_without_one_runs_uncovered_calls_in_numpy(vnd, monkeypatch):
    """set_white_noise_device(True) raises only for a call the device covers; the others run the NumPy code."""
    from vndecorrelate_amd import analysis
    monkeypatch.setattr(analysis, '_gpu_present', lambda: False)
    wn = vnd.WhiteNoise(sample_rate_hz=8000, duration_seconds=0.01, seed=3, width=0.5)
    x = np.random.default_rng(1).standard_normal((1000, 2)).astype(np.float32)
    xf = np.asfortranarray(x)
    assert not vnd.white_noise_covers(xf.shape, wn.num_outs, wn.width, wn.white_noise_filter, xf.flags.c_contiguous)
    vnd.set_white_noise_device(True)
    assert np.array_equal(wn.decorrelate(xf), _numpy_white_noise(wn, xf))
    with pytest.raises(RuntimeError, match='no gfx950 device'):
        wn.decorrelate(x)


def test_routing_table(vnd):
    covers = vnd.white_noise_covers
    rng = np.random.default_rng(0)
    h = lambda m, c: rng.standard_normal((m, c))      # noqa: E731
    n = 1000
    # (shape, num_outs, width, fir, c_contiguous) -> covered
    table = [
        ((n, 2), 2, None, h(30, 2), True, True),        # stereo
        ((n,), 2, None, h(30, 2), True, True),          # mono -> stereo (fan-out)
        ((n,), 2, 0.5, h(30, 2), True, True),
        ((n,), 1, None, h(30, 1), True, False),         # mono with one output: the reference's shapes disagree
        ((n,), 3, None, h(30, 3), True, False),
        ((n, 1), 1, None, h(30, 1), True, True),
        ((n, 3), 3, None, h(30, 3), True, True),
        ((n, 8), 8, None, h(30, 8), True, True),
        ((n, 2), 2, 0.5, h(30, 2), True, True),
        ((n, 3), 3, 0.5, h(30, 3), True, False),        # width needs stereo
        ((n, 8), 8, 0.0, h(30, 8), True, False),
        ((n, 2), 3, None, h(30, 3), True, False),       # channel count differs from num_outs
        ((n, 3), 2, None, h(30, 2), True, False),
        ((n, 2), 2, None, h(30, 1), True, False),       # filter narrower than num_outs
        ((n, 2), 2, None, h(30, 3), True, True),        # wider one: its first columns
        ((n, 2), 2, None, h(30, 2).astype(np.float32), True, False),
        ((n, 2), 2, None, h(30, 2)[:, 0], True, False),  # 1-D filter
        ((n, 2), 2, None, np.where(np.arange(60).reshape(30, 2) == 7, np.inf, 1.0), True, False),
        ((n, 2), 2, None, np.where(np.arange(60).reshape(30, 2) == 7, np.nan, 1.0), True, False),
        ((n, 2), 2, None, list(h(30, 2)), True, False),
        ((29, 2), 2, None, h(30, 2), True, False),      # N < M: NumPy raises
        ((30, 2), 2, None, h(30, 2), True, True),       # N == M
        ((30,), 2, None, h(30, 2), True, True),
        ((n, 2), 2, None, np.zeros((0, 2)), True, False),   # M == 0
        ((0, 2), 2, None, h(1, 2), True, False),
        ((n, 2), 2, None, h(30, 2), False, False),      # NumPy's sums follow the memory layout
        ((n, 2, 1), 2, None, h(30, 2), True, False),
        ((n, 33), 33, None, h(30, 33), True, False),    # past the channels whose sums the device orders as NumPy
    ]
    for shape, outs, width, fir, contiguous, want in table:
        assert covers(shape, outs, width, fir, contiguous) is want, (shape, outs, width, getattr(fir, 'dtype', None))
